"""The field set F of the gradient-field tests (tests/test_foliation_field_host.py,
tests/test_gpu_foliation_classes.py): the expressions of tests/test_foliation_host.py::case, a
depth-8-stack program, a PUSH_P / DIV_P program and a complex program, with their oracle fields
and the three checks both tests apply.  Test infrastructure only."""
import gzip
import os

import numpy as np

import foliation_ref as R
from pdeval import opcodes as OPC
from pdeval import problem_defs as P
from pdeval.flatten import pack

HERE = os.path.dirname(os.path.abspath(__file__))
MS = (5, 9, 12)          # m^2 = 25 (one partial chunk), 81 (full + partial), 144
FIELD_TOL = 5e-10        # relative field error e moves |J|/S by ~2e; 2e <= tau/100, tau = 1e-7
ORACLE_TOL = 5e-12       # the oracle against SymPy's exact gradient, two decades inside FIELD_TOL

BASE = 'rho**2*z'
PARA = 'sqrt(rho**2 + z**2) - z'
MUST_MATCH = [(BASE, f'exp({BASE})'), (BASE, f'square({BASE})'), (BASE, f'inv({BASE})'), (BASE, f'sqrt({BASE})'),
              (PARA, f'exp_neg({PARA})'), ('rho/z', 'rho/Abs(z)')]
POWERS = 'rho**3/(1 + z**2) + exp(z)/z**2'    # compiles to PUSH_P ... DIV_P


def deep8():
    """A balanced tree of 128 distinct leaves, sums and products alternating by level: the
    flattener cannot order it below a stack of 8."""
    cnt = [0]

    def tree(d):
        if d == 1:
            cnt[0] += 1
            k = cnt[0]
            return f'sqrt(rho + {k})' if k % 2 else f'exp(z/{k + 1})'
        a, b = tree(d - 1), tree(d - 1)
        return f'({a} + {b})' if d % 2 else f'({a})*({b})'
    return tree(8)


def complex_program():
    """A constant-free complex program: the imaginary unit alone."""
    return np.array([OPC.PDOP['HEADER'] | (1 << 8) | OPC.FLAG_COMPLEX, OPC.PDOP['PUSH_I']], dtype=np.int32)


def case_exprs(pd_):
    """The 7 paper solutions, then the re-parametrisations, rho/z and rho/Abs(z)."""
    exprs = list(pd_.known_solutions)
    for a, b in MUST_MATCH:
        for s in (a, b):
            if s not in exprs:
                exprs.append(s)
    return exprs


def words(pd_, s):
    return np.array(pd_.compile(pd_.parse(s)), dtype=np.int32)


def op_names(w):
    out, i = [], 1
    while i < len(w):
        out.append(OPC.OP_NAME.get(int(w[i]) & 0xff))
        i += OPC.op_len(int(w[i]))
    return out


_F = None


def field_set():
    """F: dict(pd, exprs (None for the complex program), progs, ops, off, fields {m: [len(F), 2,
    m*m] oracle fields}); computed once and shared, never modified."""
    global _F
    if _F is None:
        pd_ = P.force_free()
        exprs = case_exprs(pd_) + [deep8(), POWERS]
        progs = [words(pd_, s) for s in exprs] + [complex_program()]
        assert (int(progs[len(exprs) - 2][0]) >> 8) & 0xff == 8
        names = op_names(progs[len(exprs) - 1])
        assert 'PUSH_P' in names and 'DIV_P' in names, names
        assert 'rho/Abs(z)' in exprs
        ops, off = pack([list(map(int, w)) for w in progs])
        fields = {m: np.stack([R.oracle_field(w, m) for w in progs]) for m in MS}
        for f in fields.values():
            f.setflags(write=False)
        _F = dict(pd=pd_, exprs=exprs + [None], progs=progs, ops=np.asarray(ops, dtype=np.int32),
                  off=np.asarray(off, dtype=np.int64), fields=fields)
    return _F


def check_fields(got, n_finite, want, what=''):
    """The three checks of a computed field [rows, 2, mm] (and n_finite [rows]) against the
    oracle's: the NaN mask equal, at each finite point |g - g_oracle|_2 <= FIELD_TOL |g_oracle|_2,
    n_finite equal.  Prints the worst relative error before it asserts."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, np.argwhere(np.isnan(got) != np.isnan(want))[:5])
    fin = np.isfinite(want[:, 0, :])
    with np.errstate(invalid='ignore'):
        err = np.sqrt(((got - want) ** 2).sum(axis=1))
        nrm = np.sqrt((want ** 2).sum(axis=1))
    rel = np.where(fin, err / np.where(fin & (nrm > 0), nrm, 1.0), 0.0)
    print(f'{what}: worst relative field error {rel.max() if rel.size else 0.0:.3e} (bound {FIELD_TOL:g})')
    assert np.all(err[fin] <= FIELD_TOL * nrm[fin]), (what, float(rel.max()), np.argwhere(rel > FIELD_TOL)[:5])
    assert np.array_equal(np.asarray(n_finite), fin.sum(axis=1)), (what, n_finite, fin.sum(axis=1))


def d3_strings(n):
    """The 7 paper solutions, then the first n rows of the validated depth-3 stream."""
    path = os.path.join(HERE, 'golden', 'streams', 'force_free_d3_validated.txt.gz')
    with gzip.open(path, 'rt') as f:
        rows = [ln.rstrip('\n').split('\t')[-1] for ln in f]   # (index, depth, expression)
    return list(P.force_free().known_solutions) + rows[:n]

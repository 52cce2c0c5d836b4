"""GPU tests of the complex field pass (PDEVAL_FOL_CPLX; DESIGN.md §14 "Complex-valued rows") against SymPy
derivatives evaluated with mpmath at 40 digits, the rule restated in numpy and tests/foliation_axis_ref.py."""
import mpmath
import numpy as np
import pytest
import sympy as sp

import foliation_axis_ref as A
import foliation_cases as FC
import foliation_ref as R
from pdeval import foliation as FOL
from pdeval import problem_defs as P
from pdeval.opcodes import FLAG_COMPLEX

pytestmark = pytest.mark.gpu

AXIS, CPLX = 1, 4    # PDEVAL_FOL_AXIS, PDEVAL_FOL_CPLX (literals: the file collects on a tree without the flag)
DEEP = '(exp(rho) + sqrt(z**2 + 1))*(exp(z) + sqrt(rho + 1)) + (exp(rho*z) + rho)*(z + exp_neg(rho))'   # stack 3
PARA = 'sqrt(rho**2 + z**2) - z'
# (real partner, complex row): unflagged and non-real on the whole grid (the n_finite selection);
# flagged, the phase varies; unflagged, the phase varies; flagged, stack 3
PAIRS = [('rho**2 + z**2', 'sqrt(neg(rho**2 + z**2))'), ('rho**2*z', 'exp(sqrt(neg(1))*rho**2*z)'),
         (PARA, f'exp(sqrt(neg({PARA})))'), (DEEP, f'sqrt(neg(1))*({DEEP})')]
RHO = ['rho**2', 'sqrt(neg(rho))', 'pow_3_2(neg(rho))']       # the rho-axis class under FOL_AXIS
NO_DIR = 'rho + sqrt(neg(1))*z'                               # a complex direction: no real foliation
PART = 'rho*sqrt(neg(z))'                                     # real where z < 0: the real pass classifies it
EXPRS = [s for p in PAIRS for s in p] + RHO + [NO_DIR, PART]
FLAGGED = [False, False, False, True, False, False, False, True, False, True, True, True, False]   # FLAG_COMPLEX of EXPRS
MS = (16, 12)                                                 # four full chunks; 144 = two full and a partial one


def cplx_rule(u, a, b, tau=R.TAU):
    """The per-point rule (include/pdeval.h) on complex arrays: ([2, mm] field, phase defect)."""
    with np.errstate(all='ignore'):
        ha, hb = np.hypot(a.real, a.imag), np.hypot(b.real, b.imag)
        pa = ha >= hb
        w, o, h, ho = np.where(pa, a, b), np.where(pa, b, a), np.where(pa, ha, hb), np.where(pa, hb, ha)
        tr, ti = o.real * w.real + o.imag * w.imag, o.imag * w.real - o.real * w.imag
        q = tr / h
        fin = np.isfinite(u) & np.isfinite(a) & np.isfinite(b)
        zero = fin & (h == 0)
        ok = fin & ~zero & (np.abs(ti) <= tau * (h * ho)) & np.isfinite(q)
        f = [np.where(zero, 0.0, np.where(ok, np.where(pa == first, h, q), np.nan)) for first in (True, False)]
        return np.stack(f), np.abs(ti) / (h * ho)


def reference(pd_, m):
    """([rows, 2, mm] fields, the rows the complex pass takes) of EXPRS from mpmath jets; asserts that
    no point sits near the tau threshold (the phase defect is rounding-level or O(1))."""
    fields, took = [], []
    with mpmath.workdps(40):
        pts = [(mpmath.mpf(float(x)), mpmath.mpf(float(y))) for x in R.grid_points(m)[0] for y in R.grid_points(m)[1]]
        for k, s in enumerate(EXPRS):
            e = pd_.parse(s)
            u, a, b = (np.array([complex(f(*pt)) for pt in pts]) for f in
                       (sp.lambdify((pd_.x, pd_.y), g, 'mpmath') for g in (e, sp.diff(e, pd_.x), sp.diff(e, pd_.y))))
            real = (u.imag == 0) & (a.imag == 0) & (b.imag == 0)
            took.append(FLAGGED[k] or int(real.sum()) < R.MIN_POINTS)
            f, defect = cplx_rule(u, a, b)
            assert not ((defect > 1e-12) & (defect < 1e-2)).any(), (s, m, defect)
            fields.append(f if took[-1] else np.where(real, np.stack([a.real, b.real]), np.nan))
    return np.stack(fields), np.array(took)


@pytest.fixture(scope='module')
def case():
    """The reference per m, built (and its inputs checked against the tau threshold) before the GPU is
    opened; then EXPRS compiled by a BatchValidator, resident on its device.  Never modified."""
    import torch
    from pdeval.batch import BatchValidator
    ref = {m: reference(P.force_free(), m) for m in MS}
    bv = BatchValidator('force_free', device=0)
    p = bv.prepare_strings(EXPRS)
    ops, off = np.asarray(p['ops'], dtype=np.int32), np.asarray(p['off'], dtype=np.int64)
    assert ((ops[off[:-1]] & FLAG_COMPLEX) != 0).tolist() == FLAGGED and (int(ops[off[7]]) >> 8) & 0xff >= 3
    prog = (torch.from_numpy(ops).to('cuda:0'), int(ops.size), torch.from_numpy(off).to('cuda:0'), len(EXPRS))
    yield bv, prog, ref
    bv.close()


def _params(m, flags):
    return FOL.FolParams(R.TAU, m, R.MIN_POINTS, flags)


@pytest.mark.parametrize('m', MS)
def test_fields(case, m):
    """Flag set: NaN pattern, n_finite and FIELD_TOL against the reference, no bad point under the point
    test; rows not taken are bit-identical to the flag-off field, where the complex rows are all NaN."""
    bv, prog, (want, took) = case[0], case[1], case[2][m]
    got, nfin = (t.cpu().numpy() for t in FOL.gradient_fields(bv.ctx, *prog, None, _params(m, CPLX)))
    off, nfin0 = (t.cpu().numpy() for t in FOL.gradient_fields(bv.ctx, *prog, None, _params(m, 0)))
    FC.check_fields(got, nfin, want, f'cplx m={m}')
    for k in range(len(EXPRS)):
        nu, nb, _ = R.pair_stats(got[k], want[[k]])
        assert nb[0] == 0 and nu[0] == R.pair_stats(want[k], want[[k]])[0][0], (EXPRS[k], nu, nb)
    assert np.array_equal(got[~took].view(np.int64), off[~took].view(np.int64)) and np.array_equal(nfin[~took], nfin0[~took])
    assert np.isnan(off[took]).all() and not nfin0[took].any() and nfin[EXPRS.index(NO_DIR)] == 0


@pytest.mark.parametrize('axis', (0, AXIS))
@pytest.mark.parametrize('m', MS)
def test_classes(case, m, axis):
    """Every complex row lands in its real partner's class, with the restatement's ids; with the axis
    rule the RHO rows are one class of kind 1; NO_DIR stays unclassified; a registry fed in two
    batches gives the same ids."""
    bv, prog, ref = case
    prm = _params(m, CPLX | axis)
    ids = FOL.classify(bv.ctx, *prog, np.arange(len(EXPRS)), prm).class_id
    assert np.array_equal(ids, A.class_ids(A.sequential_leaders(ref[m][0], axis=bool(axis)))), ids
    assert all(ids[2 * k + 1] == ids[2 * k] >= 0 for k in range(len(PAIRS))), ids
    assert ids[EXPRS.index(NO_DIR)] == -1 and ids[EXPRS.index(PART)] == ids[2]
    if axis:
        r0 = EXPRS.index(RHO[0])
        assert ids[r0] == ids[r0 + 1] == ids[r0 + 2] >= 0, ids
        fields, _ = FOL.gradient_fields(bv.ctx, *prog, None, prm)
        assert FOL.field_kinds(bv.ctx, fields, prm)[r0:r0 + 3].tolist() == [1, 1, 1]
    with bv.foliation_registry(prm) as reg:
        parts = [reg.assign(*prog, np.arange(0, 5)), reg.assign(*prog, np.arange(5, len(EXPRS)))]
        assert np.array_equal(np.concatenate(parts), ids)


def test_flag_plumbing(case, tmp_path):
    """BatchValidator passes cplx= through; a file saved without the flag is refused with it; the flag
    without n_finite is PDEVAL_ERR_ARG."""
    bv, prog, _ = case
    cls, acc, _ = bv.foliation_classes(list(PAIRS[0]), cplx=True)
    assert acc.tolist() == [0, 1] and cls.class_id.tolist() == [0, 0]
    with bv.foliation_registry(cplx=True) as reg:
        ids, acc = bv.assign_foliation(reg, list(PAIRS[0]))
        assert acc.tolist() == [0, 1] and ids.tolist() == [0, 0]
    with bv.foliation_registry() as reg:
        reg.save(tmp_path / 'plain.npz')
    with pytest.raises(ValueError, match='flags'):
        FOL.FoliationRegistry.load(bv.ctx, tmp_path / 'plain.npz', FOL.fol_params(cplx=True))
    buf = prog[0].new_zeros(2 * 256, dtype=prog[2].dtype)     # room for one row's field
    with pytest.raises(RuntimeError, match='pdeval error 1.*d_n_finite'):       # (PdevalError)
        bv.ctx.gradient_fields(prog[0].data_ptr(), prog[1], prog[2].data_ptr(), prog[3], 0, 1, buf.data_ptr(), 0,
                               _params(16, CPLX))

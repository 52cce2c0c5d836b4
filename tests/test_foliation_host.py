"""The Jacobian match kernel's per-point code on the CPU (tests/hostsim/sim_foliation.cpp: the
point test and the leader round of pdeval_foliation.h built by g++ for one lane) on gradient
fields from the oracle's jets, against a plain numpy restatement (tests/foliation_ref.py) and
SymPy's exact Jacobian.  The GPU tests (test_gpu_foliation.py) check the gfx950 build itself."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import sympy as sp

import foliation_ref as R
from pdeval import opcodes as OPC
from pdeval import problem_defs as P

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SO = os.path.join(HERE, 'hostsim', '_build', 'libsim_foliation.so')
SRC = [os.path.join(ROOT, 'pde-engine_amd', 'csrc', f) for f in
       ('pdeval_foliation.h', 'pdeval_kernels.h', 'jet.h', 'dd.h')] + \
      [os.path.join(HERE, 'hostsim', 'sim_foliation.cpp')]
M = 12

BASE = 'rho**2*z'
PARA = 'sqrt(rho**2 + z**2) - z'
MUST_MATCH = [(BASE, f'exp({BASE})'), (BASE, f'square({BASE})'), (BASE, f'inv({BASE})'), (BASE, f'sqrt({BASE})'),
              (PARA, f'exp_neg({PARA})'), ('rho/z', 'rho/Abs(z)')]


@pytest.fixture(scope='module')
def sim():
    if not os.path.exists(SO) or any(os.path.getmtime(s) > os.path.getmtime(SO) for s in SRC):
        os.makedirs(os.path.dirname(SO), exist_ok=True)
        subprocess.check_call(['g++', '-O2', '-std=c++17', '-shared', '-fPIC', '-DPD_HOST_SIM',
                               '-I' + os.path.join(HERE, 'hostsim'), '-o', SO,
                               os.path.join(HERE, 'hostsim', 'sim_foliation.cpp')])
    lib = C.CDLL(SO)
    vp, dbl = C.c_void_p, C.c_double
    lib.sim_fol_match.argtypes = [vp, vp, C.c_int, dbl, C.c_int, vp, vp, vp]
    lib.sim_fol_classes.argtypes = [vp, C.c_int, C.c_int, dbl, C.c_int, vp, vp]
    return lib


def _words(pd_, s):
    return np.array(pd_.compile(pd_.parse(s)), dtype=np.int32)


def _complex_program():
    """A constant-free complex program: the imaginary unit alone."""
    return np.array([OPC.PDOP['HEADER'] | (1 << 8) | OPC.FLAG_COMPLEX, OPC.PDOP['PUSH_I']], dtype=np.int32)


@pytest.fixture(scope='module')
def case():
    """The 7 paper solutions, then the re-parametrisations, rho/z, rho/Abs(z) and a complex
    program: their oracle fields and the numpy restatement's leaders."""
    pd_ = P.force_free()
    exprs = list(pd_.known_solutions)
    for a, b in MUST_MATCH:
        for s in (a, b):
            if s not in exprs:
                exprs.append(s)
    progs = [_words(pd_, s) for s in exprs] + [_complex_program()]
    fields = np.stack([R.oracle_field(w, M) for w in progs])
    leader, q, matched = R.sequential_leaders(fields)
    return dict(pd=pd_, exprs=exprs, progs=progs, fields=fields, leader=leader, q=q, matched=matched)


def test_point_test_matches_numpy(sim, case):
    """sim_fol_match (the kernel's point test and counts) on every ordered pair of the case's
    fields: verdict, n_used and n_bad equal to the numpy restatement, qmax bit for bit."""
    f = np.ascontiguousarray(case['fields'])
    n, mm = len(f), M * M
    for i in range(n):
        nu_r, nb_r, q_r = R.pair_stats(f[i], f)
        for k in range(n):
            nu, nb, q = C.c_int(0), C.c_int(0), C.c_double(0)
            hit = sim.sim_fol_match(f[i].ctypes.data, f[k].ctypes.data, mm, R.TAU, R.MIN_POINTS, C.byref(nu),
                                    C.byref(nb), C.byref(q))
            assert (nu.value, nb.value) == (nu_r[k], nb_r[k]), (i, k)
            assert q.value == q_r[k], (i, k, q.value, q_r[k])
            assert bool(hit) == bool(nu_r[k] >= R.MIN_POINTS and nb_r[k] == 0)


def test_expected_classes(sim, case):
    """The restatement's verdicts on the cases the classes are for: f(u) joins u, the 7 paper
    solutions are 7 leaders, rho/Abs(z) matches rho/z where both are real, a complex program is
    unclassified; matched and unmatched pairs are decades apart."""
    ex, lead = case['exprs'], case['leader']
    ix = ex.index
    assert [int(lead[k]) for k in range(7)] == list(range(7))
    for a, b in MUST_MATCH:
        assert lead[ix(a)] == lead[ix(b)] >= 0, (a, b)
        assert R.matches(case['fields'][ix(b)], case['fields'][[ix(a)]])[0], (a, b)
    assert lead[ix(BASE)] == 1 and lead[ix(PARA)] == 4
    assert lead[ix('rho/z')] == 2          # the Radial solution is a function of z/rho
    assert lead[-1] == -1                  # the complex program
    assert len(set(lead[lead >= 0].tolist())) == 7
    q, m = case['q'], case['matched']
    assert q[m].max() < 1e-12 and q[~m].min() > 1e-3, (q[m].max(), q[~m].min())


def test_leader_rounds_match_sequential_definition(sim, case):
    """sim_fol_classes -- rounds of up to 32 probes with the host-compiled round rule and point
    test -- gives the restatement's sequential leaders on the case's fields; so do 80 rows (more
    than two rounds of 32 probes) in a shuffled order."""
    f = np.ascontiguousarray(case['fields'])
    lead = np.zeros(len(f), dtype=np.int64)
    rounds = C.c_int(0)
    ncls = sim.sim_fol_classes(f.ctypes.data, len(f), M * M, R.TAU, R.MIN_POINTS, lead.ctypes.data, C.byref(rounds))
    assert np.array_equal(lead, case['leader']) and ncls == 7 and rounds.value == 1
    # many classes: scaled mixtures a*u_i + b*u_j of two paper solutions are distinct foliations
    rng = np.random.default_rng(3)
    base = case['fields'][:7]
    rows = []
    for _ in range(40):
        i, j = rng.choice(7, 2, replace=False)
        a, b = rng.uniform(0.5, 2.0, 2)
        mix = a * base[i] + b * base[j]
        rows += [mix, 3.0 * mix]      # and a re-scaling of each
    big = np.ascontiguousarray(np.stack(rows)[rng.permutation(80)])
    want, _, _ = R.sequential_leaders(big)
    lead = np.zeros(80, dtype=np.int64)
    ncls = sim.sim_fol_classes(big.ctypes.data, 80, M * M, R.TAU, R.MIN_POINTS, lead.ctypes.data, C.byref(rounds))
    assert np.array_equal(lead, want) and ncls == len(set(want.tolist())) > 32 and rounds.value >= 2


def test_exact_jacobian_agrees(case):
    """SymPy's simplify(u_rho v_z - u_z v_rho) == 0 agrees with the verdict on the pairs that must
    match and on every pair of paper solutions."""
    pd_, ex, f = case['pd'], case['exprs'], case['fields']
    rho, z = pd_.x, pd_.y
    pairs = [(ex.index(a), ex.index(b)) for a, b in MUST_MATCH] + [(i, j) for i in range(7) for j in range(i)]
    for i, j in pairs:
        u, v = pd_.parse(ex[i]), pd_.parse(ex[j])
        jac = sp.diff(u, rho) * sp.diff(v, z) - sp.diff(u, z) * sp.diff(v, rho)
        if jac.has(sp.Abs, sp.sign):
            # (simplify does not combine sign(z)/z with 1/Abs(z): decide each half plane exactly)
            zp = sp.Symbol('zp', positive=True)
            exact = all(sp.simplify(jac.subs(z, sg * zp)) == 0 for sg in (1, -1))
        else:
            exact = sp.simplify(jac) == 0
        assert exact == bool(R.matches(f[j], f[[i]])[0]), (ex[i], ex[j])

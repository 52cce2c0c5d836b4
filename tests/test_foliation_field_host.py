"""The gradient field kernel's per-point code on the CPU (tests/hostsim/sim_foliation_field.cpp:
the program guard, the sample points, the order-1 interpretation and the finite rule of
pdeval_foliation.h built by g++ for one lane) against the oracle's fields
(tests/foliation_ref.py::oracle_field) on the field set F (tests/foliation_cases.py) at
m = 5, 9, 12.  The GPU tests (test_gpu_foliation_classes.py) check the gfx950 build itself.

The bound 5e-10 on the relative field error rests on the oracle being well inside it:
test_oracle_against_exact_gradient compares the oracle's (u_rho, u_z) with SymPy's exact diff
evaluated at 50 digits and requires 5e-12.  No expression of F had to be dropped for it: the
largest oracle error measured on F is 5.0e-15 (printed by the test)."""
import ctypes as C
import os
import subprocess

import mpmath
import numpy as np
import pytest
import sympy as sp

import foliation_cases as FC
import foliation_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SIM = os.path.join(HERE, 'hostsim')
SO = os.path.join(SIM, '_build', 'libsim_foliation_field.so')
GUARD = os.path.join(SIM, '_build', 'guard_foliation_field')
SRC = [os.path.join(ROOT, 'pde-engine_amd', 'csrc', f) for f in
       ('pdeval_foliation.h', 'pdeval_kernels.h', 'jet.h', 'dd.h')] + \
      [os.path.join(ROOT, 'include', 'pdeval.h'), os.path.join(SIM, 'sim_foliation_field.cpp')]
GRID = np.array(R.FF_GRID, dtype=np.float64)


def _stale(out, srcs):
    return not os.path.exists(out) or any(os.path.getmtime(s) > os.path.getmtime(out) for s in srcs)


@pytest.fixture(scope='module')
def sim():
    if _stale(SO, SRC):
        os.makedirs(os.path.dirname(SO), exist_ok=True)
        subprocess.check_call(['g++', '-O2', '-std=c++17', '-shared', '-fPIC', '-DPD_HOST_SIM', '-I' + SIM, '-o', SO,
                               os.path.join(SIM, 'sim_foliation_field.cpp')])
    lib = C.CDLL(SO)
    vp, i64 = C.c_void_p, C.c_int64
    lib.sim_fol_fields.argtypes = [vp, i64, vp, i64, vp, i64, vp, C.c_int, vp, vp]
    lib.sim_fol_point.argtypes = [vp, C.c_int, C.c_int, vp]
    return lib


def _fields(sim, ops, off, m, lst=None, n=None):
    ops = np.ascontiguousarray(ops, dtype=np.int32)
    off = np.ascontiguousarray(off, dtype=np.int64)
    n = len(off) - 1 if n is None else n
    lst = None if lst is None else np.ascontiguousarray(lst, dtype=np.int64)
    rows = n if lst is None else len(lst)
    field = np.zeros((rows, 2, m * m))
    nfin = np.full(rows, -7, dtype=np.int32)
    declined = sim.sim_fol_fields(ops.ctypes.data, ops.size, off.ctypes.data, n, None if lst is None else lst.ctypes.data,
                                  rows, GRID.ctypes.data, m, field.ctypes.data, nfin.ctypes.data)
    return field, nfin, declined


def test_sample_points_are_the_restatements(sim):
    """fol_point_xy gives grid_points' doubles bit for bit (the oracle and the kernel evaluate at
    the same points)."""
    for m in FC.MS + (16,):
        xs, ys = R.grid_points(m)
        xy = np.zeros(2)
        for p in range(m * m):
            sim.sim_fol_point(GRID.ctypes.data, m, p, xy.ctypes.data)
            assert (xy[0], xy[1]) == (xs[p // m], ys[p % m]), (m, p)


def test_oracle_against_exact_gradient():
    """The reference's own error on F: the oracle's (u_rho, u_z) against SymPy's exact diff at 50
    digits, at every point where the oracle's field is finite: <= 5e-12 |g|."""
    F = FC.field_set()
    pd_ = F['pd']
    mpmath.mp.dps = 50
    worst = 0.0
    for k, s in enumerate(F['exprs']):
        if s is None:
            continue
        u = pd_.parse(s)
        g = sp.lambdify((pd_.x, pd_.y), [sp.diff(u, pd_.x), sp.diff(u, pd_.y)], modules='mpmath', cse=True)
        for m in FC.MS:
            xs, ys = R.grid_points(m)
            f = F['fields'][m][k]
            for p in np.flatnonzero(np.isfinite(f[0])):
                ex = g(mpmath.mpf(float(xs[p // m])), mpmath.mpf(float(ys[p % m])))
                assert all(mpmath.im(v) == 0 for v in ex), (s, m, p)
                err = mpmath.sqrt((mpmath.mpf(float(f[0][p])) - ex[0]) ** 2 + (mpmath.mpf(float(f[1][p])) - ex[1]) ** 2)
                nrm = mpmath.sqrt(ex[0] ** 2 + ex[1] ** 2)
                rel = float(err / nrm) if nrm != 0 else float(err)
                worst = max(worst, rel)
                assert rel <= FC.ORACLE_TOL, (s[:60], m, int(p), rel)
    print(f'oracle against the exact gradient: worst relative error {worst:.3e} (bound {FC.ORACLE_TOL:g})')


def test_fields_match_oracle(sim):
    """F at m = 5, 9, 12, in list order and through a permuted list: NaN mask, 5e-10 and n_finite
    (foliation_cases.check_fields); the complex program is declined and all NaN."""
    F = FC.field_set()
    n = len(F['progs'])
    perm = np.random.default_rng(11).permutation(n)
    for m in FC.MS:
        got, nfin, declined = _fields(sim, F['ops'], F['off'], m)
        assert declined == 1 and np.isnan(got[-1]).all() and nfin[-1] == 0
        FC.check_fields(got, nfin, F['fields'][m], f'host m={m}')
        got, nfin, _ = _fields(sim, F['ops'], F['off'], m, lst=perm)
        FC.check_fields(got, nfin, F['fields'][m][perm], f'host m={m} permuted list')
    assert np.isfinite(F['fields'][12][:-1, 0, :]).sum(axis=1).min() >= R.MIN_POINTS   # every real row is usable


def test_guard_rows_are_nan(sim):
    """Offsets outside [0, n_words] and list entries outside [0, n) give all-NaN rows with
    n_finite 0, next to good rows that are untouched by them."""
    F = FC.field_set()
    m = 9
    ops = F['ops'][:int(F['off'][3])]                       # the words of programs 0..2 only
    # candidates 0..2 good; 3 = [n_words, n_words + 5): end past n_words; 4 = [n_words + 5, 2) and
    # 5 = [2, -4): end before begin; 6 = [-4, 7): negative begin; 7 = [7, 7): empty
    off = np.array([0, F['off'][1], F['off'][2], F['off'][3], F['off'][3] + 5, 2, -4, 7, 7], dtype=np.int64)
    n = len(off) - 1
    got, nfin, declined = _fields(sim, ops, off, m)
    want = F['fields'][m]
    FC.check_fields(got[:3], nfin[:3], want[:3], 'host guard, good rows')
    assert declined == 5 and np.isnan(got[3:]).all() and not nfin[3:].any()
    lst = np.array([1, -1, n, 2, 1 << 40, 0], dtype=np.int64)
    got, nfin, declined = _fields(sim, ops, off, m, lst=lst)
    FC.check_fields(got[[0, 3, 5]], nfin[[0, 3, 5]], want[[1, 2, 0]], 'host guard, list')
    assert declined == 3 and np.isnan(got[[1, 2, 4]]).all() and not nfin[[1, 2, 4]].any()


def test_guard_reads_nothing_under_sanitizers():
    """The same code in a stand-alone program (tests/hostsim/guard_foliation_field.cpp, its own
    main) built with -fsanitize=address,undefined on exact-size heap blocks: bad offsets and bad
    list entries give NaN rows and no read outside the arrays."""
    src = os.path.join(SIM, 'guard_foliation_field.cpp')
    if _stale(GUARD, SRC + [src]):
        os.makedirs(os.path.dirname(GUARD), exist_ok=True)
        subprocess.check_call(['g++', '-O1', '-g', '-std=c++17', '-DPD_HOST_SIM', '-fsanitize=address,undefined',
                               '-fno-sanitize-recover=all', '-I' + SIM, '-o', GUARD, src])
    r = subprocess.run([GUARD], capture_output=True, text=True)
    assert r.returncode == 0 and 'guard: 0 failures' in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])

"""The foliation class registry on the CPU (tests/hostsim/sim_foliation_registry.cpp: the pair
scan of fol_assign_kernel on the chunk-major store, the rounds of Stage B and the product's host
bookkeeping pdeval_fol_book.h, built by g++ for one lane) on the oracle fields of
foliation_cases.case_exprs at m = 5 and m = 12: a list assigned in any consecutive batches gets the
class ids of the numpy restatement of the sequential rule (tests/foliation_ref.py).  The GPU tests
(test_gpu_foliation_registry.py) check the gfx950 build itself."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import foliation_cases as FC
import foliation_ref as R
from pdeval.foliation import classes_from_leader

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SIM = os.path.join(HERE, 'hostsim')
SO = os.path.join(SIM, '_build', 'libsim_foliation_registry.so')
GUARD = os.path.join(SIM, '_build', 'guard_fol_registry')
SRC = [os.path.join(ROOT, 'pde-engine_amd', 'csrc', f) for f in
       ('pdeval_foliation.h', 'pdeval_fol_book.h', 'pdeval_kernels.h', 'jet.h', 'dd.h')] + \
      [os.path.join(ROOT, 'include', 'pdeval.h'), os.path.join(SIM, 'sim_foliation_registry.cpp')]
MS = (5, 12)     # m^2 = 25 (one partial chunk), 144 (two full chunks and a partial one)


def _stale(out, srcs):
    return not os.path.exists(out) or any(os.path.getmtime(s) > os.path.getmtime(out) for s in srcs)


@pytest.fixture(scope='module')
def sim():
    if _stale(SO, SRC):
        os.makedirs(os.path.dirname(SO), exist_ok=True)
        subprocess.check_call(['g++', '-O2', '-std=c++17', '-shared', '-fPIC', '-DPD_HOST_SIM', '-I' + SIM, '-o', SO,
                               os.path.join(SIM, 'sim_foliation_registry.cpp')])
    lib = C.CDLL(SO)
    vp, i64 = C.c_void_p, C.c_int64
    lib.sim_reg_create.argtypes = [C.c_int, C.c_double, C.c_int, i64]
    lib.sim_reg_create.restype = vp
    lib.sim_reg_destroy.argtypes = [vp]
    lib.sim_reg_first.argtypes = [vp, vp, i64, vp]
    lib.sim_reg_assign.argtypes = [vp, vp, i64, vp, vp, vp]
    lib.sim_reg_assign.restype = i64
    lib.sim_reg_size.argtypes = [vp, vp, vp]
    lib.sim_reg_leaders.argtypes = [vp, vp, vp, vp]
    lib.sim_reg_load.argtypes = [vp, vp, vp, vp, i64]
    return lib


@pytest.fixture(scope='module')
def cases():
    """{m: (oracle fields of case_exprs, the restatement's class ids)}; never modified."""
    F = FC.field_set()
    n = len(FC.case_exprs(F['pd']))
    out = {}
    for m in MS:
        f = np.ascontiguousarray(F['fields'][m][:n])
        want = classes_from_leader(R.sequential_leaders(f)[0]).class_id
        f.setflags(write=False)
        out[m] = (f, want)
    return out


def _stream(sim, fields, cuts, m, keys=None):
    """Class ids of `fields` assigned in the consecutive batches the cut positions delimit, and
    the registry's (n_classes, rows_seen, keys, sizes, leader fields)."""
    reg = sim.sim_reg_create(m * m, R.TAU, R.MIN_POINTS, 1)
    try:
        ids = np.full(len(fields), -7, dtype=np.int64)
        edges = [0] + list(cuts) + [len(fields)]
        for a, b in zip(edges[:-1], edges[1:]):
            part = np.ascontiguousarray(fields[a:b])
            out = np.full(b - a, -7, dtype=np.int64)
            k = None if keys is None else np.ascontiguousarray(keys[a:b])
            got = sim.sim_reg_assign(reg, part.ctypes.data, b - a, None if k is None else k.ctypes.data, None,
                                     out.ctypes.data)
            assert got >= 0
            ids[a:b] = out
        L, seen = C.c_int64(0), C.c_int64(0)
        sim.sim_reg_size(reg, C.byref(L), C.byref(seen))
        lk, ls = np.zeros(L.value, dtype=np.int64), np.zeros(L.value, dtype=np.int64)
        lf = np.zeros((L.value, 2, m * m))
        sim.sim_reg_leaders(reg, lf.ctypes.data, lk.ctypes.data, ls.ctypes.data)
        return ids, (L.value, seen.value, lk, ls, lf)
    finally:
        sim.sim_reg_destroy(reg)


@pytest.mark.parametrize('m', MS)
def test_any_split_gives_the_sequential_classes(sim, cases, m):
    """One cut at k = 0, 1, 7, len - 1, len, and single rows: the class ids equal the restatement's
    on the whole list; leaders, sizes and keys are the restatement's too."""
    f, want = cases[m]
    n = len(f)
    assert want.max() == 6                               # the 7 paper classes (at m = 5 one row is unclassified)
    for cuts in ([0], [1], [7], [n - 1], [n], list(range(1, n))):
        ids, (L, seen, lk, ls, lf) = _stream(sim, f, cuts, m)
        assert np.array_equal(ids, want), (m, cuts, ids, want)
        assert L == 7 and seen == n
        first_row = np.array([int(np.flatnonzero(want == c)[0]) for c in range(L)])
        assert np.array_equal(lk, first_row), (cuts, lk)          # default keys: the running row number
        assert np.array_equal(ls, np.bincount(want[want >= 0], minlength=L))
        assert np.array_equal(lf, f[first_row])                   # the leaders' fields, bit for bit


def test_unclassified_rows_and_keys(sim, cases):
    """An all-NaN row gets -1, leads nothing and still counts as a row seen; caller keys are kept
    for the leaders."""
    f, want = cases[12]
    nan_row = np.full((1,) + f.shape[1:], np.nan)
    rows = np.concatenate([f[:3], nan_row, f[3:]])
    keys = 500 + 3 * np.arange(len(rows), dtype=np.int64)
    ids, (L, seen, lk, ls, _) = _stream(sim, rows, [2, 4, 9], 12, keys)
    assert ids[3] == -1 and np.array_equal(np.delete(ids, 3), want)
    assert L == 7 and seen == len(rows) and ls.sum() == len(rows) - 1
    lead_rows = [int(np.flatnonzero(ids == c)[0]) for c in range(L)]
    assert np.array_equal(lk, keys[lead_rows])


def test_stage_a_is_first_match(sim, cases):
    """sim_reg_first against foliation_ref.matches leader by leader, with a duplicated leader: the
    smaller index wins."""
    f, _ = cases[12]
    m = 12
    leaders = np.ascontiguousarray(np.concatenate([f[1:7], f[2:3]]))     # leader 6 repeats leader 1
    reg = sim.sim_reg_create(m * m, R.TAU, R.MIN_POINTS, 0)
    try:
        keys = np.arange(len(leaders), dtype=np.int64)
        assert sim.sim_reg_load(reg, leaders.ctypes.data, keys.ctypes.data, np.ones_like(keys).ctypes.data,
                                len(leaders)) == 0
        first = np.full(len(f), -7, dtype=np.int64)
        sim.sim_reg_first(reg, np.ascontiguousarray(f).ctypes.data, len(f), first.ctypes.data)
        for i in range(len(f)):
            hit = R.matches(f[i], leaders)
            assert first[i] == (int(np.argmax(hit)) if hit.any() else -1), i
        assert first[2] == 1 and (first == 6).sum() == 0
    finally:
        sim.sim_reg_destroy(reg)


def test_bookkeeping_under_sanitizers():
    """The bookkeeping and the store layout in a stand-alone program
    (tests/hostsim/guard_fol_registry.cpp, its own main) built with -fsanitize=address,undefined
    on exact-size heap blocks and run directly: growth from capacity 1 through 70 leaders, load
    into an empty and a non-empty registry, keys absent and present, a Stage A result outside
    [0, L) rejected and not followed."""
    src = os.path.join(SIM, 'guard_fol_registry.cpp')
    if _stale(GUARD, SRC + [src]):
        os.makedirs(os.path.dirname(GUARD), exist_ok=True)
        subprocess.check_call(['g++', '-O1', '-g', '-std=c++17', '-DPD_HOST_SIM', '-fsanitize=address,undefined',
                               '-fno-sanitize-recover=all', '-I' + SIM, '-o', GUARD, src])
    r = subprocess.run([GUARD], capture_output=True, text=True)
    assert r.returncode == 0 and 'guard: 0 failures' in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])

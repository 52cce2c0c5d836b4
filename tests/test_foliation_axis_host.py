"""The axis rule of the foliation classes (PDEVAL_FOL_AXIS; DESIGN.md §14 "The axis rule") on the
CPU: the per-point code of pdeval_foliation.h built by g++ for one lane
(tests/hostsim/sim_foliation_axis.cpp) on the oracle's gradient fields, against the numpy
restatement tests/foliation_axis_ref.py.  With the flag clear everything equals
tests/foliation_ref.py.  The GPU tests (test_gpu_foliation_axis.py) check the gfx950 build."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import foliation_axis_ref as A
import foliation_ref as R
from pdeval import problem_defs as P

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SIM = os.path.join(HERE, 'hostsim')
SO = os.path.join(SIM, '_build', 'libsim_foliation_axis.so')
SRC = [os.path.join(ROOT, 'pde-engine_amd', 'csrc', f) for f in
       ('pdeval_foliation.h', 'pdeval_fol_book.h', 'pdeval_kernels.h', 'jet.h', 'dd.h')] + \
      [os.path.join(ROOT, 'include', 'pdeval.h'), os.path.join(SIM, 'sim_foliation_axis.cpp')]
MS = (5, 9, 12)      # m^2 = 25 (one partial chunk), 81 (full + partial), 144 (two full + partial)
AXIS = 1             # PDEVAL_FOL_AXIS


@pytest.fixture(scope='module')
def sim():
    if not os.path.exists(SO) or any(os.path.getmtime(s) > os.path.getmtime(SO) for s in SRC):
        os.makedirs(os.path.dirname(SO), exist_ok=True)
        subprocess.check_call(['g++', '-O2', '-std=c++17', '-shared', '-fPIC', '-DPD_HOST_SIM', '-I' + SIM, '-o', SO,
                               os.path.join(SIM, 'sim_foliation_axis.cpp')])
    lib = C.CDLL(SO)
    vp, dbl, i64 = C.c_void_p, C.c_double, C.c_int64
    lib.sim_axis_match.argtypes = [vp, vp, C.c_int, dbl, C.c_int, C.c_int, vp, vp, vp]
    lib.sim_axis_classes.argtypes = [vp, C.c_int, C.c_int, dbl, C.c_int, C.c_int, vp, vp]
    lib.sim_axis_stream.argtypes = [vp, i64, C.c_int, dbl, C.c_int, C.c_int, vp, C.c_int, vp, vp]
    lib.sim_axis_stream.restype = i64
    lib.sim_axis_kinds.argtypes = [vp, i64, C.c_int, C.c_int, vp]
    return lib


@pytest.fixture(scope='module')
def fields():
    """{m: oracle fields of foliation_axis_ref.EXPRS}, chosen by check: every pair of
    one-coordinate rows expected to match reaches n_used >= min_points under the rule in the
    restatement, at every m.  Never modified."""
    pd_ = P.force_free()
    ops, off, _ = P.compile_strings(pd_, A.EXPRS)
    out = {}
    for m in MS:
        f = np.ascontiguousarray(R.oracle_fields(ops, off, m))
        for group in A.CLASSES_AXIS[:2]:
            for i in group:
                nu, nb, _ = A.pair_stats(f[i], f[sorted(group)], axis=True)
                assert (nu >= R.MIN_POINTS).all() and (nb == 0).all(), (m, A.EXPRS[i], nu, nb)
        f.setflags(write=False)
        out[m] = f
    return out


def _sim_pair(sim, row, probe, mm, flags):
    nu, nb, q = C.c_int(0), C.c_int(0), C.c_double(0)
    hit = sim.sim_axis_match(row.ctypes.data, probe.ctypes.data, mm, R.TAU, R.MIN_POINTS, flags, C.byref(nu),
                             C.byref(nb), C.byref(q))
    return bool(hit), nu.value, nb.value, q.value


@pytest.mark.parametrize('m', MS)
def test_point_rule_matches_numpy(sim, fields, m):
    """Every ordered pair of the fields: used and bad counts, the verdict and qmax (bit for bit)
    equal the restatement's with the flag set and clear; with it clear they equal
    foliation_ref.pair_stats; the verdict and the counts are symmetric under the exchange of row
    and probe (J is antisymmetric bit for bit, the rule symmetric)."""
    f, mm = fields[m], m * m
    n = len(f)
    for flags in (0, AXIS):
        got = {}
        for i in range(n):
            nu_r, nb_r, q_r = A.pair_stats(f[i], f, axis=bool(flags))
            if not flags:
                nu_0, nb_0, q_0 = R.pair_stats(f[i], f)
                assert np.array_equal(nu_r, nu_0) and np.array_equal(nb_r, nb_0) and np.array_equal(q_r, q_0)
            for k in range(n):
                hit, nu, nb, q = _sim_pair(sim, f[i], f[k], mm, flags)
                assert (nu, nb) == (nu_r[k], nb_r[k]), (flags, i, k)
                assert q == q_r[k] and np.isfinite(q), (flags, i, k, q, q_r[k])
                assert hit == bool(nu_r[k] >= R.MIN_POINTS and nb_r[k] == 0)
                got[i, k] = (hit, nu, nb, q)
        for i in range(n):
            for k in range(i):
                assert got[i, k] == got[k, i], (flags, i, k)
    # the rule itself: rho**2 matches itself and rho**4 with it, and nothing without it
    i2, i4 = A.EXPRS.index('rho**2'), A.EXPRS.index('rho**4')
    assert _sim_pair(sim, f[i2], f[i2], mm, AXIS)[:3] == (True, mm, 0)
    assert _sim_pair(sim, f[i2], f[i4], mm, AXIS)[:3] == (True, mm, 0)
    assert _sim_pair(sim, f[i2], f[i2], mm, 0)[:3] == (False, 0, 0)


def test_rule_is_on_the_operands():
    """Hand-made points: an underflowed product, a zero gradient and a non-finite operand are not
    usable; the two axis cases are, with q = 0."""
    def one(a, b, c, d):
        row, probe = np.array([[a], [b]], dtype=np.float64), np.array([[[c], [d]]], dtype=np.float64)
        nu, nb, q = A.pair_stats(row, probe, axis=True)
        return int(nu[0]), int(nb[0]), float(q[0])
    assert one(2.0, 0.0, 3.0, 0.0) == (1, 0, 0.0)            # both along rho
    assert one(0.0, -2.0, 0.0, 3.0) == (1, 0, 0.0)           # both along z
    assert one(1e-200, 0.0, 3.0, 1e-200) == (0, 0, 0.0)      # a d underflows to 0: S == 0, d != 0
    assert one(0.0, 0.0, 3.0, 0.0) == (0, 0, 0.0)            # a zero gradient
    assert one(np.inf, 0.0, 3.0, 0.0) == (0, 0, 0.0)         # a is not finite
    assert one(2.0, 0.0, 0.0, 3.0) == (1, 1, 1.0)            # rho-only against z-only: bad as before


def test_rule_is_on_the_operands_host_build(sim):
    """The same hand-made points through the host build."""
    def one(a, b, c, d):
        row, probe = np.array([a, b], dtype=np.float64), np.array([c, d], dtype=np.float64)
        nu, nb, q = C.c_int(0), C.c_int(0), C.c_double(0)
        sim.sim_axis_match(row.ctypes.data, probe.ctypes.data, 1, R.TAU, 1, AXIS, C.byref(nu), C.byref(nb), C.byref(q))
        return nu.value, nb.value, q.value
    assert one(2.0, 0.0, 3.0, 0.0) == (1, 0, 0.0)
    assert one(0.0, -2.0, 0.0, 3.0) == (1, 0, 0.0)
    assert one(1e-200, 0.0, 3.0, 1e-200) == (0, 0, 0.0)
    assert one(0.0, 0.0, 3.0, 0.0) == (0, 0, 0.0)
    assert one(np.inf, 0.0, 3.0, 0.0) == (0, 0, 0.0)
    assert one(2.0, 0.0, 0.0, 3.0) == (1, 1, 1.0)


@pytest.mark.parametrize('m', MS)
def test_expected_classes(fields, m):
    """The restatement's classes of the list: with the flag the functions of rho alone are one
    class, those of z alone another, rho**2*z with exp(rho**2*z), rho**2 + z**2 alone; without it
    every one-coordinate row is its own leader."""
    f = fields[m]
    lead = A.sequential_leaders(f, axis=True)
    got = {}
    for i, l in enumerate(lead):
        got.setdefault(int(l), set()).add(i)
    assert sorted(got.values(), key=min) == A.CLASSES_AXIS, got
    lead0 = A.sequential_leaders(f, axis=False)
    assert np.array_equal(lead0, R.sequential_leaders(f)[0])
    n1 = len(A.RHO_ONLY) + len(A.Z_ONLY)
    assert lead0[:n1].tolist() == list(range(n1))
    assert lead0[n1:].tolist() == [n1, n1, n1 + 2]


def _longer(f, rng):
    """The 10 fields and 39 scaled copies of them with a NaN row, 50 rows in a shuffled order:
    without the flag the 35 one-coordinate rows are 35 leaders, more than one round of 32 probes."""
    rows = [f[i] for i in range(len(f))]
    rows += [(-2.5 - k) * f[k % len(f)] for k in range(50 - len(rows) - 1)]
    rows.append(np.full_like(f[0], np.nan))
    return np.ascontiguousarray(np.stack(rows)[rng.permutation(len(rows))])


@pytest.mark.parametrize('m', (5, 12))
def test_rounds_and_registry_split_equal_the_sequential_definition(sim, fields, m):
    """With the flag set and clear: the leader rounds of the host build give the restatement's
    sequential leaders, and the registry host build, the list cut at every position, its class
    ids; the leaders' kinds read from the chunk-major store equal the restatement's."""
    mm = m * m
    big = _longer(fields[m], np.random.default_rng(11))
    n = len(big)
    for flags in (0, AXIS):
        want = A.sequential_leaders(big, axis=bool(flags))
        ids_want = A.class_ids(want)
        n_cls = int(ids_want.max()) + 1
        assert n_cls == (4 if flags else 37) and (want == -1).sum() == 1
        lead = np.zeros(n, dtype=np.int64)
        rounds = C.c_int(0)
        ncls = sim.sim_axis_classes(big.ctypes.data, n, mm, R.TAU, R.MIN_POINTS, flags, lead.ctypes.data,
                                    C.byref(rounds))
        assert np.array_equal(lead, want) and ncls == n_cls
        assert rounds.value == 2 if not flags else rounds.value in (1, 2)
        lead_rows = np.array([int(np.flatnonzero(ids_want == c)[0]) for c in range(n_cls)])
        kinds_want = A.kinds(big[lead_rows])
        for cut in range(n + 1):
            ids = np.full(n, -7, dtype=np.int64)
            kinds = np.full(n, 9, dtype=np.uint8)
            cuts = np.array([cut], dtype=np.int64)
            L = sim.sim_axis_stream(big.ctypes.data, n, mm, R.TAU, R.MIN_POINTS, flags, cuts.ctypes.data, 1,
                                    ids.ctypes.data, kinds.ctypes.data)
            assert L == n_cls and np.array_equal(ids, ids_want), (flags, cut, ids, ids_want)
            assert np.array_equal(kinds[:L], kinds_want), (flags, cut)
        if flags:
            assert sorted(kinds_want.tolist()) == [0, 0, 1, 2]


@pytest.mark.parametrize('m', MS)
def test_kinds(sim, fields, m):
    """kind of every field, of a row with fewer finite points than min_points, of an all-NaN row,
    of a rho-only row with one non-zero u_z and of a zero field: the host build equals numpy."""
    f, mm = fields[m], m * m
    few = np.full_like(f[1], np.nan)
    few[:, :R.MIN_POINTS - 1] = f[1][:, :R.MIN_POINTS - 1]          # rho**2 at 15 points
    exact = np.full_like(f[1], np.nan)
    exact[:, 3:3 + R.MIN_POINTS] = f[5][:, 3:3 + R.MIN_POINTS]      # z**2 at exactly 16 points
    spoiled = f[1].copy()
    spoiled[1, mm - 1] = 1e-300                                     # one point with u_z != 0
    half = f[1].copy()
    half[1, ::2] = np.nan                                           # u_z NaN: those points are not finite
    rows = np.ascontiguousarray(np.concatenate(
        [f, few[None], exact[None], spoiled[None], half[None], np.full((1,) + f.shape[1:], np.nan),
         np.zeros((1,) + f.shape[1:])]))
    want = A.kinds(rows)
    n0 = len(f)
    assert want[:n0].tolist() == [1] * len(A.RHO_ONLY) + [2] * len(A.Z_ONLY) + [0] * len(A.GENERIC)
    assert want[n0:].tolist() == [0, 2, 0, 1 if mm // 2 >= R.MIN_POINTS else 0, 0, 0]
    got = np.full(len(rows), 9, dtype=np.uint8)
    sim.sim_axis_kinds(rows.ctypes.data, len(rows), mm, R.MIN_POINTS, got.ctypes.data)
    assert np.array_equal(got, want), (got, want)

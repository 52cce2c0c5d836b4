"""Links and components of the foliation classes (PDEVAL_FOL_LINK; DESIGN.md §14 "Links and
components") on the CPU: the pair scan of fol_link_kernel, its capped edge buffer and the
product's host bookkeeping pdeval_fol_book.h built by g++ for one lane
(tests/hostsim/sim_foliation_link.cpp) on the oracle's gradient fields, NaN-masked to partial
domains, against the numpy restatement tests/foliation_link_ref.py.  The GPU tests
(test_gpu_foliation_link.py) check the gfx950 build."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import foliation_axis_ref as A
import foliation_link_ref as K
import foliation_ref as R
from pdeval import problem_defs as P

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SIM = os.path.join(HERE, 'hostsim')
SO = os.path.join(SIM, '_build', 'libsim_foliation_link.so')
GUARD = os.path.join(SIM, '_build', 'guard_fol_links')
SRC = [os.path.join(ROOT, 'pde-engine_amd', 'csrc', f) for f in
       ('pdeval_foliation.h', 'pdeval_fol_book.h', 'pdeval_kernels.h', 'jet.h', 'dd.h')] + \
      [os.path.join(ROOT, 'include', 'pdeval.h'), os.path.join(SIM, 'sim_foliation_axis.cpp'),
       os.path.join(SIM, 'sim_foliation_link.cpp')]
MS = (5, 9, 12)      # m^2 = 25 (one partial chunk), 81 (full + partial), 144 (two full + partial)
AXIS, LINK = 1, 2    # PDEVAL_FOL_AXIS, PDEVAL_FOL_LINK


def _min_points(m):
    """16, the default, where a third of the grid holds that many points; 6 at m = 5 (thirds of 8)."""
    return R.MIN_POINTS if m * m // 3 >= R.MIN_POINTS else 6


def _stale(out, srcs):
    return not os.path.exists(out) or any(os.path.getmtime(s) > os.path.getmtime(out) for s in srcs)


@pytest.fixture(scope='module')
def sim():
    if _stale(SO, SRC):
        os.makedirs(os.path.dirname(SO), exist_ok=True)
        subprocess.check_call(['g++', '-O2', '-std=c++17', '-shared', '-fPIC', '-DPD_HOST_SIM', '-I' + SIM, '-o', SO,
                               os.path.join(SIM, 'sim_foliation_link.cpp')])
    lib = C.CDLL(SO)
    vp, i64 = C.c_void_p, C.c_int64
    lib.sim_link_create.argtypes = [C.c_int, C.c_double, C.c_int, C.c_int, i64]
    lib.sim_link_create.restype = vp
    lib.sim_link_destroy.argtypes = [vp]
    lib.sim_link_assign.argtypes = [vp, vp, i64, vp]
    lib.sim_link_assign.restype = i64
    lib.sim_link_fields.argtypes = [vp, vp, vp, i64]
    lib.sim_link_fields.restype = i64
    lib.sim_link_components.argtypes = [vp, vp, vp, vp, vp]
    lib.sim_link_components.restype = i64
    lib.sim_link_links.argtypes = [vp, vp]
    lib.sim_link_launches.argtypes = [vp]
    lib.sim_link_edge_cap.argtypes = [vp]
    lib.sim_link_edge_cap.restype = i64
    lib.sim_link_load_links.argtypes = [vp, vp, i64]
    lib.sim_link_merge.argtypes = [vp, vp, vp]
    lib.sim_link_merge.restype = i64
    return lib


@pytest.fixture(scope='module')
def lists():
    """{m: rows}: the oracle fields of foliation_axis_ref.EXPRS masked to partial domains so that
    leaders of one foliation cannot match each other -- rho**2*z on the left half and
    exp(rho**2*z) on the right half with full-domain rows of both; rho**2 + z**2 on three thirds with
    the two unions that bridge them; rho**2 and rho**4 on disjoint halves with a full rho (one
    class only under the axis rule) -- with the unmasked fields, scaled copies and an all-NaN row,
    in a fixed shuffled order.  Never modified."""
    pd_ = P.force_free()
    ops, off, _ = P.compile_strings(pd_, A.EXPRS)
    ix = {e: i for i, e in enumerate(A.EXPRS)}
    out = {}
    for m in MS:
        mm = m * m
        f = R.oracle_fields(ops, off, m)
        p = np.arange(mm)
        left, right = p < mm // 2, p >= mm // 2
        t1, t2, t3 = p < mm // 3, (p >= mm // 3) & (p < 2 * (mm // 3)), p >= 2 * (mm // 3)
        g, h, s = f[ix['rho**2*z']], f[ix['exp(rho**2*z)']], f[ix['rho**2 + z**2']]
        rows = [K.masked(g, left), K.masked(h, right), g, -3.0 * h,
                K.masked(s, t1), K.masked(s, t2), K.masked(s, t3), K.masked(s, t1 | t2), K.masked(s, t2 | t3),
                K.masked(f[ix['rho**2']], left), K.masked(f[ix['rho**4']], right), f[ix['rho']],
                f[ix['z']], f[ix['z**2']], 2.5 * s, np.full_like(g, np.nan)]
        rows = np.stack(rows)[np.random.default_rng(5 + m).permutation(len(rows))]
        rows = np.ascontiguousarray(rows)
        rows.setflags(write=False)
        out[m] = rows
    return out


class Sim:
    def __init__(self, lib, m, flags, edge_cap=64):
        self.lib, self.mm = lib, m * m
        self.h = lib.sim_link_create(self.mm, R.TAU, _min_points(m), flags, edge_cap)

    def close(self):
        self.lib.sim_link_destroy(self.h)

    def assign(self, rows):
        rows = np.ascontiguousarray(rows)
        ids = np.full(len(rows), -7, dtype=np.int64)
        assert self.lib.sim_link_assign(self.h, rows.ctypes.data, len(rows), ids.ctypes.data) >= 0
        return ids

    def link_fields(self, rows, ids):
        rows, ids = np.ascontiguousarray(rows), np.ascontiguousarray(ids, dtype=np.int64)
        return self.lib.sim_link_fields(self.h, rows.ctypes.data, ids.ctypes.data, len(rows))

    def state(self):
        """(components, sizes, links)"""
        nc, nl = C.c_int64(0), C.c_int64(0)
        L = self.lib.sim_link_components(self.h, None, None, C.byref(nc), C.byref(nl))
        comp, sizes = np.full(L, -7, dtype=np.int64), np.full(L, -7, dtype=np.int64)
        self.lib.sim_link_components(self.h, comp.ctypes.data, sizes.ctypes.data, None, None)
        edges = np.full((nl.value, 2), -7, dtype=np.int64)
        self.lib.sim_link_links(self.h, edges.ctypes.data)
        assert nc.value == len(np.unique(comp))
        return comp, sizes, edges


def _ref(m, flags):
    return K.LinkRef(R.TAU, _min_points(m), axis=bool(flags & AXIS), link=bool(flags & LINK))


def _same(sim_reg, ref):
    comp, sizes, edges = sim_reg.state()
    assert np.array_equal(edges, ref.sorted_links()), (edges.tolist(), ref.sorted_links().tolist())
    assert np.array_equal(comp, ref.components()) and np.array_equal(sizes, ref.sizes)


@pytest.mark.parametrize('m', MS)
def test_the_lists_link_as_intended(lists, m):
    """The restatement on the list: the halves of rho**2*z and the thirds of rho**2 + z**2 are
    separate classes joined into one component each, the links depend on the order of arrival
    until link_fields completes them, and without the flag nothing is linked."""
    rows = lists[m]
    for axis in (False, True):
        ref = K.LinkRef(R.TAU, _min_points(m), axis=axis)
        ids = ref.assign(rows)
        assert (ids == -1).sum() == 1
        ref.link_fields(rows, ids)
        comp = ref.components()
        assert len(ref.links) >= 3 and len(np.unique(comp)) < ref.n_classes
        # every link joins two leaders that share fewer than min_points usable points
        lead = np.stack(ref.leaders)
        for a, b in ref.links:
            nu, _, _ = A.pair_stats(lead[a], lead[b:b + 1], axis=axis)
            assert nu[0] < _min_points(m)
        off = K.LinkRef(R.TAU, _min_points(m), axis=axis, link=False)
        assert np.array_equal(off.assign(rows), ids) and not off.links
        assert np.array_equal(off.components(), np.arange(off.n_classes))


@pytest.mark.parametrize('m', MS)
def test_one_shot_and_link_fields_equal_the_restatement(sim, lists, m):
    """The whole list in one call, then link_fields over it: ids, sizes, the links as a set and
    the components equal the restatement's after each step, with FOL_AXIS on and off; with
    FOL_LINK clear the ids are the same and nothing is linked until link_fields is called."""
    rows = lists[m]
    for flags in (LINK, LINK | AXIS, 0, AXIS):
        reg, ref = Sim(sim, m, flags), _ref(m, flags)
        try:
            ids = reg.assign(rows)
            want = ref.assign(rows)
            assert np.array_equal(ids, want), (flags, ids, want)
            _same(reg, ref)
            if not flags & LINK:
                assert len(reg.state()[2]) == 0
            assert reg.link_fields(rows, ids) == ref.link_fields(rows, want)
            _same(reg, ref)
            assert reg.link_fields(rows, ids) == 0              # nothing new the second time
            bad = ids.copy()
            bad[0] = ref.n_classes
            assert reg.link_fields(rows, bad) == -1              # a class id outside [-1, L)
            _same(reg, ref)
        finally:
            reg.close()


@pytest.mark.parametrize('m', MS)
def test_the_stream_cut_at_every_position_equals_one_shot(sim, lists, m):
    """Split invariance of the arrival rule: the list cut into two batches at every position, and
    into single rows, gives the ids, links and components of the one-shot call."""
    rows = lists[m]
    n = len(rows)
    for flags in (LINK, LINK | AXIS):
        ref = _ref(m, flags)
        want = ref.assign(rows)
        for cuts in [[k] for k in range(n + 1)] + [list(range(1, n))]:
            reg = Sim(sim, m, flags)
            try:
                edges = [0] + cuts + [n]
                ids = np.concatenate([reg.assign(rows[a:b]) for a, b in zip(edges[:-1], edges[1:]) if b > a])
                assert np.array_equal(ids, want), (flags, cuts)
                _same(reg, ref)
            finally:
                reg.close()


def test_a_full_edge_buffer_counts_on_and_the_pass_is_repeated(sim, lists):
    """An edge buffer of one pair: the batch counts past it, the buffer grows to hold the count
    and the second launch gives the restatement's links."""
    m = 12
    rows = lists[m]
    reg, ref = Sim(sim, m, LINK, edge_cap=1), _ref(m, LINK)
    try:
        ids = reg.assign(rows)
        assert np.array_equal(ids, ref.assign(rows))
        assert sim.sim_link_launches(reg.h) == 2 and sim.sim_link_edge_cap(reg.h) >= len(ref.links) > 1
        _same(reg, ref)
    finally:
        reg.close()


@pytest.mark.parametrize('m', (5, 12))
def test_merge_maps_the_links(sim, lists, m):
    """Two linked registries merged: the other's leaders assigned here by the arrival rule, its
    sizes added and its links mapped through the id map, against the restatement's merge; and
    load_links with a bad edge adds nothing."""
    rows = lists[m]
    k = len(rows) // 2
    for flags in (LINK, LINK | AXIS):
        a, b, ra, rb = Sim(sim, m, flags), Sim(sim, m, flags), _ref(m, flags), _ref(m, flags)
        try:
            for reg, ref, part in ((a, ra, rows[:k]), (b, rb, rows[k:])):
                ids = reg.assign(part)
                assert np.array_equal(ids, ref.assign(part))
                assert reg.link_fields(part, ids) == ref.link_fields(part, ids)
            id_map = np.full(rb.n_classes, -7, dtype=np.int64)
            assert sim.sim_link_merge(a.h, b.h, id_map.ctypes.data) == rb.n_classes
            assert np.array_equal(id_map, ra.merge(rb))
            _same(a, ra)
            L = ra.n_classes
            for bad in ([[0, L]], [[-1, 0]], [[1, 1]], [[0, 1], [2, 2]]):
                e = np.array(bad, dtype=np.int64)
                assert sim.sim_link_load_links(a.h, e.ctypes.data, len(e)) == -1
            _same(a, ra)
        finally:
            a.close()
            b.close()


def test_links_bookkeeping_under_sanitizers():
    """The union-find and the link bookkeeping in a stand-alone program
    (tests/hostsim/guard_fol_links.cpp, its own main) built with -fsanitize=address,undefined on
    exact-size heap blocks and run directly: edge validation with out-of-range and self edges,
    growth with the registry, the merge mapping and a failed plan that leaves classes and
    components as they were."""
    src = os.path.join(SIM, 'guard_fol_links.cpp')
    if _stale(GUARD, SRC + [src]):
        os.makedirs(os.path.dirname(GUARD), exist_ok=True)
        subprocess.check_call(['g++', '-O1', '-g', '-std=c++17', '-DPD_HOST_SIM', '-fsanitize=address,undefined',
                               '-fno-sanitize-recover=all', '-I' + SIM, '-o', GUARD, src])
    r = subprocess.run([GUARD], capture_output=True, text=True)
    assert r.returncode == 0 and 'guard: 0 failures' in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])

"""GPU tests of the links and components of the foliation classes (PDEVAL_FOL_LINK; DESIGN.md §14
"Links and components"): fol_link_kernel in its REG / non-REG and AXIS instantiations, the edge
buffer's growth, the entry points and the Python layer.  The inputs are synthetic gradient fields
on the context's sample grid, NaN-masked to partial domains and passed through ``assign_fields``,
so the expected result is exact and comes from the numpy restatement tests/foliation_link_ref.py."""
import os

import numpy as np
import pytest

import foliation_link_ref as K
import foliation_ref as R
from pdeval import foliation as FOL
from pdeval._lib import FOL_AXIS, FOL_LINK, Context, PdevalError, default_fol_params, fol_params
from pdeval.foliation import classes_from_leader

pytestmark = pytest.mark.gpu

T = 32    # kFolAssignTile: the leaders of one LDS tile of fol_link_kernel


@pytest.fixture(scope='module')
def ctx():
    c = Context(0, device=0)
    yield c
    c.close()


def _params(m, flags=FOL_LINK, min_points=None):
    p = default_fol_params()
    p.m = m
    p.flags = flags
    if min_points is not None:
        p.min_points = min_points
    return p


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a, order='C', dtype=np.float64)).to(torch.device('cuda', 0))


def _grid(ctx, m):
    """rho[mm], z[mm] of the m x m sample points of the context's grid, point p = i m + j."""
    with ctx.fol_registry(_params(m)) as reg:
        xs, ys = R.grid_points(m, tuple(reg.grid))
    return np.repeat(xs, m), np.tile(ys, m)


def _quad(ctx, m, k=1.0):
    """The field of u = rho**2 + k z**2: (2 rho, 2 k z); k = 1 is the base field."""
    rho, z = _grid(ctx, m)
    return np.stack([2.0 * rho, 2.0 * k * z])


def _halves(mm):
    p = np.arange(mm)
    return p < mm // 2, p >= mm // 2


def _ref(prm):
    return K.LinkRef(prm.tau, prm.min_points, axis=bool(prm.flags & FOL_AXIS), link=bool(prm.flags & FOL_LINK))


def _same(reg, ref):
    """Sizes, the links as a set and the components equal the restatement's."""
    assert reg.n_classes == ref.n_classes and np.array_equal(reg.sizes, ref.sizes)
    links = reg.links()
    assert links.shape == (reg.n_links, 2)
    assert np.array_equal(links, ref.sorted_links()), (links.tolist(), ref.sorted_links().tolist())
    comp = reg.components()
    assert np.array_equal(comp, ref.components()), (comp, ref.components())
    assert reg.n_components == len(np.unique(comp))


# ---------------------------------------------------------------- the bridge and the chain
@pytest.mark.parametrize('m', (16, 20))
def test_bridge(ctx, m):
    """Row A is finite on the left half of the grid, row B on the right half, row C everywhere:
    classes [0, 1, 0], one link {0, 1}, components [0, 0]; without FOL_LINK no links and
    components [0, 1]."""
    base = _quad(ctx, m)
    left, right = _halves(m * m)
    rows = np.stack([K.masked(base, left), K.masked(base, right), base])
    with ctx.fol_registry(_params(m)) as reg:
        assert reg.assign_fields(_dev(rows)).tolist() == [0, 1, 0]
        assert reg.links().tolist() == [[0, 1]] and reg.n_links == 1
        assert reg.components().tolist() == [0, 0] and reg.n_components == 1
        assert reg.component_sizes() == {0: 3} and reg.sizes.tolist() == [2, 1]
        assert int(reg.params.flags) & FOL_LINK
    with ctx.fol_registry(_params(m, 0)) as reg:
        assert reg.assign_fields(_dev(rows)).tolist() == [0, 1, 0]
        assert reg.links().shape == (0, 2) and reg.n_links == 0
        assert reg.components().tolist() == [0, 1] and reg.n_components == 2
        assert reg.component_sizes() == {0: 2, 1: 1}


def test_chain_and_an_unrelated_field(ctx):
    """Three domains and two bridges give one component; u = rho z stays alone."""
    m = 16
    mm = m * m
    base = _quad(ctx, m)
    rho, z = _grid(ctx, m)
    other = np.stack([z, rho])
    p = np.arange(mm)
    t1, t2, t3 = p < 85, (p >= 85) & (p < 170), p >= 170
    rows = np.stack([K.masked(base, t1), K.masked(base, t2), K.masked(base, t3), other,
                     K.masked(base, t1 | t2), K.masked(base, t2 | t3)])
    prm = _params(m)
    ref = _ref(prm)
    want = ref.assign(rows)
    assert want.tolist() == [0, 1, 2, 3, 0, 1] and sorted(ref.links) == [(0, 1), (1, 2)]
    with ctx.fol_registry(prm) as reg:
        assert np.array_equal(reg.assign_fields(_dev(rows)), want)
        _same(reg, ref)
        assert reg.components().tolist() == [0, 0, 0, 3]
        assert reg.component_sizes() == {0: 5, 3: 1}


# ---------------------------------------------------------------- 70 leaders, REG and non-REG
@pytest.fixture(scope='module')
def seventy(ctx):
    """{m: (70 leader rows, 35 full rows, the restatement after the leaders)}: u = rho**2 + k z**2,
    k = 1 .. 35, on the left half (leaders 0 .. 34) and on the right half (35 .. 69), so that the
    link of foliation k joins a leader of the first LDS tile to one of the second (k <= 28) or of
    the third (35 + k >= 64).  Never modified."""
    out = {}
    for m in (16, 20):
        left, right = _halves(m * m)
        full = np.stack([_quad(ctx, m, 1.0 + k) for k in range(35)])
        lead = np.concatenate([np.stack([K.masked(f, left) for f in full]),
                               np.stack([K.masked(f, right) for f in full])])
        ref = _ref(_params(m))
        assert ref.assign(lead).tolist() == list(range(70)) and not ref.links
        for a in (lead, full):
            a.setflags(write=False)
        out[m] = (lead, full, ref)
    return out


@pytest.mark.parametrize('n_rows', (1, 3, 5, 130))
@pytest.mark.parametrize('m', (16, 20))
def test_seventy_leaders(ctx, seventy, m, n_rows):
    """m = 16 (REG) and m = 20 (rows re-read per surviving pair): 70 resident leaders, then one
    batch of 1, 3, 5 or 130 full-domain rows -- not multiples of the four rows of a block -- whose
    links reach into the second and third tile."""
    lead, full, _ = seventy[m]
    which = (34 - 11 * np.arange(n_rows)) % 35          # foliation 34 first: leaders 34 and 69
    rows = np.stack([(1.0 + 0.5 * i) * full[k] for i, k in enumerate(which)])
    prm = _params(m)
    ref = _ref(prm)
    ref.assign(lead)
    want = ref.assign(rows)
    assert np.array_equal(want, which) and sorted(ref.links) == sorted({(int(k), 35 + int(k)) for k in which})
    with ctx.fol_registry(prm) as reg:
        assert reg.assign_fields(_dev(lead)).tolist() == list(range(70)) and reg.n_links == 0
        assert np.array_equal(reg.assign_fields(_dev(rows)), want)
        _same(reg, ref)
        assert reg.link_fields(_dev(rows), want) == 0      # the leaders all existed: nothing to complete


# ---------------------------------------------------------------- the link scan at the tile edges
def _tile_edge_rows(ctx, m, n_lead):
    """(n_lead resident leaders, a batch of six rows, its ids): the leaders are the left halves of
    the foliations u = rho**2 + k z**2, k = 1 .. n_lead.  The batch: the right halves of two
    further foliations (new leaders n_lead and n_lead + 1), a full-domain row that is foliation 3 on
    the left half and the second new leader's on the right (class 3, link {3, n_lead + 1}), an
    all-NaN row, a multiple of the last resident leader and the first new foliation everywhere.
    By the arrival rule rows 0 .. 2, in one block with the all-NaN row, scan n_lead, n_lead + 1
    and n_lead + 2 leaders."""
    rho, z = _grid(ctx, m)
    left, right = _halves(m * m)
    fol = [np.stack([2.0 * rho, 2.0 * (1.0 + k) * z]) for k in range(n_lead + 2)]
    lead = np.stack([K.masked(f, left) for f in fol[:n_lead]])
    rows = np.stack([K.masked(fol[n_lead], right), K.masked(fol[n_lead + 1], right),
                     np.where(left, fol[3], fol[n_lead + 1]), np.full((2, m * m), np.nan),
                     -0.5 * lead[n_lead - 1], 2.5 * fol[n_lead]])
    return lead, rows, [n_lead, n_lead + 1, 3, -1, n_lead - 1, n_lead]


@pytest.mark.parametrize('n_lead', (T - 2, T, 2 * T - 1))
@pytest.mark.parametrize('m', (16, 20))
def test_link_scan_at_tile_edges(ctx, m, n_lead):
    """The link mode of the scan with T - 2, T and 2 T - 1 resident leaders, m = 16 (REG) and
    m = 20: the scan limits of the rows of one block differ and lie on both sides of a tile's
    end, and the link joins a leader of the first tile to one past it (n_lead >= T).  Then
    link_fields over the same rows with the bridging row's id set to -1 -- on the same registry,
    where nothing is new, and on one without FOL_LINK, where the bridging row is the only source
    of the link.  Ids, links and components are the restatement's; the restatement alone is
    checked first."""
    lead, rows, ids = _tile_edge_rows(ctx, m, n_lead)
    without = np.array(ids)
    without[2] = -1
    for flags in (FOL_LINK, 0):
        prm = _params(m, flags)
        ref = _ref(prm)
        assert ref.assign(lead).tolist() == list(range(n_lead)) and not ref.links
        want = ref.assign(rows)
        assert want.tolist() == ids and ref.links == ({(3, n_lead + 1)} if flags else set())
        assert n_lead < T or (n_lead + 1) // T > 3 // T          # the link crosses a tile's end
        with ctx.fol_registry(prm) as reg:
            assert reg.assign_fields(_dev(lead)).tolist() == list(range(n_lead)) and reg.n_links == 0
            assert np.array_equal(reg.assign_fields(_dev(rows)), want)
            _same(reg, ref)
            n_new = ref.link_fields(rows, without)               # the -1 rows yield nothing
            assert n_new == 0 and len(ref.links) == (1 if flags else 0)
            assert reg.link_fields(_dev(rows), without) == n_new
            _same(reg, ref)
            n_new = ref.link_fields(rows, want)
            assert n_new == (0 if flags else 1) and ref.links == {(3, n_lead + 1)}
            assert reg.link_fields(_dev(rows), want) == n_new
            _same(reg, ref)


# ---------------------------------------------------------------- the arrival rule
def test_arrival_rule_and_link_fields(ctx):
    """A row placed before the second leader yields no link in assign; link_fields, which tests
    it against all current leaders, yields it.  The same with the flag clear."""
    m = 16
    base = _quad(ctx, m)
    left, right = _halves(m * m)
    rows = np.stack([K.masked(base, left), base, K.masked(base, right)])
    for flags in (FOL_LINK, 0):
        with ctx.fol_registry(_params(m, flags)) as reg:
            ids = reg.assign_fields(_dev(rows))
            assert ids.tolist() == [0, 0, 1]
            assert reg.n_links == 0 and reg.components().tolist() == [0, 1]
            assert reg.link_fields(_dev(rows), ids) == 1
            assert reg.links().tolist() == [[0, 1]] and reg.components().tolist() == [0, 0]
            assert reg.link_fields(_dev(rows), ids) == 0
            assert reg.sizes.tolist() == [2, 1] and reg.rows_seen == 3      # classes untouched


# ---------------------------------------------------------------- stream = one-shot
@pytest.fixture(scope='module')
def stream_rows(ctx):
    """23 rows at m = 16 in a fixed shuffled order: three foliations u = rho**2 + k z**2 as left
    half, right half and two full rows each, the base field on three thirds with the two bridging
    unions, u = rho z, functions of rho alone on the left half, on the right half and everywhere
    (one class only under the axis rule, and then only through a link), and an all-NaN row.
    Never modified."""
    m = 16
    mm = m * m
    left, right = _halves(mm)
    p = np.arange(mm)
    t1, t2, t3 = p < 85, (p >= 85) & (p < 170), p >= 170
    rho, z = _grid(ctx, m)
    rows = []
    for k in (2.0, 3.0, 4.0):
        f = _quad(ctx, m, k)
        rows += [K.masked(f, left), K.masked(f, right), f, -1.5 * f]
    base = _quad(ctx, m)
    rows += [K.masked(base, t1), K.masked(base, t2), K.masked(base, t3), K.masked(base, t1 | t2),
             K.masked(base, t2 | t3)]
    rows.append(np.stack([z, rho]))
    zero = np.zeros(mm)
    rows += [K.masked(np.stack([2 * rho, zero]), left), K.masked(np.stack([4 * rho ** 3, zero]), right),
             np.stack([np.ones(mm), zero]), np.stack([zero, np.ones(mm)])]
    rows.append(np.full((2, mm), np.nan))
    rows = np.ascontiguousarray(np.stack(rows)[np.random.default_rng(3).permutation(len(rows))])
    assert rows.shape == (23, 2, mm)
    rows.setflags(write=False)
    return rows


@pytest.mark.parametrize('axis', (False, True))
def test_stream_equals_one_shot(ctx, stream_rows, axis):
    """The list cut into batches of 1, 7 and all: the same ids, the same links as a set and the
    same components, those of the restatement, with FOL_AXIS on and off; then link_fields over the
    whole list, against the restatement again."""
    rows = stream_rows
    prm = _params(16, FOL_LINK | (FOL_AXIS if axis else 0))
    ref = _ref(prm)
    want = ref.assign(rows)
    assert (want == -1).sum() == 1 and len(ref.links) >= 2
    for batch in (1, 7, len(rows)):
        with ctx.fol_registry(prm) as reg:
            ids = np.concatenate([reg.assign_fields(_dev(rows[a:a + batch])) for a in range(0, len(rows), batch)])
            assert np.array_equal(ids, want), (axis, batch)
            _same(reg, ref)
    full = _ref(prm)
    full.assign(rows)
    n_new = full.link_fields(rows, want)
    with ctx.fol_registry(prm) as reg:
        ids = reg.assign_fields(_dev(rows))
        assert reg.link_fields(_dev(rows), ids) == n_new
        _same(reg, full)
    if axis:       # the two half-domain functions of rho alone are one component, through the full one
        comp = full.components()
        lead = np.stack(full.leaders)
        rho_only = [c for c in range(full.n_classes) if np.nanmax(np.abs(lead[c][1])) == 0]
        assert len(rho_only) >= 1 and len({int(comp[c]) for c in rho_only}) == 1


# ---------------------------------------------------------------- the edge buffer
def test_edge_buffer_overflow(ctx):
    """A registry created with capacity_hint = 1 (an edge buffer of 64 pairs), 20 leaders of the
    base field on disjoint domains of 12 points (min_points = 4) and one batch of 9 full-domain
    rows, each of which joins class 0 and matches the 19 others: 171 edges, more than the buffer
    holds.  The result equals the restatement."""
    m = 16
    mm = m * m
    base = _quad(ctx, m)
    p = np.arange(mm)
    lead = np.stack([K.masked(base, (p >= 12 * d) & (p < 12 * d + 12)) for d in range(20)])
    rows = np.stack([(1.0 + i) * base for i in range(9)])
    prm = _params(m, FOL_LINK, min_points=4)
    ref = _ref(prm)
    assert ref.assign(lead).tolist() == list(range(20))
    want = ref.assign(rows)
    assert want.tolist() == [0] * 9 and len(ref.links) == 19
    with ctx.fol_registry(prm, capacity_hint=1) as reg:
        assert reg.assign_fields(_dev(lead)).tolist() == list(range(20))
        assert np.array_equal(reg.assign_fields(_dev(rows)), want)
        _same(reg, ref)
        assert reg.n_components == 1 and reg.link_ms > 0.0
        # the grown buffer serves the next batch in one launch
        assert np.array_equal(reg.assign_fields(_dev(rows)), want)
        ref.assign(rows)
        _same(reg, ref)


# ---------------------------------------------------------------- degenerate cases and errors
def test_degenerate_cases(ctx):
    """L = 0, L = 1, a batch of only unclassified rows; bad class ids, a foreign and a Kerr context
    are PDEVAL_ERR_ARG and change nothing."""
    import ctypes as C
    m = 16
    mm = m * m
    base = _quad(ctx, m)
    nan_rows = np.full((3, 2, mm), np.nan)
    with ctx.fol_registry(_params(m)) as reg:
        assert reg.components().shape == (0,) and reg.n_components == 0 and reg.links().shape == (0, 2)
        assert reg.component_sizes() == {}
        assert reg.link_fields(_dev(np.zeros((0, 2, mm))), np.zeros(0, dtype=np.int64)) == 0
        assert reg.assign_fields(_dev(nan_rows)).tolist() == [-1, -1, -1]          # L = 0, unclassified only
        assert reg.n_classes == 0 and reg.n_links == 0 and reg.rows_seen == 3
        assert reg.link_fields(_dev(nan_rows), [-1, -1, -1]) == 0
        assert reg.assign_fields(_dev(np.stack([base, 2.0 * base]))).tolist() == [0, 0]    # L = 1
        assert reg.components().tolist() == [0] and reg.n_links == 0
        assert reg.assign_fields(_dev(nan_rows)).tolist() == [-1, -1, -1]          # L = 1, unclassified only
        assert reg.link_fields(_dev(base[None]), [0]) == 0
        d = _dev(np.stack([base, base]))
        for bad in ([0, 1], [-2, 0], [0, 1 << 40]):
            with pytest.raises(PdevalError, match='pdeval error 1.*class id'):
                reg.link_fields(d, bad)
        with pytest.raises(ValueError, match='class_ids'):
            reg.link_fields(d, [0])
        lib, n_new = ctx.lib, C.c_int64(7)
        ids = np.zeros(2, dtype=np.int64)
        other = Context(0, device=0)
        kerr = Context(1, device=0)
        try:
            for foreign in (other, kerr):
                assert lib.pdeval_fol_registry_link_fields(foreign.h, reg.h, d.data_ptr(), ids.ctypes.data, 2,
                                                           C.byref(n_new)) == 1      # PDEVAL_ERR_ARG
            with pytest.raises(PdevalError, match='pdeval error 1.*force-free'):
                kerr.fol_registry(_params(m))
        finally:
            other.close()
            kerr.close()
        e = np.array([[0, 1]], dtype=np.int64)
        assert lib.pdeval_fol_registry_load_links(reg.h, e.ctypes.data, 1) == 1       # an end outside [0, L)
        assert reg.n_links == 0 and reg.sizes.tolist() == [2]


# ---------------------------------------------------------------- persistence and merge
def test_save_load_and_merge(ctx, stream_rows, tmp_path):
    """save / load round trip of the links; a file without links has none; merge of two linked
    registries against the restatement's merge; a FOL_LINK mismatch is refused by load and merge
    the way a FOL_AXIS mismatch is."""
    rows = stream_rows
    prm = _params(16)
    k = 12
    ra, rb = _ref(prm), _ref(prm)
    with ctx.fol_registry(prm) as a, ctx.fol_registry(prm) as b:
        for reg, ref, part in ((a, ra, rows[:k]), (b, rb, rows[k:])):
            ids = reg.assign_fields(_dev(part))
            assert np.array_equal(ids, ref.assign(part))
            assert reg.link_fields(_dev(part), ids) == ref.link_fields(part, ids)
            _same(reg, ref)
        assert len(ra.links) >= 1 and len(rb.links) >= 1
        path = os.path.join(tmp_path, 'reg.npz')
        a.save(path)
        with FOL.FoliationRegistry.load(ctx, path) as c:
            assert int(c.params.flags) == FOL_LINK
            _same(c, ra)
            assert np.array_equal(c.leader_fields().cpu().numpy(), a.leader_fields().cpu().numpy(), equal_nan=True)
        with pytest.raises(ValueError, match='flags = 2 in the file, 0 asked for'):
            FOL.FoliationRegistry.load(ctx, path, _params(16, 0))
        with np.load(path) as d:
            old = {name: d[name] for name in d.files if name != 'links'}
        np.savez(path, **old)
        with FOL.FoliationRegistry.load(ctx, path) as c:
            assert c.n_links == 0 and np.array_equal(c.components(), np.arange(ra.n_classes))
        with ctx.fol_registry(_params(16, 0)) as plain:
            with pytest.raises(ValueError, match='differ in flags'):
                a.merge(plain)
            with pytest.raises(ValueError, match='differ in flags'):
                plain.merge(a)
        id_map = a.merge(b)
        assert np.array_equal(id_map, ra.merge(rb))
        _same(a, ra)


# ---------------------------------------------------------------- the flag off
def test_flag_off_is_what_it_was(ctx, stream_rows):
    """A small stream with FOL_LINK clear and set: ids, sizes and the leaders' fields are the same
    bit for bit, and they are the values tests/foliation_ref.py gives."""
    rows = stream_rows
    want = classes_from_leader(R.sequential_leaders(np.array(rows))[0])
    got = {}
    for flags in (0, FOL_LINK):
        with ctx.fol_registry(_params(16, flags)) as reg:
            ids = np.concatenate([reg.assign_fields(_dev(rows[a:a + 5])) for a in range(0, len(rows), 5)])
            got[flags] = (ids, reg.sizes, reg.leader_keys, reg.leader_fields().cpu().numpy())
            assert int(reg.params.flags) == flags
    for flags in (0, FOL_LINK):
        ids, sizes, keys, lf = got[flags]
        assert np.array_equal(ids, want.class_id) and np.array_equal(sizes, want.sizes)
        lead_rows = np.array([int(np.flatnonzero(want.class_id == c)[0]) for c in range(want.n_classes)])
        assert np.array_equal(keys, lead_rows)
        assert np.array_equal(lf.view(np.int64), np.ascontiguousarray(rows[lead_rows]).view(np.int64))
    assert fol_params(None, link=True).flags == FOL_LINK and fol_params(_params(16), link=False).flags == 0
    assert fol_params(_params(16, FOL_AXIS), link=True).flags == FOL_AXIS | FOL_LINK

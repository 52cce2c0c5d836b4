"""GPU tests of the foliation class registry (DESIGN.md §14 "Registry"): fol_assign_kernel
(Stage A), the append, pdeval_fol_registry_*, pdeval.foliation.FoliationRegistry and
BatchValidator.assign_foliation, against the one-shot pdeval_foliation_classes and the numpy
restatement of the sequential rule (tests/foliation_ref.py)."""
import ctypes as C

import numpy as np
import pytest

import foliation_cases as FC
import foliation_ref as R
from pdeval import foliation as FOL
from pdeval import problem_defs as P
from pdeval._lib import Context, PdevalError, default_fol_params
from pdeval.opcodes import CLS_ACCEPT

pytestmark = pytest.mark.gpu

T = 32    # kFolAssignTile: the leaders of one LDS tile of fol_assign_kernel


@pytest.fixture(scope='module')
def ctx():
    c = Context(0, device=0)
    yield c
    c.close()


def _params(m):
    p = default_fol_params()
    p.m = m
    return p


def _torch():
    import torch
    return torch, torch.device('cuda', 0)


def _dev(a):
    torch, dev = _torch()
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@pytest.fixture(scope='module')
def stream(ctx):
    """F's programs (the depth-8, PUSH_P and complex programs among them) followed by the accepted
    rows of d3_strings(200), resident on the device; the one-shot class ids of the whole list at
    m = 16 and m = 9.  Shared, never modified."""
    from pdeval.native import compile_strings
    F = FC.field_set()
    pd_ = F['pd']
    ops2, off2, _ = compile_strings(pd_, FC.d3_strings(200))
    acc = np.flatnonzero(ctx.validate(ops2, off2)['status'] == CLS_ACCEPT).astype(np.int64)
    nf = len(F['progs'])
    ops = np.concatenate([F['ops'], np.asarray(ops2, dtype=np.int32)])
    off = np.concatenate([F['off'], np.asarray(off2, dtype=np.int64)[1:] + int(F['off'][-1])])
    rows = np.concatenate([np.arange(nf, dtype=np.int64), nf + acc])
    d_ops, d_off = _dev(ops.astype(np.int32)), _dev(off.astype(np.int64))
    prog = (d_ops, int(d_ops.numel()), d_off, len(off) - 1)
    one = {m: FOL.classify(ctx, *prog, rows, _params(m)).class_id for m in (16, 9)}
    return dict(F=F, prog=prog, rows=rows, nf=nf, one=one)


def _in_batches(reg, prog, rows, sizes):
    ids, a = [], 0
    for s in list(sizes) + [len(rows)]:
        b = min(len(rows), a + s)
        ids.append(reg.assign(*prog, rows[a:b]))
        a = b
        if a == len(rows):
            break
    return np.concatenate(ids)


@pytest.mark.parametrize('m', (16, 9))
def test_stream_equals_one_shot(ctx, stream, m):
    """The list in batches of 1, 3, 32, 33 rows and the rest: the class ids of the one-shot call on
    the whole list; on F's rows also those of the numpy restatement on the oracle's fields."""
    rows, one = stream['rows'], stream['one'][m]
    assert one.max() + 1 > 2 * T and (one == -1).any()       # several tiles of leaders; unclassified rows
    with ctx.fol_registry(_params(m), 4) as reg:
        ids = _in_batches(reg, stream['prog'], rows, (1, 3, 32, 33))
        assert ids.dtype == np.int64 and np.array_equal(ids, one), np.flatnonzero(ids != one)[:10]
        assert reg.n_classes == one.max() + 1 and reg.rows_seen == len(rows)
        assert np.array_equal(reg.sizes, np.bincount(one[one >= 0]))
        lead_rows = np.array([int(np.flatnonzero(one == c)[0]) for c in range(reg.n_classes)])
        assert np.array_equal(reg.leader_keys, lead_rows)    # default keys: the running row number
    F, nf = stream['F'], stream['nf']
    oracle = F['fields'][m] if m in F['fields'] else np.stack([R.oracle_field(w, m) for w in F['progs']])
    want = FOL.classes_from_leader(R.sequential_leaders(oracle)[0]).class_id
    assert np.array_equal(ids[:nf], want), (ids[:nf], want)


def _const_fields(angles, mm):
    """[n, 2, mm] constant fields (cos t, sin t)."""
    t = np.asarray(angles, dtype=np.float64)
    return np.ascontiguousarray(np.stack([np.cos(t), np.sin(t)], axis=1)[:, :, None] * np.ones(mm))


def _angle(k):
    return 0.3 + 0.03 * np.asarray(k, dtype=np.float64)     # k < 90: below pi, 0.03 apart, none along an axis


def _ref_assign(leaders, rows, tau=R.TAU, min_points=R.MIN_POINTS):
    """The sequential rule, leader by leader with foliation_ref.matches: class ids of `rows` after
    the resident `leaders`, and the grown leader array."""
    lead = [f for f in leaders]
    ids = np.full(len(rows), -1, dtype=np.int64)
    for i, f in enumerate(rows):
        if np.isfinite(f[0]).sum() < min_points:
            continue
        hit = R.matches(f, np.stack(lead), tau, min_points) if lead else np.zeros(0, bool)
        if hit.any():
            ids[i] = int(np.argmax(hit))
        else:
            ids[i] = len(lead)
            lead.append(f)
    return ids, lead


def _loaded(ctx, m, leaders):
    reg = ctx.fol_registry(_params(m), 0)
    L = len(leaders)
    if L:
        reg._load(_dev(leaders), np.arange(L, dtype=np.int64), np.ones(L, dtype=np.int64))
    assert reg.n_classes == L
    return reg


@pytest.mark.parametrize('m', (5, 9, 16, 20))
def test_stage_a_synthetic(ctx, m):
    """Leader k is the constant field at angle 0.3 + 0.03 k, so a row at angle j matches leader j
    only.  L = 0, 1, T-1, T, T+1, 2T+1 leaders (T = 32, the kernel's LDS tile) against 1, 4, 5 and
    65 rows (a block holds four), at m = 5 (a partial chunk), 9 (full + partial), 16 (the
    in-register limit) and 20 (the re-read path): the restatement's ids leader by leader.  Rows
    past L match nothing and become leaders; their repeats join them."""
    mm = m * m
    for L in (0, 1, T - 1, T, T + 1, 2 * T + 1):
        leaders = _const_fields(_angle(np.arange(L)), mm)
        for n in (1, 4, 5, 65):
            j = (7 * np.arange(n) + L // 2) % (L + 3)
            rows = _const_fields(_angle(j), mm)
            want, grown = _ref_assign(leaders, rows)
            with _loaded(ctx, m, leaders) as reg:
                ids = reg.assign_fields(_dev(rows))
                assert np.array_equal(ids, want), (m, L, n, ids, want)
                assert reg.n_classes == len(grown)
                assert np.array_equal(reg.leader_fields().cpu().numpy(), np.stack(grown))


@pytest.mark.parametrize('m', (5, 9, 16, 20))
def test_stage_a_edges(ctx, m):
    """Two identical leaders: the earlier one.  A leader equal to the row but for one bad point at
    the last active lane of the last chunk: no match.  A pair with min_points - 1 usable points: no
    match; with exactly min_points: a match.  An all-NaN row: -1, and no leader."""
    mm, mp = m * m, R.MIN_POINTS
    L = T + 2
    leaders = _const_fields(_angle(np.arange(L)), mm)
    leaders[T + 1] = leaders[2]                              # identical to leader 2, in the second tile
    leaders[3, :, mm - 1] = _const_fields(_angle([50]), 1)[0, :, 0]   # one point of leader 3 at another angle
    leaders[4, :, mp - 1:] = np.nan                          # leader 4: min_points - 1 finite points
    leaders[5, :, mp:] = np.nan                              # leader 5: exactly min_points
    rows = _const_fields(_angle([2, 3, 4, 5]), mm)
    rows = np.concatenate([rows, np.full((1, 2, mm), np.nan)])
    want, grown = _ref_assign(leaders, rows)
    assert want.tolist() == [2, L, L + 1, 5, -1]             # (the restatement's own verdicts)
    with _loaded(ctx, m, leaders) as reg:
        ids = reg.assign_fields(_dev(rows))
        assert np.array_equal(ids, want), (m, ids, want)
        assert reg.n_classes == L + 2 and reg.rows_seen == L + len(rows)
        # with the finite counts given (as gradient_fields returns them) the result is the same
    with _loaded(ctx, m, leaders) as reg:
        nfin = _dev(np.isfinite(rows[:, 0, :]).sum(axis=1).astype(np.int32))
        assert np.array_equal(reg.assign_fields(_dev(rows), nfin), want)


def test_growth(ctx):
    """Capacity hint 1, 70 distinct leaders appended over three calls: ids dense and stable, the
    leaders' fields equal gradient_fields of their programs bit for bit, sizes and keys right."""
    pd_ = P.force_free()
    strings = [f'rho*z + {k}*rho' for k in range(1, 71)]     # rho (z + k): 70 distinct foliations
    ops, off, _ = P.compile_strings(pd_, strings)
    d_ops, d_off = _dev(np.asarray(ops, dtype=np.int32)), _dev(np.asarray(off, dtype=np.int64))
    prog = (d_ops, int(d_ops.numel()), d_off, 70)
    keys = 1000 + 7 * np.arange(70, dtype=np.int64)
    with ctx.fol_registry(None, 1) as reg:
        ids = np.concatenate([reg.assign(*prog, np.arange(a, b), keys[a:b]) for a, b in ((0, 1), (1, 34), (34, 70))])
        assert np.array_equal(ids, np.arange(70)) and reg.n_classes == 70
        want, _ = FOL.gradient_fields(ctx, *prog)
        assert np.array_equal(reg.leader_fields().cpu().numpy(), want.cpu().numpy())
        again = reg.assign(*prog, np.arange(69, -1, -1))
        assert np.array_equal(again, np.arange(69, -1, -1)) and reg.n_classes == 70 and reg.last_new == 0
        assert np.array_equal(reg.sizes, np.full(70, 2)) and np.array_equal(reg.leader_keys, keys)
        assert reg.rows_seen == 140


def test_save_load(ctx, stream, tmp_path):
    """Half the list, save, load into a fresh registry on a fresh context, the other half: the ids
    of the uninterrupted run.  Loading at another m raises ValueError naming m."""
    rows, one, prog = stream['rows'], stream['one'][16], stream['prog']
    h = len(rows) // 2
    path = tmp_path / 'registry.npz'
    with ctx.fol_registry() as reg:
        first = reg.assign(*prog, rows[:h])
        reg.save(path)
        n_half, sizes_half = reg.n_classes, reg.sizes
    c2 = Context(0, device=0)
    try:
        with pytest.raises(ValueError, match='m = 16'):
            FOL.FoliationRegistry.load(c2, path, _params(9))
        with FOL.FoliationRegistry.load(c2, path) as reg2:
            assert reg2.n_classes == n_half and np.array_equal(reg2.sizes, sizes_half)
            second = reg2.assign(*prog, rows[h:])
            assert np.array_equal(np.concatenate([first, second]), one)
            assert np.array_equal(reg2.sizes, np.bincount(one[one >= 0]))
    finally:
        c2.close()
    g = Context(0, device=0, grid=np.array([0.05, 3.0, 64, -2.0, 2.0, 64, 0.25, 0.41]))
    try:
        with pytest.raises(ValueError, match='grid'):
            FOL.FoliationRegistry.load(g, path)
    finally:
        g.close()


def test_merge(ctx, stream):
    """Two registries fed the even and the odd rows; a.merge(b) maps each of b's classes to the
    class a holds for b's leader field, or to a new one -- the restatement leader by leader on the
    leaders' fields -- and the sizes add up to the classified rows."""
    rows, prog = stream['rows'], stream['prog']
    with ctx.fol_registry() as a, ctx.fol_registry() as b:
        ia, ib = a.assign(*prog, rows[0::2]), b.assign(*prog, rows[1::2])
        fa, fb = a.leader_fields().cpu().numpy(), b.leader_fields().cpu().numpy()
        sa, sb, kb = a.sizes, b.sizes, b.leader_keys
        want, grown = _ref_assign(fa, fb)
        got = a.merge(b)
        assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]
        assert (want < len(fa)).any() and (want >= len(fa)).any()      # both kinds occur
        assert a.n_classes == len(grown)
        sizes = np.concatenate([sa, np.zeros(len(grown) - len(sa), dtype=np.int64)])
        np.add.at(sizes, want, sb)
        assert np.array_equal(a.sizes, sizes)
        assert a.sizes.sum() == (ia >= 0).sum() + (ib >= 0).sum()
        new = want >= len(fa)
        assert np.array_equal(a.leader_keys[len(fa):], kb[new])
        assert b.n_classes == len(fb)                                  # b is left as it is


def test_tags(ctx):
    """A registry fed the seven paper solutions, then their re-parametrisations, names all seven
    (rho**2 by the equal-field rule), as test_tags_every_paper_solution."""
    pd_ = P.force_free()
    strings = FC.case_exprs(pd_)
    ops, off, _ = P.compile_strings(pd_, strings)
    d_ops, d_off = _dev(np.asarray(ops, dtype=np.int32)), _dev(np.asarray(off, dtype=np.int64))
    names = list(pd_.known_solutions.values())
    with ctx.fol_registry() as reg:
        assert reg.tags(pd_) == {}
        a = reg.assign(d_ops, int(d_ops.numel()), d_off, len(strings), np.arange(7))
        b = reg.assign(d_ops, int(d_ops.numel()), d_off, len(strings), np.arange(7, len(strings)))
        assert a.tolist() == list(range(7)) and reg.n_classes == 7 and (b >= 0).all()
        assert reg.tags(pd_) == {k: names[k] for k in range(7)}


def test_batch_validator_assign_foliation():
    """assign_foliation over the two halves of d3_strings(120) equals foliation_classes on the
    whole list; a registry of another validator is refused."""
    from pdeval.batch import BatchValidator
    strings = FC.d3_strings(120)
    h = len(strings) // 2
    bv = BatchValidator('force_free', device=0)
    try:
        cls, acc, _ = bv.foliation_classes(strings)
        with bv.foliation_registry() as reg:
            c1, a1 = bv.assign_foliation(reg, strings[:h], keys=np.arange(h))
            c2, a2 = bv.assign_foliation(reg, strings[h:], keys=np.arange(h, len(strings)))
            assert np.array_equal(np.concatenate([a1, a2 + h]), acc)
            assert np.array_equal(np.concatenate([c1, c2]), cls.class_id)
            lead_rows = np.array([int(np.flatnonzero(cls.class_id == c)[0]) for c in range(cls.n_classes)])
            assert np.array_equal(reg.leader_keys, acc[lead_rows])    # keys: indices into strings
            other = Context(0, device=0)
            try:
                with other.fol_registry() as foreign, pytest.raises(ValueError, match='another'):
                    bv.assign_foliation(foreign, strings[:4])
            finally:
                other.close()
    finally:
        bv.close()
    kv = BatchValidator('kerr', device=0)
    try:
        with pytest.raises(ValueError, match='force-free'):
            kv.foliation_registry()
    finally:
        kv.close()


def test_errors(ctx, stream):
    """A Kerr context, bad parameters, a registry used with another context, load into a non-empty
    registry and negative counts are PDEVAL_ERR_ARG; n_list = 0 is OK and changes nothing."""
    d_ops, nw, d_off, n = stream['prog']
    lib = ctx.lib
    k = Context(1, device=0)
    try:
        with pytest.raises(PdevalError, match='pdeval error 1.*force-free'):
            k.fol_registry()
    finally:
        k.close()
    for m in (3, 65):
        with pytest.raises(PdevalError, match='pdeval error 1.*bad parameters'):
            ctx.fol_registry(_params(m))
    with pytest.raises(PdevalError, match='pdeval error 1'):
        ctx.fol_registry(None, -1)
    other = Context(0, device=0)
    try:
        with ctx.fol_registry(_params(9)) as reg:
            ids = np.zeros(4, dtype=np.int64)
            f = _dev(_const_fields(_angle(np.arange(4)), 81))
            rc = lib.pdeval_fol_registry_assign_fields(other.h, reg.h, f.data_ptr(), None, 4, None, ids.ctypes.data, None)
            assert rc == 1 and b'another context' in lib.pdeval_last_error(other.h)
            rc = lib.pdeval_fol_registry_assign(other.h, reg.h, d_ops.data_ptr(), nw, d_off.data_ptr(), n, None, 4, None,
                                                ids.ctypes.data, None)
            assert rc == 1 and b'another context' in lib.pdeval_last_error(other.h)
            assert reg.n_classes == 0 and reg.rows_seen == 0
            # negative counts
            assert lib.pdeval_fol_registry_assign_fields(ctx.h, reg.h, f.data_ptr(), None, -1, None, ids.ctypes.data, None) == 1
            assert lib.pdeval_fol_registry_assign(ctx.h, reg.h, d_ops.data_ptr(), nw, d_off.data_ptr(), n, None, -1, None,
                                                  ids.ctypes.data, None) == 1
            assert lib.pdeval_fol_registry_assign(ctx.h, reg.h, d_ops.data_ptr(), -1, d_off.data_ptr(), n, None, 1, None,
                                                  ids.ctypes.data, None) == 1
            keys = np.arange(4, dtype=np.int64)
            assert lib.pdeval_fol_registry_load(ctx.h, reg.h, f.data_ptr(), keys.ctypes.data, keys.ctypes.data, -1) == 1
            # n_list = 0: OK, nothing changes, null buffers are never touched
            n_new = C.c_int64(7)
            assert lib.pdeval_fol_registry_assign(ctx.h, reg.h, None, 0, None, 0, None, 0, None, None, C.byref(n_new)) == 0
            assert lib.pdeval_fol_registry_assign_fields(ctx.h, reg.h, None, None, 0, None, None, C.byref(n_new)) == 0
            assert n_new.value == 0 and reg.n_classes == 0 and reg.rows_seen == 0
            assert reg.assign(d_ops, nw, d_off, n, np.zeros(0, dtype=np.int64)).size == 0
            # load into a non-empty registry
            assert reg.assign_fields(f).tolist() == [0, 1, 2, 3]
            with pytest.raises(PdevalError, match='pdeval error 1.*not empty'):
                reg._load(f, keys, np.ones(4, dtype=np.int64))
            assert reg.n_classes == 4 and reg.sizes.tolist() == [1, 1, 1, 1]
    finally:
        other.close()

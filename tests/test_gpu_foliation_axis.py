"""GPU tests of the axis rule of the foliation classes (PDEVAL_FOL_AXIS; DESIGN.md §14 "The axis
rule"): the AXIS instantiations of fol_match_kernel and fol_assign_kernel, fol_kind_kernel, the
entry points that carry the flag and the Python layer, against the numpy restatement
tests/foliation_axis_ref.py on the oracle's gradient fields."""
import numpy as np
import pytest

import foliation_axis_ref as A
import foliation_cases as FC
import foliation_ref as R
from pdeval import foliation as FOL
from pdeval import problem_defs as P
from pdeval._lib import Context, PdevalError, default_fol_params
from pdeval.flatten import pack

pytestmark = pytest.mark.gpu

AXIS = 1    # PDEVAL_FOL_AXIS
T = 32      # kFolAssignTile: the leaders of one LDS tile of fol_assign_kernel


@pytest.fixture(scope='module')
def ctx():
    c = Context(0, device=0)
    yield c
    c.close()


def _params(m, axis):
    p = default_fol_params()
    p.m = m
    p.flags = AXIS if axis else 0
    return p


def _torch():
    import torch
    return torch, torch.device('cuda', 0)


def _dev(a):
    torch, dev = _torch()
    return torch.from_numpy(np.array(a, order='C')).to(dev)      # (a copy: the shared fixtures are read-only)


# ---------------------------------------------------------------- the match kernel
@pytest.fixture(scope='module')
def mixed():
    """{m: 65 rows}: the oracle fields of foliation_axis_ref.EXPRS (functions of rho alone, of z
    alone, generic ones), scaled copies of them, an all-NaN row, rho**2 and z**2 at 10 points only
    (n_used < min_points) and rho**4 with every third point NaN.  Never modified."""
    pd_ = P.force_free()
    ops, off, _ = P.compile_strings(pd_, A.EXPRS)
    out = {}
    for m in (5, 9, 12):
        base = R.oracle_fields(ops, off, m)
        rows = list(base)
        k = 0
        while len(rows) < 61:
            rows.append((-2.5 - k) * base[k % len(base)])
            k += 1
        rows.append(np.full_like(base[0], np.nan))
        for i in (1, 5):
            few = np.full_like(base[i], np.nan)
            few[:, 8:18] = base[i][:, 8:18]
            rows.append(few)
        holes = base[2].copy()
        holes[:, ::3] = np.nan
        rows.append(holes)
        f = np.ascontiguousarray(np.stack(rows))
        assert f.shape == (65, 2, m * m)
        f.setflags(write=False)
        out[m] = f
    return out


def _match(ctx, rows, probes, m, axis, diagnostics=True):
    return FOL.match_fields(ctx, _dev(rows), _dev(probes), _params(m, axis), diagnostics=diagnostics)


def _check_match(ctx, rows, probes, m, axis=True):
    """mask and n_used equal the restatement's, qmax within the tolerance of
    test_gpu_foliation.py::_check_match; the path without diagnostics gives the same mask."""
    hit, used, qmax = _match(ctx, rows, probes, m, axis)
    for i, row in enumerate(rows):
        nu, nb, q = A.pair_stats(row, probes, axis=axis)
        assert np.array_equal(used[i], nu), (m, i, used[i], nu)
        assert np.array_equal(hit[i], (nu >= R.MIN_POINTS) & (nb == 0)), (m, i)
        big = q > 1e-300
        assert np.all(np.abs(qmax[i][big] - q[big]) <= 1e-9 * q[big]) and np.all(qmax[i][~big] <= 1e-300), (m, i)
        assert np.isfinite(qmax[i]).all()
    assert np.array_equal(_match(ctx, rows, probes, m, axis, diagnostics=False), hit)   # the early-exit path
    return hit, used


@pytest.mark.parametrize('m', (5, 9, 12))
def test_match_65_rows_1_probe(ctx, mixed, m):
    """65 mixed rows against rho**2, z**2 and rho**2*z with the flag: rho**2 matches itself, every
    function of rho alone with enough points matches rho**2 and no other row does."""
    f, mm = mixed[m], m * m
    i2, iz2, ig = A.EXPRS.index('rho**2'), A.EXPRS.index('z**2'), A.EXPRS.index('rho**2*z')
    kind = A.kinds(f)
    for probe, k in ((i2, 1), (iz2, 2)):
        hit, used = _check_match(ctx, f, f[[probe]], m)
        assert hit[probe, 0] and used[probe, 0] == mm
        assert np.array_equal(hit[:, 0], kind == k)
        assert (hit[:61, 0].sum(), used[62 if k == 1 else 63, 0]) == ((25 if k == 1 else 18), 10)
    hit, _ = _check_match(ctx, f, f[[ig]], m)
    assert hit[ig, 0] and not hit[kind > 0, 0].any()
    # without the flag the result is what it was: rho**2 has no usable point against itself
    hit0, used0 = _check_match(ctx, f, f[[i2]], m, axis=False)
    assert not hit0.any() and used0[i2, 0] == 0


@pytest.mark.parametrize('m', (5, 9, 12))
def test_match_1_row_32_probes(ctx, mixed, m):
    f = mixed[m]
    for row in (A.EXPRS.index('rho**2'), A.EXPRS.index('z'), 62, 64):
        hit, _ = _check_match(ctx, f[[row]], f[:32], m)
        if row < 60:
            assert hit[0].tolist() == (A.kinds(f[:32]) == A.kinds(f[[row]])[0]).tolist()
    assert not _check_match(ctx, f[[62]], f[:32], m)[0].any()        # 10 points: no match


# ---------------------------------------------------------------- classes, one-shot and streamed
def _axis_list():
    """rho first, 34 distinct generic foliations rho + k z, then z and further rows of one
    coordinate, two re-parametrisations of generic rows and a complex program (an all-NaN row):
    with the flag the leaders are rho (index 0), the 34 generic ones, z (index 35, in the second
    tile of 32) and rho**2*z."""
    exprs = ['rho'] + [f'rho + {k}*z' for k in range(1, 35)] + \
            ['z', 'rho**2', 'z**2', 'rho**4', 'exp_neg(z)', 'exp(rho**2)', 'exp(rho + 5*z)', 'rho**2*z',
             'exp(rho**2*z)']
    return exprs


@pytest.fixture(scope='module')
def listed(ctx):
    """The list resident on the device, its oracle fields at m = 16 and m = 20 and the
    restatement's sequential class ids with the flag set and clear.  Never modified."""
    pd_ = P.force_free()
    exprs = _axis_list()
    progs = [FC.words(pd_, s) for s in exprs] + [FC.complex_program()]
    ops, off = pack([list(map(int, w)) for w in progs])
    d_ops, d_off = _dev(np.asarray(ops, dtype=np.int32)), _dev(np.asarray(off, dtype=np.int64))
    prog = (d_ops, int(d_ops.numel()), d_off, len(progs))
    want = {}
    for m in (16, 20):
        f = np.stack([R.oracle_field(w, m) for w in progs])
        for axis in (False, True):
            want[m, axis] = A.class_ids(A.sequential_leaders(f, axis=axis))
        want[m, 'kinds'] = A.kinds(f)
    return dict(exprs=exprs, prog=prog, n=len(progs), want=want)


@pytest.mark.parametrize('m', (16, 20))
def test_one_shot_and_streamed_classes(ctx, listed, m):
    """m = 16 is fol_assign_kernel's in-register instantiation, m = 20 the re-reading one.  With
    the flag: the one-shot classes and the registry's at every batch split equal the
    restatement's; rho**2 joins leader 0 and z**2 the leader at index 35, past the first tile;
    exactly one leader has kind 1 and one kind 2.  Without it every one-coordinate row leads."""
    ex, prog, n = listed['exprs'], listed['prog'], listed['n']
    rows = np.arange(n, dtype=np.int64)
    want = listed['want'][m, True]
    assert want.max() + 1 == 37 > T and want[-1] == -1
    assert want[ex.index('rho**2')] == want[ex.index('rho**4')] == want[ex.index('exp(rho**2)')] == 0
    assert want[ex.index('z**2')] == want[ex.index('exp_neg(z)')] == 35 >= T
    assert want[ex.index('exp(rho + 5*z)')] == 5 and want[ex.index('exp(rho**2*z)')] == 36
    prm = _params(m, True)
    one = FOL.classify(ctx, *prog, rows, prm)
    assert np.array_equal(one.class_id, want), (one.class_id, want)
    for cut in range(n + 1):
        with ctx.fol_registry(prm, 1) as reg:
            ids = np.concatenate([reg.assign(*prog, rows[:cut]), reg.assign(*prog, rows[cut:])])
            assert np.array_equal(ids, want), (m, cut, ids, want)
            assert reg.n_classes == 37
            if cut in (0, 36, n):
                kinds = reg.kinds()
                lead_rows = np.array([int(np.flatnonzero(want == c)[0]) for c in range(37)])
                assert kinds.dtype == np.uint8 and np.array_equal(kinds, listed['want'][m, 'kinds'][lead_rows])
                assert (kinds == 1).sum() == 1 and (kinds == 2).sum() == 1 and kinds[0] == 1 and kinds[35] == 2
                assert int(reg.params.flags) & AXIS        # pdeval_fol_registry_info returns the flag
    # the flag clear: what it was
    want0 = listed['want'][m, False]
    assert want0.max() + 1 == 42                            # rho, z and the 5 further axis rows lead too
    prm0 = _params(m, False)
    assert np.array_equal(FOL.classify(ctx, *prog, rows, prm0).class_id, want0)
    for cut in (0, 1, 33, 40, n):
        with ctx.fol_registry(prm0, 1) as reg:
            ids = np.concatenate([reg.assign(*prog, rows[:cut]), reg.assign(*prog, rows[cut:])])
            assert np.array_equal(ids, want0), (m, cut)
            kinds = reg.kinds()
            assert (kinds == 1).sum() == 4 and (kinds == 2).sum() == 3 and not int(reg.params.flags)


@pytest.mark.parametrize('m', (5, 9, 12))
def test_field_kinds(ctx, mixed, m):
    """pdeval_field_kinds on the 65 mixed rows and on edge rows -- exactly min_points points, one
    non-zero u_z among zeros, u_z NaN at half the points, a zero field -- equals numpy, whatever
    the flag."""
    f, mm = mixed[m], m * m
    exact = np.full_like(f[5], np.nan)
    exact[:, 3:3 + R.MIN_POINTS] = f[5][:, 3:3 + R.MIN_POINTS]
    spoiled = f[1].copy()
    spoiled[1, mm - 1] = 1e-300
    half = f[1].copy()
    half[1, ::2] = np.nan
    rows = np.concatenate([f, exact[None], spoiled[None], half[None], np.zeros((1, 2, mm))])
    want = A.kinds(rows)
    assert want[:10].tolist() == [1, 1, 1, 1, 2, 2, 2, 0, 0, 0] and want[61:65].tolist() == [0, 0, 0, 1]
    assert want[65:].tolist() == [2, 0, 1 if mm // 2 >= R.MIN_POINTS else 0, 0]
    for axis in (False, True):
        got = FOL.field_kinds(ctx, _dev(rows), _params(m, axis))
        assert got.dtype == np.uint8 and np.array_equal(got, want), (m, got, want)
    assert FOL.field_kinds(ctx, _dev(rows[:0]), _params(m, True)).size == 0


# ---------------------------------------------------------------- tags, persistence, errors
def test_tags(ctx):
    """With the flag the class led by rho**2 is tagged Vertical field by the Jacobian rule alone
    and rho**4 falls in it; without it rho**4 is an untagged class of its own."""
    pd_ = P.force_free()
    strings = list(pd_.known_solutions) + ['rho**4']
    ops, off, _ = P.compile_strings(pd_, strings)
    d_ops, d_off = _dev(np.asarray(ops, dtype=np.int32)), _dev(np.asarray(off, dtype=np.int64))
    prog = (d_ops, int(d_ops.numel()), d_off, len(strings))
    names = list(pd_.known_solutions.values())
    assert names[0] == 'Vertical field' and strings[0] == 'rho**2'
    prm = _params(16, True)
    with ctx.fol_registry(prm) as reg:
        ids = reg.assign(*prog, np.arange(len(strings)))
        assert ids.tolist() == list(range(7)) + [0] and reg.n_classes == 7
        assert reg.tags(pd_) == {k: names[k] for k in range(7)}
        lead = reg.leader_fields()
        assert FOL.match_fields(ctx, lead[:1], lead[:1], prm)[0, 0]          # the Jacobian rule alone
        assert not FOL.match_fields(ctx, lead[:1], lead[:1], _params(16, False))[0, 0]
    cls = FOL.classify(ctx, *prog, np.arange(len(strings)), prm)
    assert cls.class_id.tolist() == list(range(7)) + [0]
    assert FOL.tag_known(ctx, pd_, cls, prog, prm) == {k: names[k] for k in range(7)}
    with ctx.fol_registry(_params(16, False)) as reg:
        ids = reg.assign(*prog, np.arange(len(strings)))
        assert ids.tolist() == list(range(8))
        assert reg.tags(pd_) == {k: names[k] for k in range(7)}              # rho**4: class 7, no tag


def test_save_load_merge(ctx, listed, tmp_path):
    """The flag survives save and load; a file without `flags` loads as 0; loading with other
    flags than the file's and merging registries of different flags raise, naming flags."""
    prog, n = listed['prog'], listed['n']
    rows = np.arange(n, dtype=np.int64)
    want = listed['want'][16, True]
    path, old = tmp_path / 'axis.npz', tmp_path / 'old.npz'
    with ctx.fol_registry(_params(16, True)) as reg:
        first = reg.assign(*prog, rows[:20])
        reg.save(path)
        with np.load(path) as d:
            assert int(d['flags']) == AXIS
            np.savez(old, **{k: d[k] for k in d.files if k != 'flags'})
        with pytest.raises(ValueError, match='flags'):
            FOL.FoliationRegistry.load(ctx, path, _params(16, False))
        with FOL.FoliationRegistry.load(ctx, path) as reg2:
            assert int(reg2.params.flags) == AXIS
            assert np.array_equal(np.concatenate([first, reg2.assign(*prog, rows[20:])]), want)
        with FOL.FoliationRegistry.load(ctx, path, _params(16, True)) as reg3:
            assert int(reg3.params.flags) == AXIS and reg3.n_classes == reg.n_classes
        with FOL.FoliationRegistry.load(ctx, old) as reg0:
            assert int(reg0.params.flags) == 0 and reg0.n_classes == reg.n_classes
            with pytest.raises(ValueError, match='flags'):
                reg.merge(reg0)
            with pytest.raises(ValueError, match='flags'):
                reg0.merge(reg)
        with pytest.raises(ValueError, match='flags'):
            FOL.FoliationRegistry.load(ctx, old, _params(16, True))
        # registries of equal flags merge: the other's axis leaders join this one's
        with ctx.fol_registry(_params(16, True)) as other:
            other.assign(*prog, rows[35:])
            k_other = other.kinds()
            ids = reg.merge(other)
            assert ids[int(np.flatnonzero(k_other == 1)[0])] == 0
            assert (reg.kinds() == 1).sum() == 1 and (reg.kinds() == 2).sum() == 1


def test_batch_validator_axis():
    """BatchValidator passes the flag on: foliation_classes(axis=True) and assign_foliation into a
    foliation_registry(axis=True) agree, the registry carries the flag and holds at most one leader
    of each axis kind; the default is unchanged."""
    from pdeval.batch import BatchValidator
    strings = FC.d3_strings(120) + ['rho**4', 'exp(rho**2)']
    h = len(strings) // 2
    bv = BatchValidator('force_free', device=0)
    try:
        cls, acc, tags = bv.foliation_classes(strings, axis=True)
        cls0, acc0, _ = bv.foliation_classes(strings)
        assert np.array_equal(acc, acc0) and cls.n_classes <= cls0.n_classes
        with bv.foliation_registry(axis=True) as reg:
            assert int(reg.params.flags) & AXIS
            c1, a1 = bv.assign_foliation(reg, strings[:h])
            c2, a2 = bv.assign_foliation(reg, strings[h:])
            assert np.array_equal(np.concatenate([a1, a2 + h]), acc)
            assert np.array_equal(np.concatenate([c1, c2]), cls.class_id)
            kinds = reg.kinds()
            assert (kinds == 1).sum() == 1 and (kinds == 2).sum() <= 1
            assert tags[int(np.flatnonzero(kinds == 1)[0])] == 'Vertical field'
        with bv.foliation_registry() as reg:
            assert int(reg.params.flags) == 0
            c1, _ = bv.assign_foliation(reg, strings[:h])
            c2, _ = bv.assign_foliation(reg, strings[h:])
            assert np.array_equal(np.concatenate([c1, c2]), cls0.class_id)
    finally:
        bv.close()


def test_kerr_context_is_an_argument_error():
    torch, dev = _torch()
    k = Context(1, device=0)
    try:
        buf = torch.zeros(256, dtype=torch.float64, device=dev)
        with pytest.raises(PdevalError, match='pdeval error 1.*force-free'):
            k.field_kinds(buf.data_ptr(), 1, buf.data_ptr(), _params(8, True))
        with pytest.raises(PdevalError, match='pdeval error 1.*force-free'):
            k.jacobian_match(buf.data_ptr(), 1, buf.data_ptr(), 1, buf.data_ptr(), params=_params(8, True))
        with pytest.raises(PdevalError, match='pdeval error 1.*force-free'):
            k.fol_registry(_params(8, True))
    finally:
        k.close()

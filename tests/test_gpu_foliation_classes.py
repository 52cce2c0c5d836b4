"""GPU tests of the gradient field kernel, pdeval_foliation_classes, the known-solution tag and
BatchValidator.foliation_classes against the oracle's fields and the numpy
restatement of the classes (tests/foliation_ref.py)."""
import numpy as np
import pytest

import foliation_cases as FC
import foliation_ref as R
from pdeval import foliation as FOL
from pdeval import problem_defs as P
from pdeval._lib import Context, PdevalError, default_fol_params
from pdeval.opcodes import CLS_ACCEPT

pytestmark = pytest.mark.gpu


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


def _upload(ops, off):
    torch, dev = _torch()
    return (torch.from_numpy(np.ascontiguousarray(ops, dtype=np.int32)).to(dev),
            torch.from_numpy(np.ascontiguousarray(off, dtype=np.int64)).to(dev))


@pytest.fixture(scope='module')
def resident():
    """F's programs resident on the device."""
    F = FC.field_set()
    d_ops, d_off = _upload(F['ops'], F['off'])
    return F, d_ops, d_off


def test_gradient_fields_match_oracle(ctx, resident):
    """F at m = 5, 9, 12 through a permuted list with n_list = 1, 5, len(F) (a block holds four
    waves: 1 and 5 rows leave a block tail at every m) and once without a list: the NaN mask, the
    5e-10 bound and n_finite against the oracle's fields."""
    F, d_ops, d_off = resident
    n = len(F['progs'])
    perm = np.random.default_rng(11).permutation(n)
    for m in FC.MS:
        want = F['fields'][m]
        for n_list in (1, 5, n):
            idx = perm[:n_list]
            got, nfin = FOL.gradient_fields(ctx, d_ops, int(d_ops.numel()), d_off, n, idx, _params(m))
            FC.check_fields(got.cpu().numpy(), nfin.cpu().numpy(), want[idx], f'gpu m={m} n_list={n_list}')
        got, nfin = FOL.gradient_fields(ctx, d_ops, int(d_ops.numel()), d_off, n, None, _params(m))
        FC.check_fields(got.cpu().numpy(), nfin.cpu().numpy(), want, f'gpu m={m} no list')
        assert np.isnan(got[-1].cpu().numpy()).all()          # the complex program


def test_gradient_fields_guard(ctx, resident):
    """Offsets outside [0, n_words] and list entries outside [0, n): all-NaN rows, n_finite 0,
    next to good rows (the words past n_words exist in the buffer but are never the program's)."""
    F, d_ops, _ = resident
    torch, dev = _torch()
    m = 9
    n_words = int(F['off'][3])                               # programs 0..2 only
    off = np.array([0, F['off'][1], F['off'][2], F['off'][3], F['off'][3] + 5, 2, -4, 7, 7], dtype=np.int64)
    d_off = torch.from_numpy(off).to(dev)
    n = len(off) - 1
    lst = np.array([1, -1, n, 2, 1 << 40, 0, 3, 4, 5, 6, 7], dtype=np.int64)
    got, nfin = FOL.gradient_fields(ctx, d_ops, n_words, d_off, n, lst, _params(m))
    got, nfin = got.cpu().numpy(), nfin.cpu().numpy()
    FC.check_fields(got[[0, 3, 5]], nfin[[0, 3, 5]], F['fields'][m][[1, 2, 0]], 'gpu guard')
    bad = [1, 2, 4, 6, 7, 8, 9, 10]
    assert np.isnan(got[bad]).all() and not nfin[bad].any()


@pytest.fixture(scope='module')
def small():
    """The 7 paper solutions, their re-parametrisations (MUST_MATCH), rho/z, rho/Abs(z) and the
    complex program: F's rows without the two extra programs, at m = 12."""
    F = FC.field_set()
    rows = list(range(len(FC.case_exprs(F['pd'])))) + [len(F['progs']) - 1]
    want, q, matched = R.sequential_leaders(F['fields'][12][rows])
    return F, np.array(rows, dtype=np.int64), want


def test_classes_small_case(ctx, resident, small):
    """pdeval_foliation_classes from programs: the restatement's sequential leaders on the
    oracle's fields, 7 classes, the complex row unclassified, one round."""
    F, d_ops, d_off = resident
    _, rows, want = small
    torch, dev = _torch()
    d_list = torch.from_numpy(rows).to(dev)
    torch.cuda.synchronize(dev)
    leader, ncls, rounds = ctx.foliation_classes(d_ops.data_ptr(), int(d_ops.numel()), d_off.data_ptr(),
                                                 len(F['progs']), d_list.data_ptr(), len(rows), _params(12))
    pos = np.where(want >= 0, rows[np.maximum(want, 0)], -1)      # leaders as candidate indices
    assert np.array_equal(leader, pos), (leader, pos)
    assert ncls == 7 and rounds == 1 and leader[-1] == -1
    assert leader[:7].tolist() == list(range(7))
    cls = FOL.classify(ctx, d_ops, int(d_ops.numel()), d_off, len(F['progs']), rows, _params(12))
    assert np.array_equal(cls.leader, pos) and cls.n_classes == 7 and cls.unclassified.tolist() == [len(rows) - 1]
    # without a list the rows are the candidates themselves
    k = len(rows) - 1                                             # the real rows: candidates 0 .. k-1
    lead0, ncls0, _ = ctx.foliation_classes(d_ops.data_ptr(), int(d_ops.numel()), d_off.data_ptr(), k, 0, k,
                                            _params(12))
    assert np.array_equal(lead0, want[:k]) and ncls0 == 7


N_D3 = 400


@pytest.fixture(scope='module')
def d3(ctx):
    """The 7 paper solutions and the first 400 rows of the validated depth-3 stream, validated on
    the device; the accepted rows' oracle fields at m = 16 and the restatement's leaders.  (On the
    oracle's classes the prefix gives 369 accepted rows, 199 classes, 6 rows unclassified: seven
    rounds of 32 probes.)"""
    from pdeval.native import compile_strings
    pd_ = P.force_free()
    strings = FC.d3_strings(N_D3)
    ops, off, _ = compile_strings(pd_, strings)
    acc = np.flatnonzero(ctx.validate(ops, off)['status'] == CLS_ACCEPT).astype(np.int64)
    fields = np.stack([R.oracle_field(ops[off[i]:off[i + 1]], 16) for i in acc])
    want, q, matched = R.sequential_leaders(fields)
    d_ops, d_off = _upload(ops, off)
    cls = FOL.classify(ctx, d_ops, int(d_ops.numel()), d_off, len(strings), acc)
    tags = FOL.tag_known(ctx, pd_, cls, (d_ops, int(d_ops.numel()), d_off, len(strings)))
    return dict(pd=pd_, strings=strings, acc=acc, fields=fields, want=want, q=q, cls=cls, tags=tags)


def test_classes_more_than_one_round(d3):
    """More than 32 classes: the device's leaders equal the restatement's on the oracle's fields of
    the same rows, in >= 2 rounds.  The condition the comparison rests on is asserted on the
    oracle's own numbers: no (row, earlier leader) pair has qmax in [1e-10, 1e-4]."""
    q, want, acc, cls = d3['q'], d3['want'], d3['acc'], d3['cls']
    assert not ((q >= 1e-10) & (q <= 1e-4)).any(), q[(q >= 1e-10) & (q <= 1e-4)]
    pos = np.where(want >= 0, acc[np.maximum(want, 0)], -1)
    assert len(set(want[want >= 0].tolist())) > 32
    assert np.array_equal(cls.leader, pos), np.flatnonzero(cls.leader != pos)[:10]
    assert cls.n_rounds >= 2 and cls.n_classes == len(set(want[want >= 0].tolist()))


def test_tags_matching_paper_solutions(d3):
    """The classes led by the six paper solutions that match themselves under the Jacobian test
    carry their names, rho/z lands in the Radial class, none of those names is given to two
    classes, and a class named Vertical field is led by rho**2's own field (the oracle's, to its
    rounding)."""
    cls, tags, acc, names = d3['cls'], d3['tags'], d3['acc'], list(d3['pd'].known_solutions.values())
    assert acc[:7].tolist() == list(range(7))
    for k in range(1, 7):
        assert cls.leader[k] == k and tags.get(int(cls.class_id[k])) == names[k], (k, names[k], tags)
    row = int(np.flatnonzero(acc == d3['strings'].index('rho/z', 7))[0])
    assert cls.leader[row] == 2 and tags[int(cls.class_id[row])] == 'Radial'
    # one class per name the Jacobian test decides; the further rows that are rho**2 itself, such
    # as square(rho), lead classes of their own (the limit of the definition) with the same name
    jac = [nm for nm in tags.values() if nm != names[0]]
    assert sorted(jac) == sorted(set(jac))
    f0 = d3['fields'][0]
    for c, nm in tags.items():
        if nm == names[0]:
            lead = int(np.flatnonzero(cls.class_id == c)[0])
            assert np.allclose(d3['fields'][lead], f0, rtol=1e-12, atol=0, equal_nan=True), d3['strings'][acc[lead]]


def test_tags_every_paper_solution(d3):
    """Every class led by a paper solution carries its name, all seven.

    'Vertical field' is rho**2, a function of rho alone: u_z = 0, so against itself both products
    of J vanish, S = 0, no point is usable and the Jacobian test does not match the field with
    itself (DESIGN.md §14 "A limit of the definition"; the restatement on the oracle's field gives
    n_used = 0 of 256 too).  Its class gets the name by tag_known's second rule: the leader's
    field equals the known solution's at every sample point."""
    cls, tags, names = d3['cls'], d3['tags'], list(d3['pd'].known_solutions.values())
    got = {names[k]: tags.get(int(cls.class_id[k])) for k in range(7)}
    print(got)
    assert all(got[nm] == nm for nm in names), got


def test_tag_by_equal_field_only(ctx):
    """The equal-field rule names rho**2 and nothing else: rho**4 is the same foliation but a
    leader of its own with no usable point against rho**2 (the limit of the definition), its
    field differs, and it stays untagged; with the leaders' fields given or computed alike."""
    from pdeval.native import compile_strings
    pd_ = P.force_free()
    strings = ['rho**4', 'rho**2', 'rho**2*z']
    ops, off, _ = compile_strings(pd_, strings)
    d_ops, d_off = _upload(ops, off)
    nw = int(d_ops.numel())
    cls = FOL.classify(ctx, d_ops, nw, d_off, 3, np.arange(3))
    assert cls.leader.tolist() == [0, 1, 2]
    want = {1: 'Vertical field', 2: 'X-point'}
    assert FOL.tag_known(ctx, pd_, cls, (d_ops, nw, d_off, 3)) == want
    fields, _ = FOL.gradient_fields(ctx, d_ops, nw, d_off, 3)
    assert FOL.tag_known(ctx, pd_, cls, fields) == want


def test_batch_validator_foliation_classes(small):
    """BatchValidator.foliation_classes on the strings of the small case: the rows the device
    accepts get the small case's leaders; a Kerr validator raises ValueError."""
    from pdeval.batch import BatchValidator
    F, rows, want = small
    strings = FC.case_exprs(F['pd'])
    bv = BatchValidator('force_free', device=0)
    try:
        cls, acc, tags = bv.foliation_classes(strings, _params(12))
    finally:
        bv.close()
    assert set(range(7)) <= set(acc.tolist())
    assert np.array_equal(cls.leader, want[acc]), (acc, cls.leader, want[acc])
    assert cls.n_classes == 7 and tags[2] == 'Radial' and tags[1] == 'X-point'
    kv = BatchValidator('kerr', device=0)
    try:
        with pytest.raises(ValueError, match='force-free'):
            kv.foliation_classes(['1 - x'])
    finally:
        kv.close()


def test_errors(ctx, resident):
    """A Kerr context, m = 3 and 65 and n_list < 0 are PDEVAL_ERR_ARG from both entry points;
    n_list = 0 is OK and launches nothing (null buffers are never touched)."""
    F, d_ops, d_off = resident
    torch, dev = _torch()
    n, nw = len(F['progs']), int(d_ops.numel())
    buf = torch.zeros(2 * 65 * 65, dtype=torch.float64, device=dev)
    k = Context(1, device=0)
    try:
        with pytest.raises(PdevalError, match='pdeval error 1.*force-free'):
            k.gradient_fields(d_ops.data_ptr(), nw, d_off.data_ptr(), n, 0, 1, buf.data_ptr(), params=_params(8))
        with pytest.raises(PdevalError, match='pdeval error 1.*force-free'):
            k.foliation_classes(d_ops.data_ptr(), nw, d_off.data_ptr(), n, 0, 1, _params(8))
    finally:
        k.close()
    for m in (3, 65):
        with pytest.raises(PdevalError, match='pdeval error 1'):
            ctx.gradient_fields(d_ops.data_ptr(), nw, d_off.data_ptr(), n, 0, 1, buf.data_ptr(), params=_params(m))
        with pytest.raises(PdevalError, match='pdeval error 1'):
            ctx.foliation_classes(d_ops.data_ptr(), nw, d_off.data_ptr(), n, 0, 1, _params(m))
    with pytest.raises(PdevalError, match='pdeval error 1'):
        ctx.gradient_fields(d_ops.data_ptr(), nw, d_off.data_ptr(), n, 0, -1, buf.data_ptr(), params=_params(8))
    with pytest.raises(PdevalError, match='pdeval error 1'):
        ctx.foliation_classes(d_ops.data_ptr(), nw, d_off.data_ptr(), n, 0, -1, _params(8))
    ctx.gradient_fields(0, 0, 0, 0, 0, 0, 0, params=_params(8))
    leader, ncls, rounds = ctx.foliation_classes(0, 0, 0, 0, 0, 0, _params(8))
    assert leader.size == 0 and ncls == 0 and rounds == 0

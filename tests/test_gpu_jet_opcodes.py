"""Every jet opcode on the device against the 50-digit Taylor coefficients of
tests/jet_opcode_cases.py: the jets and tier-2 error bounds of pdeval_eval_points, the four
precision tiers of pdeval_point_eval against the exact determinant at p*, and the grid kernels
through the oracle (which test_jet_opcodes_host.py anchors to the same reference)."""
import numpy as np
import pytest

import jet_opcode_cases as JC
import oracle_lib as O
from pdeval import _lib
from pdeval.opcodes import CLS_ZERO_GRADIENT, FLAG_COMPLEX, PDOP
from test_hostsim import sim  # noqa: F401  (the host build of the device source)
from test_jet_opcodes_host import _host_jets

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def gold():
    return JC.golden()


@pytest.fixture(scope='module')
def ctx(gold):          # (the reference is loaded before the context is opened)
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.fixture(scope='module')
def kappa():
    return float(_lib.default_params(0).noise_kappa)


@pytest.mark.parametrize('tier2', [False, True])
def test_device_jets_and_bounds(ctx, sim, gold, kappa, tier2):  # noqa: F811
    """Checks (a), (b), (c) on the device's jets and bounds at the 70 points (one full block of
    64 lanes and a partial one); the device's E within a factor 4 of the host build's."""
    stats, bad = JC.Stats(), []
    for ip, (name, w, flags, single, _) in enumerate(JC.programs()):
        if flags & FLAG_COMPLEX:
            continue
        out, jt = ctx.eval_points(w, JC.XS, JC.YS, tier2=tier2, jets=True)
        assert (out[:, 3] == 1.0).all(), (name, out[:, 3])
        JC.check_jets(name, w, gold.hi[ip], gold.lo[ip], jt[:, 0], jt[:, 1] if tier2 else None, kappa, single,
                      stats, bad)
        if tier2:
            _, eh = _host_jets(sim, w, 1)
            ed = jt[:, 1]
            if not ((ed <= 4 * eh) & (eh <= 4 * ed)).all():
                bad.append(('E device / host', name, float(ed.max()), float(eh.max())))
        else:
            assert not jt[:, 1].any(), name
    print('\n' + stats.table(f'device, tier2 = {int(tier2)}'))
    assert not bad, (len(bad), bad[:8])


def test_device_point_tiers(ctx, gold, kappa):
    """pdeval_point_eval in its four precisions against the exact determinant at p*."""
    bad = []
    for ip, (name, w, flags, _, true) in enumerate(JC.programs()):
        for tier in JC.tiers_of(flags):
            out, _ = ctx.point_eval(w, tier)
            JC.check_tier(name, tier, out[0], gold.det[ip], kappa, true, bad)
    assert not bad, (len(bad), bad[:8])


def test_device_double_double_tier_reads_the_low_part(ctx, gold, kappa):
    progs = JC.programs()
    for ip, det_twin in gold.det_twin.items():
        name, w = progs[ip][:2]
        a, b = ctx.point_eval(w, 2)[0][0], ctx.point_eval(JC.rounded_twin(w), 2)[0][0]
        lim = kappa * max(a[4], b[4])
        assert abs(det_twin - gold.det[ip]) > lim, (name, det_twin, gold.det[ip], lim)
        assert abs(a[0] - b[0]) > lim, (name, a, b)
        bad = []
        JC.check_tier(name + '.twin', 2, b, det_twin, kappa, False, bad)
        assert not bad, bad


def _grid_noise_over_scale(w, kappa, cplx):
    """max over the default 64 x 64 grid of noise_kappa * noise_p / S_p (the oracle's)."""
    gx = 0.05 + (np.arange(64) + 0.37) * (3.0 - 0.05) / 64
    gy = -2.0 + (np.arange(64) + 0.41) * (2.0 - -2.0) / 64
    m = 0.0
    for x in gx:
        for y in gy:
            _, S, noise, fin = O.point(0, w, float(x), float(y), cplx=cplx)
            if fin and S > 0:
                m = max(m, kappa * noise / S)
    return m


REPS = 9


@pytest.fixture(scope='module')
def grid_runs(ctx):
    """The whole table through one validate call with full_grid = 1, and the oracle's.  The table
    is repeated REPS times: the one-coordinate pass runs in full-batch launches only (one wave per
    candidate, more than 1024 candidates)."""
    progs = JC.programs() * REPS
    assert len(progs) > 1024
    ops = np.concatenate([w for _, w, *_ in progs])
    off = np.concatenate([[0], np.cumsum([len(w) for _, w, *_ in progs])]).astype(np.int64)
    prm = _lib.default_params(0)
    prm.full_grid = 1
    dev = ctx.validate(ops, off, prm)
    counts = ctx.pass_counts()
    return dev, O.validate(0, ops, off, prm=O.params(full_grid=1)), counts


def test_grid_kernels_match_the_oracle(grid_runs):
    """status, n_bad and n_nonfinite of the grid kernels equal the oracle's (which
    test_jet_opcodes_host.py anchors to the 50-digit reference) with no slack, and the table
    reached the stack-3, stack-8 and one-coordinate kernels.  The lean passes hand a program to
    the generic kernel by design when it holds POWN with n > 8 (the decoder's pown_lean rule):
    exactly those programs of the table are handed off, and no other."""
    dev, ora, counts = grid_runs
    names = JC.NAMES * REPS
    for key in ('status', 'n_bad', 'n_nonfinite'):
        diff = np.flatnonzero(dev[key] != ora[key])
        assert not len(diff), (key, [(names[i], int(dev[key][i]), int(ora[key][i])) for i in diff[:10]])
    big = [(int(w[0]) >> 8) & 0xff for _, w, *_ in JC.programs()
           if any(op == PDOP['POWN'] and (o & 0xff) > 8 for op, o, *_ in JC.decode(w))]
    assert sorted(big) == [1, 1, 3]
    assert counts['grid_slow'] == REPS * sum(d <= 2 for d in big), counts
    assert counts['grid_slow_stack3'] == REPS * sum(d == 3 for d in big), counts
    assert counts['grid_slow_complex'] == 0, counts
    assert counts['defer_stack3'] > 0 and counts['defer_stack8'] > 0 and counts['one_coord'] > 0, counts


def test_grid_q_matches_the_oracle(grid_runs, kappa):
    """|q_dev - q_oracle| <= max_p(noise_kappa noise_p / S_p) + 4 * 2^-52 q_oracle, but for the
    ZERO_GRADIENT programs.

    This test found the force-free q_grid up to 6.0e-9 (relative) from the oracle's on 48 programs
    ('mul': 0.799940494615816 against 0.7999404897815695): it was the maximum of |res| * rcp(S)
    with the bare hardware reciprocal.  GridMax<false> now takes one Newton step on the quotient
    (q_refined, pdeval_kernels.h)."""
    dev, ora, _ = grid_runs
    bad, worst = [], 0.0
    assert np.array_equal(dev['q_grid'][:len(JC.NAMES)], dev['q_grid'][-len(JC.NAMES):], equal_nan=True)
    for i, (name, w, flags, *_) in enumerate(JC.programs()):
        if ora['status'][i] == CLS_ZERO_GRADIENT:
            continue
        d, o = float(dev['q_grid'][i]), float(ora['q_grid'][i])
        if np.isfinite(d) and np.isfinite(o) and o > 0:
            worst = max(worst, abs(d - o) / o)
        lim = 4 * JC.EPS * o
        if not abs(d - o) <= lim:
            lim += _grid_noise_over_scale(w, kappa, bool(flags & FLAG_COMPLEX))   # (only where needed)
        if not abs(d - o) <= lim:
            bad.append((name, d, o, lim))
    print(f'\nq_grid: largest |q_dev - q_oracle| / q_oracle = {worst:.3e}, {len(bad)} programs beyond the bound')
    assert not bad, (len(bad), bad[:10])

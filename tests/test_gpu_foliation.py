"""GPU tests of the Jacobian match kernel of the foliation classes against the
numpy restatement (tests/foliation_ref.py) on gradient fields from the oracle's jets."""
import numpy as np
import pytest

import foliation_ref as R
from pdeval import problem_defs as P
from pdeval._lib import Context, PdevalError, default_fol_params

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    c = Context(0, device=0)
    yield c
    c.close()


@pytest.fixture(scope='module')
def pd_():
    return P.force_free()


def _params(m):
    p = default_fol_params()
    p.m = m
    return p


def _torch():
    import torch
    return torch, torch.device('cuda', 0)


@pytest.fixture(scope='module')
def fields12(pd_):
    """Oracle fields at m = 12 of the paper solutions and re-parametrisations, and mixtures."""
    exprs = list(pd_.known_solutions) + ['exp(rho**2*z)', 'sqrt(rho**2*z)', 'inv(rho**2*z)', 'rho/z', 'rho/Abs(z)',
                                         'exp_neg(sqrt(rho**2 + z**2) - z)']
    ops, off, _ = P.compile_strings(pd_, exprs)
    base = R.oracle_fields(ops, off, 12)
    rng = np.random.default_rng(5)
    rows = list(base)
    while len(rows) < 65:
        i, j = rng.choice(7, 2, replace=False)
        a, b = rng.uniform(0.5, 2.0, 2)
        rows.append(a * base[i] + b * base[j])
        rows.append(-2.5 * rows[-1])
    few = np.full_like(base[1], np.nan)        # a row with 10 finite points: n_used < min_points
    few[:, 40:50] = base[1][:, 40:50]
    return exprs, np.ascontiguousarray(np.stack(rows[:64] + [few]))


def _match(ctx, rows, probes, m, diagnostics=True):
    from pdeval.foliation import match_fields
    torch, dev = _torch()
    r = torch.from_numpy(np.ascontiguousarray(rows)).to(dev)
    p = torch.from_numpy(np.ascontiguousarray(probes)).to(dev)
    return match_fields(ctx, r, p, _params(m), diagnostics=diagnostics)


def _check_match(ctx, rows, probes, m=12):
    hit, used, qmax = _match(ctx, rows, probes, m)
    for i, row in enumerate(rows):
        nu, nb, q = R.pair_stats(row, probes)
        assert np.array_equal(used[i], nu), i
        assert np.array_equal(hit[i], (nu >= R.MIN_POINTS) & (nb == 0)), i
        big = q > 1e-300
        assert np.all(np.abs(qmax[i][big] - q[big]) <= 1e-9 * q[big]) and np.all(qmax[i][~big] <= 1e-300), i
    assert np.array_equal(_match(ctx, rows, probes, m, diagnostics=False), hit)   # the early-exit path
    return hit, used


def test_jacobian_match_65_rows_1_probe(ctx, fields12):
    exprs, f = fields12
    hit, used = _check_match(ctx, f, f[[1]])
    assert hit[1, 0] and hit[7, 0] and hit[8, 0] and hit[9, 0]        # rho**2*z and its f(u)
    assert not hit[0, 0] and not hit[2:7, 0].any()
    assert used[64, 0] == 10 and not hit[64, 0]                       # too few usable points: no match


def test_jacobian_match_1_row_32_probes(ctx, fields12):
    exprs, f = fields12
    hit, _ = _check_match(ctx, f[[8]], f[:32])
    assert hit[0].tolist() == [k in (1, 7, 8, 9) for k in range(32)]
    few_hit, few_used = _check_match(ctx, f[[64]], f[:32])
    assert not few_hit.any() and few_used.max() <= 10


def test_jacobian_match_33_probes_is_an_argument_error(ctx, fields12):
    torch, dev = _torch()
    f = torch.from_numpy(fields12[1][:33]).to(dev)
    mask = torch.zeros(33, dtype=torch.int32, device=dev)
    with pytest.raises(PdevalError, match='pdeval error 1'):
        ctx.jacobian_match(f.data_ptr(), 33, f.data_ptr(), 33, mask.data_ptr(), params=_params(12))
    ctx.jacobian_match(f.data_ptr(), 33, f.data_ptr(), 32, mask.data_ptr(), params=_params(12),
                       stream=torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)


def test_leader_rounds_on_device_masks(ctx, fields12):
    """Rounds of up to 32 probes over the device's masks (the rule of pdeval_foliation.h fol_round,
    restated here) give the restatement's sequential leaders on the 65 rows."""
    exprs, f = fields12
    want, q, matched = R.sequential_leaders(f)
    assert not ((q >= 1e-10) & (q <= 1e-4)).any()     # the reference's own margin
    leader = np.full(len(f), -1, dtype=np.int64)
    un = [i for i in range(len(f)) if np.isfinite(f[i][0]).sum() >= R.MIN_POINTS]
    rounds = 0
    while un:
        npb = min(32, len(un))
        hit = _match(ctx, f[un], f[un[:npb]], 12, diagnostics=False)
        leaders, nxt = [], []
        for r, row in enumerate(un):
            lk = [k for k in leaders if hit[r, k]]
            if lk:
                leader[row] = un[lk[0]]
            elif r < npb:
                leaders.append(r)
                leader[row] = row
            else:
                nxt.append(row)
        un, rounds = nxt, rounds + 1
    assert np.array_equal(leader, want) and rounds >= 2 and leader[64] == -1


def test_kerr_context_is_an_argument_error():
    torch, dev = _torch()
    k = Context(1, device=0)
    try:
        buf = torch.zeros(256, dtype=torch.float64, device=dev)
        with pytest.raises(PdevalError, match='pdeval error 1.*force-free'):
            k.jacobian_match(buf.data_ptr(), 1, buf.data_ptr(), 1, buf.data_ptr(), params=_params(8))
    finally:
        k.close()


def test_bad_parameters(ctx):
    torch, dev = _torch()
    buf = torch.zeros(2 * 65 * 65, dtype=torch.float64, device=dev)
    for m in (3, 65):
        with pytest.raises(PdevalError, match='pdeval error 1'):
            ctx.jacobian_match(buf.data_ptr(), 1, buf.data_ptr(), 1, buf.data_ptr(), params=_params(m))

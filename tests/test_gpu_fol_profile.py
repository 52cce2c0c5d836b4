"""GPU tests of the profiles (pdeval_fol_profile; DESIGN.md §14 "Profiles: psi(u) and the current") against
the rule of include/pdeval.h applied with mpmath at 40 digits to the same input doubles.  A deviation is
|got - ref| / scale, scale = the running sum of |increment| of the sum in question; for psi' it is exp(P)
times the scale of P, after an allowance of 2 ulp (the device library's exp is within 1 ulp; the rounding of
the reference to a double, rounded up).  Tolerance: 100x the largest deviation of a sequential fp64
restatement on the same table (a parallel scan associates differently), which the reference measures:
synthetic tables 3.0e-16 (m = 4), 5.0e-16 (12), 1.4e-15 (16), 1.2e-15 (23), 3.8e-15 (64), the device's own
tables 3.7e-16 to 8.4e-16; the device was measured at 2.0e-16 to 1.3e-15 (DESIGN.md has the table)."""
import math

import mpmath
import numpy as np
import pytest

import fol_reduce_ref as F
from pdeval import foliation as FOL
from pdeval import problem_defs as P
from pdeval._lib import Context, PdevalError, default_fol_params

pytestmark = pytest.mark.gpu

MIN_POINTS = 8
E2E = [F.RADIAL, f'exp({F.RADIAL})', F.BENT, 'rho**2']


def prm(m, min_points=MIN_POINTS):
    p = default_fol_params()
    p.m, p.min_points = m, min_points
    return p


def reference(table, min_points=MIN_POINTS):
    """The rule on every row of table [rows, 3, mm]: n, perm, the profile rounded to doubles, the scales of
    P, psi and Q, and 'f64', the largest deviation of the sequential fp64 restatement (printed)."""
    rows, _, mm = table.shape
    out = dict(n=np.zeros(rows, np.int32), perm=np.full((rows, mm), -1, np.int32),
               val=np.full((rows, 4, mm), np.nan), scale=np.zeros((rows, 3, mm)))
    f64 = np.full((rows, 4, mm), np.nan)
    with mpmath.workdps(40):
        for r, (u, kap, g) in enumerate(table):
            order = sorted((float(u[p]) + 0.0, int(p)) for p in np.flatnonzero(np.isfinite(table[r]).all(0)))
            out['n'][r] = len(order)
            if len(order) < min_points:
                continue
            s, sc = [mpmath.mpf(0)] * 3, [mpmath.mpf(0)] * 3       # P, psi, Q and their scales
            f, prev = [0.0, 0.0, 0.0], None
            for i, (ui, p) in enumerate(order):
                k, gg = float(kap[p]), float(g[p])
                if i:
                    u0, k0, g0, dp0, fdp0 = prev
                    d = mpmath.mpf(ui) - u0
                    inc = [(mpmath.mpf(k) + k0) * d / 2]
                    dp = mpmath.exp(s[0] + inc[0])
                    inc += [(dp + dp0) * d / 2, (gg * dp ** 2 + g0 * dp0 ** 2) * d / 2]
                    s = [a + b for a, b in zip(s, inc)]
                    sc = [a + abs(b) for a, b in zip(sc, inc)]
                    fd = ui - u0
                    f[0] += 0.5 * (k + k0) * fd
                    fdp = float(np.exp(f[0]))
                    f[1] += 0.5 * (fdp + fdp0) * fd
                    f[2] += 0.5 * (gg * fdp * fdp + g0 * fdp0 * fdp0) * fd
                else:
                    dp, fdp = mpmath.mpf(1), 1.0
                assert abs(s[0]) < 20
                prev = (ui, k, gg, dp, fdp)
                out['perm'][r, i] = p
                out['val'][r, :, i] = ui, float(dp), float(s[1]), float(s[2])
                out['scale'][r, :, i] = [float(x) for x in sc]
                f64[r, :, i] = ui, fdp, f[1], f[2]
    out['f64'] = deviation(out, f64)
    print(f'reference mm={mm}: sequential fp64 restatement {out["f64"]:.3e}')
    return out


def deviation(ref, got):
    """The largest scaled deviation of got [rows, 4, mm] (u, psi', psi, Q) from the reference; u, the NaN
    fill and an exact value at scale 0 are compared exactly (inf otherwise)."""
    val, sc = ref['val'], ref['scale']
    assert np.array_equal(got[:, 0], val[:, 0], equal_nan=True) and np.array_equal(np.isnan(got), np.isnan(val))
    scale = np.stack([val[:, 1] * sc[:, 0], sc[:, 1], sc[:, 2]], 1)
    allow = np.stack([2 * np.spacing(val[:, 1]), 0 * sc[:, 1], 0 * sc[:, 2]], 1)
    with np.errstate(invalid='ignore', divide='ignore'):
        excess = np.maximum(np.abs(got[:, 1:] - val[:, 1:]) - allow, 0.0)
        dev = np.where(excess > 0, excess / scale, 0.0)
    return float(np.nanmax(dev, initial=0.0))


def synthetic(m):
    """One table per m: shuffled / ascending / descending u, ties (half the row is -0.0 or +0.0), NaNs and
    an inf, kappa == +0.0, an all-NaN kappa, MIN_POINTS - 1 and MIN_POINTS valid points."""
    mm, rng = m * m, np.random.default_rng(m)
    u = rng.permutation(np.linspace(-1.5, 2.5, mm) + rng.uniform(-1e-3, 1e-3, mm))
    smooth = lambda x: np.stack([x, 2 * np.sin(3 * x) - 1, np.cos(2 * x) + 0.5 * x])     # noqa: E731
    rnd = lambda x: np.stack([x, rng.uniform(-1, 1, mm), rng.uniform(-1, 1, mm)])        # noqa: E731
    ties = rng.permutation(np.concatenate([np.where(rng.random(mm - mm // 2) < 0.5, -0.0, 0.0),
                                           rng.choice([-1.0, 0.5], mm // 2)]))
    holes = rnd(u)
    for q in range(3):
        holes[q, rng.choice(mm, max(1, mm // 10), replace=False)] = np.nan
    holes[1, np.flatnonzero(np.isfinite(holes).all(0))[0]] = np.inf
    flat = rnd(u)
    flat[1] = 0.0
    none = rnd(u)
    none[1] = np.nan
    few = [rnd(u), rnd(u)]
    for t, keep in zip(few, (MIN_POINTS - 1, MIN_POINTS)):
        t[2, rng.permutation(mm)[keep:]] = np.nan
    return np.ascontiguousarray(np.stack([smooth(u), smooth(np.sort(u)), smooth(np.sort(u)[::-1]), rnd(ties), holes,
                                          flat, none] + few))


def check(ref, prof, perm, n):
    """n, perm and the fill exactly; the values within 100x the fp64 restatement's deviation."""
    prof, perm, n = prof.cpu().numpy(), perm.cpu().numpy(), n.cpu().numpy()
    assert np.array_equal(n, ref['n']) and np.array_equal(perm, ref['perm'])
    dev = deviation(ref, prof)
    print(f'device {dev:.3e} (fp64 restatement {ref["f64"]:.3e})')
    assert dev <= 100 * ref['f64']
    return prof


@pytest.fixture(scope='module')
def bv():
    from pdeval.batch import BatchValidator
    v = BatchValidator('force_free', device=0)
    yield v
    v.close()


@pytest.mark.parametrize('m', (4, 12, 16, 23, 64))
def test_synthetic_tables(bv, m):
    """The kernel alone at every block shape: N = 64 (one wave), 256, 256 exactly, 1024 with padding, 4096."""
    import torch
    tab = synthetic(m)
    ref = reference(tab)
    assert ref['n'].tolist()[5:] == [m * m, 0, MIN_POINTS - 1, MIN_POINTS] and ref['n'][4] >= MIN_POINTS
    prof = check(ref, *FOL.profiles(bv.ctx, torch.from_numpy(tab).to('cuda:0'), prm(m)))
    assert (prof[5, 1] == 1.0).all()                                  # kappa == +0.0: psi' == 1 exactly
    u = prof[5, 0]
    assert np.abs(prof[5, 2] - (u - u[0])).max() <= 100 * ref['f64'] * (u[-1] - u[0])
    assert np.isnan(prof[6:8]).all()


@pytest.mark.parametrize('m', (12, 16))
def test_public_path(bv, m):
    """BatchValidator.reduction_profiles against the reference on the device's own table: Radial (vacuum,
    psi = u), exp(Radial) (psi' = u_0 / u), Bent (current), rho**2 (free: no profile), Radial at Omega = 1
    (current); a [K, rows, 3, m*m] table gives the bytes of the single calls."""
    p = prm(m, 16)
    single = []
    for w, rows, kinds in ((0, E2E, [F.VACUUM, F.VACUUM, F.CURRENT, F.FREE]), (1, E2E[:1], [F.CURRENT])):
        kind, prof, perm, n = bv.reduction_profiles(rows, omega=w, params=p)
        tab = bv.reduction_kinds(rows, omega=w, table=True, params=p)[3]
        assert kind.tolist() == kinds
        single.append(check(reference(tab.cpu().numpy(), 16), prof, perm, n))
    prof = single[0]
    u = prof[:2, 0]
    assert np.abs(prof[0, 1] - 1).max() <= 1e-9 and np.abs(prof[0, 2] - (u[0] - u[0, 0])).max() <= 1e-9
    print('exp(Radial): trapezoid against u_0 log(u / u_0):', np.abs(prof[1, 2] - u[1, 0] * np.log(u[1] / u[1, 0])).max())
    assert np.abs(prof[2, 1] - 1).max() <= 1e-9 and np.abs(prof[2, 3]).max() > 1e-3     # Bent: kappa ~ 0, Q not
    assert np.isnan(prof[3]).all() and np.abs(single[1][0, 3]).max() > 1e-3
    tab = bv.reduction_kinds(E2E[:1], omega=[0, 1], table=True, params=p)[3]
    multi = FOL.profiles(bv.ctx, tab, p)
    assert tuple(multi[0].shape) == (2, 1, 4, m * m) and tuple(multi[1].shape) == (2, 1, m * m)
    assert np.array_equal(multi[0].cpu().numpy()[:, 0].view(np.int64), np.stack([single[0][0], single[1][0]]).view(np.int64))


def test_bad_arguments(bv):
    """A Kerr context, m = 3, min_points = 0 and a NULL profile pointer return PDEVAL_ERR_ARG."""
    import torch
    tab = torch.zeros((1, 3, 16), dtype=torch.float64, device='cuda:0')
    kerr = Context(P.kerr().problem_id, device=0)
    with pytest.raises(PdevalError, match='pdeval error 1:'):
        FOL.profiles(kerr, tab, prm(4))
    kerr.close()
    out = torch.zeros((1, 4, 16), dtype=torch.float64, device='cuda:0')
    for p in (prm(3), prm(4, 0)):
        with pytest.raises(PdevalError, match='pdeval error 1:'):
            bv.ctx.fol_profile(tab.data_ptr(), 1, out.data_ptr(), params=p)
    with pytest.raises(PdevalError, match='pdeval error 1:'):
        bv.ctx.fol_profile(tab.data_ptr(), 1, 0, params=prm(4))

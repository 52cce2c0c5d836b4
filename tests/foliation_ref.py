"""A plain numpy restatement of the foliation-class test (include/pdeval.h) on the
CPU oracle's jets -- the reference of tests/test_foliation_host.py and tests/test_gpu_foliation.py.
Test infrastructure only."""
import numpy as np

import oracle_lib as O

FF_GRID = (0.05, 3.0, 64, -2.0, 2.0, 64, 0.37, 0.41)   # the force-free default grid (DESIGN.md "Grids")
TAU, MIN_POINTS = 1e-7, 16                              # pdeval_default_fol_params


def grid_points(m, grid=FF_GRID):
    """xs[i], ys[j] of the m x m sample grid: lo + (i + phase) * (hi - lo) / m."""
    i = np.arange(m, dtype=np.float64)
    xs = grid[0] + (i + grid[6]) * ((grid[1] - grid[0]) / m)
    ys = grid[3] + (i + grid[7]) * ((grid[4] - grid[3]) / m)
    return xs, ys


def oracle_field(words, m, grid=FF_GRID):
    """[2, m*m]: (u_rho, u_z) from the oracle's real jets, x index major; NaN where u or its
    gradient is not finite, and everywhere for a program the oracle's real pass declines."""
    xs, ys = grid_points(m, grid)
    f = np.full((2, m * m), np.nan)
    w = np.ascontiguousarray(words, dtype=np.int32)
    for i, x in enumerate(xs):
        for j, y in enumerate(ys):
            try:
                jet = O.jet(0, w, float(x), float(y))
            except ValueError:
                return np.full((2, m * m), np.nan)
            if np.all(np.isfinite(jet[:3])):
                f[:, i * m + j] = jet[1:3]
    return f


def oracle_fields(ops, off, m, grid=FF_GRID):
    ops = np.asarray(ops, dtype=np.int32)
    return np.stack([oracle_field(ops[off[i]:off[i + 1]], m, grid) for i in range(len(off) - 1)]) \
        if len(off) > 1 else np.zeros((0, 2, m * m))


def pair_stats(row, probes, tau=TAU):
    """One row field [2, mm] against probe fields [k, 2, mm]: (n_used[k], n_bad[k], qmax[k])."""
    a, b = row[0][None, :], row[1][None, :]
    c, d = probes[:, 0, :], probes[:, 1, :]
    with np.errstate(all='ignore'):
        ad, bc = a * d, b * c
        J = ad - bc
        S = np.abs(ad) + np.abs(bc)
        used = np.isfinite(J) & np.isfinite(S) & (S > 0)
        bad = used & (np.abs(J) > tau * S)
        q = np.where(used, np.abs(J) / np.where(used, S, 1.0), 0.0)
    return used.sum(axis=1), bad.sum(axis=1), q.max(axis=1) if q.shape[1] else np.zeros(len(probes))


def matches(row, probes, tau=TAU, min_points=MIN_POINTS):
    nu, nb, _ = pair_stats(row, probes, tau)
    return (nu >= min_points) & (nb == 0)


def sequential_leaders(fields, tau=TAU, min_points=MIN_POINTS):
    """The definition: in order, row i joins the first-created leader it matches and otherwise
    becomes a leader; -1 with fewer than min_points finite points.  Also returns the qmax of
    every (row, earlier leader) pair with enough usable points, and whether it matched."""
    n = len(fields)
    leader = np.full(n, -1, dtype=np.int64)
    leaders = []
    lf = np.zeros((0,) + fields.shape[1:])
    q_all, m_all = [], []
    for i in range(n):
        if np.isfinite(fields[i][0]).sum() < min_points:
            continue
        hit = np.zeros(0, bool)
        if leaders:
            nu, nb, q = pair_stats(fields[i], lf[:len(leaders)], tau)
            hit = (nu >= min_points) & (nb == 0)
            ok = nu >= min_points
            q_all.append(q[ok])
            m_all.append(hit[ok])
        if hit.any():
            leader[i] = leaders[int(np.argmax(hit))]
        else:
            leader[i] = i
            leaders.append(i)
            if len(leaders) > len(lf):
                lf = np.concatenate([lf, np.zeros((max(64, len(lf)),) + fields.shape[1:])])
            lf[len(leaders) - 1] = fields[i]
    q_all = np.concatenate(q_all) if q_all else np.zeros(0)
    m_all = np.concatenate(m_all) if m_all else np.zeros(0, bool)
    return leader, q_all, m_all

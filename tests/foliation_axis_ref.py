"""A plain numpy restatement of the foliation-class test with the axis rule (include/pdeval.h,
PDEVAL_FOL_AXIS; DESIGN.md §14 "The axis rule") and of the kind of a field -- the reference of
tests/test_foliation_axis_host.py and tests/test_gpu_foliation_axis.py.  With axis=False every
function is tests/foliation_ref.py's.  Test infrastructure only."""
import numpy as np

from foliation_ref import MIN_POINTS, TAU

# the expressions of the axis tests: functions of rho alone, of z alone, and generic ones
RHO_ONLY = ['rho', 'rho**2', 'rho**4', 'exp(rho**2)']
Z_ONLY = ['z', 'z**2', 'exp_neg(z)']
GENERIC = ['rho**2*z', 'exp(rho**2*z)', 'rho**2 + z**2']
EXPRS = RHO_ONLY + Z_ONLY + GENERIC
# the classes of EXPRS with the rule, as sets of positions
CLASSES_AXIS = [{0, 1, 2, 3}, {4, 5, 6}, {7, 8}, {9}]


def pair_stats(row, probes, tau=TAU, axis=False):
    """One row field [2, mm] against probe fields [k, 2, mm]: (n_used[k], n_bad[k], qmax[k]).
    axis: a point with S == 0 is usable, and never bad, when a, b, c, d are all finite and either
    b == 0, d == 0, a != 0, c != 0 or a == 0, c == 0, b != 0, d != 0; its q is 0."""
    a, b = row[0][None, :], row[1][None, :]
    c, d = probes[:, 0, :], probes[:, 1, :]
    with np.errstate(all='ignore'):
        ad, bc = a * d, b * c
        J = ad - bc
        S = np.abs(ad) + np.abs(bc)
        used = np.isfinite(J) & np.isfinite(S) & (S > 0)
        bad = used & (np.abs(J) > tau * S)
        q = np.where(used, np.abs(J) / np.where(used, S, 1.0), 0.0)
        if axis:
            fin = np.isfinite(a) & np.isfinite(b) & np.isfinite(c) & np.isfinite(d)
            along_rho = (b == 0) & (d == 0) & (a != 0) & (c != 0)
            along_z = (a == 0) & (c == 0) & (b != 0) & (d != 0)
            extra = ~used & (S == 0) & fin & (along_rho | along_z)
            used = used | extra
    return used.sum(axis=1), bad.sum(axis=1), q.max(axis=1) if q.shape[1] else np.zeros(len(probes))


def matches(row, probes, tau=TAU, min_points=MIN_POINTS, axis=False):
    nu, nb, _ = pair_stats(row, probes, tau, axis)
    return (nu >= min_points) & (nb == 0)


def sequential_leaders(fields, tau=TAU, min_points=MIN_POINTS, axis=False):
    """The definition: in order, row i joins the first-created leader it matches and otherwise
    becomes a leader; -1 with fewer than min_points finite points."""
    n = len(fields)
    leader = np.full(n, -1, dtype=np.int64)
    leaders = []
    for i in range(n):
        if np.isfinite(fields[i][0]).sum() < min_points:
            continue
        hit = matches(fields[i], fields[leaders], tau, min_points, axis) if leaders else np.zeros(0, bool)
        if hit.any():
            leader[i] = leaders[int(np.argmax(hit))]
        else:
            leader[i] = i
            leaders.append(i)
    return leader


def class_ids(leader):
    """Dense class ids in order of creation from a leader array (-1 stays -1)."""
    ids = np.full(len(leader), -1, dtype=np.int64)
    seen = {}
    for i, l in enumerate(leader):
        if l >= 0:
            ids[i] = seen.setdefault(int(l), len(seen))
    return ids


def kinds(fields, min_points=MIN_POINTS):
    """uint8[n]: 1 iff u_z == 0 at every finite point (u_rho and u_z both finite) and u_rho != 0 at
    >= min_points of them; 2 the mirror image; 0 otherwise."""
    a, b = fields[:, 0, :], fields[:, 1, :]
    fin = np.isfinite(a) & np.isfinite(b)
    anz, bnz = fin & (a != 0), fin & (b != 0)
    k1 = (bnz.sum(axis=1) == 0) & ((anz & ~bnz).sum(axis=1) >= min_points)
    k2 = (anz.sum(axis=1) == 0) & ((bnz & ~anz).sum(axis=1) >= min_points)
    return np.where(k1, 1, np.where(k2, 2, 0)).astype(np.uint8)

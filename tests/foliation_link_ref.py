"""A plain numpy restatement of the links and components of the foliation classes
(include/pdeval.h, PDEVAL_FOL_LINK; DESIGN.md §14 "Links and components") on top of
tests/foliation_ref.py / foliation_axis_ref.py -- the reference of tests/test_foliation_link_host.py
and tests/test_gpu_foliation_link.py.  Rows are taken one at a time, so the result cannot depend
on how a list is cut into batches.  Test infrastructure only."""
import numpy as np

import foliation_axis_ref as A
from foliation_ref import MIN_POINTS, TAU


def components(n_classes, links):
    """int64[n_classes]: the smallest class id of each class's connected component under `links`
    (pairs of class ids), by repeated relabelling -- no union-find, on purpose."""
    comp = np.arange(n_classes, dtype=np.int64)
    changed = True
    while changed:
        changed = False
        for a, b in links:
            lo = min(comp[a], comp[b])
            if comp[a] != lo or comp[b] != lo:
                comp[comp == comp[a]] = lo
                comp[comp == comp[b]] = lo
                changed = True
    return comp


class LinkRef:
    """A registry restated: the leaders' fields in creation order, the class sizes and the links
    as a set of (lo, hi) pairs."""

    def __init__(self, tau=TAU, min_points=MIN_POINTS, axis=False, link=True):
        self.tau, self.min_points, self.axis, self.link = tau, min_points, axis, link
        self.leaders, self.sizes, self.links = [], [], set()

    @property
    def n_classes(self):
        return len(self.leaders)

    def _hits(self, row):
        if not self.leaders:
            return np.zeros(0, bool)
        return A.matches(row, np.stack(self.leaders), self.tau, self.min_points, self.axis)

    def assign(self, fields):
        """The sequential leader rule with the arrival rule: row r joins the first leader it
        matches among those that exist when it arrives, class c, and (link) every other such
        leader l it matches gives the link {c, l}; a row that matches none becomes a leader and
        gives no link; a row with fewer than min_points finite points gets -1 and gives none."""
        ids = np.full(len(fields), -1, dtype=np.int64)
        for r, row in enumerate(fields):
            if np.isfinite(row[0]).sum() < self.min_points:
                continue
            hit = np.flatnonzero(self._hits(row))
            if hit.size == 0:
                self.leaders.append(np.array(row))
                self.sizes.append(1)
                ids[r] = len(self.leaders) - 1
                continue
            c = int(hit[0])
            ids[r] = c
            self.sizes[c] += 1
            if self.link:
                self.links |= {(c, int(l)) for l in hit[1:]}
        return ids

    def link_fields(self, fields, ids):
        """Rows with their class ids against all current leaders: {ids[r], l} for every leader
        l != ids[r] that row r matches.  Returns the number of new links."""
        before = len(self.links)
        for row, c in zip(fields, ids):
            if c < 0:
                continue
            for l in np.flatnonzero(self._hits(row)):
                if int(l) != int(c):
                    self.links.add((min(int(c), int(l)), max(int(c), int(l))))
        return len(self.links) - before

    def merge(self, other):
        """other's leaders assigned here in their order (sizes carried over), its links mapped
        through the returned id map; a link whose ends land in one class is dropped."""
        ids = self.assign(other.leaders) if other.leaders else np.zeros(0, dtype=np.int64)
        for k, c in enumerate(ids):
            self.sizes[int(c)] += other.sizes[k] - 1
        for a, b in other.links:
            x, y = int(ids[a]), int(ids[b])
            if x != y:
                self.links.add((min(x, y), max(x, y)))
        return ids

    def sorted_links(self):
        return np.array(sorted(self.links), dtype=np.int64).reshape(-1, 2)

    def components(self):
        return components(self.n_classes, sorted(self.links))


def masked(field, keep):
    """`field` [2, mm] with NaN at the points where `keep` (bool[mm]) is False."""
    out = np.array(field, dtype=np.float64)
    out[:, ~np.asarray(keep, dtype=bool)] = np.nan
    return out

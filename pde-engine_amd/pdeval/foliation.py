"""Foliation classes of force-free candidates: the Jacobian match.

A force-free solution is a foliation -- the level sets of ``u`` -- so every ``f(u)`` is the same
solution.  Two candidates belong to one class iff ``J = u_rho v_z - u_z v_rho`` vanishes on an
``m x m`` sample grid (``include/pdeval.h``, ``pdeval_fol_params``).  :func:`match_fields` runs
that test on the device for gradient fields the caller supplies; :func:`classes_from_leader`
turns a leader array into dense class ids and sizes.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np

from ._lib import FOL_MAX_PROBES, FolParams, default_fol_params


@dataclass
class FoliationClasses:
    leader: np.ndarray        # int64[n_rows]: index of the row's class leader, -1 unclassified
    class_id: np.ndarray      # int64[n_rows]: dense class id in order of creation, -1 unclassified
    sizes: np.ndarray         # int64[n_classes]: rows per class
    unclassified: np.ndarray  # positions of the rows with leader -1

    @property
    def n_classes(self) -> int:
        return int(self.sizes.size)


def classes_from_leader(leader: np.ndarray) -> FoliationClasses:
    """Dense ids, sizes and the unclassified rows of a leader array.  A leader precedes its
    members in list order, so first appearance is the order of creation."""
    leader = np.asarray(leader, dtype=np.int64)
    cls = np.full(leader.shape, -1, dtype=np.int64)
    ok = leader >= 0
    uniq, first, inv = np.unique(leader[ok], return_index=True, return_inverse=True)
    rank = np.empty(uniq.size, dtype=np.int64)
    rank[np.argsort(first, kind='stable')] = np.arange(uniq.size)
    cls[ok] = rank[inv]
    sizes = np.bincount(cls[ok], minlength=uniq.size).astype(np.int64)
    return FoliationClasses(leader, cls, sizes, np.flatnonzero(~ok))


def match_fields(ctx, rows, probes, params: Optional[FolParams] = None, diagnostics: bool = False):
    """bool[n_rows, n_probes] of row fields against probe fields (torch float64 tensors
    [., 2, m*m] on ``ctx``'s device), 32 probes per ``pdeval_jacobian_match`` launch; with
    ``diagnostics`` also n_used (int32) and qmax (float64) of the same shape."""
    import torch
    prm = params if params is not None else default_fol_params()
    dev = rows.device
    rows = rows.contiguous()
    nr, npb = int(rows.shape[0]), int(probes.shape[0])
    hit = np.zeros((nr, npb), dtype=bool)
    used = np.zeros((nr, npb), dtype=np.int32)
    qmax = np.zeros((nr, npb))
    st = torch.cuda.Stream(dev)
    st.wait_stream(torch.cuda.current_stream(dev))
    for k0 in range(0, npb, FOL_MAX_PROBES):
        k1 = min(npb, k0 + FOL_MAX_PROBES)
        if nr == 0:
            break
        with torch.cuda.stream(st):
            mask = torch.zeros(nr, dtype=torch.int32, device=dev)
            nu = torch.zeros((nr, k1 - k0), dtype=torch.int32, device=dev) if diagnostics else None
            qm = torch.zeros((nr, k1 - k0), dtype=torch.float64, device=dev) if diagnostics else None
            pr = probes[k0:k1].contiguous()
            ctx.jacobian_match(rows.data_ptr(), nr, pr.data_ptr(), k1 - k0, mask.data_ptr(),
                               nu.data_ptr() if diagnostics else 0, qm.data_ptr() if diagnostics else 0, prm,
                               st.cuda_stream)
        st.synchronize()
        bits = mask.cpu().numpy().view(np.uint32)
        hit[:, k0:k1] = (bits[:, None] >> np.arange(k1 - k0, dtype=np.uint32)[None, :]) & 1
        if diagnostics:
            used[:, k0:k1] = nu.cpu().numpy()
            qmax[:, k0:k1] = qm.cpu().numpy()
    return (hit, used, qmax) if diagnostics else hit

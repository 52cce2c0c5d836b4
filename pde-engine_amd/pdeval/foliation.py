"""Foliation classes of force-free candidates: the Jacobian match.

A force-free solution is a foliation -- the level sets of ``u`` -- so every ``f(u)`` is the same
solution.  Two candidates belong to one class iff ``J = u_rho v_z - u_z v_rho`` vanishes on an
``m x m`` sample grid (``include/pdeval.h``, ``pdeval_fol_params``).  :func:`classify` builds the
classes of accepted candidates from programs resident on the device (fields, matches and rounds
stay there), :func:`tag_known` names the classes that are re-parametrisations of a paper
solution, :func:`gradient_fields` returns the fields themselves, :func:`match_fields` runs the
test on fields the caller holds and :func:`classes_from_leader` turns a leader array into dense
class ids and sizes.
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
    n_rounds: int = 0         # device rounds that built the classes (classify), else 0

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


def _ptr(t) -> int:
    """The device address of a torch tensor, or the integer address itself."""
    return int(t.data_ptr()) if hasattr(t, 'data_ptr') else int(t)


def _device(ctx):
    import torch
    return torch.device('cuda', ctx.device)


def gradient_fields(ctx, d_ops, n_words: int, d_offsets, n: int, idx=None, params: Optional[FolParams] = None):
    """(fields, n_finite): the torch float64 [n_rows, 2, m*m] gradient fields and int32 [n_rows]
    finite counts, on ``ctx``'s device, of the candidates ``idx`` (None: all ``n``) of the resident
    programs ``d_ops`` / ``d_offsets`` (torch tensors or device addresses)."""
    import torch
    prm = params if params is not None else default_fol_params()
    dev = _device(ctx)
    rows = n if idx is None else len(idx)
    mm = int(prm.m) * int(prm.m)
    st = torch.cuda.Stream(dev)
    st.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(st):
        d_list = None if idx is None else torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int64)).to(dev)
        field = torch.empty((rows, 2, mm), dtype=torch.float64, device=dev)
        nfin = torch.zeros(rows, dtype=torch.int32, device=dev)
        ctx.gradient_fields(_ptr(d_ops), n_words, _ptr(d_offsets), n, 0 if d_list is None else d_list.data_ptr(),
                            rows, field.data_ptr(), nfin.data_ptr(), prm, st.cuda_stream)
    st.synchronize()
    return field, nfin


def classify(ctx, d_ops, n_words: int, d_offsets, n: int, accepted_idx,
             params: Optional[FolParams] = None) -> FoliationClasses:
    """The foliation classes of the candidates ``accepted_idx`` of the programs resident on
    ``ctx``'s device (``d_ops`` / ``d_offsets``: torch tensors or device addresses), by
    ``pdeval_foliation_classes``: fields, matches and rounds on the device, only the masks come
    back.  ``leader`` holds candidate indices (entries of ``accepted_idx``); ``n_rounds`` is set
    on the result."""
    import torch
    dev = _device(ctx)
    idx = np.ascontiguousarray(accepted_idx, dtype=np.int64)
    d_list = torch.from_numpy(idx).to(dev)
    torch.cuda.current_stream(dev).synchronize()   # (the call runs on the context's own stream)
    leader, _, rounds = ctx.foliation_classes(_ptr(d_ops), n_words, _ptr(d_offsets), n, d_list.data_ptr(),
                                              len(idx), params)
    cls = classes_from_leader(leader)
    cls.n_rounds = rounds
    return cls


def tag_known(ctx, pd_, classes: FoliationClasses, fields_or_programs, params: Optional[FolParams] = None):
    """The known-solution tag: {class_id: name} of the classes whose leader matches one of
    ``pd_.known_solutions``.  The known solutions are compiled and their fields computed by the
    field kernel; every class leader's field is matched against them with ``jacobian_match``.
    ``fields_or_programs`` supplies the leaders' fields: either the torch float64 [n_rows, 2, m*m]
    fields of the classified rows (row order of ``classes``), or the tuple ``(d_ops, n_words,
    d_offsets, n)`` of the resident programs ``classes.leader`` indexes, whose leader fields are
    then computed here.  A leader whose field equals a known solution's at every sample point (the
    same finite points, the same values) matches it too: equal gradients are the same ``u`` up to
    a constant, and the Jacobian test alone cannot say so for a function of one coordinate, which
    has no usable point against itself (``rho**2``, the Vertical field).  A class
    that matches two names is reported under the first of them in the order of the
    ``pd_.known_solutions`` dictionary."""
    import torch
    from . import problem_defs as P
    prm = params if params is not None else default_fol_params()
    dev = _device(ctx)
    if classes.n_classes == 0:
        return {}
    # a leader precedes its members: the first row of each class is its leader
    ok = np.flatnonzero(classes.class_id >= 0)
    _, first = np.unique(classes.class_id[ok], return_index=True)
    lead_rows = ok[first]
    if isinstance(fields_or_programs, tuple):
        d_ops, n_words, d_offsets, n = fields_or_programs
        lead_fields, _ = gradient_fields(ctx, d_ops, n_words, d_offsets, n, classes.leader[lead_rows], prm)
    else:
        lead_fields = fields_or_programs[torch.from_numpy(lead_rows).to(dev)].contiguous()
    names = list(pd_.known_solutions.values())
    ops, off, _ = P.compile_strings(pd_, list(pd_.known_solutions))
    k_ops = torch.from_numpy(np.ascontiguousarray(ops, dtype=np.int32)).to(dev)
    k_off = torch.from_numpy(np.ascontiguousarray(off, dtype=np.int64)).to(dev)
    known_fields, _ = gradient_fields(ctx, k_ops, int(k_ops.numel()), k_off, len(names), None, prm)
    hit = match_fields(ctx, lead_fields, known_fields, prm)
    for k in range(len(names)):
        kf = known_fields[k]
        if bool(torch.isfinite(kf).any()):
            same = (lead_fields == kf) | (torch.isnan(lead_fields) & torch.isnan(kf))
            hit[:, k] |= same.flatten(1).all(1).cpu().numpy()
    return {int(c): names[int(np.argmax(hit[c]))] for c in range(len(lead_rows)) if hit[c].any()}

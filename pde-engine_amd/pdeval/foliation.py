"""Foliation classes of force-free candidates: the Jacobian match.

A force-free solution is a foliation -- the level sets of ``u`` -- so every ``f(u)`` is the same
solution.  Two candidates belong to one class iff ``J = u_rho v_z - u_z v_rho`` vanishes on an
``m x m`` sample grid (``include/pdeval.h``, ``pdeval_fol_params``).  :func:`classify` builds the
classes of accepted candidates from programs resident on the device (fields, matches and rounds
stay there), :func:`tag_known` names the classes that are re-parametrisations of a paper
solution, :func:`gradient_fields` returns the fields themselves, :func:`match_fields` runs the
test on fields the caller holds and :func:`classes_from_leader` turns a leader array into dense
class ids and sizes.  :class:`FoliationRegistry` keeps the classes across batches: the leaders'
fields stay on the device and every batch of a stream is assigned against them.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np

from ._lib import FOL_AXIS, FOL_LINK, FOL_MAX_PROBES, FolParams, default_fol_params, fol_params  # noqa: F401


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


def field_kinds(ctx, fields, params: Optional[FolParams] = None) -> np.ndarray:
    """uint8[n_rows]: 1 for a row whose field is that of a function of ``rho`` alone (``u_z == 0`` at
    every finite point, ``u_rho != 0`` at ``min_points`` of them or more), 2 for a function of ``z``
    alone, 0 otherwise (``pdeval_field_kinds``).  ``fields``: a torch float64 tensor [rows, 2, m*m]
    on ``ctx``'s device.  Does not depend on ``params.flags``."""
    import torch
    prm = params if params is not None else default_fol_params()
    dev = _device(ctx)
    mm = int(prm.m) ** 2
    if fields.dtype != torch.float64 or fields.dim() != 3 or tuple(fields.shape[1:]) != (2, mm) or fields.device != dev:
        raise ValueError(f'fields: expected a float64 tensor [rows, 2, {mm}] on {dev}')
    fields = fields.contiguous()
    rows = int(fields.shape[0])
    st = torch.cuda.Stream(dev)
    st.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(st):
        kind = torch.zeros(rows, dtype=torch.uint8, device=dev)
        if rows:
            ctx.field_kinds(fields.data_ptr(), rows, kind.data_ptr(), prm, st.cuda_stream)
    st.synchronize()
    return kind.cpu().numpy()


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
    then computed here.  With ``FOL_AXIS`` in ``params.flags`` the match includes the axis rule, and
    the Vertical field (``rho**2``) is found by it.  A leader whose field equals a known solution's at every sample point (the
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


class FoliationRegistry:
    """The foliation classes of a stream of batches (``pdeval_fol_registry_*``, DESIGN.md §14
    "Registry"): the class leaders' gradient fields stay resident on ``ctx``'s device, a batch is
    assigned against them in one pass, new leaders are appended and class ids -- dense int64 in
    order of creation -- never change.  Assigning a list in any number of consecutive batches
    gives the class ids :func:`classify` gives on the whole list.  Without ``FOL_AXIS`` in the
    flags of ``params`` a function of one coordinate matches nothing, not even itself, so each such
    row is a leader; with it they form one class per axis.  Calls are synchronous, on the context's stream; close the registry before its
    context.

    The match is not transitive, so two classes can hold the same foliation: their leaders share
    too few finite points to match each other while a row that covers both matches both.  With
    ``FOL_LINK`` in the flags every assigned row also records a link between its class and every
    other leader it matches among those that existed when it arrived; :meth:`link_fields` does the
    same against all current leaders for rows the caller still holds, with or without the flag.
    :meth:`components` joins the linked classes; ids, sizes and leaders never depend on it."""

    def __init__(self, ctx, params: Optional[FolParams] = None, capacity_hint: int = 0):
        import ctypes as C
        from ._lib import _check
        self.ctx, self.lib = ctx, ctx.lib
        self.h = C.c_void_p()
        _check(ctx.h, self.lib.pdeval_fol_registry_create(ctx.h, C.byref(params) if params is not None else None,
                                                          int(capacity_hint), C.byref(self.h)))
        self.params = FolParams()
        grid = np.zeros(8)
        _check(ctx.h, self.lib.pdeval_fol_registry_info(self.h, C.byref(self.params), grid.ctypes.data, None))
        self.grid = grid
        self.mm = int(self.params.m) ** 2

    # ---- lifetime
    def close(self):
        if getattr(self, 'h', None):
            self.lib.pdeval_fol_registry_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            if self.ctx.h:          # (a closed context has released the device already)
                self.close()
        except Exception:
            pass

    def _call(self, rc):
        from ._lib import _check
        _check(self.ctx.h, rc)

    @staticmethod
    def _keys(keys, n):
        if keys is None:
            return None
        k = np.ascontiguousarray(keys, dtype=np.int64)
        if k.shape != (n,):
            raise ValueError(f'keys: expected {n} entries, got shape {k.shape}')
        return k

    # ---- assignment
    def assign(self, d_ops, n_words: int, d_offsets, n: int, idx, keys=None) -> np.ndarray:
        """int64 class ids of the candidates ``idx`` of the programs resident on the device
        (``d_ops`` / ``d_offsets``: torch tensors or device addresses), -1 for a row with too few
        finite points.  ``keys``: the caller's identifier of each row (kept for new leaders);
        None = the running row number over all calls."""
        import ctypes as C
        import torch
        dev = _device(self.ctx)
        idx = np.ascontiguousarray(idx, dtype=np.int64)
        keys = self._keys(keys, len(idx))
        d_list = torch.from_numpy(idx).to(dev)
        torch.cuda.current_stream(dev).synchronize()   # (the call runs on the context's own stream)
        cls = np.full(len(idx), -1, dtype=np.int64)
        n_new = C.c_int64(0)
        self._call(self.lib.pdeval_fol_registry_assign(
            self.ctx.h, self.h, _ptr(d_ops) or None, n_words, _ptr(d_offsets) or None, n, d_list.data_ptr() or None,
            len(idx), None if keys is None else keys.ctypes.data, cls.ctypes.data, C.byref(n_new)))
        self.last_new = int(n_new.value)
        return cls

    def assign_fields(self, fields, n_finite=None, keys=None) -> np.ndarray:
        """The same on fields the caller holds: a torch float64 tensor [rows, 2, m*m] on the
        context's device (and optionally the int32 finite counts ``gradient_fields`` returns)."""
        import ctypes as C
        import torch
        dev = _device(self.ctx)
        if fields.dtype != torch.float64 or fields.dim() != 3 or tuple(fields.shape[1:]) != (2, self.mm) \
                or fields.device != dev:
            raise ValueError(f'fields: expected a float64 tensor [rows, 2, {self.mm}] on {dev}')
        fields = fields.contiguous()
        rows = int(fields.shape[0])
        keys = self._keys(keys, rows)
        nf = None
        if n_finite is not None:
            nf = n_finite.to(device=dev, dtype=torch.int32).contiguous()
            if tuple(nf.shape) != (rows,):
                raise ValueError(f'n_finite: expected {rows} entries')
        torch.cuda.current_stream(dev).synchronize()
        cls = np.full(rows, -1, dtype=np.int64)
        n_new = C.c_int64(0)
        self._call(self.lib.pdeval_fol_registry_assign_fields(
            self.ctx.h, self.h, fields.data_ptr() or None, None if nf is None else nf.data_ptr(), rows,
            None if keys is None else keys.ctypes.data, cls.ctypes.data, C.byref(n_new)))
        self.last_new = int(n_new.value)
        return cls

    # ---- links and components
    def link_fields(self, fields, class_ids) -> int:
        """Tests ``fields`` (a torch float64 tensor [rows, 2, m*m] on the context's device) against
        all current leaders and adds the link ``{class_ids[r], l}`` for every leader ``l`` other
        than its own that row ``r`` matches (``class_ids``: what ``assign`` returned for these rows;
        -1 skips the row).  Returns the number of links that were not known before."""
        import ctypes as C
        import torch
        dev = _device(self.ctx)
        if fields.dtype != torch.float64 or fields.dim() != 3 or tuple(fields.shape[1:]) != (2, self.mm) \
                or fields.device != dev:
            raise ValueError(f'fields: expected a float64 tensor [rows, 2, {self.mm}] on {dev}')
        fields = fields.contiguous()
        rows = int(fields.shape[0])
        ids = np.ascontiguousarray(class_ids, dtype=np.int64)
        if ids.shape != (rows,):
            raise ValueError(f'class_ids: expected {rows} entries, got shape {ids.shape}')
        torch.cuda.current_stream(dev).synchronize()
        n_new = C.c_int64(0)
        self._call(self.lib.pdeval_fol_registry_link_fields(self.ctx.h, self.h, fields.data_ptr() or None,
                                                            ids.ctypes.data, rows, C.byref(n_new)))
        return int(n_new.value)

    def _components(self):
        import ctypes as C
        comp = np.zeros(self.n_classes, dtype=np.int64)
        nc, nl = C.c_int64(0), C.c_int64(0)
        self._call(self.lib.pdeval_fol_registry_components(self.h, comp.ctypes.data, C.byref(nc), C.byref(nl)))
        return comp, int(nc.value), int(nl.value)

    def components(self) -> np.ndarray:
        """int64[n_classes]: the smallest class id of each class's component (the classes joined by
        links, directly or through others).  Without links every class is its own component."""
        return self._components()[0]

    @property
    def n_components(self) -> int:
        return self._components()[1]

    @property
    def n_links(self) -> int:
        return self._components()[2]

    def links(self) -> np.ndarray:
        """int64[n_links, 2]: the links, sorted, deduplicated, the smaller class id first."""
        edges = np.zeros((self.n_links, 2), dtype=np.int64)
        self._call(self.lib.pdeval_fol_registry_links(self.h, edges.ctypes.data))
        return edges

    def component_sizes(self) -> dict:
        """{component_id: rows}: the class sizes summed per component."""
        comp, sizes = self.components(), self.sizes
        return {int(c): int(sizes[comp == c].sum()) for c in np.unique(comp)}

    @property
    def link_ms(self) -> float:
        """Device time of the link kernel's launches in the most recent assign or link_fields call."""
        import ctypes as C
        ms = C.c_double(0.0)
        self._call(self.lib.pdeval_fol_registry_link_ms(self.h, C.byref(ms)))
        return float(ms.value)

    # ---- what the registry holds
    def _size(self):
        import ctypes as C
        a, b = C.c_int64(0), C.c_int64(0)
        self._call(self.lib.pdeval_fol_registry_size(self.h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    @property
    def n_classes(self) -> int:
        return self._size()[0]

    @property
    def rows_seen(self) -> int:
        return self._size()[1]

    def _host(self):
        L = self.n_classes
        keys, sizes = np.zeros(L, dtype=np.int64), np.zeros(L, dtype=np.int64)
        self._call(self.lib.pdeval_fol_registry_leaders(self.h, None, keys.ctypes.data, sizes.ctypes.data))
        return keys, sizes

    @property
    def sizes(self) -> np.ndarray:
        return self._host()[1]

    @property
    def leader_keys(self) -> np.ndarray:
        return self._host()[0]

    @property
    def stage_a_ms(self) -> float:
        """Device time of Stage A's launch in the most recent assign call (0 if it ran none)."""
        import ctypes as C
        ms = C.c_double(0.0)
        self._call(self.lib.pdeval_fol_registry_info(self.h, None, None, C.byref(ms)))
        return float(ms.value)

    def kinds(self) -> np.ndarray:
        """uint8[n_classes]: :func:`field_kinds` of the leaders (``pdeval_fol_registry_kinds``): 1 for
        a leader that is a function of ``rho`` alone, 2 of ``z`` alone, 0 otherwise."""
        kinds = np.zeros(self.n_classes, dtype=np.uint8)
        if kinds.size:
            self._call(self.lib.pdeval_fol_registry_kinds(self.h, kinds.ctypes.data))
        return kinds

    def leader_fields(self):
        """The leaders' fields, a torch float64 tensor [L, 2, m*m] on the context's device (a copy:
        the store itself is chunk-major)."""
        import torch
        dev = _device(self.ctx)
        L = self.n_classes
        out = torch.empty((L, 2, self.mm), dtype=torch.float64, device=dev)
        torch.cuda.current_stream(dev).synchronize()
        if L:
            self._call(self.lib.pdeval_fol_registry_leaders(self.h, out.data_ptr(), None, None))
        return out

    def tags(self, pd_, by_component: bool = False):
        """{class_id: name} of the classes that re-parametrise one of ``pd_.known_solutions``, by
        the two rules of :func:`tag_known` applied to the leaders' fields: the leader matches the
        known solution under the Jacobian test, or its field equals the known one's at every
        sample point.  ``by_component``: {component_id: name} instead; a component is named if any
        of its classes is, and if several names apply the first in ``known_solutions`` order wins."""
        import torch
        from . import problem_defs as P
        if self.n_classes == 0:
            return {}
        dev = _device(self.ctx)
        lead_fields = self.leader_fields()
        names = list(pd_.known_solutions.values())
        ops, off, _ = P.compile_strings(pd_, list(pd_.known_solutions))
        k_ops = torch.from_numpy(np.ascontiguousarray(ops, dtype=np.int32)).to(dev)
        k_off = torch.from_numpy(np.ascontiguousarray(off, dtype=np.int64)).to(dev)
        known, _ = gradient_fields(self.ctx, k_ops, int(k_ops.numel()), k_off, len(names), None, self.params)
        hit = match_fields(self.ctx, lead_fields, known, self.params)
        for k in range(len(names)):
            kf = known[k]
            if bool(torch.isfinite(kf).any()):
                same = (lead_fields == kf) | (torch.isnan(lead_fields) & torch.isnan(kf))
                hit[:, k] |= same.flatten(1).all(1).cpu().numpy()
        if by_component:
            comp = self.components()
            chit = np.zeros((len(hit), len(names)), dtype=bool)
            np.logical_or.at(chit, comp, hit)
            return {int(c): names[int(np.argmax(chit[c]))] for c in np.unique(comp) if chit[c].any()}
        return {int(c): names[int(np.argmax(hit[c]))] for c in range(len(hit)) if hit[c].any()}

    def merge(self, other: 'FoliationRegistry') -> np.ndarray:
        """Takes ``other``'s classes into this registry: the sequential rule applied to
        ``other``'s leaders, in their order, after this registry's own -- each joins the first
        class of this registry it matches or becomes a new one (keeping its key) -- and
        ``other``'s class sizes are added.  Returns the int64 map from ``other``'s class ids to
        this registry's.  Members of ``other``'s classes follow their leader without being
        tested again.  ``other``'s links are carried over through the returned map (a link whose
        ends land in one class here is dropped); with ``FOL_LINK`` the merged leaders also link by
        the arrival rule, as rows assigned here.  ``other`` is left as it is and may live on another
        context of the same device, with the same m, grid and flags."""
        if int(other.params.m) != int(self.params.m) or not np.array_equal(other.grid, self.grid):
            raise ValueError('merge: the registries differ in m or grid')
        if (int(other.params.flags) ^ int(self.params.flags)) & (FOL_AXIS | FOL_LINK):
            raise ValueError(f'merge: the registries differ in flags ({int(self.params.flags)} here, '
                             f'{int(other.params.flags)} in the other): their classes follow different rules')
        keys, sizes = other._host()
        if len(keys) == 0:
            return np.zeros(0, dtype=np.int64)
        edges = np.ascontiguousarray(other.links())
        ids = self.assign_fields(other.leader_fields(), keys=keys)
        extra = sizes - 1
        self._call(self.lib.pdeval_fol_registry_add_sizes(self.h, ids.ctypes.data, extra.ctypes.data, len(ids)))
        if len(edges):
            self._call(self.lib.pdeval_fol_registry_merge_links(self.h, edges.ctypes.data, len(edges), ids.ctypes.data,
                                                                len(ids)))
        return ids

    # ---- persistence
    def save(self, path):
        """One .npz: the leaders' fields, keys and sizes, the links, m, tau, min_points, flags and
        the context's 8 grid doubles."""
        keys, sizes = self._host()
        with open(path, 'wb') as f:
            np.savez(f, fields=self.leader_fields().cpu().numpy(), keys=keys, sizes=sizes, links=self.links(),
                     m=np.int64(self.params.m), tau=np.float64(self.params.tau),
                     min_points=np.int64(self.params.min_points), flags=np.int64(self.params.flags),
                     grid=self.grid)

    @classmethod
    def load(cls, ctx, path, params: Optional[FolParams] = None, capacity_hint: int = 0) -> 'FoliationRegistry':
        """A registry on ``ctx`` holding the saved leaders as they were (no re-matching: ids are
        preserved).  ``params`` (None: the file's) must agree with the file's ``m`` and ``flags`` (a
        file without ``flags`` was saved with 0), and the file's grid with the context's: otherwise
        ValueError naming the field.  A file without ``links`` has none."""
        import torch
        with np.load(path) as d:
            fields, keys, sizes = d['fields'], d['keys'], d['sizes']
            m, tau, min_points, grid = int(d['m']), float(d['tau']), int(d['min_points']), d['grid']
            flags = int(d['flags']) if 'flags' in d.files else 0
            links = d['links'] if 'links' in d.files else np.zeros((0, 2), dtype=np.int64)
        if params is None:
            params = default_fol_params()
            params.m, params.tau, params.min_points, params.flags = m, tau, min_points, flags
        if int(params.m) != m:
            raise ValueError(f'{path}: m = {m} in the file, {int(params.m)} asked for')
        if (int(params.flags) ^ flags) & (FOL_AXIS | FOL_LINK):
            raise ValueError(f'{path}: flags = {flags} in the file, {int(params.flags)} asked for')
        reg = cls(ctx, params, max(capacity_hint, len(keys)))
        try:
            if not np.array_equal(reg.grid, grid):
                raise ValueError(f'{path}: grid = {grid.tolist()} in the file, {reg.grid.tolist()} in the context')
            if fields.shape != (len(keys), 2, m * m) or sizes.shape != keys.shape:
                raise ValueError(f'{path}: fields {fields.shape} do not fit {len(keys)} classes at m = {m}')
            dev = _device(ctx)
            d_f = torch.from_numpy(np.ascontiguousarray(fields, dtype=np.float64)).to(dev)
            keys = np.ascontiguousarray(keys, dtype=np.int64)
            sizes = np.ascontiguousarray(sizes, dtype=np.int64)
            torch.cuda.current_stream(dev).synchronize()
            reg._load(d_f, keys, sizes)
            links = np.ascontiguousarray(links, dtype=np.int64)
            if links.ndim != 2 or links.shape[1] != 2:
                raise ValueError(f'{path}: links {links.shape} are not pairs')
            if len(links):
                reg._call(reg.lib.pdeval_fol_registry_load_links(reg.h, links.ctypes.data, len(links)))
        except Exception:
            reg.close()
            raise
        return reg

    def _load(self, d_fields, keys, sizes):
        self._call(self.lib.pdeval_fol_registry_load(self.ctx.h, self.h, d_fields.data_ptr() or None, keys.ctypes.data,
                                                     sizes.ctypes.data, len(keys)))

#!/usr/bin/env python3
"""Foliation classes of the depth-4 force-free set on one GPU.

Validates the 142,004 rows of data/force_free_d4_validated.npz on the device, classifies the
accepted rows at the default parameters (m = 16) with pdeval_foliation_classes and tags the
classes that re-parametrise a paper solution.  Times the field kernel alone and the whole
classification with HIP events (one warm-up run, then the median of --repeats runs) and prints
one JSON object, also written to --out.  With --axis the classification is measured a second
time in the same process with the axis rule (PDEVAL_FOL_AXIS: the functions of one coordinate
form one class per axis) and reported under "axis", next to the figures without it; "leader_kinds"
counts the class leaders that are functions of rho alone or of z alone.  With --cplx it is measured
once more with PDEVAL_FOL_CPLX (the rows that are not real-valued take the complex field pass)
under "cplx" (and "axis_cplx"): the rows whose field the complex pass changed (compared on the
device), the rows its selection rule names (restated on the host), those among the rows
unclassified without the flag that it classifies, the paper names they join, and the field
kernels' time with the flag ("field_ms": both kernels) next to "field_kernel_ms" without it.
With --reduce the reduction kinds of the accepted rows (pdeval_fol_reduce, Omega = 0) are reported
under "reduce": their histogram, the kind of each class tagged with a paper name, the classes whose
members disagree (with a few of their rows as examples) and the kernels' time -- against the classes
of the axis rule when --axis is given, otherwise the plain ones.  With --settle as well, the rows whose
fp64 |X| / S_X falls between 1e-12 and 1e-3 are evaluated again in double-double
(pdeval_fol_reduce_dd) and reported under "reduce"/"settle": how many, their kinds before and after,
the tier's time and the mixed classes before and after.  With --cplx and --reduce the reduce call is
repeated with PDEVAL_FOL_CPLX and reported under "cplx"/"reduce" (and "axis_cplx"/"reduce"): the kinds
of the rows the complex pass took, the classes still mixed and the time of its launches.  With --reduce
and --omega 0,1/2,1 the kinds at each of these rotation rates come from one pdeval_fol_reduce_multi call
and are reported under "reduce"/"omega": the histogram per Omega, the kinds of each tagged class at each
Omega, and the call's time next to that of one pdeval_fol_reduce call per value (with --cplx both carry
PDEVAL_FOL_CPLX).  With --reduce and --profile the table of the accepted rows is integrated by
pdeval_fol_profile and reported under "reduce"/"profile": per kind the rows that get a profile, per tagged
class n, the range of u and psi' and Q at the last sample, and the kernel's time next to that of
torch.sort, gathers and torch.cumsum on the same table (and, under "m64", on 256 rows at m = 64).

    python scripts/foliation_d4.py --axis --cplx --reduce --settle --out foliation_d4.json
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'pde-engine_amd'))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from pdeval import foliation as FOL  # noqa: E402
from pdeval import problem_defs as P  # noqa: E402
from pdeval._lib import Context, default_fol_params, fol_params  # noqa: E402
from pdeval.opcodes import CLS_ACCEPT, FLAG_COMPLEX, MAX_STACK  # noqa: E402

SETTLE_BAND = (1e-12, 1e-3)   # no true zero above, no true non-zero below


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--data', default=os.path.join(ROOT, 'data', 'force_free_d4_validated.npz'))
    ap.add_argument('--device', type=int, default=0)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--axis', action='store_true', help='also measure with the axis rule (PDEVAL_FOL_AXIS)')
    ap.add_argument('--cplx', action='store_true', help='also measure with the complex field pass (PDEVAL_FOL_CPLX)')
    ap.add_argument('--reduce', action='store_true', help='also report the reduction kinds (pdeval_fol_reduce)')
    ap.add_argument('--settle', action='store_true',
                    help='with --reduce: settle the rows in the band in double-double (pdeval_fol_reduce_dd)')
    ap.add_argument('--omega', default=None,
                    help='with --reduce: a comma-separated list of at most 8 rotation rates, e.g. 0,1/2,1: the kinds at '
                         'each of them in one pass (pdeval_fol_reduce_multi)')
    ap.add_argument('--profile', action='store_true',
                    help='with --reduce: psi(u) and the current of every accepted row (pdeval_fol_profile)')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.repeats < 5:
        ap.error('--repeats must be at least 5')
    d = np.load(a.data)
    ops = np.ascontiguousarray(d['ops'], dtype=np.int32)
    off = np.ascontiguousarray(d['offsets'], dtype=np.int64)
    n = len(off) - 1
    pd_ = P.force_free()
    dev = torch.device('cuda', a.device)
    ctx = Context(pd_.problem_id, device=a.device)
    acc = np.flatnonzero(ctx.validate(ops, off)['status'] == CLS_ACCEPT).astype(np.int64)
    d_ops = torch.from_numpy(ops).to(dev)
    d_off = torch.from_numpy(off).to(dev)
    d_acc = torch.from_numpy(acc).to(dev)
    prm = default_fol_params()
    mm = int(prm.m) ** 2
    field = torch.empty((len(acc), 2, mm), dtype=torch.float64, device=dev)
    nfin = torch.zeros(len(acc), dtype=torch.int32, device=dev)
    st = torch.cuda.Stream(dev)
    torch.cuda.synchronize(dev)

    def field_ms(prm=prm):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(st):
            e0.record(st)
            ctx.gradient_fields(d_ops.data_ptr(), ops.size, d_off.data_ptr(), n, d_acc.data_ptr(), len(acc),
                                field.data_ptr(), nfin.data_ptr(), prm, st.cuda_stream)
            e1.record(st)
        st.synchronize()
        return e0.elapsed_time(e1)

    def total_ms(p):
        # (the call is synchronous and runs on the context's own stream: the two events bracket it)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        res = ctx.foliation_classes(d_ops.data_ptr(), ops.size, d_off.data_ptr(), n, d_acc.data_ptr(), len(acc), p)
        e1.record(st)
        st.synchronize()
        return e0.elapsed_time(e1), res

    def classes(p):
        """The classification under parameters p, one warm-up run, then the median of the repeats:
        (the figures, the FoliationClasses, the tags)."""
        total_ms(p)
        runs = [total_ms(p) for _ in range(a.repeats)]
        leader, n_classes, n_rounds = runs[-1][1]
        cls = FOL.classes_from_leader(leader)
        tags = FOL.tag_known(ctx, pd_, cls, (d_ops, ops.size, d_off, n), p)
        paper, paper_n = {}, {}
        for c, name in sorted(tags.items()):    # (a name can head several classes: rows equal to rho**2)
            paper[name] = paper.get(name, 0) + int(cls.sizes[c])
            paper_n[name] = paper_n.get(name, 0) + 1
        # the leaders' kinds: a leader precedes its members, so the unique leader entries are the leaders
        lead = np.unique(leader[leader >= 0])
        lead_fields, _ = FOL.gradient_fields(ctx, d_ops, ops.size, d_off, n, lead, p)
        kinds = FOL.field_kinds(ctx, lead_fields, p)
        return {
            'flags': int(p.flags), 'classes': int(n_classes), 'unclassified': int(cls.unclassified.size),
            'rounds': int(n_rounds),
            'leader_kinds': {'rho_axis': int((kinds == 1).sum()), 'z_axis': int((kinds == 2).sum())},
            'total_ms': statistics.median(t for t, _ in runs), 'total_ms_all': [t for t, _ in runs],
            'paper_classes': paper, 'paper_class_counts': paper_n,
            'largest_classes': sorted((int(s) for s in cls.sizes), reverse=True)[:10],
        }, cls, tags

    def with_cplx(p, base):
        """classes(p) for p with FOL_CPLX, and what the complex pass adds to base, the classes of the
        same parameters without it.  "changed_rows" is observed on the device: the rows whose field
        bits or n_finite differ between the two field calls (a selected row that is NaN throughout
        either way does not show).  "selected_rows" restates the kernel's selection rule on the host
        from the headers and the real pass's counts."""
        res, cls, tags = classes(p)
        field_ms(p)
        c_ms = [field_ms(p) for _ in range(a.repeats)]
        f0, n0 = FOL.gradient_fields(ctx, d_ops, ops.size, d_off, n, acc, fol_params(p, cplx=False))
        f1, n1 = FOL.gradient_fields(ctx, d_ops, ops.size, d_off, n, acc, p)
        changed = (f0.view(torch.int64) != f1.view(torch.int64)).flatten(1).any(1) | (n0 != n1)
        hdr = ops[off[acc]].astype(np.int64)
        flagged = (hdr & FLAG_COMPLEX) != 0
        selected = ((hdr & 0xff) == 0) & (((hdr >> 8) & 0xff) <= MAX_STACK) & \
            (flagged | (n0.cpu().numpy() < int(p.min_points)))
        new = (base.class_id < 0) & (cls.class_id >= 0)
        joined = {}
        for c in cls.class_id[new]:
            name = tags.get(int(c), '(unnamed)')
            joined[name] = joined.get(name, 0) + 1
        res.update({'field_ms': statistics.median(c_ms), 'field_ms_all': c_ms, 'changed_rows': int(changed.sum()),
                    'changed_rows_not_selected': int((changed.cpu().numpy() & ~selected).sum()),
                    'selected_rows': int(selected.sum()), 'flagged_rows': int(flagged.sum()),
                    'newly_classified': int(new.sum()), 'newly_classified_names': joined,
                    'new_rows_in_old_classes': int(np.isin(cls.leader[new], base.leader[base.leader >= 0]).sum())})
        if a.reduce:
            res['reduce'] = reduce_cplx(p, cls)
        return res

    def reduce_cplx(p, cls):
        """pdeval_fol_reduce with FOL_CPLX against the same call without it, on the classes cls of p: the
        kinds of the rows the complex pass took (the rows whose outputs differ), the classes still mixed
        or without a kind, and both calls' time -- one warm-up run, then the median of the repeats;
        "cplx_launch_ms" is their difference, the two launches of fol_reduce_cplx_kernel."""
        out, ms = {}, {}
        for name, q in (('off', fol_params(p, cplx=False)), ('on', p)):
            kind = torch.zeros(len(acc), dtype=torch.uint8, device=dev)
            counts = torch.zeros((len(acc), 4), dtype=torch.int32, device=dev)
            qmax = torch.zeros((len(acc), 3), dtype=torch.float64, device=dev)
            t = []
            for _ in range(a.repeats + 1):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                with torch.cuda.stream(st):
                    e0.record(st)
                    ctx.fol_reduce(d_ops.data_ptr(), ops.size, d_off.data_ptr(), n, d_acc.data_ptr(), len(acc),
                                   kind.data_ptr(), 0.0, counts.data_ptr(), qmax.data_ptr(), 0, q, st.cuda_stream)
                    e1.record(st)
                st.synchronize()
                t.append(e0.elapsed_time(e1))
            ms[name], out[name] = t[1:], (kind.cpu().numpy(), counts.cpu().numpy(), qmax.cpu().numpy())
        (k0, c0, q0), (k1, c1, q1) = out['off'], out['on']
        took = (k0 != k1) | (c0 != c1).any(1) | (q0.view(np.int64) != q1.view(np.int64)).any(1)
        by_class = FOL.class_kinds(cls.class_id, k1)
        qt = q1[took]
        return {'reduce_ms': statistics.median(ms['off']), 'reduce_cplx_ms': statistics.median(ms['on']),
                'cplx_launch_ms': statistics.median(ms['on']) - statistics.median(ms['off']),
                'reduce_ms_all': ms['off'], 'reduce_cplx_ms_all': ms['on'],
                'none_without_flag': int((k0 == 0).sum()), 'rows_taken': int(took.sum()),
                'taken_kinds_before': {FOL.KIND_NAMES[x]: int((k0[took] == x).sum()) for x in range(4)},
                'taken_kinds': {FOL.KIND_NAMES[x]: int((k1[took] == x).sum()) for x in range(4)},
                'kinds': {FOL.KIND_NAMES[x]: int((k1 == x).sum()) for x in range(4)},
                'mixed_classes': sorted(int(c) for c, ks in by_class.items() if len(ks) > 1),
                'classes_without_kind': sorted(int(c) for c, ks in by_class.items() if ks == (0,)),
                'taken_qmax_below_tau_max': float(qt[qt <= p.tau].max(initial=0.0)),
                'taken_qmax_above_tau_min': float(qt[qt > p.tau].min(initial=np.inf))}

    def settle(qmax, cls, k, mixed):
        """The settle tier on the fp64 pass's qmax (a device tensor; k, mixed: its kinds and the
        mixed classes before): the rows whose qmax falls in SETTLE_BAND, selected on the device, through
        pdeval_fol_reduce_dd -- one warm-up run, then the median of the repeats (its four launches)."""
        pos = torch.nonzero(((qmax > SETTLE_BAND[0]) & (qmax < SETTLE_BAND[1])).any(1)).flatten()
        cand = d_acc[pos]
        k2 = torch.zeros(len(pos), dtype=torch.uint8, device=dev)
        c2 = torch.zeros((len(pos), 4), dtype=torch.int32, device=dev)
        q2 = torch.zeros((len(pos), 3), dtype=torch.float64, device=dev)

        def settle_ms():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(st):
                e0.record(st)
                ctx.fol_reduce_dd(d_ops.data_ptr(), ops.size, d_off.data_ptr(), n, cand.data_ptr(), len(pos),
                                  k2.data_ptr(), c2.data_ptr(), q2.data_ptr(), 0.0, prm, st.cuda_stream)
                e1.record(st)
            st.synchronize()
            return e0.elapsed_time(e1)

        settle_ms()
        s_ms = [settle_ms() for _ in range(a.repeats)]
        rows = pos.cpu().numpy()
        after = k.copy()
        after[rows] = k2.cpu().numpy()
        by_class = FOL.class_kinds(cls.class_id, after)
        still = sorted(c for c, ks in by_class.items() if len(ks) > 1)
        strings = d['exprs'] if 'exprs' in d.files else None
        return {'settle': {
            'band': list(SETTLE_BAND), 'rows_in_band': int(rows.size), 'settle_ms': statistics.median(s_ms),
            'settle_ms_all': s_ms,
            'kinds_before': {FOL.KIND_NAMES[x]: int((k[rows] == x).sum()) for x in range(4)},
            'kinds_after': {FOL.KIND_NAMES[x]: int((after[rows] == x).sum()) for x in range(4)},
            'rows': [{'candidate': int(acc[r]), 'class': int(cls.class_id[r]), 'before': FOL.KIND_NAMES[int(k[r])],
                      'after': FOL.KIND_NAMES[int(after[r])], 'qmax_fp64': qmax[r].tolist(), 'qmax_dd': q2[i].tolist(),
                      **({'string': str(strings[acc[r]])} if strings is not None else {})}
                     # (the rows whose kind changed first, then those still current, 16 in all)
                     for i, r in sorted(enumerate(rows), key=lambda t: (k[t[1]] == after[t[1]],
                                                                        after[t[1]] != FOL.RED_CURRENT))[:16]],
            'mixed_classes_before': sorted(int(c) for c in mixed), 'mixed_classes_after': [int(c) for c in still]}}

    def reduce(cls, tags):
        """The reduction kinds of the accepted rows against the classes cls: one warm-up run, then
        the median of the repeats (both launches of the kernel, counts and qmax included, no table)."""
        kind = torch.zeros(len(acc), dtype=torch.uint8, device=dev)
        counts = torch.zeros((len(acc), 4), dtype=torch.int32, device=dev)
        qmax = torch.zeros((len(acc), 3), dtype=torch.float64, device=dev)

        def reduce_ms():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(st):
                e0.record(st)
                ctx.fol_reduce(d_ops.data_ptr(), ops.size, d_off.data_ptr(), n, d_acc.data_ptr(), len(acc),
                               kind.data_ptr(), 0.0, counts.data_ptr(), qmax.data_ptr(), 0, prm, st.cuda_stream)
                e1.record(st)
            st.synchronize()
            return e0.elapsed_time(e1)

        reduce_ms()
        r_ms = [reduce_ms() for _ in range(a.repeats)]
        k, q = kind.cpu().numpy(), qmax.cpu().numpy()
        by_class = FOL.class_kinds(cls.class_id, k)
        mixed = {c: ks for c, ks in by_class.items() if len(ks) > 1}
        strings = d['exprs'] if 'exprs' in d.files else None
        examples = {}
        for c in sorted(mixed, key=lambda c: -int(cls.sizes[c]))[:8]:
            rows = np.flatnonzero(cls.class_id == c)
            examples[str(c)] = {
                'size': int(rows.size), 'tag': tags.get(c),
                'kinds': {FOL.KIND_NAMES[x]: int((k[rows] == x).sum()) for x in mixed[c]},
                'rows': [{'candidate': int(acc[r]), 'kind': FOL.KIND_NAMES[int(k[r])], 'qmax': q[r].tolist(),
                          **({'string': str(strings[acc[r]])} if strings is not None else {})}
                         for x in mixed[c] for r in rows[k[rows] == x][:2]]}
        settled = settle(qmax, cls, k, mixed) if a.settle else {}
        return {
            **settled,
            'kernel_ms': statistics.median(r_ms), 'kernel_ms_all': r_ms,
            'kinds': {FOL.KIND_NAMES[x]: int((k == x).sum()) for x in range(4)},
            'kinds_classified': {FOL.KIND_NAMES[x]: int((k[cls.class_id >= 0] == x).sum()) for x in range(4)},
            'paper_kinds': {f'{name} ({c})': [FOL.KIND_NAMES[x] for x in by_class[c]] for c, name in sorted(tags.items())},
            'mixed_classes': len(mixed), 'mixed_examples': examples,
            # the margin of the rule on this set: the rows' qmax nearest to tau from either side
            'qmax_below_tau_max': float(q[q <= prm.tau].max(initial=0.0)),
            'qmax_above_tau_min': float(q[q > prm.tau].min(initial=np.inf)),
        }

    def profile(cls, tags, p, rows):
        """pdeval_fol_profile on the table of the first `rows` accepted rows under parameters p (Omega = 0)
        against what a caller had before it -- torch.sort on u, gathers and torch.cumsum on the same
        table: one warm-up run each, then the median of the repeats.  Per kind the rows that get a
        profile (n >= min_points); per tagged class (rows within the first `rows`) n, the range of u,
        psi' and Q at the last sample and whether psi' == 1 throughout (the class's u is already psi)."""
        rows = min(rows, len(acc))
        mm_ = int(p.m) ** 2
        kind = torch.zeros(rows, dtype=torch.uint8, device=dev)
        tab = torch.empty((rows, 3, mm_), dtype=torch.float64, device=dev)
        prof = torch.empty((rows, 4, mm_), dtype=torch.float64, device=dev)
        perm = torch.empty((rows, mm_), dtype=torch.int32, device=dev)
        cnt = torch.empty(rows, dtype=torch.int32, device=dev)
        with torch.cuda.stream(st):
            ctx.fol_reduce(d_ops.data_ptr(), ops.size, d_off.data_ptr(), n, d_acc.data_ptr(), rows, kind.data_ptr(), 0.0,
                           0, 0, tab.data_ptr(), p, st.cuda_stream)
        st.synchronize()

        def by_torch():
            ok = torch.isfinite(tab).all(1)
            u, order = torch.sort(torch.where(ok, tab[:, 0] + 0.0, torch.inf), dim=1, stable=True)
            ok = torch.gather(ok, 1, order)
            kap = torch.where(ok, torch.gather(tab[:, 1], 1, order), 0.0)
            g = torch.where(ok, torch.gather(tab[:, 2], 1, order), 0.0)
            d = torch.zeros_like(u)
            d[:, 1:] = torch.where(ok[:, 1:], u[:, 1:] - u[:, :-1], 0.0)
            mid = lambda f: torch.cat([torch.zeros_like(f[:, :1]), 0.5 * (f[:, 1:] + f[:, :-1])], 1) * d   # noqa: E731
            dp = torch.exp(torch.cumsum(mid(kap), 1))
            return u, dp, torch.cumsum(mid(dp), 1), torch.cumsum(mid(g * dp * dp), 1), order, ok.sum(1)

        def call_ms(kernel):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(st):
                e0.record(st)
                if kernel:
                    ctx.fol_profile(tab.data_ptr(), rows, prof.data_ptr(), perm.data_ptr(), cnt.data_ptr(), p, st.cuda_stream)
                else:
                    by_torch()
                e1.record(st)
            st.synchronize()
            return e0.elapsed_time(e1)

        ms = {}
        for kernel in (True, False):
            call_ms(kernel)
            ms[kernel] = [call_ms(kernel) for _ in range(a.repeats)]
        k, nn, pr = kind.cpu().numpy(), cnt.cpu().numpy(), prof.cpu().numpy()
        have = nn >= int(p.min_points)
        paper = {}
        for c, name in sorted(tags.items()):
            for r in np.flatnonzero(cls.class_id[:rows] == c)[:1]:     # the class's first row stands for it
                last = int(nn[r]) - 1
                e = paper[f'{name} ({c})'] = {'candidate': int(acc[r]), 'kind': FOL.KIND_NAMES[int(k[r])], 'n': int(nn[r])}
                if have[r]:
                    e.update({'u_range': [float(pr[r, 0, 0]), float(pr[r, 0, last])], 'dpsi_last': float(pr[r, 1, last]),
                              'Q_last': float(pr[r, 3, last]), 'dpsi_is_one': bool((pr[r, 1, :last + 1] == 1.0).all()),
                              'dpsi_minus_one_max': float(np.abs(pr[r, 1, :last + 1] - 1.0).max())})
        return {'m': int(p.m), 'rows': rows, 'kernel_ms': statistics.median(ms[True]), 'kernel_ms_all': ms[True],
                'torch_ms': statistics.median(ms[False]), 'torch_ms_all': ms[False],
                'rows_with_profile': {FOL.KIND_NAMES[x]: int((have & (k == x)).sum()) for x in range(4)},
                'paper_profiles': paper}

    def reduce_omega(cls, tags, p):
        """The reduction kinds at every Omega of --omega in one pdeval_fol_reduce_multi call against one
        pdeval_fol_reduce call per value, both with counts and qmax and without a table: one warm-up
        run, then the median of the repeats.  Per Omega the histogram, per tagged class its kinds."""
        from pdeval.batch import omega2_value
        names = [s.strip() for s in a.omega.split(',')]
        ws = [omega2_value(s)[0] for s in names]
        kind = torch.zeros((len(ws), len(acc)), dtype=torch.uint8, device=dev)
        counts = torch.zeros((len(ws), len(acc), 4), dtype=torch.int32, device=dev)
        qmax = torch.zeros((len(ws), len(acc), 3), dtype=torch.float64, device=dev)
        single = (torch.zeros_like(kind), torch.zeros_like(counts), torch.zeros_like(qmax))

        def call_ms(multi):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(st):
                e0.record(st)
                if multi:
                    ctx.fol_reduce_multi(d_ops.data_ptr(), ops.size, d_off.data_ptr(), n, d_acc.data_ptr(), len(acc),
                                         kind.data_ptr(), ws, counts.data_ptr(), qmax.data_ptr(), 0, p, st.cuda_stream)
                else:
                    for i, w in enumerate(ws):
                        ctx.fol_reduce(d_ops.data_ptr(), ops.size, d_off.data_ptr(), n, d_acc.data_ptr(), len(acc),
                                       single[0][i].data_ptr(), w, single[1][i].data_ptr(), single[2][i].data_ptr(), 0,
                                       p, st.cuda_stream)
                e1.record(st)
            st.synchronize()
            return e0.elapsed_time(e1)

        ms = {}
        for multi in (True, False):
            call_ms(multi)
            ms[multi] = [call_ms(multi) for _ in range(a.repeats)]
        k = kind.cpu().numpy()
        same = all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip((kind, counts, qmax), single))
        by_class = [FOL.class_kinds(cls.class_id, k[i]) for i in range(len(ws))]
        return {'omega': names, 'omega2': ws, 'flags': int(p.flags),
                'multi_ms': statistics.median(ms[True]), 'multi_ms_all': ms[True],
                'single_calls_ms': statistics.median(ms[False]), 'single_calls_ms_all': ms[False],
                'bits_equal_single_calls': bool(same),
                'kinds': {s: {FOL.KIND_NAMES[x]: int((k[i] == x).sum()) for x in range(4)} for i, s in enumerate(names)},
                'paper_kinds': {f'{name} ({c})': {s: [FOL.KIND_NAMES[x] for x in by_class[i][c]] for i, s in enumerate(names)}
                                for c, name in sorted(tags.items())}}

    field_ms()
    f_ms = [field_ms() for _ in range(a.repeats)]
    out = {
        'data': os.path.basename(a.data), 'm': int(prm.m), 'tau': float(prm.tau), 'min_points': int(prm.min_points),
        'rows': int(n), 'accepted': int(len(acc)),
        'field_kernel_ms': statistics.median(f_ms), 'field_kernel_ms_all': f_ms,
        'repeats': a.repeats,
        'device': torch.cuda.get_device_name(dev),
    }
    plain, plain_cls, plain_tags = classes(fol_params(prm, axis=False))
    out.update(plain)
    if a.axis:
        out['axis'], axis_cls, axis_tags = classes(fol_params(prm, axis=True))
    if a.reduce:
        red_cls, red_tags = (axis_cls, axis_tags) if a.axis else (plain_cls, plain_tags)
        out['reduce'] = reduce(red_cls, red_tags)
        if a.omega:
            out['reduce']['omega'] = reduce_omega(red_cls, red_tags, fol_params(prm, cplx=a.cplx))
        if a.profile:
            out['reduce']['profile'] = profile(red_cls, red_tags, prm, len(acc))
            big = fol_params(prm)
            big.m = 64
            out['reduce']['profile']['m64'] = profile(red_cls, {}, big, 256)
    if a.cplx:
        out['cplx'] = with_cplx(fol_params(prm, axis=False, cplx=True), plain_cls)
        if a.axis:
            out['axis_cplx'] = with_cplx(fol_params(prm, axis=True, cplx=True), axis_cls)
    ctx.close()
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()

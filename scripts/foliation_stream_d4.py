#!/usr/bin/env python3
"""Foliation classes of the depth-4 force-free set as a stream, through a registry (DESIGN.md §14
"Registry").

Validates the 142,004 rows of data/force_free_d4_validated.npz on the device and sends the
accepted rows, in stream order, through a FoliationRegistry in batches of --batch (4,096) rows.
Checks that the class ids equal those of the one-shot pdeval_foliation_classes on the whole list,
from the same run.  Per batch: the leaders resident before it, Stage A's kernel time (HIP events,
taken by the registry around its launch) and the whole assign call (HIP events around it).  The
stream's total (one warm-up pass, then the median of --repeats passes, a fresh registry each) stands
next to the one-shot call's, measured the same way in the same process.  For the last batch only
it also times the path available without a registry: the existing fol_match_kernel over the same
resident leaders in blocks of 32, one launch and one download of the masks per block.  Prints one
JSON line, also written to --out.  With --axis everything is measured a second time in the same
process with the axis rule (PDEVAL_FOL_AXIS: the functions of one coordinate form one class per
axis) and reported under "axis", next to the figures without it; "leader_kinds" counts the
registry's leaders that are functions of rho alone or of z alone, "paper_classes" the rows of the
classes tagged with a paper solution.  With --link (combinable with --axis) the stream is measured
once more with PDEVAL_FOL_LINK under "link" (and "axis_link"): the link pass's device time per batch
(HIP events around its launches, "link_ms"), the number of links and components, the ten largest
components, "paper_component_counts" (how many components carry each paper name) and the
components that hold classes tagged with two different paper names.

    python scripts/foliation_stream_d4.py --axis --link --out foliation_stream_d4.json
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
from pdeval._lib import FOL_LINK, FOL_MAX_PROBES, Context, default_fol_params, fol_params  # noqa: E402
from pdeval.opcodes import CLS_ACCEPT  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--data', default=os.path.join(ROOT, 'data', 'force_free_d4_validated.npz'))
    ap.add_argument('--device', type=int, default=0)
    ap.add_argument('--batch', type=int, default=4096)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--axis', action='store_true', help='also measure with the axis rule (PDEVAL_FOL_AXIS)')
    ap.add_argument('--link', action='store_true', help='also measure with the link pass (PDEVAL_FOL_LINK)')
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
    prm0 = default_fol_params()
    prog = (d_ops, int(ops.size), d_off, n)
    st = torch.cuda.Stream(dev)
    torch.cuda.synchronize(dev)

    def timed(fn):
        # (the calls are synchronous and run on the context's own stream: the two events bracket them)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        res = fn()
        e1.record(st)
        st.synchronize()
        return e0.elapsed_time(e1), res

    def measure(prm):
        """Everything under parameters prm: (the result, whether the stream's ids equal the one-shot's)."""
        def one_shot():
            return timed(lambda: ctx.foliation_classes(d_ops.data_ptr(), ops.size, d_off.data_ptr(), n, d_acc.data_ptr(),
                                                       len(acc), prm))

        edges = list(range(0, len(acc), a.batch)) + [len(acc)]

        def stream_pass(keep=None):
            """One pass of the stream through a fresh registry: (ids, per-batch records); `keep`
            receives the registry before its last batch is assigned."""
            reg = ctx.fol_registry(prm)
            ids, per = [], []
            for b0, b1 in zip(edges[:-1], edges[1:]):
                L = reg.n_classes
                if keep is not None and b1 == len(acc):
                    keep(reg, b0, b1)
                ms, part = timed(lambda: reg.assign(*prog, acc[b0:b1]))
                ids.append(part)
                per.append({'rows': int(b1 - b0), 'L_before': int(L), 'stage_a_ms': round(reg.stage_a_ms, 4),
                            'assign_ms': round(ms, 4), 'new': int(reg.last_new)})
                if linked:
                    per[-1]['link_ms'] = round(reg.link_ms, 4)
            n_classes = reg.n_classes
            if keep is not None:     # the last, untimed pass: what the registry holds
                kinds, sizes = reg.kinds(), reg.sizes
                paper, paper_n = {}, {}
                for c, name in sorted(reg.tags(pd_).items()):
                    paper[name] = paper.get(name, 0) + int(sizes[c])
                    paper_n[name] = paper_n.get(name, 0) + 1
                extra.update(leader_kinds={'rho_axis': int((kinds == 1).sum()), 'z_axis': int((kinds == 2).sum())},
                             paper_classes=paper, paper_class_counts=paper_n)
                if linked:
                    comp = reg.components()
                    csize = reg.component_sizes()
                    names = {}
                    for c, name in reg.tags(pd_).items():
                        names.setdefault(int(comp[c]), set()).add(name)
                    comp_n = {}
                    for name in reg.tags(pd_, by_component=True).values():
                        comp_n[name] = comp_n.get(name, 0) + 1
                    top = sorted(csize.items(), key=lambda kv: (-kv[1], kv[0]))[:10]
                    extra['links'] = {
                        'links': int(reg.n_links), 'components': int(reg.n_components),
                        'largest_components': [{'component': c, 'rows': r, 'classes': int((comp == c).sum()),
                                                'names': sorted(names.get(c, ()))} for c, r in top],
                        'paper_component_counts': comp_n,
                        'two_names': {str(c): sorted(v) for c, v in names.items() if len(v) > 1}}
            reg.close()
            return np.concatenate(ids), per, n_classes

        loop, extra = {}, {}
        linked = bool(int(prm.flags) & FOL_LINK)

        def block_loop(reg, b0, b1):
            """The last batch against the resident leaders by fol_match_kernel, 32 leaders a launch."""
            lead = reg.leader_fields()
            rows, _ = FOL.gradient_fields(ctx, *prog, acc[b0:b1], prm)
            FOL.match_fields(ctx, rows, lead[:FOL_MAX_PROBES], prm)          # warm-up
            ms, hit = timed(lambda: FOL.match_fields(ctx, rows, lead, prm))
            loop.update(ms=ms, launches=-(-int(lead.shape[0]) // FOL_MAX_PROBES), L=int(lead.shape[0]),
                        first=np.where(hit.any(axis=1), hit.argmax(axis=1), -1))

        one_shot()
        stream_pass()
        shots = [one_shot() for _ in range(a.repeats)]
        passes = [stream_pass() for _ in range(a.repeats)]
        ids, per, n_classes = stream_pass(keep=block_loop)
        leader = shots[-1][1][0]
        want = FOL.classes_from_leader(leader).class_id
        equal = bool(np.array_equal(ids, want)) and all(np.array_equal(p[0], want) for p in passes)
        # Stage A's first[] of the last batch, from the ids: an id below L_before is a Stage A match
        last = per[-1]
        first_a = np.where(ids[edges[-2]:] < last['L_before'], ids[edges[-2]:], -1)
        totals = [sum(b['assign_ms'] for b in p[1]) for p in passes]
        res = {
            'flags': int(prm.flags), 'classes': int(n_classes), 'batches': len(per), 'batch': a.batch,
            'rounds_one_shot': int(shots[-1][1][2]), 'unclassified': int((want < 0).sum()),
            'leader_kinds': extra['leader_kinds'], 'paper_classes': extra['paper_classes'],
            'paper_class_counts': extra['paper_class_counts'],
            'ids_equal_one_shot': equal, 'one_shot_classes': int(shots[-1][1][1]),
            'per_batch': per,
            'stream_total_ms': statistics.median(totals), 'stream_total_ms_all': totals,
            'stage_a_total_ms': sum(b['stage_a_ms'] for b in per),
            'one_shot_total_ms': statistics.median(t for t, _ in shots), 'one_shot_total_ms_all': [t for t, _ in shots],
            'last_batch': {'rows': last['rows'], 'L': loop['L'], 'stage_a_ms': last['stage_a_ms'],
                           'block32_loop_ms': loop['ms'], 'block32_launches': loop['launches'],
                           'block32_over_stage_a': loop['ms'] / last['stage_a_ms'] if last['stage_a_ms'] else None,
                           'first_equal': bool(np.array_equal(loop['first'], first_a))},
        }
        if linked:
            res.update(extra['links'])
            res['link_total_ms'] = sum(b['link_ms'] for b in per)
            res['link_over_stage_a'] = res['link_total_ms'] / res['stage_a_total_ms'] if res['stage_a_total_ms'] else None
        return res, equal

    out = {
        'data': os.path.basename(a.data), 'm': int(prm0.m), 'tau': float(prm0.tau),
        'min_points': int(prm0.min_points), 'rows': int(len(acc)), 'repeats': a.repeats,
        'device': torch.cuda.get_device_name(dev),
    }
    res, equal = measure(fol_params(prm0, axis=False))
    out.update(res)
    if a.axis:
        out['axis'], equal_axis = measure(fol_params(prm0, axis=True))
        equal = equal and equal_axis
    if a.link:
        out['link'], equal_link = measure(fol_params(prm0, axis=False, link=True))
        equal = equal and equal_link
        if a.axis:
            out['axis_link'], equal_link = measure(fol_params(prm0, axis=True, link=True))
            equal = equal and equal_link
    ctx.close()
    text = json.dumps(out)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')
    if not equal:
        sys.exit('the stream\'s class ids differ from the one-shot call\'s')


if __name__ == '__main__':
    main()

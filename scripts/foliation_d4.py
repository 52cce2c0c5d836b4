#!/usr/bin/env python3
"""Foliation classes of the depth-4 force-free set on one GPU.

Validates the 142,004 rows of data/force_free_d4_validated.npz on the device, classifies the
accepted rows at the default parameters (m = 16) with pdeval_foliation_classes and tags the
classes that re-parametrise a paper solution.  Times the field kernel alone and the whole
classification with HIP events (one warm-up run, then the median of --repeats runs) and prints
one JSON object, also written to --out.  With --axis the classification is measured a second
time in the same process with the axis rule (PDEVAL_FOL_AXIS: the functions of one coordinate
form one class per axis) and reported under "axis", next to the figures without it; "leader_kinds"
counts the class leaders that are functions of rho alone or of z alone.

    python scripts/foliation_d4.py --axis --out foliation_d4.json
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
from pdeval.opcodes import CLS_ACCEPT  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--data', default=os.path.join(ROOT, 'data', 'force_free_d4_validated.npz'))
    ap.add_argument('--device', type=int, default=0)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--axis', action='store_true', help='also measure with the axis rule (PDEVAL_FOL_AXIS)')
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

    def field_ms():
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
        """The classification under parameters p: one warm-up run, then the median of the repeats."""
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
        }

    field_ms()
    f_ms = [field_ms() for _ in range(a.repeats)]
    out = {
        'data': os.path.basename(a.data), 'm': int(prm.m), 'tau': float(prm.tau), 'min_points': int(prm.min_points),
        'rows': int(n), 'accepted': int(len(acc)),
        'field_kernel_ms': statistics.median(f_ms), 'field_kernel_ms_all': f_ms,
        'repeats': a.repeats,
        'device': torch.cuda.get_device_name(dev),
    }
    out.update(classes(fol_params(prm, axis=False)))
    if a.axis:
        out['axis'] = classes(fol_params(prm, axis=True))
    ctx.close()
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()

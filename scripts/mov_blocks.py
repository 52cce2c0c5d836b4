#!/usr/bin/env python3
"""Per-basic-block table of the register moves of one kernel, from its device assembly.

    make -C pde-engine_amd/csrc asm-grid EXTRA=-g1      # assembly with .loc line info
    python scripts/mov_blocks.py /tmp/pdeval_grid_gfx950.s [--kernel NAME] [--json OUT]

For every basic block of the kernel (default: force-free pass 1, grid_kernel<0, false, false>)
it prints the instruction count, the VALU and FP64 VALU counts, the v_mov_b64 count split by
source (constant 0, other constant, VGPR pair, SGPR pair) and the source lines (.loc) the moves
were emitted for, and the kernel's totals.  With line info the blocks map to their opcode
handler (the JetOps function a move's line belongs to).
"""
import argparse
import collections
import json
import re
import sys

KERNEL = '_ZN2pd11grid_kernelILi0ELb0ELb0EEEvNS_10KernelArgsEPlPii'
FP64 = re.compile(r'^v_(fma|fmac|mul|add|max|min|rcp|rsq|sqrt|div_scale|div_fmas|div_fixup|ldexp|frexp_mant|'
                  r'trig_preop|fract|floor|ceil|rndne|trunc|cmp\w*|cmpx\w*|cvt)_\w*f64')


def kernel_lines(path, name):
    out, on = [], False
    with open(path) as f:
        for ln in f:
            if not on:
                on = ln.startswith(name + ':')
                continue
            if ln.startswith('.Lfunc_end') or ln.lstrip().startswith('.end_amdhsa_kernel'):
                break
            out.append(ln.rstrip('\n'))
    if not out:
        sys.exit('kernel %s not found in %s' % (name, path))
    return out


def classify_mov(operands):
    src = operands.split(',')[1].strip()
    if src.startswith('v['):
        return 'vgpr'
    if src.startswith('s[') or src in ('vcc', 'exec'):
        return 'sgpr'
    return 'zero' if src in ('0', '0.0') else 'const'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('asm')
    ap.add_argument('--kernel', default=KERNEL)
    ap.add_argument('--json')
    ap.add_argument('--min-moves', type=int, default=4, help='blocks with fewer moves are summed, not listed')
    a = ap.parse_args()

    files = {}
    blocks = []
    cur = None
    loc = None
    cur_loop = 'no loop'

    def new_block(label):
        nonlocal cur
        cur = dict(label=label, loop=cur_loop, n=0, valu=0, fp64=0, salu=0, lds=0, mov64=collections.Counter(),
                   mov32=0, lines=collections.Counter())
        blocks.append(cur)

    with open(a.asm) as f:
        for ln in f:
            m = re.match(r'\s+\.file\s+(\d+)\s+"[^"]*"\s+"([^"]+)"', ln)
            if m:
                files[m.group(1)] = m.group(2)
    new_block('entry')
    for ln in kernel_lines(a.asm, a.kernel):
        s = ln.strip()
        if not s or s.startswith(';'):
            continue
        m = re.match(r'^(\.LBB\w+):', s)
        if m:
            new_block(m.group(1))
            h = re.search(r'Header=(BB\w+) Depth=(\d+)', s)
            if h:
                cur_loop = '%s depth %s' % h.groups()
            elif 'Loop Header' in s or 'Parent Loop' in s:
                cur_loop = 'header ' + m.group(1)[2:]
            else:
                cur_loop = 'no loop'
            cur['loop'] = cur_loop
            continue
        m = re.match(r'^\.loc\s+(\d+)\s+(\d+)', s)
        if m:
            loc = '%s:%s' % (files.get(m.group(1), m.group(1)), m.group(2))
            continue
        if s.startswith('.') or s.endswith(':'):
            continue
        op, _, rest = s.partition(' ')
        cur['n'] += 1
        if op.startswith('v_'):
            cur['valu'] += 1
            if FP64.match(op):
                cur['fp64'] += 1
            if op.startswith('v_mov_b64'):
                cur['mov64'][classify_mov(rest.split(';')[0])] += 1
                cur['lines'][loc] += 1
            elif op.startswith('v_mov_b32'):
                cur['mov32'] += 1
        elif op.startswith('s_'):
            cur['salu'] += 1
        elif op.startswith('ds_'):
            cur['lds'] += 1
        if op.startswith(('s_branch', 's_cbranch', 's_endpgm', 's_setpc')):
            new_block(cur['label'] + '+')

    tot = collections.Counter()
    kinds = collections.Counter()
    by_line = collections.Counter()
    for b in blocks:
        for k in ('n', 'valu', 'fp64', 'salu', 'lds', 'mov32'):
            tot[k] += b[k]
        kinds.update(b['mov64'])
        by_line.update(b['lines'])
    n64 = sum(kinds.values())
    print('kernel %s' % a.kernel)
    print('instructions %d  VALU %d  FP64 VALU %d  SALU %d  LDS %d  v_mov_b32 %d' %
          (tot['n'], tot['valu'], tot['fp64'], tot['salu'], tot['lds'], tot['mov32']))
    print('v_mov_b64 %d: zero %d, vgpr %d, sgpr %d, other constant %d' %
          (n64, kinds['zero'], kinds['vgpr'], kinds['sgpr'], kinds['const']))
    print('\nloop (innermost header of the blocks)   insts  VALU  FP64  mov64  zero  vgpr')
    loops = collections.OrderedDict()
    for b in blocks:
        t = loops.setdefault(b['loop'], collections.Counter())
        for k in ('n', 'valu', 'fp64'):
            t[k] += b[k]
        t['mov64'] += sum(b['mov64'].values())
        t['zero'] += b['mov64']['zero']
        t['vgpr'] += b['mov64']['vgpr']
    for k, t in loops.items():
        if t['n'] >= 50:
            print('%-38s %6d %5d %5d %6d %5d %5d' % (k, t['n'], t['valu'], t['fp64'], t['mov64'], t['zero'], t['vgpr']))
    print('\nblock                     insts VALU FP64  mov64 (0/vgpr/sgpr/const)  lines of the moves')
    rest = 0
    for b in sorted(blocks, key=lambda b: -sum(b['mov64'].values())):
        m = sum(b['mov64'].values())
        if m < a.min_moves:
            rest += m
            continue
        top = ', '.join('%s x%d' % kv for kv in b['lines'].most_common(4))
        print('%-25s %5d %4d %4d  %3d (%d/%d/%d/%d)  %s' % (b['label'], b['n'], b['valu'], b['fp64'], m, b['mov64']['zero'],
              b['mov64']['vgpr'], b['mov64']['sgpr'], b['mov64']['const'], top))
    print('(%d moves in blocks with fewer than %d)' % (rest, a.min_moves))
    print('\nv_mov_b64 by source line')
    for k, v in by_line.most_common(40):
        print('  %-28s %d' % (k, v))
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(dict(kernel=a.kernel, totals=dict(tot), mov64=n64, mov64_kinds=dict(kinds),
                           mov64_by_line=dict(by_line),
                           blocks=[dict(label=b['label'], insts=b['n'], valu=b['valu'], fp64=b['fp64'],
                                        mov64=dict(b['mov64']), lines=dict(b['lines']))
                                   for b in blocks if sum(b['mov64'].values())]), f, indent=1)


if __name__ == '__main__':
    main()

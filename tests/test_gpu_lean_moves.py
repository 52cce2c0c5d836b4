"""The force-free interpreter's opcode loop without its per-opcode register moves
(pdeval_grid.h PD_LEAN_MOVES: the pinned ordinate is carried through the loop).

A table of hand-assembled programs puts every handler of the lean passes -- PUSH_X/Y/P/C, RDIVC,
RDIV_P, DIV, RDIV, POWN 2-5, POW, SQRT, EXP, LOG -- at stack depth 1 and as the right operand at
depth 2, each directly after a push, after a hoisted prefix of rho alone (exp(rho)*z shapes) and
after a NEG (which the decoder folds), with rows that are not finite on part of the grid (log,
sqrt and a fractional power of z, of exp(rho)*z).  The batch is repeated past 1024 candidates, so
that pass 1 runs one wave per candidate with its hoisted prefixes, and every output is held to
the CPU oracle's: classes and counts exactly, res_ref by tests/test_gpu_parity.py's rule, q_grid
and q_ref by tests/test_gpu_jet_opcodes.py's rule for q_grid, the fingerprint values (u at four
grid points) by the rule for jets of tests/jet_opcode_cases.py (REL_TOL).
"""
import collections

import numpy as np
import pytest

import jet_opcode_cases as JC
import oracle_lib as O
from pdeval import _lib
from pdeval import workload as WL
from pdeval.opcodes import CLS_ZERO_GRADIENT

pytestmark = pytest.mark.gpu

REL_TOL = 1e-10          # tests/test_gpu_parity.py: residuals of point rejects against the oracle
REF = (0.8, 6.0 / 7.0)   # the force-free reference point p*

_o = JC._o
PX, PY = JC.PX, JC.PY
X, Y = JC.X, JC.Y
UNARY = {'RDIVC': _o('RDIVC', imm=2.5), 'RDIV_P': _o('RDIV_P', (3, Y)), 'POWN2': _o('POWN', 2),
         'POWN3': _o('POWN', 3), 'POWN4': _o('POWN', 4), 'POWN5': _o('POWN', 5), 'POW': _o('POW', imm=1.5),
         'SQRT': _o('SQRT'), 'EXP': _o('EXP'), 'LOG': _o('LOG')}
PUSHES = {'PUSH_X': PX, 'PUSH_Y': PY, 'PUSH_P': _o('PUSH_P', (3, X)), 'PUSH_C': _o('PUSH_C', imm=2.5)}
BINARY = ('DIV', 'RDIV')
HANDLERS = list(PUSHES) + list(UNARY) + list(BINARY)
NEG7 = [PX, _o('MUL_Y'), _o('ADDC', imm=-7.0), _o('NEG')]       # 7 - x y, in (1, 13) on the grid
POS7 = [PX, _o('MUL_Y'), _o('ADDC', imm=7.0)]                   # 7 + x y
PREFIX = [PX, _o('EXP')]                                        # exp(x): hoisted once per grid row
LEFT = [PX, _o('ADD_Y')]                                        # the left operand of the depth-2 rows


def _table():
    """(handler, context, program, stack depth): context 'push' / 'prefix' / 'neg' / 'start'."""
    t = []
    for h, u in UNARY.items():
        t += [(h, 'push', [PX, u, _o('MUL_Y')], 1), (h, 'push', [PY, u, _o('MUL_X')], 1),
              (h, 'prefix', PREFIX + [_o('MUL_Y'), u], 1), (h, 'neg', NEG7 + [u], 1),
              (h, 'push', LEFT + [PX, u, _o('MUL')], 2), (h, 'push', LEFT + [PY, u, _o('ADD')], 2),
              (h, 'prefix', PREFIX + [PY, u, _o('MUL')], 2), (h, 'neg', LEFT + NEG7 + [u, _o('ADD')], 2)]
    for h in BINARY:
        b = _o(h)
        t += [(h, 'push', POS7 + [PY, b], 2), (h, 'prefix', PREFIX + [PY, b], 2), (h, 'neg', POS7 + NEG7 + [b], 2),
              (h, 'push', LEFT + POS7 + [PY, b, _o('ADD')], 3), (h, 'prefix', PREFIX + POS7 + [PY, b, _o('MUL')], 3),
              (h, 'neg', LEFT + POS7 + NEG7 + [b, _o('ADD')], 3)]
    for h, p in PUSHES.items():
        tail = [_o('MUL_Y'), _o('ADD_X')] if h != 'PUSH_Y' else [_o('MUL_X'), _o('ADD_Y')]
        t += [(h, 'start', [p] + tail, 1), (h, 'push', [PY if h != 'PUSH_Y' else PX, p, _o('MUL')], 2),
              (h, 'prefix', PREFIX + [_o('MUL_Y'), p, _o('ADD')], 2), (h, 'neg', NEG7 + [p, _o('MUL')], 2)]
    return t


TABLE = _table()


def _walk(prog):
    """[(opcode name with POWN's exponent, stack depth after it, the opcode before it)]."""
    out, d, prev = [], 0, None
    for name, operand, _ in prog:
        nm = name + str(operand) if name == 'POWN' else name
        d += 1 if name.startswith('PUSH') else -1 if name in ('ADD', 'SUB', 'MUL', 'DIV', 'RDIV', 'RSUB') else 0
        out.append((nm, d, prev))
        prev = name
    return out


@pytest.fixture(scope='module')
def runs():
    words = [JC.assemble(p, d) for _, _, p, d in TABLE]
    reps = 1024 // len(words) + 1
    ops = np.concatenate(words * reps)
    off = np.concatenate([[0], np.cumsum([len(w) for w in words] * reps)]).astype(np.int64)
    nu = len(words)
    ctx = _lib.Context(0)
    try:
        dev = ctx.validate(ops, off)
        counts = ctx.pass_counts()
    finally:
        ctx.close()
    dev = {k: v for k, v in dev.items() if isinstance(v, np.ndarray) and len(v) == len(off) - 1}
    for k, v in dev.items():     # every repetition of the table gives the same bits
        assert np.array_equal(v[:nu], v[-nu:], equal_nan=v.dtype.kind == 'f'), k
    ora = O.validate(0, ops[:off[nu]], off[:nu + 1])
    hoist = WL.flops_per_program(0, ops[:off[nu]], off[:nu + 1], hoisted=True)
    return words, {k: v[:nu] for k, v in dev.items()}, ora, hoist, counts, len(off) - 1


def test_table_places_every_handler(runs):
    """Every handler at depths 1 and 2 (the binary ones: result at depth 1 and 2), after a push,
    after a hoisted prefix and after a NEG -- read back from the programs, not from the labels."""
    _, _, _, hoist, counts, n = runs
    assert n > 1024 and len(TABLE) >= 100
    depths, ctxs = collections.defaultdict(set), collections.defaultdict(set)
    for row, (h, c, prog, _) in enumerate(TABLE):
        first = 0 if c == 'start' else len(PREFIX) if c == 'prefix' else 1
        hits = [(i, d, prev) for i, (nm, d, prev) in enumerate(_walk(prog)) if nm == h and i >= first]
        if h in PUSHES and c != 'start':
            hits = [t for t in hits if t[1] == 2]
        assert len(hits) == 1, (h, c, prog)
        i, d, prev = hits[0]
        depths[h].add(d)
        if c == 'push':
            assert prev.startswith('PUSH'), (h, prog)
        elif c == 'neg':
            assert prev == 'NEG', (h, prog)
        elif c == 'prefix':
            assert hoist[row] > 0 and i >= len(PREFIX) and prog[:len(PREFIX)] == PREFIX, (h, prog, hoist[row])
        ctxs[h].add(c)
    for h in HANDLERS:
        assert depths[h] >= {1, 2}, (h, depths[h])
        assert ctxs[h] >= {'push', 'prefix', 'neg'}, (h, ctxs[h])
    # the batch ran in pass 1 and, the depth-3 rows, in pass 2; nothing was handed to the generic kernel
    assert counts['defer_stack3'] > 0 and counts['grid_slow'] == 0 and counts['grid_slow_stack3'] == 0, counts


def test_classes_and_counts_equal_oracle(runs):
    _, dev, ora, _, _, _ = runs
    for k in ('status', 'n_bad', 'n_nonfinite'):
        diff = np.flatnonzero(dev[k] != ora[k])
        assert not diff.size, (k, [(TABLE[i][:2], int(dev[k][i]), int(ora[k][i])) for i in diff[:10]])
    assert not (ora['status'] == CLS_ZERO_GRADIENT).any()
    assert (dev['n_nonfinite'] > 0).sum() >= 10      # the rows not finite on part of the grid took part


def test_point_residuals_equal_oracle(runs):
    _, dev, ora, _, _, _ = runs
    d, o = dev['res_ref'], ora['res_ref']
    n = 0
    for i in range(len(o)):
        if ora['status'][i] != 1 or not np.all(np.isfinite(o[i])) or not np.all(np.isfinite(d[i])):
            continue
        err = abs(abs(d[i, 0]) - abs(o[i, 0])) / max(abs(o[i, 0]), 1e-300)
        assert err <= REL_TOL, (TABLE[i][:2], d[i, 0], o[i, 0], err)
        n += 1
    assert n >= 50


def _noise_over_scale(w, kappa, points):
    m = 0.0
    for x, y in points:
        _, S, noise, fin = O.point(0, w, float(x), float(y))
        if fin and S > 0:
            m = max(m, kappa * noise / S)
    return m


def test_q_grid_and_q_ref_equal_oracle(runs):
    """|q_dev - q_oracle| <= 4 * 2^-52 q_oracle + max_p(noise_kappa noise_p / S_p), p over the grid
    (q_grid) or p = p* (q_ref): the rule of tests/test_gpu_jet_opcodes.py."""
    words, dev, ora, _, _, _ = runs
    kappa = float(_lib.default_params(0).noise_kappa)
    gx = 0.05 + (np.arange(64) + 0.37) * (3.0 - 0.05) / 64
    gy = -2.0 + (np.arange(64) + 0.41) * (2.0 - -2.0) / 64
    grid = [(x, y) for x in gx for y in gy]
    bad, worst = [], {'q_grid': 0.0, 'q_ref': 0.0}
    for key, pts in (('q_grid', grid), ('q_ref', [REF])):
        for i, w in enumerate(words):
            d, o = float(dev[key][i]), float(ora[key][i])
            if not np.isfinite(o):
                if np.isfinite(d):
                    bad.append((key, TABLE[i][:2], d, o))
                continue
            if o > 0 and np.isfinite(d):
                worst[key] = max(worst[key], abs(d - o) / o)
            lim = 4 * JC.EPS * o
            if not abs(d - o) <= lim:
                lim += _noise_over_scale(w, kappa, pts)      # (only where needed)
            if not abs(d - o) <= lim:
                bad.append((key, TABLE[i][:2], d, o, lim))
    print(f'\nlargest |q_dev - q_oracle| / q_oracle: {worst}, {len(bad)} beyond the bound')
    assert not bad, (len(bad), bad[:10])


def test_fingerprints_equal_oracle(runs):
    """u at the four fingerprint points: within JC.REL_TOL (1e-11 relative, the rule for the
    oracle's jets) of the oracle's value; not finite exactly where the oracle's is not."""
    _, dev, ora, _, _, _ = runs
    d, o = dev['fingerprint'], ora['fingerprint']
    fin = np.isfinite(o)
    assert np.array_equal(np.isfinite(d), fin), [TABLE[i][:2] for i in np.flatnonzero((np.isfinite(d) != fin).any(axis=1))[:10]]
    err = np.abs(d[fin] - o[fin]) / np.maximum(np.abs(o[fin]), 1e-300)
    print(f'\nfingerprint: largest relative difference {err.max():.3e} over {fin.sum()} values')
    rows = np.flatnonzero((np.where(fin, np.abs(d - o), 0.0) > JC.REL_TOL * np.abs(o)).any(axis=1))
    assert not rows.size, [(TABLE[i][:2], d[i].tolist(), o[i].tolist()) for i in rows[:10]]
    assert fin.sum() >= 2 * len(TABLE)

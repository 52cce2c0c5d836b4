"""The one-coordinate pass (csrc/pdeval_grid.h PD_ONECOORD, grid_one_kernel): force-free candidates
u = f(rho) or u = f(z) evaluated at 64 grid points instead of 4,096 give, bit for bit, every
output of the run with PDEVAL_ONECOORD=0, in which pass 1 evaluates them on the whole grid."""
import os

import numpy as np
import pytest

import golden_data as G
from pdeval import _lib, problem_defs as P, workload as WL
from pdeval._lib import Context

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ('status', 'verdict', 'n_bad', 'n_nonfinite', 'q_grid', 'q_ref', 'res_ref', 'fingerprint')

# ---- the decoder's classification (decode_kernel: msk[], the lean checks), restated
_PUSH_X, _PUSH_Y, _PUSH_C, _PUSH_P = 1, 2, 3, 29
_BIN = {4, 5, 6, 7, 8, 9}
_IMM = {3, 10, 11, 12, 21}
_X_OPS, _Y_OPS = {14, 16, 18, 26}, {15, 17, 19, 27}
_P_OPS = {30, 31, 32, 33, 34}
_UNARY = {10, 11, 12, 13, 20, 21, 22, 23, 24, 25} | _X_OPS | _Y_OPS | _P_OPS
_FLAG_COMPLEX, _FLAG_NOCOORD = 1 << 16, 1 << 17
_PS_COMPLEX = 4


def one_coord_kind(words) -> int:
    """1: a real program the lean pass takes, of stack <= 2, whose value depends on x alone;
    2: on y alone; 0: anything else."""
    w = [int(v) & 0xffffffff for v in words]
    hdr = w[0]
    if len(w) < 2 or (hdr & 0xff) != 0 or (hdr & (_FLAG_COMPLEX | _FLAG_NOCOORD)):
        return 0
    msk, d, dmax, pc = [0] * 5, 0, 0, 1
    while pc < len(w):
        op = w[pc] & 0xff
        ln = (5 if w[pc] & 0x100 else 3) if op in _IMM else 1
        if pc + ln > len(w):
            return 0
        if op in _IMM and (w[pc] & 0x200) and (op == 21 or (w[pc] & 0x100) or w[pc + 1] > 15):
            return 0
        n, on_y = (w[pc] >> 8) & 0xff, (w[pc] >> 16) & 1
        if op == 20 and n > 8:
            return 0
        if (op in _P_OPS or op == _PUSH_P) and not 2 <= n < 17:
            return 0
        if op in (_PUSH_X, _PUSH_Y, _PUSH_C, _PUSH_P):
            d += 1
            if d > 3:
                return 0
            dmax = max(dmax, d)
            msk[d] = 1 if op == _PUSH_X else 2 if op == _PUSH_Y else 0 if op == _PUSH_C else (2 if on_y else 1)
        elif op in _BIN:
            if d < 2:
                return 0
            d -= 1
            msk[d] |= msk[d + 1]
        elif op in _UNARY:
            if d < 1:
                return 0
            msk[d] |= 1 if op in _X_OPS else 2 if op in _Y_OPS else (2 if on_y else 1) if op in _P_OPS else 0
        else:
            return 0
        pc += ln
    if d != 1 or dmax > 2 or ((hdr >> 8) & 0xff) > 2:
        return 0
    return msk[1] if msk[1] in (1, 2) else 0


def kinds(ops, off) -> np.ndarray:
    return np.array([one_coord_kind(ops[off[i]:off[i + 1]]) for i in range(len(off) - 1)], dtype=np.uint8)


def _concat(parts):
    ops = np.concatenate([p[0] for p in parts]).astype(np.int32)
    lens = np.concatenate([np.diff(p[1]) for p in parts])
    return ops, np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def _run(ops, off, onecoord: bool, params=None):
    """Every output of one batch in a fresh context (PDEVAL_* are read when it is created), the
    work-list sizes and the point-stage states of the call."""
    old = os.environ.get('PDEVAL_ONECOORD')
    os.environ['PDEVAL_ONECOORD'] = '1' if onecoord else '0'
    try:
        ctx = Context(0)
    finally:
        if old is None:
            os.environ.pop('PDEVAL_ONECOORD', None)
        else:
            os.environ['PDEVAL_ONECOORD'] = old
    try:
        r = ctx.validate(ops, off, params)
        r['counts'] = ctx.pass_counts()
        r['pstate'] = ctx.point_states(len(off) - 1)
        return r
    finally:
        ctx.close()


def _assert_same(on, off_):
    for k in KEYS:
        same = np.array_equal(on[k], off_[k], equal_nan=on[k].dtype.kind == 'f')
        assert same, (k, np.flatnonzero(np.any((on[k] != off_[k]).reshape(len(on[k]), -1), axis=1))[:10])


def _eligible(kind, pstate) -> np.ndarray:
    # (default params: full_grid, so a point reject's grid runs too)
    return (kind > 0) & ((pstate & _PS_COMPLEX) == 0) & ((pstate & 3) != 0)


@pytest.fixture(scope='module')
def d4():
    d = np.load(os.path.join(ROOT, 'data', 'force_free_d4_validated.npz'))
    ops, off = d['ops'], d['offsets']
    return ops, off, kinds(ops, off)


# grid abscissa 10 and ordinate 40 of the default grid (pdeval.hip default_grid / build_points)
GX10 = 0.05 + (10 + 0.37) * ((3.0 - 0.05) / 64)
GY40 = -2.0 + (40 + 0.41) * ((2.0 - -2.0) / 64)
HAND = ['rho + 1', 'exp(rho)', 'sqrt(z + 1)', 'log(z)', f'1/(rho - {GX10!r})', f'1/(z - {GY40!r})',
        'log(rho - 1/2)', '3', 'exp(rho)*z', '(exp(rho) + 1)/(rho + 2) + (sqrt(rho) + 3)/(log(rho) + 4)']
HAND_KIND = [1, 1, 2, 2, 1, 2, 1, 0, 0, 0]


@pytest.fixture(scope='module')
def mixed(d4):
    """The first 2,000 programs of x alone and of y alone of the d4 set and the hand-written ones,
    run with the pass on and off."""
    ops, off, kind = d4
    hops, hoff, _ = P.compile_strings(P.force_free(), HAND)
    assert [one_coord_kind(hops[hoff[i]:hoff[i + 1]]) for i in range(len(HAND))] == HAND_KIND
    assert (int(hops[hoff[-2]]) >> 8) & 0xff == 3   # the last one: of rho alone, stack 3
    idx = np.concatenate([np.flatnonzero(kind == 1)[:2000], np.flatnonzero(kind == 2)[:2000]])
    assert len(idx) == 4000
    bops, boff = _concat([WL.gather_programs(ops, off, idx), (hops, hoff)])
    bkind = np.concatenate([kind[idx], HAND_KIND]).astype(np.uint8)
    return bops, boff, bkind, _run(bops, boff, True), _run(bops, boff, False)


def test_onecoord_on_equals_off(mixed):
    """One batch of 4,000 one-coordinate programs of the d4 set and hand-written ones (light and
    heavy, non-finite on some rows / lanes only, and three the rule does not take): every output
    is exactly equal, the new list holds exactly the programs the restated rule takes, and they
    are the only ones pass 1 loses."""
    ops, off, kind, on, off_ = mixed
    n = len(off) - 1
    _assert_same(on, off_)
    for r in (on, off_):   # the rows meant to be non-finite in part are so
        for i in (n - 8, n - 7, n - 6, n - 5, n - 4):
            assert 0 < r['n_nonfinite'][i] < 4096, (HAND[i - (n - len(HAND))], r['n_nonfinite'][i])
    assert on['n_nonfinite'][n - 6] == 64 and on['n_nonfinite'][n - 5] == 64   # one row, one lane
    assert np.array_equal(on['pstate'], off_['pstate'])
    elig = _eligible(kind, on['pstate'])
    assert elig[:4000].mean() > 0.9
    assert on['counts']['one_coord'] == int(elig.sum())
    assert off_['counts']['one_coord'] == 0
    # pass 1 evaluates what no list takes from it: the one-coordinate list is the only difference
    leave = ('defer_stack3', 'complex', 'grid_slow')
    p1_on = n - sum(on['counts'][k] for k in leave) - on['counts']['one_coord']
    p1_off = n - sum(off_['counts'][k] for k in leave)
    assert p1_on + on['counts']['one_coord'] == p1_off


def test_onecoord_tier2_handoff(mixed):
    """The tier-2 lists of the same batch have the same sizes on and off (the library reports
    their sizes, not their entries; the classes and counts tier 2 would rewrite are compared
    entry by entry in test_onecoord_on_equals_off)."""
    _, _, _, on, off_ = mixed
    for k in ('tier2', 'tier2_stack3', 'tier2_stack8', 'tier2_complex', 'tier2_complex_stack8'):
        assert on['counts'][k] == off_['counts'][k], k


def test_onecoord_d4_set(d4):
    """The whole d4 set (142,004 programs) in one device call: on equals off exactly."""
    ops, off, kind = d4
    on, off_ = _run(ops, off, True), _run(ops, off, False)
    _assert_same(on, off_)
    assert on['counts']['one_coord'] == int(_eligible(kind, on['pstate']).sum()) > 10000
    assert off_['counts']['one_coord'] == 0


def test_onecoord_not_with_omega(mixed):
    """Omega != 0 (rotate_A makes a function of z alone depend on rho): the list stays empty, and
    the one-coordinate rows of the Omega = 1 reference fixtures keep the reference's verdict and
    text (the expectations of test_plugin_omega1_reference_verdicts)."""
    ops, off, _, _, _ = mixed
    prm = _lib.default_params(0)
    prm.omega2 = 1.0
    assert _run(ops, off, True, prm)['counts']['one_coord'] == 0
    from problems import load_problem
    from problems.force_free.validator import PreciseFoliationValidator
    import sympy as sp
    rows = G.decided(G.ref_rows('ff_omega1_known.jsonl', 'ff_omega1_d3_s600.jsonl'))
    rops, roff, _ = P.compile_strings(P.force_free(), [r['expr'] for r in rows])
    rows = [r for r, k in zip(rows, kinds(rops, roff)) if k]
    assert len(rows) >= 10
    prob = load_problem('force_free')
    locs = {**prob.symbols, **prob.constants, **prob.unary_ops}
    v = PreciseFoliationValidator(Omega=1)
    got = v.validate_batch([sp.sympify(r['expr'], locals=locs) for r in rows], check_regularity=False,
                           fast_point_only=False)
    bad = [(r['expr'], r['reason'], g) for g, r in zip(got, rows) if g != (r['ok'], r['reason'])]
    # (only the symbolic stage's branch text of a grid reject, as in the parity test)
    assert all(g[0] is False and 'expanded det' in rr for _, rr, g in bad) and len(bad) <= 2, bad[:5]

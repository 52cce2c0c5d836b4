"""Hand-assembled programs for every jet opcode and an independent 50-digit reference.

The table TABLE holds opcode words written by hand (no compiler in between, so nothing can
fold an opcode away); `ref_jet` is a second interpreter of the same words in truncated Taylor
arithmetic on mpmath numbers at 60 digits.  It shares no code and no recurrence with
csrc/jet.h or the oracle: a quotient is a product with the composed reciprocal series, powers
and POWN use closed-form binomial coefficients, EXP / LOG their closed-form series, and a
composition sums explicit powers of the inner jet.

The reference of the whole table at the 70 POINTS is kept in tests/golden/jet_opcodes.npz
(tests/golden/gen_jet_opcodes.py writes it; test_jet_opcodes_host.py recomputes a fixed sample
and requires the stored digits).

Coefficient order is the device's: d = i + j ascending, j ascending within d.
"""
import os
import struct

import mpmath as mp
import numpy as np

from pdeval.opcodes import FLAG_COMPLEX, IMM_DD, PDOP, P_OPS, op_len

MP = mp.mp.clone()
MP.dps = 60
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'jet_opcodes.npz')
MARGIN = 1e-3           # smallest allowed distance to a pole, branch point or Abs kink
NC = 15
IDX = [(d - j, j) for d in range(5) for j in range(d + 1)]          # k -> (i, j)
JI = {ij: k for k, ij in enumerate(IDX)}
# k -> the (k1, k2) pairs of a truncated product
_MUL = [[(JI[(i1, j1)], JI[(i - i1, j - j1)]) for i1 in range(i + 1) for j1 in range(j + 1)] for i, j in IDX]

THIRD = 'third'         # the immediate 1/3 as a double-double: PDEVAL_IMM_DD, low word first
THIRD_HI = 1.0 / 3.0
THIRD_LO = float(MP.mpf(1) / 3 - MP.mpf(THIRD_HI))
SQRT2 = 1.4142135623730951    # the irrational exponent of POW (a double)
X, Y = 0, 1


# ------------------------------------------------------------------ assembler
def _f64_words(v):
    lo, hi = struct.unpack('<ii', struct.pack('<d', float(v)))
    return [lo, hi]


def assemble(prog, depth, flags=0):
    """int32 words of [(opcode name, operand, immediate), ...]; operand: n for POWN, (n, axis)
    for PUSH_P / *_P, None otherwise; immediate: a double, THIRD or None.  The header's stack
    depth is the library's pdeval_program_depth, which must equal `depth`."""
    from pdeval import _lib
    w = [0]
    for name, operand, imm in prog:
        op = PDOP[name]
        word = op
        if op == PDOP['POWN']:
            word |= int(operand) << 8
        elif op in P_OPS:
            n, axis = operand
            word |= (int(n) << 8) | (int(axis) << 16)
        if imm is None:
            w.append(word)
        elif imm == THIRD:
            w += [word | IMM_DD] + _f64_words(THIRD_HI) + _f64_words(THIRD_LO)
        else:
            w += [word] + _f64_words(imm)
    # (the library checks the header against the depth it finds: -8 where they differ)
    w[0] = (depth << 8) | flags
    w = np.array(w, dtype=np.int32)
    got = _lib.program_depth(w)
    assert got == depth == (int(w[0]) >> 8) & 0xff, (prog, got, depth)
    return w


def rounded_twin(words):
    """The program with every PDEVAL_IMM_DD immediate rounded to its double: low words dropped,
    flag cleared."""
    out, pc = [int(words[0])], 1
    while pc < len(words):
        w = int(words[pc])
        n = op_len(w)
        if n == 5:
            out += [w & ~IMM_DD, int(words[pc + 1]), int(words[pc + 2])]
        else:
            out += [int(v) for v in words[pc:pc + n]]
        pc += n
    return np.array(out, dtype=np.int32)


def decode(words):
    """[(opcode, operand bits 8-23, hi, lo or None)] of a program (header skipped)."""
    out, pc = [], 1
    while pc < len(words):
        w = int(words[pc]) & 0xffffffff
        n = op_len(w)
        hi = lo = None
        if n >= 3:
            hi = struct.unpack('<d', struct.pack('<ii', int(words[pc + 1]), int(words[pc + 2])))[0]
        if n == 5:
            lo = struct.unpack('<d', struct.pack('<ii', int(words[pc + 3]), int(words[pc + 4])))[0]
        out.append((w & 0xff, (w >> 8) & 0xffff, hi, lo))
        pc += n
    return out


# ------------------------------------------------------------------ the program table
def _o(name, operand=None, imm=None):
    return (name, operand, imm)


PX, PY = _o('PUSH_X'), _o('PUSH_Y')
# g = x*y + x/(x + y**2 + 1) + 7: in [1, 14] on the point range, every coefficient non-zero
INNER = [PX, _o('MUL_Y'), PX, PX, _o('ADD_P', (2, Y)), _o('ADDC', imm=1.0), _o('DIV'), _o('ADD'),
         _o('ADDC', imm=7.0)]
# eight pairwise different operands, each pushed as one more stack slot
OPERANDS = [[PX], [PY], [PX, _o('ADDC', imm=1.0)], [PY, _o('MULC', imm=2.0), _o('ADDC', imm=5.0)],
            [PX, _o('MUL_Y'), _o('ADDC', imm=7.0)], [PX, _o('EXP')], [_o('PUSH_P', (2, Y)), _o('ADDC', imm=2.0)],
            [PX, _o('SQRT'), _o('ADDC', imm=1.0)]]
P_NS = (2, 3, 4, 5, 15, 16)
POW_ALPHAS = (1.5, -0.5, 1.75, SQRT2)


def _table():
    t = []   # (name, program, depth, flags, single-opcode, true solution)

    def add(name, prog, depth, flags=0, single=False, true=False):
        t.append((name, prog, depth, flags, single, true))
    add('push_x', [PX], 1, single=True)
    add('push_y', [PY], 1, single=True)
    add('push_c.mul_x', [_o('PUSH_C', imm=2.5), _o('MUL_X')], 1, single=True)
    add('add', [PX, PY, _o('ADD')], 2, single=True)
    add('mul', [PX, PY, _o('MUL')], 2, single=True)
    add('addc', [PX, _o('ADDC', imm=2.5)], 1, single=True)
    add('mulc', [PY, _o('MULC', imm=2.5)], 1, single=True)
    add('rdivc', [PX, _o('RDIVC', imm=2.5)], 1, single=True)
    add('neg', [PX, _o('NEG')], 1, single=True)
    for name, lead in (('ADD_X', PY), ('ADD_Y', PX), ('MUL_X', PY), ('MUL_Y', PX), ('SUB_X', PY), ('SUB_Y', PX),
                       ('DIV_X', PY), ('DIV_Y', PX)):
        add(name.lower(), [lead, _o(name)], 1, single=True)
    for k, n in enumerate(P_NS):
        add(f'pown{n}', [PY if k & 1 else PX, _o('POWN', n)], 1, single=True)
    for a in POW_ALPHAS:
        add(f'pow{a:.4g}', [PX, _o('POW', imm=a)], 1, single=True)
    add('exp', [PY, _o('EXP')], 1, single=True)
    add('log', [PX, _o('LOG')], 1, single=True)
    add('abs', [PY, _o('ABS')], 1, single=True)
    add('sqrt', [PX, _o('SQRT')], 1, single=True)
    # fused coordinate powers: every opcode with every n, the axes alternating (the operand is
    # the other coordinate, so the result depends on both)
    for k, n in enumerate(P_NS):
        add(f'push_p{n}', [_o('PUSH_P', (n, k & 1))], 1, single=True)
    for name in ('ADD_P', 'SUB_P', 'MUL_P', 'DIV_P', 'RDIV_P'):
        for k, n in enumerate(P_NS):
            ax = (k + 1) & 1 if name in ('MUL_P', 'RDIV_P') else k & 1
            add(f'{name.lower()}{n}{"xy"[ax]}', [PX if ax else PY, _o(name, (n, ax))], 1, single=True)
    # immediates that are no double: 1/3 with its low part, in programs whose determinant moves
    # with the constant (part 3's twins)
    add('dd.push_c', [_o('PUSH_C', imm=THIRD), _o('MUL_X'), _o('MUL_Y')], 1)
    add('dd.addc', [PX, _o('MUL_Y'), _o('ADDC', imm=THIRD), _o('POWN', 2)], 1)
    add('dd.mulc', [PX, _o('MUL_Y'), _o('MULC', imm=THIRD), _o('EXP')], 1)
    add('dd.rdivc', [PX, _o('MUL_Y'), _o('ADDC', imm=7.0), _o('RDIVC', imm=THIRD)], 1)
    # the non-commutative binary opcodes at every stack depth: d operands, folded d - 1 times
    for name in ('SUB', 'RSUB', 'DIV', 'RDIV'):
        for d in range(2, 9):
            add(f'{name.lower()}.d{d}', sum(OPERANDS[:d], []) + [_o(name)] * (d - 1), d, single=d == 2)
    add('mix.d8', sum(OPERANDS, []) + [_o(n) for n in ('DIV', 'RSUB', 'MUL', 'SUB', 'RDIV', 'ADD', 'DIV')], 8)
    # compositions on an inner jet with every coefficient non-zero
    add('c.exp', INNER + [_o('EXP')], 3)
    add('c.log', INNER + [_o('LOG')], 3)
    add('c.sqrt', INNER + [_o('SQRT')], 3)
    add('c.pow-0.5', INNER + [_o('POW', imm=-0.5)], 3)
    add('c.pow1.414', INNER + [_o('POW', imm=SQRT2)], 3)
    add('c.pown5', INNER + [_o('POWN', 5)], 3)
    add('c.pown16', INNER + [_o('POWN', 16)], 3)
    add('c.abs', [PX, _o('MUL_Y'), _o('ABS'), _o('ADD_P', (3, X))], 1)
    add('c.rdiv_p', INNER + [_o('RDIV_P', (5, Y))], 3)
    add('c.div_p', INNER + [_o('DIV_P', (4, X))], 3)
    # complex-valued programs (PDEVAL_FLAG_COMPLEX): the only ones with PUSH_I
    zc = [PX, _o('PUSH_I'), _o('MUL_Y'), _o('ADD')]                       # x + i y
    add('z.pown2', zc + [_o('POWN', 2)], 2, FLAG_COMPLEX)
    add('z.sqrt', zc + [_o('SQRT'), _o('MUL_X')], 2, FLAG_COMPLEX)
    add('z.pow1.5', zc + [_o('POW', imm=1.5), _o('ADD_Y')], 2, FLAG_COMPLEX)
    add('z.exp.div', [PX, _o('PUSH_I'), _o('MUL'), _o('EXP'), _o('MUL_Y'), PX, _o('PUSH_I'), _o('ADD'), _o('DIV')],
        3, FLAG_COMPLEX)                                                    # y exp(i x) / (x + i)
    # true solutions of the force-free equation
    add('true.dipole', [PY, _o('MULC', imm=-2.0), _o('EXP'), _o('MUL_P', (2, X))], 1, true=True)
    add('true.r2', [_o('PUSH_P', (2, X)), _o('ADD_P', (2, Y))], 1, true=True)
    add('true.neg', [PX, _o('DIV_Y'), _o('ADDC', imm=1.0), _o('NEG'), _o('MUL_Y')], 1, true=True)
    return t


TABLE = _table()
NAMES = [t[0] for t in TABLE]
assert len(set(NAMES)) == len(NAMES)
_words = None


def programs():
    """[(name, words, flags, single-opcode, true solution)] -- assembled once (needs libpdeval.so
    for pdeval_program_depth)."""
    global _words
    if _words is None:
        _words = [(n, assemble(p, d, f), f, s, tr) for n, p, d, f, s, tr in TABLE]
    return _words


def opcodes_of(words):
    return sorted({op for op, *_ in decode(words)})


# ------------------------------------------------------------------ the points
def _points():
    """p* = (0.8, 6/7) and 69 seeded points of the default grid range rho in [0.05, 3], z in
    [-2, 2]; |z| >= 0.1 keeps the programs that divide by z (or take Abs of it) MARGIN away from
    their pole (kink)."""
    rng = np.random.default_rng(20240229)
    xs, ys = [0.8], [6 / 7]
    while len(xs) < 70:
        x, y = rng.uniform(0.05, 3.0), rng.uniform(-2.0, 2.0)
        if abs(y) >= 0.1:
            xs.append(float(x))
            ys.append(float(y))
    return np.array(xs), np.array(ys)


XS, YS = _points()


# ------------------------------------------------------------------ the reference interpreter
class Unfit(Exception):
    """A (program, point) pair that violates the condition on the points."""


def _const(c):
    return [c] + [MP.mpf(0)] * (NC - 1)


def _var(v, axis):
    j = _const(v)
    j[JI[(1, 0) if axis == 0 else (0, 1)]] = MP.mpf(1)
    return j


def _mul(a, b):
    out = []
    for terms in _MUL:
        s = MP.mpf(0)
        for k1, k2 in terms:
            if a[k1] != 0 and b[k2] != 0:
                s += a[k1] * b[k2]
        out.append(s)
    return out


def _compose(a, f):
    """sum_k f[k] (a - a[0])**k, truncated at order 4."""
    h = [MP.mpf(0)] + a[1:]
    out = _const(f[0])
    hk = _const(MP.mpf(1))
    for k in range(1, 5):
        hk = _mul(hk, h)
        if f[k] != 0:
            out = [o + f[k] * c for o, c in zip(out, hk)]
    return out


def _pcoef(v, n, axis):
    j = _const(MP.mpf(0))
    for k in range(min(n, 4) + 1):
        j[JI[(k, 0) if axis == 0 else (0, k)]] = MP.binomial(n, k) * v ** (n - k)
    return j


class _Ref:
    def __init__(self, cplx, third_exact=False):
        self.cplx = cplx
        self.third_exact = third_exact      # PDEVAL_IMM_DD immediates stand for the rational 1/3
        self.margin = MP.inf

    def imm(self, hi, lo):
        if hi is None:
            return None
        if lo is None:
            return MP.mpf(hi)
        if self.third_exact:
            assert (hi, lo) == (THIRD_HI, THIRD_LO)
            return MP.mpf(1) / 3
        return MP.mpf(hi) + MP.mpf(lo)

    def near(self, dist):
        self.margin = min(self.margin, dist)
        if dist < MARGIN:
            raise Unfit(f'within {float(dist):.3g} of a pole, branch point or kink')

    def branch(self, a0):
        """a0 as the argument of LOG / SQRT / POW: away from the branch point 0 and, in the
        complex programs, from the cut on the negative real axis; positive in the real ones."""
        self.near(abs(a0))
        if self.cplx:
            if MP.re(a0) < 0:
                self.near(abs(MP.im(a0)))
        elif a0 < 0:
            raise Unfit('not real')

    def recip(self, b):
        self.near(abs(b[0]))
        return _compose(b, [(-1) ** k / b[0] ** (k + 1) for k in range(5)])

    def div(self, a, b):
        return _mul(a, self.recip(b))

    def binop(self, op, a, b):
        if op == PDOP['ADD']:
            return [p + q for p, q in zip(a, b)]
        if op == PDOP['SUB']:
            return [p - q for p, q in zip(a, b)]
        if op == PDOP['RSUB']:
            return [q - p for p, q in zip(a, b)]
        if op == PDOP['MUL']:
            return _mul(a, b)
        if op == PDOP['DIV']:
            return self.div(a, b)
        assert op == PDOP['RDIV']
        return self.div(b, a)

    def run(self, words, x, y):
        x, y = MP.mpf(x), MP.mpf(y)
        st = []
        for op, operand, hi, lo in decode(words):
            nm = {v: k for k, v in PDOP.items()}[op]
            imm = self.imm(hi, lo)
            if nm == 'PUSH_X':
                st.append(_var(x, 0))
            elif nm == 'PUSH_Y':
                st.append(_var(y, 1))
            elif nm == 'PUSH_C':
                st.append(_const(imm))
            elif nm == 'PUSH_I':
                assert self.cplx
                st.append(_const(MP.mpc(0, 1)))
            elif nm in ('ADD', 'SUB', 'RSUB', 'MUL', 'DIV', 'RDIV'):
                b = st.pop()
                a = st.pop()
                st.append(self.binop(op, a, b))
            elif nm == 'ADDC':
                st[-1] = [st[-1][0] + imm] + st[-1][1:]
            elif nm == 'MULC':
                st[-1] = [c * imm for c in st[-1]]
            elif nm == 'RDIVC':
                st[-1] = self.div(_const(imm), st[-1])
            elif nm == 'NEG':
                st[-1] = [-c for c in st[-1]]
            elif nm in ('ADD_X', 'ADD_Y', 'SUB_X', 'SUB_Y', 'MUL_X', 'MUL_Y', 'DIV_X', 'DIV_Y'):
                v = _var(x, 0) if nm.endswith('X') else _var(y, 1)
                bop = {'ADD': 'ADD', 'SUB': 'SUB', 'MUL': 'MUL', 'DIV': 'DIV'}[nm[:3]]
                st[-1] = self.binop(PDOP[bop], st[-1], v)
            elif nm == 'POWN':
                n = operand & 0xff
                a0 = st[-1][0]
                st[-1] = _compose(st[-1], [MP.binomial(n, k) * a0 ** (n - k) if k <= n else MP.mpf(0)
                                           for k in range(5)])
            elif nm in ('POW', 'SQRT'):
                al = MP.mpf(hi) if nm == 'POW' else MP.mpf(1) / 2
                a0 = st[-1][0]
                self.branch(a0)
                st[-1] = _compose(st[-1], [MP.binomial(al, k) * MP.power(a0, al - k) for k in range(5)])
            elif nm == 'EXP':
                e = MP.exp(st[-1][0])
                st[-1] = _compose(st[-1], [e / MP.factorial(k) for k in range(5)])
            elif nm == 'LOG':
                a0 = st[-1][0]
                self.branch(a0)
                st[-1] = _compose(st[-1], [MP.log(a0)] + [(-1) ** (k + 1) / (k * a0 ** k) for k in range(1, 5)])
            elif nm == 'ABS':
                a0 = st[-1][0]
                if self.cplx and MP.im(a0) != 0:
                    raise Unfit('Abs of a non-real value')
                self.near(abs(a0))
                if MP.re(a0) < 0:
                    st[-1] = [-c for c in st[-1]]
            else:
                assert op in P_OPS, op
                n, axis = operand & 0xff, (operand >> 8) & 1
                v = y if axis else x
                p = _pcoef(v, n, axis)
                if nm == 'PUSH_P':
                    st.append(p)
                    continue
                if nm in ('DIV_P',):
                    # t / v**n is a function of (t, v) with its pole at v = 0
                    self.near(abs(v))
                    st[-1] = _mul(st[-1], _compose(p, [(-1) ** k / p[0] ** (k + 1) for k in range(5)]))
                    continue
                bop = {'ADD_P': 'ADD', 'SUB_P': 'SUB', 'MUL_P': 'MUL'}.get(nm)
                st[-1] = self.binop(PDOP[bop], st[-1], p) if bop else self.div(p, st[-1])
        assert len(st) == 1
        u = st[0]
        for c in u:
            if not (MP.isfinite(c)):
                raise Unfit('not finite')
            if not self.cplx and MP.im(c) != 0:
                raise Unfit('not real')
        return u


def ref_jet(words, x, y):
    """(15 coefficients at 60 digits, margin): the Taylor coefficients of the program at the
    exact binary point (x, y), and the smallest distance of an intermediate value to a pole,
    branch point or Abs kink.  Raises Unfit where the condition on the points is violated."""
    r = _Ref(bool(int(words[0]) & FLAG_COMPLEX))
    u = r.run(words, x, y)
    return u, r.margin


def split(v):
    """v as a (hi, lo) pair of doubles; hi is v correctly rounded."""
    hi = float(v)
    return hi, float(v - MP.mpf(hi))


def split_jet(u):
    """complex128 (hi, lo) arrays of 15 coefficients; lo rounded to a float32, as the golden file
    stores it (hi + lo: 23 digits)."""
    hi, lo = np.zeros(NC, complex), np.zeros(NC, complex)
    for k, c in enumerate(u):
        rh, rl = split(MP.re(c))
        ih, il = split(MP.im(c))
        hi[k], lo[k] = complex(rh, ih), complex(np.float32(rl), np.float32(il))
    return hi, lo


# ------------------------------------------------------------------ the determinant at p*
def _dx(a, axis):
    out = _const(MP.mpf(0))
    for k, (i, j) in enumerate(IDX):
        src = (i + 1, j) if axis == 0 else (i, j + 1)
        if src in JI:
            out[k] = a[JI[src]] * (src[axis])
    return out


def det_from_jet(u, rho):
    """The force-free determinant (Omega = 0) from the order-4 jet of u: truncated arithmetic on
    the derivatives; each differentiation spends one order and the determinant is of order 4, so
    its constant coefficient is exact."""
    r = _Ref(True)
    sub = lambda a, b: [p - q for p, q in zip(a, b)]   # noqa: E731
    add = lambda a, b: [p + q for p, q in zip(a, b)]   # noqa: E731
    ur, uz = _dx(u, 0), _dx(u, 1)
    A = sub(add(_dx(ur, 0), _dx(uz, 1)), r.div(ur, _var(rho, 0)))
    B = add(_mul(ur, ur), _mul(uz, uz))
    LT = lambda f: sub(_mul(uz, _dx(f, 0)), _mul(ur, _dx(f, 1)))   # noqa: E731
    LA, LB = LT(A), LT(B)
    return sub(_mul(LA, LT(LB)), _mul(LB, LT(LA)))[0]


def ref_det(words, third_exact=True):
    """det at p* = (4/5, 6/7) from the reference jets at 60 digits; PDEVAL_IMM_DD immediates
    stand for 1/3 (third_exact) or for hi + lo."""
    x, y = MP.mpf(4) / 5, MP.mpf(6) / 7
    return det_from_jet(_Ref(True, third_exact).run(words, x, y), x)


# ------------------------------------------------------------------ SymPy form (part 3's reference)
def sympy_expr(words, rho, z):
    """The program as a SymPy expression: PDEVAL_IMM_DD immediates as the rational 1/3, other
    immediates and POW exponents as the exact value of their double."""
    import sympy as sp
    st = []

    def num(v):
        r = sp.Rational(v)
        return r if r.q <= 1 << 20 else sp.Float(v, 70)
    for op, operand, hi, lo in decode(words):
        nm = {v: k for k, v in PDOP.items()}[op]
        imm = None if hi is None else (sp.Rational(1, 3) if lo is not None else num(hi))
        if nm == 'PUSH_X':
            st.append(rho)
        elif nm == 'PUSH_Y':
            st.append(z)
        elif nm == 'PUSH_C':
            st.append(imm)
        elif nm == 'PUSH_I':
            st.append(sp.I)
        elif nm in ('ADD', 'SUB', 'RSUB', 'MUL', 'DIV', 'RDIV'):
            b = st.pop()
            a = st.pop()
            st.append({'ADD': a + b, 'SUB': a - b, 'RSUB': b - a, 'MUL': a * b, 'DIV': a / b, 'RDIV': b / a}[nm])
        elif nm == 'ADDC':
            st[-1] = st[-1] + imm
        elif nm == 'MULC':
            st[-1] = st[-1] * imm
        elif nm == 'RDIVC':
            st[-1] = imm / st[-1]
        elif nm == 'NEG':
            st[-1] = -st[-1]
        elif nm in ('ADD_X', 'ADD_Y', 'SUB_X', 'SUB_Y', 'MUL_X', 'MUL_Y', 'DIV_X', 'DIV_Y'):
            v = rho if nm.endswith('X') else z
            t = st[-1]
            st[-1] = {'ADD': t + v, 'SUB': t - v, 'MUL': t * v, 'DIV': t / v}[nm[:3]]
        elif nm == 'POWN':
            st[-1] = st[-1] ** (operand & 0xff)
        elif nm == 'POW':
            st[-1] = st[-1] ** imm
        elif nm == 'SQRT':
            st[-1] = sp.sqrt(st[-1])
        elif nm == 'EXP':
            st[-1] = sp.exp(st[-1])
        elif nm == 'LOG':
            st[-1] = sp.log(st[-1])
        elif nm == 'ABS':
            st[-1] = sp.Abs(st[-1])
        else:
            p = (z if (operand >> 8) & 1 else rho) ** (operand & 0xff)
            t = st[-1] if nm != 'PUSH_P' else None
            if nm == 'PUSH_P':
                st.append(p)
            else:
                st[-1] = {'ADD_P': t + p, 'SUB_P': t - p, 'MUL_P': t * p, 'DIV_P': t / p, 'RDIV_P': p / t}[nm]
    assert len(st) == 1
    return st[0]


# ------------------------------------------------------------------ the stored reference
class Golden:
    """tests/golden/jet_opcodes.npz: jets (hi + lo, complex128 [program, point, 15]; lo was stored
    as a float32), margins
    [program, point], det / det_twin at p* as 50-digit strings 're im'."""

    def __init__(self):
        z = np.load(GOLDEN)
        progs = programs()
        ops = np.concatenate([w for _, w, *_ in progs])
        assert np.array_equal(z['ops'], ops) and np.array_equal(z['xs'], XS) and np.array_equal(z['ys'], YS), \
            'tests/golden/jet_opcodes.npz is stale: run tests/golden/gen_jet_opcodes.py'
        self.hi = z['jets_hi'].astype(complex)
        self.lo = z['jets_lo'].astype(complex)
        self.hi[z['imag_index']] += 1j * z['imag_hi']
        self.lo[z['imag_index']] += 1j * z['imag_lo']
        self.margin = z['margin']
        self.det = [self._c(s) for s in z['det']]
        self.det_twin = {int(i): self._c(s) for i, s in zip(z['twin_index'], z['det_twin'])}

    @staticmethod
    def _c(s):
        re, im = str(s).split()
        return MP.mpc(re, im)


_golden = None


def golden():
    global _golden
    if _golden is None:
        _golden = Golden()
    return _golden


# ------------------------------------------------------------------ the checks (host build and device)
EPS = 2.0 ** -52
REL_TOL = 1e-11          # the rule test_oracle_golden.py applies to the oracle's jets
DET_REL_TOL = 1e-10      # the project's REL_TOL of a reported residual
OP_NAME = {v: k for k, v in PDOP.items()}


class Stats:
    """Per opcode: the largest |c - exact| / (2^-52 E) and the largest error relative to
    max(1, max |c exact|) seen over the programs that hold the opcode."""

    def __init__(self):
        self.ratio, self.rel = {}, {}

    def add(self, words, ratio, rel):
        for op in opcodes_of(words):
            self.ratio[op] = max(self.ratio.get(op, 0.0), ratio)
            self.rel[op] = max(self.rel.get(op, 0.0), rel)

    def table(self, title):
        rows = [f'{title}', f'{"opcode":10s} {"max |err|/(eps E)":>18s} {"max rel err":>12s}']
        for op in sorted(self.rel):
            rows.append(f'{OP_NAME[op]:10s} {self.ratio.get(op, 0.0):18.3f} {self.rel[op]:12.2e}')
        return '\n'.join(rows)


def check_jets(name, words, hi, lo, jets, errs, kappa, single, stats, bad):
    """Checks (a), (b), (c) of one real program: hi, lo, jets [points, 15] and, in tier-2 mode,
    errs [points, 15] (None in tier-1 mode).  Violations are appended to `bad`."""
    hi, lo = hi.real, lo.real
    err = np.abs((jets - hi) - lo)
    scale = np.maximum(1.0, np.abs(hi).max(axis=1))[:, None]
    rel = err / scale
    for k, c in zip(*np.nonzero(~(rel <= REL_TOL))):
        bad.append(('a', name, int(k), int(c), float(jets[k, c]), float(hi[k, c]), float(rel[k, c])))
    ratio = 0.0
    if errs is not None:
        zero = errs == 0.0
        for k, c in zip(*np.nonzero(zero & (jets != hi))):
            bad.append(('b: E = 0, not the rounded exact value', name, int(k), int(c), float(jets[k, c]),
                        float(hi[k, c])))
        with np.errstate(divide='ignore', invalid='ignore'):
            r = np.where(zero, 0.0, err / (EPS * errs))
        for k, c in zip(*np.nonzero(~(r <= kappa))):
            bad.append(('b', name, int(k), int(c), float(err[k, c]), float(errs[k, c]), float(r[k, c])))
        ratio = float(np.nanmax(r))
        if single:
            for k, c in zip(*np.nonzero(~(EPS * errs <= REL_TOL * scale))):
                bad.append(('c', name, int(k), int(c), float(errs[k, c]), float(scale[k, 0])))
    stats.add(words, ratio, float(np.nanmax(rel)))


def _within(v, exact, lim, dd_tier):
    """|v - exact| <= lim for a result of the fp64 tiers.  A double-double tier returns the high
    double of its result, which cannot lie within 2^-100 of anything that is no double: there the
    test is that some value within lim of the exact one rounds to v, the most a double can show."""
    if not dd_tier:
        return abs(MP.mpf(v) - exact) <= lim
    return float(exact - lim) <= v <= float(exact + lim)


def check_tier(name, tier, out, det, kappa, true, bad):
    """Part 3 on one run {Re res, Im res, |res|, S, noise, finite} against the exact det."""
    re, im, ab, _, noise, fin = (float(v) for v in out)
    if fin != 1.0:
        bad.append(('finite', name, tier, fin))
        return
    lim = kappa * noise
    if not _within(re, MP.re(det), lim, tier >= 2):
        bad.append(('re', name, tier, re, float(MP.re(det)), lim))
    if not _within(im, MP.im(det), lim, tier >= 2):
        bad.append(('im', name, tier, im, float(MP.im(det)), lim))
    if tier >= 2 and abs(det) >= 1e-20 and not abs(MP.mpf(ab) - abs(det)) <= DET_REL_TOL * abs(det):
        bad.append(('dd accuracy', name, tier, ab, float(abs(det))))
    if true and not ab <= lim:
        bad.append(('true solution', name, tier, ab, lim))


def tiers_of(flags):
    return (1, 3) if flags & FLAG_COMPLEX else (0, 1, 2, 3)

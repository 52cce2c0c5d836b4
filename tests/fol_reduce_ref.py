"""The reduction kinds (include/pdeval.h pdeval_fol_reduce, DESIGN.md §14 "Reduction kinds") restated
in numpy, and their 40-digit reference: SymPy derivatives evaluated with mpmath -- the reference of
tests/test_fol_reduce_host.py and tests/test_gpu_fol_reduce.py.  Test infrastructure only."""
import math

import mpmath
import numpy as np
import sympy as sp

import foliation_ref as R
from pdeval import problem_defs as P

KNOWN = list(P.force_free().known_solutions)     # Vertical, X-point, Radial, Dipolar, Parabolic, Hyperbolic, Bent
RADIAL, BENT = KNOWN[2], KNOWN[6]
DEEP = '(exp(rho) + sqrt(z**2 + 1))*(exp(z) + sqrt(rho + 1)) + (exp(rho*z) + rho)*(z + exp_neg(rho))'   # stack 3
# stack 4: past the shallow kernel's stack (kRedShallowD = 3); not a solution either
DEEP4 = f'({DEEP})*((exp(z) + sqrt(rho**2 + 1))*(exp(rho) + sqrt(z + 3)) + (exp_neg(rho*z) + z)*(rho + exp_neg(z)))'
CPLX = 'sqrt(neg(rho**2 + z**2))'
ROWS = KNOWN + ['z', 'rho**4', 'rho**2 + z**2', 'exp(z)', 'rho**2 + 2*z', 'exp(rho**2*z)',
                'sqrt(sqrt(rho**2+z**2) - z)', f'exp({BENT})', f'({BENT})**2 + 1/(1 + {BENT})', f'exp({RADIAL})',
                DEEP, DEEP4, CPLX]
NONE, FREE, VACUUM, CURRENT = 0, 1, 2, 3
# what the issue states at Omega = 0 (DEEP, DEEP4: whatever the reference says; CPLX: none)
KINDS0 = {'rho**2': FREE, 'z': FREE, 'rho**2 + z**2': FREE, 'rho**4': FREE, BENT: CURRENT, f'exp({BENT})': CURRENT,
          CPLX: NONE, **{s: VACUUM for s in KNOWN[1:6]}, f'exp({RADIAL})': VACUUM}
SAME_CLASS = [(RADIAL, f'exp({RADIAL})'), (BENT, f'exp({BENT})'), ('rho**2', 'rho**4')]
ORDER3 = [(i, d - i) for d in range(4) for i in range(d, -1, -1)]    # (i, j) of coefficient ji(i, j) = 0 .. 9


def ji(i, j):
    return (i + j) * (i + j + 1) // 2 + j


def forms(c, x, w, mag):
    """(L_T A, L_T B, W) of jets c[..., 10] at rho = x[...], or (mag) their magnitude shadows: the
    operations of red_forms (pdeval_fol_reduce.h) in its order, on float64 or mpf object arrays."""
    a = np.abs if mag else (lambda v: v)
    s = 1 if mag else -1
    C = lambda i, j: a(c[..., ji(i, j)])   # noqa: E731
    x2w, r0 = (x * x) * w, 1.0 / x
    f0, f1 = 1.0 + s * x2w, (2.0 * s) * a(x) * w
    g0, g1 = a(r0) + a(x) * w, w + s * (r0 * r0)
    p00, p10, p01 = C(1, 0) * 1.0, C(2, 0) * 2.0, C(1, 1) * 1.0
    q00, q10, q01 = C(0, 1) * 1.0, C(1, 1) * 1.0, C(0, 2) * 2.0
    l00 = C(2, 0) * 2.0 + C(0, 2) * 2.0
    l10 = C(3, 0) * 6.0 + C(1, 2) * 2.0
    l01 = C(2, 1) * 2.0 + C(0, 3) * 6.0
    A00 = f0 * l00 + s * (g0 * p00)
    A10 = (f0 * l10 + f1 * l00) + s * (g0 * p10 + g1 * p00)
    A01 = f0 * l01 + s * (g0 * p01)
    n00 = p00 * p00 + q00 * q00
    n10 = 2.0 * (p00 * p10 + q00 * q10)
    n01 = 2.0 * (p00 * p01 + q00 * q01)
    B00, B10, B01 = f0 * n00, f0 * n10 + f1 * n00, f0 * n01
    LA = q00 * A10 + s * (p00 * A01)
    LB = q00 * B10 + s * (p00 * B01)
    return np.stack([LA, LB, B00 * LA + s * (A00 * LB)])


def rule(c, x, w=0.0, tau=R.TAU, min_points=R.MIN_POINTS):
    """The per-point and per-row rule on jets c[rows, mm, 10] at rho = x[mm] (float64 or mpf objects; a
    point that does not exist holds NaN): dict of kind[rows], counts[rows, 4], qmax[rows, 3] (as doubles),
    X, S [3, rows, mm], fin, and the table's kappa, G, the NaN pattern included."""
    f64 = lambda v: np.asarray(v).astype(np.float64)   # noqa: E731
    with np.errstate(all='ignore'):
        X, S = forms(c, x, w, False), forms(c, x, w, True)
        fin = (np.abs(f64(c)) < 2.0 ** 160).all(-1) & np.isfinite(f64(X)).all(0) & np.isfinite(f64(S)).all(0)
        bad = fin[None] & (np.abs(X) > tau * S).astype(bool)
        pos = f64(S) > 0
        q = np.where(pos & fin[None], f64(np.abs(X) / np.where(pos, S, 1)), 0.0)
        ok = bad[1]
        kappa, G = (np.where(ok, f64(v / np.where(ok, X[1], 1)), np.nan) for v in (-X[0], X[2]))
    counts = np.stack([fin.sum(-1), *bad.sum(-1)], -1).astype(np.int32)
    kind = np.where(counts[:, 0] < min_points, NONE, np.where((counts[:, 1] == 0) & (counts[:, 2] == 0), FREE,
                                                               np.where(counts[:, 3] == 0, VACUUM, CURRENT)))
    return dict(kind=kind.astype(np.uint8), counts=counts, qmax=q.max(-1).T, q=q, X=X, S=S, fin=fin, kappa=kappa, G=G)


def closed_form_jets(rows, m, mp=True):
    """Taylor coefficients c[rows, mm, 10] of the strings' closed-form SymPy derivatives at the m x m
    sample points (foliation_ref.grid_points, x index major) and the points' rho[mm]: mpf objects at the
    caller's mpmath precision, or (mp=False) doubles by numpy.  A point where u or a derivative is
    not real and finite is NaN throughout."""
    pd_ = P.force_free()
    xs, ys = R.grid_points(m)
    px, py = np.repeat(xs, m), np.tile(ys, m)
    out = np.empty((len(rows), m * m, 10), dtype=object if mp else np.float64)
    for r, s in enumerate(rows):
        e = pd_.parse(s)
        ds = [sp.diff(e, pd_.x, i, pd_.y, j) / (math.factorial(i) * math.factorial(j)) for i, j in ORDER3]
        f = sp.lambdify((pd_.x, pd_.y), ds, 'mpmath' if mp else 'numpy', cse=True)
        if mp:
            out[r] = [[mpmath.mpmathify(v) for v in f(mpmath.mpf(float(a)), mpmath.mpf(float(b)))] for a, b in zip(px, py)]
            ok = np.array([all(isinstance(v, mpmath.mpf) and mpmath.isfinite(v) for v in pt) for pt in out[r]])
            out[r, ~ok, :] = mpmath.nan
        else:
            with np.errstate(all='ignore'):   # (complex arguments: a root of a negative value is not real, not a warning)
                v = np.stack([np.asarray(d) + 0 * px for d in f(px + 0j, py + 0j)], -1)
            out[r] = np.where((v.imag == 0).all(-1, keepdims=True), v.real, np.nan)
    return out, (np.array([mpmath.mpf(float(a)) for a in px], dtype=object) if mp else px)


def reference(m, w=0.0, rows=ROWS):
    """rule() of the 40-digit jets of `rows`, with 'table_dev': the largest scaled deviation of the fp64
    restatement on closed-form numpy derivatives from it, over kappa and G where |L_T B| / S_LB >= 1e-3
    (|d kappa| against S_LA / |L_T B|, |d G| against S_W / |L_T B|: the quotients' own rounding scale).
    Asserts the margin: no row maximum of |X| / S_X lies between 1e-12 and 1e-3."""
    with mpmath.workdps(40):
        c, x = closed_form_jets(rows, m)
        ref = rule(c, x, w)
        at = ref['table_at'] = ref['fin'] & (ref['q'][1] >= 1e-3)
        ref['table_scale'] = [np.asarray(ref['S'][k] / np.where(at, np.abs(ref['X'][1]), 1)).astype(np.float64) for k in (0, 2)]
    q = ref['qmax']
    assert not ((q > 1e-12) & (q < 1e-3)).any(), (m, w, [(rows[r], q[r]) for r in np.argwhere((q > 1e-12) & (q < 1e-3))[:, 0]])
    c64, x64 = closed_form_jets(rows, m, mp=False)
    ref['table_dev'] = table_deviation(ref, rule(c64, x64, w))
    return ref


def table_deviation(ref, got):
    """max over kappa and G of |got - ref| / scale at ref['table_at'] (got: a dict with kappa, G [rows, mm])."""
    dev = 0.0
    for name, sc in zip(('kappa', 'G'), ref['table_scale']):
        at = ref['table_at']
        with np.errstate(all='ignore'):
            d = np.abs(np.asarray(got[name], dtype=np.float64)[at] - ref[name][at])
            d = np.where(d == 0, 0.0, d / sc[at])   # (scale 0: an exact zero, to be met exactly)
        assert not np.isnan(d).any(), name
        dev = max(dev, float(d.max(initial=0.0)))
    return dev

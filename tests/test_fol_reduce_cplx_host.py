"""The reduction kinds of complex-valued rows (PDEVAL_FOL_CPLX in pdeval_fol_reduce): their 40-digit
reference -- SymPy derivatives to order 3 evaluated with mpmath as complex jets, the rule restated in numpy on
tests/fol_reduce_ref.py -- and red_point_cplx built by g++ (tests/hostsim/sim_fol_reduce_cplx.cpp) against it."""
import os
import subprocess

import mpmath
import numpy as np
import pytest
import sympy as sp

import fol_reduce_ref as F
import foliation_ref as R
from pdeval import problem_defs as P
from pdeval.opcodes import FLAG_COMPLEX

I = 'sqrt(neg(1))'
G = F.RADIAL
# functions of Radial (vacuum) whose programs need a stack of 3 (both LDS slots) and of 4 (the private-memory body).
# (fol_reduce_ref.DEEP, DEEP4 and exp(i Bent) have sample points with |X| / S inside the margin: not used.)
V3 = f'(exp({G}) + sqrt({G} + 1))*(exp_neg({G}) + ({G})**2)'
V4 = f'(exp({G}) + sqrt({G} + 1))*(exp_neg({G}) + sqrt({G} + 2)) + (exp(2*{G}) + {G})*(({G})**2 + exp_neg(3*{G}))'
# (real partner, complex twin): free, selected unflagged; vacuum, flagged; current; stack 3; stack 4
PAIRS = [('rho**2 + z**2', 'sqrt(neg(rho**2 + z**2))'), (G, f'exp({I}*({G}))'), (F.BENT, f'sqrt(neg({F.BENT}))'),
         (V3, f'{I}*({V3})'), (V4, f'{I}*({V4})')]
# no real direction; real where z < 0: the real pass decides it (rho*sqrt(neg(z)) has a point inside the margin at m = 16)
NO_DIR, PART = f'rho + {I}*z', 'sqrt(neg(z))'
ROWS = [s for p in PAIRS for s in p] + [NO_DIR, PART]
OMEGA = list(PAIRS[1])                                # current in both at Omega = 1


def reference(m, w=0.0, rows=ROWS, tau=R.TAU):
    """kind[rows], counts[rows, 4], fin[rows, mm], bad[3, rows, mm], took[rows] and the complex128 jets of `rows`
    at Omega^2 = w.  A row the complex pass takes (PDEVAL_FLAG_COMPLEX, or real at fewer than MIN_POINTS points)
    follows the complex rule, any other fol_reduce_ref.rule on its real jets.  Asserts the margins at every point:
    |X| / S <= 1e-12 or >= 1e-3, phase defect <= 1e-12 or >= 1e-2."""
    pd_, f64 = P.force_free(), lambda v: np.asarray(v).astype(np.float64)   # noqa: E731
    ops, off, _ = P.compile_strings(pd_, rows)
    px, py = (g(v, m) for g, v in zip((np.repeat, np.tile), R.grid_points(m)))
    with mpmath.workdps(40), np.errstate(all='ignore'):
        c = np.empty((len(rows), m * m, 10), dtype=object)
        for r, s in enumerate(rows):
            e = pd_.parse(s)
            f = sp.lambdify((pd_.x, pd_.y), [sp.diff(e, pd_.x, i, pd_.y, j) / (sp.factorial(i) * sp.factorial(j))
                                             for i, j in F.ORDER3], 'mpmath', cse=True)
            c[r] = [[mpmath.mpc(v) for v in f(mpmath.mpf(float(a)), mpmath.mpf(float(b)))] for a, b in zip(px, py)]
        x = np.array([mpmath.mpf(float(a)) for a in px], dtype=object)
        c128 = c.astype(np.complex128)
        real = (c128.imag == 0).all(-1)
        took = ((np.asarray(ops)[np.asarray(off)[:-1]] & FLAG_COMPLEX) != 0) | (real.sum(-1) < R.MIN_POINTS)
        X, S = np.abs(F.forms(c, x, w, False)), F.forms(np.abs(c), x, w, True)
        a, b = c128[..., 1], c128[..., 2]                                  # u_rho, u_z: the test of fol_cplx_point
        hh, ti = np.abs(a) * np.abs(b), np.abs((np.where(np.abs(a) >= np.abs(b), b * a.conj(), a * b.conj())).imag)
        defect = np.where(hh > 0, ti / np.where(hh > 0, hh, 1), 0.0)
        fin = (defect <= tau) & (np.abs(c128) < 2.0 ** 160).all(-1) & np.isfinite(f64(X)).all(0) & np.isfinite(f64(S)).all(0)
        q = np.where(f64(S) > 0, f64(X / np.where(f64(S) > 0, S, 1)), 0.0)
        for name, v, lo, hi in (('q', q[:, took[:, None] & fin], 1e-12, 1e-3), ('defect', defect[took], 1e-12, 1e-2)):
            assert not ((v > lo) & (v < hi)).any(), (name, m, w, v[(v > lo) & (v < hi)])
        bad = fin[None] & (X > tau * S).astype(bool)
        rl = F.rule(np.where(real[..., None], np.vectorize(lambda v: v.real, otypes=[object])(c), mpmath.nan), x, w, tau)
        assert not ((rl['q'] > 1e-12) & (rl['q'] < 1e-3))[:, ~took].any()
    fin = np.where(took[:, None], fin, rl['fin'])
    bad = np.where(took[None, :, None], bad, rl['fin'][None] & (rl['q'] > tau))
    counts = np.stack([fin.sum(-1), *bad.sum(-1)], -1).astype(np.int32)
    kind = np.where(counts[:, 0] < R.MIN_POINTS, 0, np.where((counts[:, 1] == 0) & (counts[:, 2] == 0), F.FREE,
                                                             np.where(counts[:, 3] == 0, F.VACUUM, F.CURRENT)))
    return dict(kind=kind.astype(np.uint8), counts=counts, fin=fin, bad=bad, took=took, c=c128, x=px)


@pytest.mark.parametrize('w', (0.0, 1.0))
def test_red_point_cplx_against_40_digits(w, tmp_path):
    """The finite mask and the three bad masks of red_point_cplx on the complex128 jets equal the reference's at
    every point of every row the complex pass takes; NO_DIR has no finite point; each twin has its partner's kind."""
    sim, exe, path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'hostsim'), str(tmp_path / 'sim'), str(tmp_path / 'in')
    subprocess.check_call(['g++', '-O2', '-std=c++17', '-DPD_HOST_SIM', '-I' + sim, '-o', exe,
                           os.path.join(sim, 'sim_fol_reduce_cplx.cpp')])
    ref = reference(12, w, ROWS if w == 0.0 else OMEGA)
    c = np.ascontiguousarray(ref['c'][ref['took']])
    with open(path, 'wb') as f:
        f.write(np.array([c.shape[0], c.shape[1]], np.int32).tobytes() + np.array([w, R.TAU]).tobytes() + ref['x'].tobytes() + c.tobytes())
    got = np.array(subprocess.check_output([exe, path], text=True).split(), dtype=int).reshape(c.shape[0], c.shape[1], 4).astype(bool)
    assert np.array_equal(got[..., 0], ref['fin'][ref['took']])
    assert np.array_equal(got[..., 1:].transpose(2, 0, 1), ref['bad'][:, ref['took']])
    kind = ref['kind'].tolist()
    if w:
        assert kind == [F.CURRENT, F.CURRENT]
    else:
        assert kind[ROWS.index(NO_DIR)] == 0 and not ref['fin'][ROWS.index(NO_DIR)].any()
        assert kind[:10] == [F.FREE] * 2 + [F.VACUUM] * 2 + [F.CURRENT] * 2 + [F.VACUUM] * 4, kind

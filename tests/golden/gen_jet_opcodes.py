#!/usr/bin/env python3
"""Writes tests/golden/jet_opcodes.npz: the 50-digit reference of tests/jet_opcode_cases.py.

  jets_hi, jets_lo  [program, point, 15]: the Taylor coefficients as hi + lo, hi the correctly
                    rounded double, lo a float32 (23 digits in all; keeps the file small);
  imag_hi, imag_lo  the same for the imaginary parts of the complex programs (imag_index)
  margin            [program, point]: distance to the nearest pole, branch point or Abs kink
  det               per program, 're im' at 50 digits: the exact determinant at p* = (4/5, 6/7)
                    (SymPy, exact rationals: _exact_det_at of test_oracle_golden.py, Omega = 0;
                    PDEVAL_IMM_DD immediates as the rational 1/3)
  twin_index, det_twin  the same for the rounded twin of every PDEVAL_IMM_DD program
  ops, xs, ys       the table's words and the points, so that a stale file is noticed

Every (program, point) pair must satisfy the condition on the points (jet_opcode_cases.Unfit
is raised otherwise): nothing is skipped.  Run from the repository root after build():
    python tests/golden/gen_jet_opcodes.py
"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, 'pde-engine_amd'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)


def exact_det(words):
    import sympy as sp
    import jet_opcode_cases as JC
    from test_oracle_golden import _exact_det_at
    rho, z = sp.symbols('rho z', real=True)
    u = JC.sympy_expr(words, rho, z)
    v = _exact_det_at(u, rho, z, {rho: sp.Rational(4, 5), z: sp.Rational(6, 7)})
    v = sp.N(v.doit(), 60)
    re, im = v.as_real_imag()
    return f'{sp.N(re, 50)} {sp.N(im, 50)}'


def main():
    import jet_opcode_cases as JC
    progs = JC.programs()
    n, m = len(progs), len(JC.XS)
    hi, lo = np.zeros((n, m, 15), complex), np.zeros((n, m, 15), complex)
    margin = np.zeros((n, m))
    t0 = time.time()
    for ip, (name, w, *_) in enumerate(progs):
        for k in range(m):
            u, mg = JC.ref_jet(w, JC.XS[k], JC.YS[k])     # raises Unfit: fix the table, skip nothing
            hi[ip, k], lo[ip, k] = JC.split_jet(u)
            margin[ip, k] = min(float(mg), 1e300)
    print(f'jets: {time.time() - t0:.1f} s, smallest margin {margin.min():.3g}', flush=True)
    det, twin_index, det_twin = [], [], []
    for ip, (name, w, *_) in enumerate(progs):
        t0 = time.time()
        det.append(exact_det(w))
        # the jet route (jet_opcode_cases.ref_det) must give the same number
        d = JC.ref_det(w)
        ref = JC.Golden._c(det[-1])
        assert abs(d - ref) <= 1e-40 * max(abs(ref), 1), (name, d, ref)
        if any(l is not None for *_, l in JC.decode(w)):
            twin_index.append(ip)
            det_twin.append(exact_det(JC.rounded_twin(w)))
        print(f'{name:16s} det {det[-1][:24]} ({time.time() - t0:.1f} s)', flush=True)
    cx = np.array([ip for ip, p in enumerate(progs) if p[2] & JC.FLAG_COMPLEX])
    assert not np.delete(hi, cx, axis=0).imag.any() and np.isfinite(lo.view(float).astype(np.float32)).all()
    np.savez_compressed(JC.GOLDEN, jets_hi=hi.real, jets_lo=lo.real.astype(np.float32), imag_index=cx,
                        imag_hi=hi[cx].imag, imag_lo=lo[cx].imag.astype(np.float32), margin=margin, det=np.array(det),
                        twin_index=np.array(twin_index), det_twin=np.array(det_twin),
                        ops=np.concatenate([w for _, w, *_ in progs]), xs=JC.XS, ys=JC.YS)
    print('wrote', JC.GOLDEN, os.path.getsize(JC.GOLDEN), 'bytes')


if __name__ == '__main__':
    main()

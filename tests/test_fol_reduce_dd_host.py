"""The settle tier of the reduction kinds (pdeval_fol_reduce_dd; DESIGN.md §14 "Settled in double-double")
on the CPU: the double-double order-3 interpreter and red_point_dd built by g++ as a stand-alone program
(tests/hostsim/sim_fol_reduce_dd.cpp) against rule() on the 40-digit closed-form jets.  The bound 1e-12 S
is the lower edge of the band the tier settles; measured 1.5e-23 (a 31-digit stand-in: 2.4e-19)."""
import os
import subprocess

import mpmath
import numpy as np
import pytest

import fol_reduce_ref as F
import foliation_ref as R
from pdeval import problem_defs as P

SIM = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'hostsim')
M = 12
# functions of rho/z whose fp64 jets cancel: W == 0, yet |W| / S_W reaches 1e-5 in fp64
BORDER = ['exp(rho/z)/(1 - exp(rho/z))',
          'inv(rho/(-rho**2*z + z**3 + z))/(-rho**2 + z**2 + 1)',
          'rho/(rho + z*exp_neg(rho/z))',
          'rho/(rho - z*exp_neg(rho/z))']
ROWS24 = F.ROWS + BORDER


@pytest.mark.parametrize('w', (0.0, 1.0))
def test_double_double_rule_against_40_digits(w, tmp_path):
    """fin and the three bad masks equal the 40-digit reference's at every point, X agrees within 1e-12 S at
    every finite point, kinds and counts follow; at Omega = 0 the border rows are vacuum, |W| / S_W <= 1e-12."""
    exe, path = str(tmp_path / 'sim'), str(tmp_path / 'in.bin')
    subprocess.check_call(['g++', '-O2', '-std=c++17', '-DPD_HOST_SIM', '-I' + SIM, '-o', exe,
                           os.path.join(SIM, 'sim_fol_reduce_dd.cpp')])
    ops, off, _ = P.compile_strings(P.force_free(), ROWS24)
    ops, off = np.ascontiguousarray(ops, np.int32), np.ascontiguousarray(off, np.int64)
    with open(path, 'wb') as f:
        f.write(np.array([len(ROWS24), M, R.MIN_POINTS, ops.size], np.int32).tobytes())
        f.write(np.array([w, R.TAU] + list(R.FF_GRID)).tobytes() + off.tobytes() + ops.tobytes())
    lines = [[float.fromhex(v) if 'x' in v or 'n' in v else int(v) for v in ln.split()]     # (%a doubles, plain ints)
             for ln in subprocess.check_output([exe, path], text=True).splitlines()]
    head = np.array(lines[0::M * M + 1])
    pts = np.array([ln for i, ln in enumerate(lines) if i % (M * M + 1)]).reshape(len(ROWS24), M * M, 13)
    ref = F.reference(M, w, ROWS24)
    assert np.array_equal(head[:, 0], ref['kind']) and np.array_equal(head[:, 1:5], ref['counts'])
    assert np.array_equal(pts[..., 0].astype(bool), ref['fin'])
    worst = 0.0
    with mpmath.workdps(40):
        bad = ref['fin'][None] & (np.abs(ref['X']) > R.TAU * ref['S']).astype(bool)
        assert np.array_equal(pts[..., 1:4].astype(bool).transpose(2, 0, 1), bad)
        for r, p in np.argwhere(ref['fin']):
            for k in range(3):
                x = mpmath.mpf(float(pts[r, p, 4 + 2 * k])) + mpmath.mpf(float(pts[r, p, 5 + 2 * k]))
                d, s = abs(x - ref['X'][k][r, p]), ref['S'][k][r, p]
                assert d <= s * mpmath.mpf('1e-12'), (ROWS24[r], int(p), k, float(d), float(s))
                worst = max(worst, float(d / s) if s else 0.0)
    print(f'Omega^2 = {w}: largest |X_dd - X_40| / S_40 = {worst:.3e}')
    for r in range(len(F.ROWS), len(ROWS24) if w == 0.0 else 0):
        assert head[r, 7] <= 1e-12 and head[r, 0] == F.VACUUM == head[ROWS24.index(F.RADIAL), 0], (ROWS24[r], head[r])

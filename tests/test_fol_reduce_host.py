"""The reduction kinds (pdeval_fol_reduce; DESIGN.md §14 "Reduction kinds") on the CPU: the PD_HD
per-point rule of pdeval_fol_reduce.h built by g++ as a stand-alone program
(tests/hostsim/sim_fol_reduce.cpp) on the oracle's jets, against the numpy restatement
tests/fol_reduce_ref.py on the same jets.  The GPU tests
(test_gpu_fol_reduce.py) check the gfx950 build."""
import os
import subprocess

import numpy as np
import pytest

import fol_reduce_ref as F
import foliation_ref as R
import oracle_lib as O
from pdeval import problem_defs as P

HERE = os.path.dirname(os.path.abspath(__file__))
SIM = os.path.join(HERE, 'hostsim')
M = 12


@pytest.fixture(scope='module')
def jets():
    """(c[rows, mm, 10], rho[mm]): the first ten coefficients of the oracle's real order-4 jets of
    fol_reduce_ref.ROWS at the m = 12 sample points; NaN for a program its real pass declines."""
    pd_ = P.force_free()
    ops, off, _ = P.compile_strings(pd_, F.ROWS)
    xs, ys = R.grid_points(M)
    c = np.full((len(F.ROWS), M * M, 10), np.nan)
    for r in range(len(F.ROWS)):
        w = np.ascontiguousarray(ops[off[r]:off[r + 1]], dtype=np.int32)
        try:
            c[r] = [O.jet(0, w, float(x), float(y))[:10] for x in xs for y in ys]
        except ValueError:
            pass
    return c, np.repeat(xs, M)


@pytest.fixture(scope='module')
def sim(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('sim') / 'sim_fol_reduce')
    subprocess.check_call(['g++', '-O2', '-std=c++17', '-DPD_HOST_SIM', '-I' + SIM, '-o', exe,
                           os.path.join(SIM, 'sim_fol_reduce.cpp')])

    def run(c, x, w, path):
        with open(path, 'wb') as f:
            f.write(np.array([c.shape[0], c.shape[1], R.MIN_POINTS, 0], np.int32).tobytes())
            f.write(np.array([w, R.TAU]).tobytes() + np.ascontiguousarray(x).tobytes() + np.ascontiguousarray(c).tobytes())
        lines = subprocess.check_output([exe, path], text=True).splitlines()
        head = [ln.split() for ln in lines[0::2]]
        tab = np.array([[float.fromhex(v) for v in ln.split()] for ln in lines[1::2]]).reshape(len(head), 2, -1)
        return (np.array([[int(v) for v in h[:5]] for h in head]), np.array([[float.fromhex(v) for v in h[5:]] for h in head]),
                tab)
    return run


@pytest.mark.parametrize('w', (0.0, 1.0))
def test_host_build_equals_numpy(sim, jets, w, tmp_path):
    """Kinds, the four counts, the row maxima and the table (kappa, G and their NaN pattern) of the
    host build equal the restatement's on the same jets, the doubles bit for bit; at Omega = 0 the named
    rows carry the kinds of the method and the rows of one class one kind."""
    c, x = jets
    head, q, tab = sim(c, x, w, str(tmp_path / 'in.bin'))
    ref = F.rule(c, x, w)
    assert np.array_equal(head[:, 0], ref['kind']) and np.array_equal(head[:, 1:], ref['counts'])
    assert np.array_equal(q, ref['qmax'])
    assert np.array_equal(tab[:, 0], ref['kappa'], equal_nan=True) and np.array_equal(tab[:, 1], ref['G'], equal_nan=True)
    kind = dict(zip(F.ROWS, head[:, 0]))
    assert w or (all(kind[s] == k for s, k in F.KINDS0.items()) and all(kind[a] == kind[b] for a, b in F.SAME_CLASS))


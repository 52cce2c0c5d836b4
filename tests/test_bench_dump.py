"""bench.py --dump-outputs on the CPU: the writer alone, on arrays shaped like
ProblemBench.host_outputs.  Every array lands as float32 / float64 with finite values only (an
inf / NaN entry of a float64 output as 0, its kind in <name>_nonfinite) and can be put together
again exactly, a batch above DUMP_ROWS is cut to one seed-0 sample of rows shared by all arrays
and equal from call to call, and a default-size Kerr batch (3 reference points) stays under
64 MB."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import bench  # noqa: E402

KINDS = np.array([0.0, np.inf, -np.inf, np.nan])     # the codes of <name>_nonfinite


def _outputs(n, nref, seed=1):
    rng = np.random.default_rng(seed)
    r = {'status': rng.integers(0, 8, n).astype(np.uint8),
         'q_ref': rng.standard_normal(n),
         'res_ref': rng.standard_normal((n, nref)),
         'q_grid': rng.standard_normal(n),
         'n_bad': rng.integers(0, 4097, n).astype(np.int32),
         'n_nonfinite': rng.integers(0, 4097, n).astype(np.int32),
         'fingerprint': rng.standard_normal((n, 4))}
    r['q_ref'][::7] = np.nan
    r['fingerprint'][::5, 1] = np.inf
    r['fingerprint'][::11, 2] = -np.inf
    r['fingerprint'][::13] = np.nan
    r['verdict'] = r['status'] == 0
    return r


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def _restored(got, k):
    """Output k as the step left it: the dumped values, with the inf / NaN entries back."""
    if k + '_nonfinite' not in got:
        return got[k]
    code = got[k + '_nonfinite'].astype(np.int64)
    assert np.all(got[k][code != 0] == 0.0), k
    return np.where(code != 0, KINDS[code], got[k])


def _check_files(got, r):
    floats = [k for k, v in r.items() if v.dtype == np.float64]
    assert sorted(got) == sorted(list(r) + [k + '_nonfinite' for k in floats])
    for k, v in got.items():
        assert v.dtype in (np.float32, np.float64), k
        assert np.all(np.isfinite(v)), k
    for k in floats:
        assert got[k + '_nonfinite'].shape == got[k].shape, k


def test_small_batch_dumped_whole(tmp_path):
    r = _outputs(1001, 3)
    bench.dump_outputs(str(tmp_path / 'o'), r)
    got = _load(tmp_path / 'o')
    _check_files(got, r)
    for k, v in r.items():
        assert got[k].shape == v.shape
        assert np.array_equal(_restored(got, k), v.astype(np.float64), equal_nan=True), k
    assert set(np.unique(got['fingerprint_nonfinite'])) == {0.0, 1.0, 2.0, 3.0}


def test_large_batch_sampled_with_fixed_rows(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, 'DUMP_ROWS', 257)
    r = _outputs(5003, 1)
    r['q_grid'] = np.arange(5003, dtype=np.float64)       # the row numbers themselves
    bench.dump_outputs(str(tmp_path / 'a'), r)
    bench.dump_outputs(str(tmp_path / 'b'), r)
    a, b = _load(tmp_path / 'a'), _load(tmp_path / 'b')
    _check_files(a, r)
    rows = a['q_grid'].astype(np.int64)
    assert len(rows) == 257 and np.all(np.diff(rows) > 0) and rows[-1] < 5003
    assert sorted(a) == sorted(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    for k, v in r.items():
        assert np.array_equal(_restored(a, k), v[rows].astype(np.float64), equal_nan=True), k


def test_default_sample_stays_under_64_mb():
    # status, verdict as f32; the counts f64; the float64 outputs (Kerr nref = 3) with their f32 kinds
    per_row = 4 + 4 + 8 + 8 + (8 + 4) * (1 + 3 + 1 + 4)
    assert bench.DUMP_ROWS * per_row <= 64e6

"""GPU tests of the reduction kinds at several rotation rates in one pass (pdeval_fol_reduce_multi; DESIGN.md §14
"Reduction kinds at several rotation rates"): every slice against the 40-digit rule of tests/fol_reduce_ref.py and,
byte for byte, against a pdeval_fol_reduce call at that Omega^2.  The reference's own margin assertion holds at each
Omega^2 used here on every row (checked on the CPU before the list was fixed; it runs again in `case`)."""
import functools

import numpy as np
import pytest

import fol_reduce_ref as F
import test_fol_reduce_cplx_host as C
from pdeval import foliation as FOL
from pdeval import problem_defs as P
from pdeval._lib import Context, PdevalError

pytestmark = pytest.mark.gpu

MS = (12, 16)                                  # 144 points: a partial last chunk; 256: full chunks
OMEGAS = ([0.0], [0.0, 1.0], [1.0, 0.25, 0.0, 1 / 9, 4.0, 0.0, 2.0, 0.5])   # K = 1, 2 and 8 (a repeat, not monotone)
ROWS = F.ROWS + C.ROWS                         # the real rows (stacks 3 and 4, CPLX), then the complex ones
N, NF = len(ROWS), len(F.ROWS)
LIST = list(range(N)) + [N + 5, N]             # every row, an entry out of range, the program with bad offsets
reference = functools.lru_cache(None)(F.reference)    # one 40-digit reference per (m, Omega^2), shared and never modified


@pytest.fixture(scope='module')
def case():
    """The references (built, and their margins asserted, before the GPU is opened), then ROWS resident on a
    validator's device with one more candidate whose offsets run past the program words."""
    import torch
    from pdeval.batch import BatchValidator
    for m in MS:
        for w in OMEGAS[2]:
            reference(m, w)
    bv = BatchValidator('force_free', device=0)
    p = bv.prepare_strings(ROWS)
    ops, off = np.asarray(p['ops'], dtype=np.int32), np.asarray(p['off'], dtype=np.int64)
    off = np.append(off, off[-1] + 7)          # candidate N: [n_words, n_words + 7), never dereferenced
    yield bv, (torch.from_numpy(ops).to('cuda:0'), int(ops.size), torch.from_numpy(off).to('cuda:0'), N + 1)
    bv.close()


def prm(m, cplx=False):
    return FOL.fol_params(FOL.FolParams(C.R.TAU, m, C.R.MIN_POINTS, 0), cplx=cplx)


@pytest.mark.parametrize('omegas', OMEGAS, ids=lambda w: f'K{len(w)}')
@pytest.mark.parametrize('m', MS)
def test_against_reference(case, m, omegas):
    """Slice k: kinds and counts of the real rows equal reference(m, omegas[k]) exactly, the table has its NaN pattern
    and deviates from its kappa and G by at most 100x the fp64 restatement's own deviation."""
    bv, prog = case
    kind, counts, qmax, tab = FOL.reduce_stream(bv.ctx, *prog, idx=LIST, params=prm(m), omega2=omegas, table=True)
    assert kind.shape == (len(omegas), len(LIST)) and tab.shape == (len(omegas), len(LIST), 3, m * m)
    tab = tab.cpu().numpy()
    for k, w in enumerate(omegas):
        r = reference(m, w)
        assert np.array_equal(kind[k, :NF], r['kind']) and np.array_equal(counts[k, :NF], r['counts']), (k, w)
        assert np.array_equal(np.isnan(tab[k, :NF, 1]), np.isnan(r['kappa'])) and np.array_equal(np.isnan(tab[k, :NF, 0]), ~r['fin'])
        dev = F.table_deviation(r, dict(kappa=tab[k, :NF, 1], G=tab[k, :NF, 2]))
        print(f'm={m} Omega^2={w}: closed-form fp64 {r["table_dev"]:.3e}, device {dev:.3e}')
        assert dev <= 100 * r['table_dev']


@pytest.mark.parametrize('cplx', (False, True))
@pytest.mark.parametrize('omegas', OMEGAS, ids=lambda w: f'K{len(w)}')
@pytest.mark.parametrize('m', MS)
def test_bits_of_single_calls(case, m, omegas, cplx):
    """Every slice of every output equals, as bytes, what pdeval_fol_reduce writes at that Omega^2, without and with
    PDEVAL_FOL_CPLX; the two bad list entries are none in every slice, and a row that is none at one Omega is none
    at all of them."""
    bv, prog = case
    multi = FOL.reduce_stream(bv.ctx, *prog, idx=LIST, params=prm(m, cplx), omega2=omegas, table=True)
    for k, w in enumerate(omegas):
        single = FOL.reduce_stream(bv.ctx, *prog, idx=LIST, params=prm(m, cplx), omega2=w, table=True)
        for a, b in zip(multi, single):
            a, b = (np.ascontiguousarray(v.cpu().numpy() if hasattr(v, 'cpu') else v) for v in (a[k], b))
            assert a.shape == b.shape and a.tobytes() == b.tobytes(), (k, w)
    kind, counts, qmax, tab = multi
    assert not kind[:, N:].any() and not counts[:, N:].any() and not qmax[:, N:].any() and np.isnan(tab[:, N:].cpu().numpy()).all()
    assert ((kind == 0) == (kind[0] == 0)).all()
    assert ((kind[:, F.ROWS.index(F.CPLX)] != 0) == cplx).all()      # the complex row: a kind only with the flag


def test_bad_arguments(case):
    """n_omega = 0 and 9, a negative Omega^2 in the middle of the list and a Kerr context return PDEVAL_ERR_ARG."""
    bv, prog = case
    for ws in ([], [0.5] * 9, [0.0, -1.0, 1.0]):
        with pytest.raises(PdevalError, match='pdeval error 1:'):
            FOL.reduce_stream(bv.ctx, *prog, omega2=ws)
    kerr = Context(P.kerr().problem_id, device=0)
    with pytest.raises(PdevalError, match='pdeval error 1:'):
        FOL.reduce_stream(kerr, *prog, omega2=[0.0, 1.0])
    kerr.close()
    with pytest.raises(ValueError):
        FOL.reduce_stream(bv.ctx, *prog, omega2=[0.0, 1.0], settle=(1e-12, 1e-3))

"""GPU tests of the settle tier of the reduction kinds (pdeval_fol_reduce_dd, reduce_stream's settle; DESIGN.md
§14 "Settled in double-double") against the rule on 40-digit closed-form jets (tests/fol_reduce_ref.py)."""
import numpy as np
import pytest

import fol_reduce_ref as F
from pdeval import foliation as FOL
from pdeval import problem_defs as P
from pdeval._lib import Context, PdevalError, default_fol_params
from test_fol_reduce_dd_host import BORDER, ROWS24

pytestmark = pytest.mark.gpu

MS = (16, 12)                                  # four full chunks; 144 = two full and a partial one
BAND = (1e-12, 1e-3)
N = len(ROWS24)
LIST = list(range(N)) + [N + 5]                # every row, then an entry out of range
AT1 = [F.RADIAL] + BORDER                      # current at Omega = 1


@pytest.fixture(scope='module')
def case():
    """The references per m (built, and their margins asserted, before the GPU is opened), then a
    BatchValidator with ROWS24 resident on its device.  Never modified."""
    import torch
    from pdeval.batch import BatchValidator
    ref = {(m, w): F.reference(m, w, rows) for m in MS for w, rows in ((0.0, ROWS24), (1.0, AT1))}
    bv = BatchValidator('force_free', device=0)
    p = bv.prepare_strings(ROWS24)
    depth = (np.asarray(p['ops'])[np.asarray(p['off'])[:-1]] >> 8) & 0xff
    assert depth[ROWS24.index(F.DEEP)] == 3 and depth[ROWS24.index(F.DEEP4)] == 4    # both instantiations run
    d_ops = torch.from_numpy(np.asarray(p['ops'], dtype=np.int32)).to('cuda:0')
    d_off = torch.from_numpy(np.asarray(p['off'], dtype=np.int64)).to('cuda:0')
    yield ref, bv, (d_ops, int(d_ops.numel()), d_off, N)
    bv.close()


def prm(m):
    p = default_fol_params()
    p.m = m
    return p


def run_dd(bv, prog, idx, m, omega2=0.0):
    """(kind, counts, qmax) of Context.fol_reduce_dd on the candidates idx; the outputs start as garbage."""
    import torch
    d_ops, n_words, d_off, n = prog
    lst = torch.tensor(idx, dtype=torch.int64, device=d_ops.device)
    out = [torch.full(s, v, dtype=t, device=d_ops.device) for s, v, t in
           (((len(idx),), 9, torch.uint8), ((len(idx), 4), -7, torch.int32), ((len(idx), 3), 5.0, torch.float64))]
    bv.ctx.fol_reduce_dd(d_ops.data_ptr(), n_words, d_off.data_ptr(), n, lst.data_ptr(), len(idx),
                         *(t.data_ptr() for t in out), omega2, prm(m))
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


@pytest.mark.parametrize('m', MS)
def test_every_row_in_double_double(case, m):
    """Kinds and counts equal the 40-digit reference's exactly, DEEP (stack 3, the LDS instantiation) and DEEP4
    (stack 4, the private one) among them; the out-of-range entry and the complex row: kind 0, no counts; the
    border rows are vacuum, as Radial; no qmax is left in the band; at Omega = 1 they all carry current."""
    ref, bv, prog = case
    kind, counts, qmax = run_dd(bv, prog, LIST, m)
    print('qmax', qmax.tolist())
    assert np.array_equal(kind[:N], ref[m, 0.0]['kind']) and np.array_equal(counts[:N], ref[m, 0.0]['counts'])
    for row in (N, ROWS24.index(F.CPLX)):
        assert kind[row] == 0 and not counts[row].any() and not qmax[row].any()
    assert all(counts[ROWS24.index(s), 0] >= F.R.MIN_POINTS for s in (F.DEEP, F.DEEP4))
    assert all(kind[ROWS24.index(s)] == F.VACUUM == kind[ROWS24.index(F.RADIAL)] for s in BORDER), kind
    assert ((qmax <= BAND[0]) | (qmax >= BAND[1])).all()
    kind1, counts1, _ = run_dd(bv, prog, [ROWS24.index(s) for s in AT1], m, 1.0)
    assert (kind1 == F.CURRENT).all() and np.array_equal(kind1, ref[m, 1.0]['kind'])
    assert np.array_equal(counts1, ref[m, 1.0]['counts'])


@pytest.mark.parametrize('m', MS)
def test_settle_replaces_only_the_band(case, m):
    """reduce_stream with settle against without: rows whose fp64 qmax lies outside the band keep their bits,
    the table keeps its bits throughout, rows inside carry the double-double results; no border row stays
    current, and at m = 16 (fp64 |W| / S_W of 1.26e-5 to 1.64e-5 there) some row is settled.
    BatchValidator.reduction_kinds forwards the option."""
    ref, bv, prog = case
    k0, c0, q0, t0 = FOL.reduce_stream(bv.ctx, *prog, idx=LIST, params=prm(m), table=True)
    k1, c1, q1, t1, pos = FOL.reduce_stream(bv.ctx, *prog, idx=LIST, params=prm(m), table=True, settle=BAND)
    band = ((q0 > BAND[0]) & (q0 < BAND[1])).any(1)
    print('fp64 qmax of the border rows', q0[N - len(BORDER):N].tolist(), 'settled', pos.tolist())
    assert np.array_equal(pos, np.flatnonzero(band)) and (m != 16 or pos.size)
    dd = run_dd(bv, prog, LIST, m)
    for new, old, settled in zip((k1, c1, q1), (k0, c0, q0), dd):
        assert np.array_equal(new[~band], old[~band]) and np.array_equal(new[band], settled[band])
    assert np.array_equal(t1.cpu().numpy().view(np.int64), t0.cpu().numpy().view(np.int64))
    assert (k1[N - len(BORDER):N] != F.CURRENT).all()
    via = bv.reduction_kinds(ROWS24, params=prm(m), settle=BAND)
    assert np.array_equal(via[0], k1[:N]) and np.array_equal(via[4], pos)


def test_bad_arguments(case):
    """A Kerr context, a negative or NaN omega2 and a null d_counts with n_list > 0 return PDEVAL_ERR_ARG."""
    import torch
    _, bv, (d_ops, n_words, d_off, n) = case
    keep = torch.zeros(64, dtype=torch.int64, device=d_ops.device)
    buf = keep.data_ptr()
    kerr = Context(P.kerr().problem_id, device=0)
    for ctx, counts, w in ((kerr, buf, 0.0), (bv.ctx, buf, -1.0), (bv.ctx, buf, float('nan')), (bv.ctx, 0, 0.0)):
        with pytest.raises(PdevalError, match='pdeval error 1:'):
            ctx.fol_reduce_dd(d_ops.data_ptr(), n_words, d_off.data_ptr(), n, 0, 2, buf, counts, buf, w)
    kerr.close()

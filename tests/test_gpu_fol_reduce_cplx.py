"""GPU tests of the reduction kinds of complex-valued rows (pdeval_fol_reduce with PDEVAL_FOL_CPLX)
against the 40-digit reference of tests/test_fol_reduce_cplx_host.py: kinds and counts exactly; qmax is printed."""
import numpy as np
import pytest

import fol_reduce_ref as F
import test_fol_reduce_cplx_host as C
from pdeval import foliation as FOL
from pdeval.opcodes import FLAG_COMPLEX

pytestmark = pytest.mark.gpu
MS = (16, 12)                                  # four full chunks; 144 = two full and a partial one
N = len(C.ROWS)
LIST = list(range(N)) + [N + 5]                # every row, then an entry out of range


@pytest.fixture(scope='module')
def case():
    """The references per m (margins asserted before the GPU is opened), then ROWS resident on a validator's device."""
    import torch
    from pdeval.batch import BatchValidator
    ref = {(m, w): C.reference(m, w, rows) for m in MS for w, rows in ((0.0, C.ROWS), (1.0, C.OMEGA))}
    bv = BatchValidator('force_free', device=0)
    p = bv.prepare_strings(C.ROWS)
    ops, off = np.asarray(p['ops'], dtype=np.int32), np.asarray(p['off'], dtype=np.int64)
    took = ref[16, 0.0]['took']
    depth, flagged = ((ops[off[:-1]] >> 8) & 0xff)[took], ((ops[off[:-1]] & FLAG_COMPLEX) != 0)[took]
    assert (depth == 3).any() and (depth > 3).any()           # both instantiations run, the shallow one with both slots
    assert flagged.any() and not flagged.all()                # both selections
    yield ref, bv, (torch.from_numpy(ops).to('cuda:0'), int(ops.size), torch.from_numpy(off).to('cuda:0'), N)
    bv.close()


def prm(m, cplx=True):
    return FOL.fol_params(FOL.FolParams(C.R.TAU, m, C.R.MIN_POINTS, 0), cplx=cplx)


@pytest.mark.parametrize('m', MS)
def test_kinds_and_counts(case, m):
    """Flag set: kind and counts equal the reference's, each twin has its partner's kind, NO_DIR and the bad entry are
    none with zero counts.  Flag clear: the complex rows are none; every other row and the table keep their bits."""
    ref, bv, prog = case
    r = ref[m, 0.0]
    kind, counts, qmax, tab = FOL.reduce_stream(bv.ctx, *prog, idx=LIST, params=prm(m), table=True)
    k0, c0, q0, t0 = FOL.reduce_stream(bv.ctx, *prog, idx=LIST, params=prm(m, False), table=True)
    print(f'm={m} qmax of the complex rows', {int(i): qmax[i].tolist() for i in np.flatnonzero(r['took'])})
    assert np.array_equal(kind[:N], r['kind']) and np.array_equal(counts[:N], r['counts'])
    assert all(kind[2 * k] == kind[2 * k + 1] != 0 for k in range(len(C.PAIRS))), kind
    for row in (N, C.ROWS.index(C.NO_DIR)):
        assert kind[row] == 0 and not counts[row].any() and not qmax[row].any()
    keep = np.append(~r['took'], True)
    assert not k0[~keep].any() and not c0[~keep].any()
    for a, b in ((kind, k0), (counts, c0), (qmax.view(np.int64), q0.view(np.int64))):
        assert np.array_equal(a[keep], b[keep])
    assert np.array_equal(tab.cpu().numpy().view(np.int64), t0.cpu().numpy().view(np.int64))


@pytest.mark.parametrize('m', MS)
def test_omega_settle_and_validator(case, m):
    """Omega^2 = 1: Radial and its twin carry current.  settle with cplx: real rows bit-identical to the call without
    cplx, complex rows as the unsettled flagged call.  BatchValidator.reduction_kinds(cplx=True) agrees."""
    ref, bv, prog = case
    kind, counts, _, _ = FOL.reduce_stream(bv.ctx, *prog, idx=[C.ROWS.index(s) for s in C.OMEGA], params=prm(m), omega2=1.0)
    assert kind.tolist() == [F.CURRENT] * 2 == ref[m, 1.0]['kind'].tolist() and np.array_equal(counts, ref[m, 1.0]['counts'])
    took = np.append(ref[m, 0.0]['took'], False)
    plain = FOL.reduce_stream(bv.ctx, *prog, idx=LIST, params=prm(m))
    with_c = FOL.reduce_stream(bv.ctx, *prog, idx=LIST, params=prm(m), settle=(1e-12, 1e-3))
    without = FOL.reduce_stream(bv.ctx, *prog, idx=LIST, params=prm(m, False), settle=(1e-12, 1e-3))
    for a, b, c in zip(with_c[:3], without[:3], plain[:3]):
        assert np.array_equal(a[~took], b[~took]) and np.array_equal(a[took], c[took])
    via = bv.reduction_kinds(C.ROWS, params=prm(m, False), cplx=True)
    assert np.array_equal(via[0], ref[m, 0.0]['kind']) and np.array_equal(via[1], ref[m, 0.0]['counts'])

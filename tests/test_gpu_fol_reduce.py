"""GPU tests of the reduction kinds (pdeval_fol_reduce; DESIGN.md §14 "Reduction kinds") against SymPy
derivatives evaluated with mpmath at 40 digits and the rule restated in numpy (tests/fol_reduce_ref.py).
Table tolerance: 100x the largest scaled deviation of the fp64 restatement on closed-form derivatives
from the 40-digit values on the same rows (jets round differently from closed forms), measured by the
reference itself: 1.26e-13 at m = 12 and 1.22e-13 at m = 16."""
import numpy as np
import pytest

import fol_reduce_ref as F
from pdeval import foliation as FOL
from pdeval import problem_defs as P
from pdeval._lib import Context, PdevalError, default_fol_params

pytestmark = pytest.mark.gpu

MS = (16, 12)                                  # four full chunks; 144 = two full and a partial one
OMEGA = [F.RADIAL, 'z', 'rho**2']              # vacuum, free, free at Omega = 0; current, vacuum, free at Omega = 1
LIST = list(range(len(F.ROWS))) + [len(F.ROWS) + 5]   # every row, then an entry out of range


@pytest.fixture(scope='module')
def case():
    """The references per m (built, and their margins asserted, before the GPU is opened), then a
    BatchValidator with fol_reduce_ref.ROWS resident on its device.  Never modified."""
    import torch
    from pdeval.batch import BatchValidator
    ref = {(m, w): F.reference(m, w, rows) for m in MS for w, rows in ((0.0, F.ROWS), (1.0, OMEGA))}
    bv = BatchValidator('force_free', device=0)
    p = bv.prepare_strings(F.ROWS)
    depth = (np.asarray(p['ops'])[np.asarray(p['off'])[:-1]] >> 8) & 0xff
    assert depth[F.ROWS.index(F.DEEP)] == 3 and depth[F.ROWS.index(F.DEEP4)] == 4    # both instantiations run
    dev = torch.device('cuda', 0)
    d_ops = torch.from_numpy(np.asarray(p['ops'], dtype=np.int32)).to(dev)
    d_off = torch.from_numpy(np.asarray(p['off'], dtype=np.int64)).to(dev)
    yield ref, bv, (d_ops, int(d_ops.numel()), d_off, len(F.ROWS))
    bv.close()


def prm(m):
    p = default_fol_params()
    p.m = m
    return p


@pytest.mark.parametrize('m', MS)
def test_kinds_counts_table(case, m):
    """Kinds and the four counts equal the reference's exactly (the out-of-range entry and the complex row:
    kind 0, no counts); the named rows carry the kinds of the method and the rows of one class one kind;
    kappa and G have the reference's NaN pattern and its values within the bound."""
    ref, bv, prog = case
    r = ref[m, 0.0]
    kind, counts, qmax, tab = FOL.reduce_stream(bv.ctx, *prog, idx=LIST, params=prm(m), table=True)
    n = len(F.ROWS)
    print('qmax', qmax.tolist())
    assert np.array_equal(kind[:n], r['kind']) and np.array_equal(counts[:n], r['counts'])
    assert kind[n] == 0 and not counts[n].any() and kind[F.ROWS.index(F.CPLX)] == 0
    named = dict(zip(F.ROWS, kind[:n]))
    assert all(named[s] == k for s, k in F.KINDS0.items()), named
    assert all(named[a] == named[b] for a, b in F.SAME_CLASS)
    assert ((qmax <= 1e-12) | (qmax >= 1e-3)).all()
    tab = tab.cpu().numpy()
    assert np.isnan(tab[n]).all()
    assert np.array_equal(np.isnan(tab[:n, 1]), np.isnan(r['kappa'])) and np.array_equal(np.isnan(tab[:n, 2]), np.isnan(r['G']))
    assert np.array_equal(np.isnan(tab[:n, 0]), ~r['fin'])
    dev = F.table_deviation(r, dict(kappa=tab[:n, 1], G=tab[:n, 2]))
    print(f'table m={m}: closed-form fp64 {r["table_dev"]:.3e}, device {dev:.3e}')
    assert dev <= 100 * r['table_dev']


@pytest.mark.parametrize('m', MS)
def test_omega_and_entry_points(case, m):
    """Omega is wired through: Radial, z, rho**2 are vacuum, free, free at Omega = 0 and current, vacuum,
    free at Omega = 1, with the reference's counts; the same through BatchValidator.reduction_kinds; the
    optional outputs may be absent; class_kinds shows a class holding two kinds."""
    import torch
    ref, bv, _ = case
    for w, want in ((0, [F.VACUUM, F.FREE, F.FREE]), (1, [F.CURRENT, F.VACUUM, F.FREE])):
        kind, counts, _, tab = bv.reduction_kinds(OMEGA, omega=w, params=prm(m))
        rows = [F.ROWS.index(s) for s in OMEGA] if w == 0 else slice(None)
        assert kind.tolist() == want == ref[m, float(w)]['kind'][rows].tolist() and tab is None
        assert np.array_equal(counts, ref[m, float(w)]['counts'][rows])
    kind, counts, _, _ = bv.reduction_kinds(F.ROWS, params=prm(m))
    assert np.array_equal(kind, ref[m, 0.0]['kind']) and np.array_equal(counts, ref[m, 0.0]['counts'])
    d_ops, n_words, d_off, n = case[2]
    only = torch.full((n,), 9, dtype=torch.uint8, device=d_ops.device)
    bv.ctx.fol_reduce(d_ops.data_ptr(), n_words, d_off.data_ptr(), n, 0, n, only.data_ptr(), params=prm(m))
    torch.cuda.synchronize()
    assert np.array_equal(only.cpu().numpy(), kind)
    assert FOL.class_kinds([0, 0, 1, -1, 1], [2, 2, 3, 0, 1]) == {0: (2,), 1: (1, 3)}


def test_bad_arguments(case):
    """A Kerr context, a negative or non-finite omega2 and a bad m return PDEVAL_ERR_ARG."""
    _, bv, prog = case
    kerr = Context(P.kerr().problem_id, device=0)
    with pytest.raises(PdevalError, match='pdeval error 1:'):
        FOL.reduce_stream(kerr, *prog)
    kerr.close()
    for kw in (dict(omega2=-1.0), dict(omega2=float('nan')), dict(omega2=float('inf')), dict(params=prm(3))):
        with pytest.raises(PdevalError, match='pdeval error 1:'):
            FOL.reduce_stream(bv.ctx, *prog, **kw)

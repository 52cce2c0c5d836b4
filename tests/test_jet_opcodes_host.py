"""Every jet opcode of the device source, built for the CPU (tests/hostsim), and of the oracle,
against the 50-digit Taylor coefficients of tests/jet_opcode_cases.py -- and the claim of tier 2
(DESIGN.md §6): |computed - exact| <= noise_kappa * 2^-52 * E, coefficient by coefficient.
The point stage's four precision tiers (sim_point_tier) are checked against the exact
determinant at p* = (4/5, 6/7)."""
import numpy as np
import pytest

import jet_opcode_cases as JC
import oracle_lib as O
from pdeval import _lib
from pdeval.opcodes import FLAG_COMPLEX, PDOP, P_OPS
from test_hostsim import sim  # noqa: F401  (the host build of the device source)


@pytest.fixture(scope='module')
def gold():
    return JC.golden()


@pytest.fixture(scope='module')
def kappa():
    return float(_lib.default_params(0).noise_kappa)


def test_table_covers_what_it_claims():
    progs = JC.programs()
    seen = {}            # opcode -> operands
    for name, w, flags, single, true in progs:
        dec = JC.decode(w)
        assert any(op == PDOP['PUSH_I'] for op, *_ in dec) == bool(flags & FLAG_COMPLEX), name
        for op, operand, hi, lo in dec:
            seen.setdefault(op, set()).add((operand, hi, lo is not None))
    assert sorted(seen) == list(range(1, 35))
    for op in [PDOP['POWN']] + sorted(P_OPS):
        assert {o & 0xff for o, *_ in seen[op]} == set(JC.P_NS), op
        if op != PDOP['POWN']:
            assert {(o >> 8) & 1 for o, *_ in seen[op]} == {0, 1}, op
    assert {hi for _, hi, _ in seen[PDOP['POW']]} >= set(JC.POW_ALPHAS)
    for nm in ('ADDC', 'MULC', 'RDIVC', 'PUSH_C'):
        assert {dd for *_, dd in seen[PDOP[nm]]} == {False, True}, nm
    names = {n for n, *_ in progs}
    assert names >= {f'{o}.d{d}' for o in ('sub', 'rsub', 'div', 'rdiv') for d in range(2, 9)}
    for name, w, *_ in progs:
        if name.split('.')[0] in ('sub', 'rsub', 'div', 'rdiv', 'mix'):
            assert (int(w[0]) >> 8) & 0xff == int(name.split('.d')[1]), name
    mix = next(w for n, w, *_ in progs if n == 'mix.d8')
    assert set(range(PDOP['ADD'], PDOP['RDIV'] + 1)) <= set(JC.opcodes_of(mix))
    assert len(JC.XS) == 70 and (JC.XS[0], JC.YS[0]) == (0.8, 6 / 7)


def test_reference_meets_the_condition_on_the_points(gold):
    """No (program, point) pair is skipped: each is finite, real (but for the complex programs),
    and MARGIN away from every pole, branch point and Abs kink; Abs sees both signs."""
    progs = JC.programs()
    assert gold.hi.shape == (len(progs), 70, 15)
    assert np.isfinite(gold.hi.view(float)).all() and np.isfinite(gold.lo.view(float)).all()
    assert (gold.margin >= JC.MARGIN).all(), gold.margin.min()
    for ip, (name, w, flags, *_) in enumerate(progs):
        if not flags & FLAG_COMPLEX:
            assert not gold.hi[ip].imag.any() and not gold.lo[ip].imag.any(), name
    assert (JC.YS > 0).any() and (JC.YS < 0).any()        # the argument of the ABS programs
    # inner jets of the compositions: every coefficient non-zero
    inner = JC.assemble(JC.INNER, 3)
    for k in (0, 17, 69):
        u, _ = JC.ref_jet(inner, JC.XS[k], JC.YS[k])
        assert all(c != 0 for c in u)


def test_golden_file_is_the_reference(gold):
    """A fixed sample of rows recomputed: the stored digits exactly; the exact determinant of
    every program (SymPy, exact rationals) equals the one the reference jets give at p*."""
    progs = JC.programs()
    for ip in range(0, len(progs), 5):
        for k in (0, 23, 64, 69):
            u, mg = JC.ref_jet(progs[ip][1], JC.XS[k], JC.YS[k])
            hi, lo = JC.split_jet(u)
            assert np.array_equal(hi, gold.hi[ip, k]) and np.array_equal(lo, gold.lo[ip, k]), (progs[ip][0], k)
            assert min(float(mg), 1e300) == gold.margin[ip, k]
    for ip, (name, w, *_) in enumerate(progs):
        d = JC.ref_det(w)
        assert abs(d - gold.det[ip]) <= 1e-40 * max(abs(gold.det[ip]), 1), (name, d, gold.det[ip])
    for ip, d in gold.det_twin.items():
        t = JC.ref_det(JC.rounded_twin(progs[ip][1]))
        assert abs(t - d) <= 1e-40 * max(abs(d), 1), (progs[ip][0], t, d)


def test_reference_matches_sympy_derivatives():
    """The mpmath interpreter against SymPy's exact derivatives of the same words."""
    import sympy as sp
    rho, z = sp.symbols('rho z', real=True)
    progs = {n: w for n, w, *_ in JC.programs()}
    for name in ('c.pow1.414', 'div.d5', 'rdiv_p15y', 'c.abs'):
        w = progs[name]
        u = JC.sympy_expr(w, rho, z)
        x0, y0 = JC.XS[3], JC.YS[3]
        pt = {rho: sp.Rational(x0), z: sp.Rational(y0)}
        ref, _ = JC.ref_jet(w, x0, y0)
        for k, (i, j) in enumerate(JC.IDX):
            der = sp.diff(u, rho, i, z, j) if (i or j) else u
            exact = JC.MP.mpf(str(sp.N(der.subs(pt).doit(), 50))) / (JC.MP.factorial(i) * JC.MP.factorial(j))
            assert abs(ref[k] - exact) <= 1e-40 * max(1, abs(exact)), (name, i, j)


def _host_jets(sim, w, tier2):  # noqa: F811
    jets, errs = np.zeros((70, 15)), np.zeros((70, 15))
    res = np.zeros(4)
    for k in range(70):
        rc = sim.sim_point(0, w.ctypes.data, len(w), JC.XS[k], JC.YS[k], tier2, jets[k].ctypes.data,
                           errs[k].ctypes.data, res.ctypes.data)
        assert rc == 0, (rc, k)
    return jets, errs


@pytest.mark.parametrize('tier2', [0, 1])
def test_device_source_jets_and_bounds(sim, gold, kappa, tier2):  # noqa: F811
    """(a) accuracy in both modes; in tier-2 mode (b) the bound E is sound with the factor
    noise_kappa and (c) not vacuous on the single-opcode programs."""
    stats, bad = JC.Stats(), []
    for ip, (name, w, flags, single, _) in enumerate(JC.programs()):
        if flags & FLAG_COMPLEX:
            continue
        jets, errs = _host_jets(sim, w, tier2)
        JC.check_jets(name, w, gold.hi[ip], gold.lo[ip], jets, errs if tier2 else None, kappa, single, stats, bad)
    print('\n' + stats.table(f'host build, tier2 = {tier2}'))
    assert not bad, (len(bad), bad[:8])


def test_oracle_jets(gold):
    """(d) the oracle on the same words and points passes (a) -- the complex programs in its
    complex mode."""
    stats, bad = JC.Stats(), []
    for ip, (name, w, flags, *_) in enumerate(JC.programs()):
        cplx = bool(flags & FLAG_COMPLEX)
        jets = np.array([O.jet(0, w, JC.XS[k], JC.YS[k], cplx=cplx) for k in range(70)])
        if cplx:
            scale = np.maximum(1.0, np.abs(gold.hi[ip]).max(axis=1))[:, None]
            rel = np.abs((jets - gold.hi[ip]) - gold.lo[ip]) / scale
            assert (rel <= JC.REL_TOL).all(), (name, rel.max())
        else:
            JC.check_jets(name, w, gold.hi[ip], gold.lo[ip], jets, None, 0.0, False, stats, bad)
    print('\n' + stats.table('oracle'))
    assert not bad, (len(bad), bad[:8])


def _tier(sim, w, tier):  # noqa: F811
    out = np.zeros(6)
    rc = sim.sim_point_tier(0, w.ctypes.data, len(w), 0, tier, out.ctypes.data)
    assert rc == 0, rc
    return out


def test_point_stage_tiers(sim, gold, kappa):  # noqa: F811
    """sim_point_tier (fp64, complex, double-double, complex double-double) against the exact
    determinant at p*: within noise_kappa x its own noise bound, the double-double tiers to 1e-10
    relative, true solutions within their noise."""
    bad = []
    for ip, (name, w, flags, _, true) in enumerate(JC.programs()):
        for tier in JC.tiers_of(flags):
            JC.check_tier(name, tier, _tier(sim, w, tier), gold.det[ip], kappa, true, bad)
    assert not bad, (len(bad), bad[:8])


def test_double_double_tier_reads_the_low_part(sim, gold, kappa):  # noqa: F811
    """Each PDEVAL_IMM_DD program against its twin with the constant rounded to a double: the
    exact determinants differ by more than the tier's noise, and so do the tier's results."""
    progs = JC.programs()
    assert len(gold.det_twin) == 4
    for ip, det_twin in gold.det_twin.items():
        name, w = progs[ip][:2]
        a, b = _tier(sim, w, 2), _tier(sim, JC.rounded_twin(w), 2)
        lim = kappa * max(a[4], b[4])
        assert abs(det_twin - gold.det[ip]) > lim, (name, det_twin, gold.det[ip], lim)
        assert abs(a[0] - b[0]) > lim, (name, a, b)
        # and each tier-2 value is its own determinant
        bad = []
        JC.check_tier(name + '.twin', 2, b, det_twin, kappa, False, bad)
        assert not bad, bad

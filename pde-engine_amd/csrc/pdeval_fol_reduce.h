// pdeval_fol_reduce.h -- the reduction kind of a force-free foliation (DESIGN.md §14 "Reduction
// kinds"): which field lives on the level sets of an accepted u.
//
// With psi = psi(u) the stream equation becomes  psi' A + psi'' B = -I I'(psi), where
//   A = (1 - rho^2 w)(u_rr + u_zz) - (1 + rho^2 w) u_r / rho,   B = (1 - rho^2 w)(u_r^2 + u_z^2),
// w = Omega^2 (validator.py:323-332).  The right side is a function of u alone, so the derivative
// along the level sets, L_T = u_z d_rho - u_r d_z, annihilates it:  psi' L_T A + psi'' L_T B = 0.
// The validator's determinant says that this has a solution psi(u); the three quantities
//   L_T A,   L_T B,   W = B L_T A - A L_T B
// say which:
//   free     L_T A == 0 and L_T B == 0: A and B are functions of u alone, every psi(u) solves the
//            equation and the current is whatever -(psi' A + psi'' B) gives;
//   vacuum   not free, W == 0: L_T(A / B) = 0, and psi'' / psi' = -A / B has a current-free
//            solution, unique up to an affine map;
//   current  W != 0: psi is fixed by psi'' / psi' = kappa = -L_T A / L_T B and carries the current
//            I I' = G psi',  G = W / L_T B
//            (psi' A + psi'' B = psi' (A + kappa B) = psi' (A L_T B - B L_T A) / L_T B = -G psi').
// The kind does not change under u -> f(u): it is a property of the class.  It depends on Omega.
//
// This header holds the per-point rule, which also compiles for the host under -DPD_HOST_SIM
// (tests/hostsim/sim_fol_reduce.cpp, sim_fol_reduce_dd.cpp, sim_fol_reduce_cplx.cpp), its
// double-double twin of the settle tier, its complex twin of the PDEVAL_FOL_CPLX pass, the
// kernels' argument blocks and their launchers.
#pragma once
#include "pdeval_foliation.h"

namespace pd {

// ---------------------------------------------------------------- the per-point rule (host + device)
// From the order-3 jet of u (ten Taylor coefficients c[ji(i, j)]), at rho = x, with p = u_rho and
// q = u_z as jets (FFEpi::P / Q), lap = u_rr + u_zz and N = p^2 + q^2 to order 1, and the two
// factors as jets in the rho direction, f = 1 - rho^2 w = (1 - x^2 w, -2 x w) and
// g = (1 + rho^2 w) / rho = (1/x + x w, w - 1/x^2):
//   A = f lap - g p,  B = f N                                (order 1: A00, A10, A01)
//   L_T A = q00 A10 - p00 A01,  L_T B = q00 B10 - p00 B01,  W = B00 L_T A - A00 L_T B.
// Each X of the three has a magnitude shadow S_X: the same expression on |c_ij| with every factor
// replaced by its modulus and every difference by a sum (f -> (1 + x^2 w, 2 x w),
// g -> (1/|x| + |x| w, w + 1/x^2)), the MAG = true evaluation of FFEpi; S_W = S_B S_LA + S_A S_LB.
// The point is finite iff the ten coefficients pass jet_coef_ok and the three X and the three S_X
// are finite.  At a finite point X is bad iff |X| > tau S_X (no division); S_X == 0 is an exact
// zero, not bad, and the point still counts (u = z: L_T B = 0 exactly).
// Contraction is off and every product is rounded on its own, so a host build computes the same
// doubles as the device.
enum { RED_LA = 0, RED_LB = 1, RED_W = 2 };
struct RedPoint {
    double X[3], S[3];
    bool fin;
    bool bad[3];
};
template <bool MAG>
PD_HD void red_forms(const double* u, double x, double w, double* X) {
#pragma clang fp contract(off)
    using E = FFEpi<double, MAG>;
    const double x2w = (x * x) * w, r0 = 1.0 / x;
    const double f0 = MAG ? 1.0 + x2w : 1.0 - x2w;
    const double f1 = (MAG ? 2.0 : -2.0) * (MAG ? fabs(x) : x) * w;
    const double g0 = MAG ? fabs(r0) + fabs(x) * w : r0 + x * w;
    const double g1 = MAG ? w + r0 * r0 : w - r0 * r0;
    const double p00 = E::P(u, 0, 0), p10 = E::P(u, 1, 0), p01 = E::P(u, 0, 1);
    const double q00 = E::Q(u, 0, 0), q10 = E::Q(u, 1, 0), q01 = E::Q(u, 0, 1);
    // lap_ij = (i+1)(i+2) c_{i+2,j} + (j+1)(j+2) c_{i,j+2}
    const double l00 = E::U(u, 2, 0) * 2.0 + E::U(u, 0, 2) * 2.0;
    const double l10 = E::U(u, 3, 0) * 6.0 + E::U(u, 1, 2) * 2.0;
    const double l01 = E::U(u, 2, 1) * 2.0 + E::U(u, 0, 3) * 6.0;
    const double A00 = f0 * l00 + E::sgn(g0 * p00);
    const double A10 = (f0 * l10 + f1 * l00) + E::sgn(g0 * p10 + g1 * p00);
    const double A01 = f0 * l01 + E::sgn(g0 * p01);
    const double n00 = p00 * p00 + q00 * q00;
    const double n10 = 2.0 * (p00 * p10 + q00 * q10);
    const double n01 = 2.0 * (p00 * p01 + q00 * q01);
    const double B00 = f0 * n00, B10 = f0 * n10 + f1 * n00, B01 = f0 * n01;
    X[RED_LA] = q00 * A10 + E::sgn(p00 * A01);
    X[RED_LB] = q00 * B10 + E::sgn(p00 * B01);
    X[RED_W] = B00 * X[RED_LA] + E::sgn(A00 * X[RED_LB]);
}
PD_HD RedPoint red_point(const double* u, double x, double w, double tau) {
#pragma clang fp contract(off)
    RedPoint r;
    red_forms<false>(u, x, w, r.X);
    red_forms<true>(u, x, w, r.S);
    r.fin = true;
#pragma unroll
    for (int i = 0; i < 10; ++i) r.fin = r.fin && fabs(u[i]) < kHugeJet;   // jet_coef_ok
#pragma unroll
    for (int k = 0; k < 3; ++k) r.fin = r.fin && finite_(r.X[k]) && finite_(r.S[k]);
#pragma unroll
    for (int k = 0; k < 3; ++k) r.bad[k] = r.fin && fabs(r.X[k]) > tau * r.S[k];
    return r;
}
// the diagnostic |X| / S_X of a finite point (IEEE division); 0 at an exact zero, never 0 / 0
PD_HD double red_q(const RedPoint& r, int k) { return r.S[k] > 0.0 ? fabs(r.X[k]) / r.S[k] : 0.0; }
// the coefficient functions of the reduced ODE at a point: kappa and G, NaN unless the point is
// finite and L_T B is bad (distinguishable from zero); G is not clamped
PD_HD void red_coefs(const RedPoint& r, double& kappa, double& G) {
    const double nan = __builtin_nan("");
    const bool ok = r.fin && r.bad[RED_LB];
    kappa = ok ? -r.X[RED_LA] / r.X[RED_LB] : nan;
    G = ok ? r.X[RED_W] / r.X[RED_LB] : nan;
}

// ---------------------------------------------------------------- the per-point rule in double-double
// The settle tier (pdeval_fol_reduce_dd): the same rule on an order-3 jet of double-doubles.  X is
// the expression tree of red_forms<false>, operation for operation, in dd (dd.h); rho is a grid
// double and enters exactly, Omega^2 is the caller's double.  The shadows stay plain fp64, on the
// moduli of the coefficients' high parts (they only scale the test: as dd_point_stage does with
// FFEpi<double, true>).  Finite: the ten |hi(c_i)| below kHugeJet, X (both words) and S finite;
// bad: |hi(X)| > tau S.  The fp64 functions above are not touched.
struct RedPointDD {
    dd X[3];
    double S[3];
    bool fin;
    bool bad[3];
};
PD_HD void red_forms_dd(const dd* u, dd x, double w, dd* X) {
    using E = FFEpi<dd, false>;
    const dd one = dd_from(1.0);
    const dd x2w = (x * x) * w, r0 = dd_div(one, x);
    const dd f0 = one - x2w;
    const dd f1 = (x * -2.0) * w;
    const dd g0 = r0 + x * w;
    const dd g1 = dd_from(w) - r0 * r0;
    const dd p00 = E::P(u, 0, 0), p10 = E::P(u, 1, 0), p01 = E::P(u, 0, 1);
    const dd q00 = E::Q(u, 0, 0), q10 = E::Q(u, 1, 0), q01 = E::Q(u, 0, 1);
    const dd l00 = E::U(u, 2, 0) * 2.0 + E::U(u, 0, 2) * 2.0;
    const dd l10 = E::U(u, 3, 0) * 6.0 + E::U(u, 1, 2) * 2.0;
    const dd l01 = E::U(u, 2, 1) * 2.0 + E::U(u, 0, 3) * 6.0;
    const dd A00 = f0 * l00 - g0 * p00;
    const dd A10 = (f0 * l10 + f1 * l00) - (g0 * p10 + g1 * p00);
    const dd A01 = f0 * l01 - g0 * p01;
    const dd n00 = p00 * p00 + q00 * q00;
    const dd n10 = (p00 * p10 + q00 * q10) * 2.0;
    const dd n01 = (p00 * p01 + q00 * q01) * 2.0;
    const dd B00 = f0 * n00, B10 = f0 * n10 + f1 * n00, B01 = f0 * n01;
    X[RED_LA] = q00 * A10 - p00 * A01;
    X[RED_LB] = q00 * B10 - p00 * B01;
    X[RED_W] = B00 * X[RED_LA] - A00 * X[RED_LB];
}
PD_HD RedPointDD red_point_dd(const dd* u, double x, double w, double tau) {
#pragma clang fp contract(off)
    RedPointDD r;
    double m[10];
#pragma unroll
    for (int i = 0; i < 10; ++i) m[i] = mag(u[i]);
    red_forms_dd(u, dd_from(x), w, r.X);
    red_forms<true>(m, x, w, r.S);
    r.fin = true;
#pragma unroll
    for (int i = 0; i < 10; ++i) r.fin = r.fin && m[i] < kHugeJet;
#pragma unroll
    for (int k = 0; k < 3; ++k) r.fin = r.fin && finite_(r.X[k]) && finite_(r.S[k]);
#pragma unroll
    for (int k = 0; k < 3; ++k) r.bad[k] = r.fin && fabs(r.X[k].hi) > tau * r.S[k];
    return r;
}
PD_HD double red_q(const RedPointDD& r, int k) { return r.S[k] > 0.0 ? fabs(r.X[k].hi) / r.S[k] : 0.0; }

// ---------------------------------------------------------------- the per-point rule of a complex-valued u
// PDEVAL_FOL_CPLX (pdeval_fol_reduce_cplx.hip; DESIGN.md §14 "Reduction kinds of complex-valued
// rows").  If u = F(g) with g real and F complex-valued of a real argument, then
// A_u = F' A_g + F'' B_g, B_u = F'^2 B_g and T_u = F' T_g, hence
//   L_T A_u = F' (F' L_T A_g + F'' L_T B_g),   L_T B_u = F'^3 L_T B_g,   W_u = F'^4 W_g:
// the three quantities of u, in complex arithmetic and tested by modulus, vanish where those of g
// do, and free, vacuum and current carry over.  X is the expression tree of red_forms<false>,
// operation for operation, on an order-3 jet of cplx; rho and Omega^2 stay real, so the factors
// f and g are doubles and scale both parts.  The shadows stay plain fp64, red_forms<true> on the
// moduli m[i] = |c_i| of the coefficients.  Finite: the ten m[i] below kHugeJet, X (both parts)
// and S finite, and the point has a real direction -- fol_cplx_point(u, u_rho, u_z, tau).fin, the
// test of the complex field pass, so the kind is defined exactly where the class is
// (rho + i z has no such point).  Bad: |X| > tau S with |X| the modulus.  The fp64 and dd
// functions above are not touched.
struct RedPointCplx {
    cplx X[3];
    double S[3];
    bool fin;
    bool bad[3];
};
PD_HD void red_forms_cplx(const cplx* u, double x, double w, cplx* X) {
#pragma clang fp contract(off)
    using E = FFEpi<cplx, false>;
    const double x2w = (x * x) * w, r0 = 1.0 / x;
    const double f0 = 1.0 - x2w;
    const double f1 = -2.0 * x * w;
    const double g0 = r0 + x * w;
    const double g1 = w - r0 * r0;
    const cplx p00 = E::P(u, 0, 0), p10 = E::P(u, 1, 0), p01 = E::P(u, 0, 1);
    const cplx q00 = E::Q(u, 0, 0), q10 = E::Q(u, 1, 0), q01 = E::Q(u, 0, 1);
    const cplx l00 = E::U(u, 2, 0) * 2.0 + E::U(u, 0, 2) * 2.0;
    const cplx l10 = E::U(u, 3, 0) * 6.0 + E::U(u, 1, 2) * 2.0;
    const cplx l01 = E::U(u, 2, 1) * 2.0 + E::U(u, 0, 3) * 6.0;
    const cplx A00 = l00 * f0 - p00 * g0;
    const cplx A10 = (l10 * f0 + l00 * f1) - (p10 * g0 + p00 * g1);
    const cplx A01 = l01 * f0 - p01 * g0;
    const cplx n00 = p00 * p00 + q00 * q00;
    const cplx n10 = (p00 * p10 + q00 * q10) * 2.0;
    const cplx n01 = (p00 * p01 + q00 * q01) * 2.0;
    const cplx B00 = n00 * f0, B10 = n10 * f0 + n00 * f1, B01 = n01 * f0;
    X[RED_LA] = q00 * A10 - p00 * A01;
    X[RED_LB] = q00 * B10 - p00 * B01;
    X[RED_W] = B00 * X[RED_LA] - A00 * X[RED_LB];
}
PD_HD RedPointCplx red_point_cplx(const cplx* u, double x, double w, double tau) {
#pragma clang fp contract(off)
    RedPointCplx r;
    double m[10];
#pragma unroll
    for (int i = 0; i < 10; ++i) m[i] = mag(u[i]);
    red_forms_cplx(u, x, w, r.X);
    red_forms<true>(m, x, w, r.S);
    r.fin = fol_cplx_point(u[0], u[ji(1, 0)], u[ji(0, 1)], tau).fin;
#pragma unroll
    for (int i = 0; i < 10; ++i) r.fin = r.fin && m[i] < kHugeJet;
#pragma unroll
    for (int k = 0; k < 3; ++k) r.fin = r.fin && finite_(r.X[k]) && finite_(r.S[k]);
#pragma unroll
    for (int k = 0; k < 3; ++k) r.bad[k] = r.fin && mag(r.X[k]) > tau * r.S[k];
    return r;
}
PD_HD double red_q(const RedPointCplx& r, int k) { return r.S[k] > 0.0 ? mag(r.X[k]) / r.S[k] : 0.0; }

// ---------------------------------------------------------------- the per-row rule (host + device)
// counts: {n_finite, bad_LA, bad_LB, bad_W} over the m x m sample points; the first case decides
struct RedCount {
    int n_fin, bad[3];
};
PD_HD int red_kind_of(const RedCount& n, int min_points) {
    if (n.n_fin < min_points) return PDEVAL_RED_NONE;
    if (n.bad[RED_LA] == 0 && n.bad[RED_LB] == 0) return PDEVAL_RED_FREE;
    if (n.bad[RED_W] == 0) return PDEVAL_RED_VACUUM;
    return PDEVAL_RED_CURRENT;
}

// The operand stack of one wave in order-3 jets: (MAXD - 1) x 10 x 64 doubles.  Two
// instantiations (DESIGN.md §14 "Reduction kinds"): the shallow one takes the programs whose
// header names a stack of at most kRedShallowD, the deep one the others up to kFolMaxD.
constexpr int kRedShallowD = 3;
template <int MAXD> constexpr int red_stack_doubles() { return (MAXD - 1) * nc(3) * 64; }

#ifndef PD_HOST_SIM
struct FolReduceArgs {
    const int32_t* ops;
    int64_t n_words;
    const int64_t* offsets;
    int64_t n;
    const int64_t* list;       // optional: row -> candidate index (NULL = identity)
    int64_t n_list;
    int n_chunk;               // ceil(m^2 / 64)
    FolGrid grid;
    PrmTab<double> prm;        // default (all 0): force-free programs carry no problem constants
    double omega2, tau;
    int min_points;
    uint8_t* kind;             // n_list
    int32_t* counts;           // optional, [n_list][4]
    double* qmax;              // optional, [n_list][3]
    double* table;             // optional, [n_list][3][m^2]: u, kappa, G
};
// both instantiations, the shallow one first, on s
void launch_fol_reduce(const FolReduceArgs& a, hipStream_t s);

// The settle tier (pdeval_fol_reduce_dd.hip): a.counts and a.qmax are required -- they are the
// accumulators of a row's waves -- and a.table is not used.  Clears them, runs both
// instantiations of fol_reduce_dd_kernel, then the finishing kernel, all on s.
void launch_fol_reduce_dd(const FolReduceArgs& a, hipStream_t s);

// The complex pass (pdeval_fol_reduce_cplx.hip, PDEVAL_FOL_CPLX), after launch_fol_reduce on the
// same stream: kind is read -- it selects the rows -- and written.  Its own block, so that
// FolReduceArgs and with it the fp64 kernels' argument layout stay as they are.
struct FolReduceCplxArgs {
    const int32_t* ops;
    int64_t n_words;
    const int64_t* offsets;
    int64_t n;
    const int64_t* list;       // optional: row -> candidate index (NULL = identity)
    int64_t n_list;
    int n_chunk;               // ceil(m^2 / 64)
    FolGrid grid;
    PrmTab<double> prm;        // default (all 0)
    double omega2, tau;
    int min_points;
    uint8_t* kind;             // n_list, as the real pass left it
    int32_t* counts;           // optional, [n_list][4]
    double* qmax;              // optional, [n_list][3]
};
// both instantiations, the shallow one first, on s
void launch_fol_reduce_cplx(const FolReduceCplxArgs& a, hipStream_t s);
#endif  // PD_HOST_SIM

// The double-double operand stack of one wave: a slot is an order-3 jet of dd per lane,
// 10 x 64 x 16 bytes; the shallow instantiation keeps its two slots in LDS (20,480 bytes), the
// deep one its seven in private memory (71,680 bytes of LDS are more than a block may have).
template <int MAXD> constexpr int red_dd_stack_words() { return (MAXD - 1) * nc(3) * 64; }
// The complex operand stack has the same shape: a slot is an order-3 jet of cplx per lane.
template <int MAXD> constexpr int red_cplx_stack_words() { return (MAXD - 1) * nc(3) * 64; }

}  // namespace pd

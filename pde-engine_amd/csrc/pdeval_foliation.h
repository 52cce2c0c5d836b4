// pdeval_foliation.h -- foliation classes of force-free candidates.
//
// A force-free solution is a foliation, the level sets of u: every f(u) is the same solution.
// Two candidates u and v describe the same foliation iff their gradients are parallel wherever
// both exist, i.e. iff the Jacobian J = u_rho v_z - u_z v_rho vanishes identically.  The test
// runs on gradient fields sampled on a small m x m grid: fol_match_kernel applies the scaled zero
// test of J to rows of fields against up to 32 probe fields, and fol_round groups rows into
// classes from the resulting masks.
//
// This header holds the per-point test and the leader round, which also compile for the host
// under -DPD_HOST_SIM (tests/hostsim/sim_foliation.cpp), the kernel's argument block and the
// launcher of pdeval_foliation.hip.
#pragma once
#include <vector>

#include "pdeval_kernels.h"

struct pdeval_ctx;

namespace pd {

// ---------------------------------------------------------------- per-point code (host + device)
// The point test of a row gradient (a, b) against a probe gradient (c, d): J = a d - b c against
// S = |a d| + |b c|, no division, as grid_fails.  The point is usable iff J and S are finite and
// S > 0 (a NaN gradient of either side, or a vanishing product pair, says nothing); it is bad
// iff |J| > tau S.  The two products are rounded separately (no FMA), so J is antisymmetric
// under the exchange of row and probe bit for bit and the host restatement computes the same
// doubles.
struct FolPoint {
    double J, S;
    bool used, bad;
};
PD_HD FolPoint fol_point_test(double a, double b, double c, double d, double tau) {
#pragma clang fp contract(off)
    const double ad = a * d, bc = b * c;
    FolPoint r;
    r.J = ad - bc;
    r.S = fabs(ad) + fabs(bc);
    r.used = finite_(r.J) && finite_(r.S) && r.S > 0.0;
    r.bad = r.used && fabs(r.J) > tau * r.S;
    return r;
}
// the diagnostic q = |J| / S of a usable point (IEEE division)
PD_HD double fol_q(const FolPoint& r) { return fabs(r.J) / r.S; }

// ---------------------------------------------------------------- the leader rule (host)
// One round of the grouping.  un: the nu still-unassigned rows in list order, the
// first np of them (np <= 32) this round's probes; mask[r]: bit k set iff row un[r] matches probe
// k.  Among the probes, one that matches an earlier leader of the round joins the first such
// leader, one that matches none becomes a leader; every other row joins the first leader of the
// round it matches -- a match with a probe that did not become a leader does not count -- or
// goes to `next`, the unassigned rows of the following round.  leader[row] receives the
// leader's candidate index (list[leader row], or the row itself without a list).  Returns the
// number of leaders created.  Leaders are created in list order and every row meets them in
// that order, so the rounds give the sequential definition: row i joins the first-created
// leader it matches and otherwise becomes a leader.
inline int fol_round(const uint32_t* mask, const int64_t* un, int64_t nu, int np, const int64_t* list,
                     int64_t* leader, std::vector<int64_t>& next) {
    uint32_t leaders = 0u;   // the probes that became leaders (bits below the current probe)
    int created = 0;
    next.clear();
    for (int64_t r = 0; r < nu; ++r) {
        const uint32_t hit = mask[r] & leaders;
        int64_t lead;
        if (hit) {
            lead = un[__builtin_ctz(hit)];
        } else if (r < np) {
            leaders |= 1u << r;
            lead = un[r];
            ++created;
        } else {
            next.push_back(un[r]);
            continue;
        }
        leader[un[r]] = list ? list[lead] : lead;
    }
    return created;
}

#ifndef PD_HOST_SIM
// ---------------------------------------------------------------- kernel arguments, launcher
struct FolMatchArgs {
    const double* rows;        // row fields, [n_rows][2][mm]
    int64_t n_rows;
    const double* probes;      // probe fields, [n_probe][2][mm]
    int n_probe;               // <= PDEVAL_FOL_MAX_PROBES
    int mm;
    double tau;
    int min_points;
    uint32_t* mask;            // n_rows
    int32_t* n_used;           // optional, n_rows x n_probe
    double* qmax;              // optional, n_rows x n_probe
};
void launch_fol_match(const FolMatchArgs& a, hipStream_t s);

// what the entry point (pdeval_foliation.hip) needs of a context (pdeval.hip)
struct FolCtx {
    int problem, device;
    hipStream_t stream;
};
void fol_ctx(pdeval_ctx* c, FolCtx* out);
// records msg as the context's pdeval_last_error text (the thread's when c is NULL); returns rc
int fol_fail(pdeval_ctx* c, int rc, const char* msg);
#endif  // PD_HOST_SIM

}  // namespace pd

// pdeval_foliation.h -- foliation classes of force-free candidates.
//
// A force-free solution is a foliation, the level sets of u: every f(u) is the same solution.
// Two candidates u and v describe the same foliation iff their gradients are parallel wherever
// both exist, i.e. iff the Jacobian J = u_rho v_z - u_z v_rho vanishes identically.  The test
// runs on gradient fields sampled on a small m x m grid: fol_field_kernel computes them from the
// resident programs, fol_match_kernel applies the scaled zero test of J to rows of fields against
// up to 32 probe fields, and fol_round groups rows into classes from the resulting masks.  A
// registry (pdeval_fol_registry.hip) keeps the leaders' fields on the device across batches: one
// pair scan (fol_chunk_test, fol_store_at) finds each row's first match among them
// (fol_assign_kernel) or every match (fol_link_kernel).
//
// This header holds the per-point code of the kernels and the leader round, which also compile
// for the host under -DPD_HOST_SIM (tests/hostsim/sim_foliation.cpp, sim_foliation_field.cpp),
// the kernels' argument blocks and the launchers.
#pragma once
#include <utility>
#include <vector>

#include "pdeval_kernels.h"
#ifndef PD_HOST_SIM
#include "pdeval_devbuf.h"   // DevBuf<T>, the owning device buffer of the entry points
#endif

struct pdeval_ctx;

namespace pd {

// ---------------------------------------------------------------- per-point code (host + device)
// The point test of a row gradient (a, b) against a probe gradient (c, d): J = a d - b c against
// S = |a d| + |b c|, no division, as grid_fails.  The point is usable iff J and S are finite and
// S > 0 (a NaN gradient of either side, or a vanishing product pair, says nothing); it is bad
// iff |J| > tau S.  The two products are rounded separately (no FMA), so J is antisymmetric
// under the exchange of row and probe bit for bit and the host restatement computes the same
// doubles.
// AXIS (PDEVAL_FOL_AXIS): a point the test above leaves unusable is usable, and never bad, when
// all four operands are finite and both gradients lie along the same coordinate axis -- b == 0,
// d == 0, a != 0, c != 0 (functions of rho alone: the cylinders rho = const) or the mirror image
// (functions of z alone).  The test is on the operands, not on the products: there both products
// are exact zeros, J = S = 0, and a product that merely underflowed does not count.  A zero
// gradient of either side still says nothing.  Symmetric under the exchange of row and probe.
// AXIS = false is the test as it was; callers that name no AXIS get it.
struct FolPoint {
    double J, S;
    bool used, bad;
};
template <bool AXIS = false>
PD_HD FolPoint fol_point_test(double a, double b, double c, double d, double tau) {
#pragma clang fp contract(off)
    const double ad = a * d, bc = b * c;
    FolPoint r;
    r.J = ad - bc;
    r.S = fabs(ad) + fabs(bc);
    r.used = finite_(r.J) && finite_(r.S) && r.S > 0.0;
    r.bad = r.used && fabs(r.J) > tau * r.S;
    if constexpr (AXIS) {
        const bool fin = finite_(a) && finite_(b) && finite_(c) && finite_(d);
        const bool along_rho = b == 0.0 && d == 0.0 && a != 0.0 && c != 0.0;
        const bool along_z = a == 0.0 && c == 0.0 && b != 0.0 && d != 0.0;
        r.used = r.used || (fin && (along_rho || along_z));
    }
    return r;
}
// the diagnostic q = |J| / S of a usable point (IEEE division); AXIS: 0 at a point usable by the
// axis rule (S == 0), never 0 / 0
template <bool AXIS = false>
PD_HD double fol_q(const FolPoint& r) {
    if constexpr (AXIS) return r.S > 0.0 ? fabs(r.J) / r.S : 0.0;
    else return fabs(r.J) / r.S;
}

// ---------------------------------------------------------------- the gradient field (host + device)
// The field of a program: (u_rho, u_z) of its order-1 jet at the m x m sample points of the
// context's grid, point p = i m + j at (xs[i], ys[j]), xs[i] = x_lo + (i + x_phase) dx,
// dx = (x_hi - x_lo) / m (rounded on the host), and likewise for y.
struct FolGrid {
    double x_lo, dx, x_ph, y_lo, dy, y_ph;
    int m;
};
PD_HD FolGrid fol_grid(const double* g, int m) {   // g: the context's 8 grid doubles
    return {g[0], (g[1] - g[0]) / m, g[6], g[3], (g[4] - g[3]) / m, g[7], m};
}
// the coordinates of point p < m^2: product and sum rounded separately, as the restatement does
PD_HD void fol_point_xy(const FolGrid& g, int p, double& x, double& y) {
#pragma clang fp contract(off)
    const int i = p / g.m, j = p - i * g.m;
    const double tx = ((double)i + g.x_ph) * g.dx, ty = ((double)j + g.y_ph) * g.dy;
    x = g.x_lo + tx;
    y = g.y_lo + ty;
}

// Every stack depth up to PDEVAL_MAX_STACK in one instantiation: with the
// operand stack in LDS the depth costs no registers, only (MAXD - 1) x 3 x 64 doubles per wave.
constexpr int kFolMaxD = PDEVAL_MAX_STACK;
constexpr int kFolStackDoubles = (kFolMaxD - 1) * nc(1) * 64;   // per wave
using FolInterp = Interp<double, 1, kFolMaxD>;

// The program of list row `row`, wave-uniform.  ok = false -- the whole row is NaN and no
// program word is read -- when the list entry lies outside [0, n) or the candidate's
// [offsets[c], offsets[c + 1]) does not lie inside [0, n_words]; otherwise the header word is
// read, and ok = false for a complex program, a non-header first word or a stack deeper than
// kFolMaxD.
struct FolProg {
    const int32_t* words;
    int len;
    bool ok;
};
__device__ __forceinline__ FolProg fol_program(const int32_t* ops, int64_t n_words, const int64_t* offsets,
                                               int64_t n, const int64_t* list, int64_t row) {
    FolProg r{ops, 0, false};
    const int64_t cand = list ? list[row] : row;
    if (cand < 0 || cand >= n) return r;
    const int64_t beg = offsets[cand], end = offsets[cand + 1];
    if (!(beg >= 0 && end > beg && end <= n_words && end - beg < (1 << 24))) return r;
    r.words = ops + beg;
    r.len = (int)(end - beg);
    const uint32_t hdr = rd_word(r.words);
    r.ok = (hdr & 0xffu) == 0u && !(hdr & PDEVAL_FLAG_COMPLEX) && (int)((hdr >> 8) & 0xffu) <= kFolMaxD;
    return r;
}

// One sample point of an ok program: rc = the interpreter's result (wave-uniform; anything but
// RUN_OK makes the whole row NaN), (a, b) = (u_rho, u_z), both NaN unless u, u_rho and u_z are all
// finite; fin = u_rho is finite (what n_finite counts).  P: the problem's constants, a default
// table (force-free programs carry none).  The kernel takes it from its arguments, in scalar
// registers: a table local to the kernel, indexed by a program word, cost 64 bytes of scratch.
struct FolField {
    double a, b;
    bool fin;
    int rc;
};
__device__ __forceinline__ FolField fol_field_point(const FolProg& pr, const FolGrid& g, int p, double* stk, int lane,
                                                    const PrmTab<double>& P) {
    double x, y;
    fol_point_xy(g, p, x, y);
    FolInterp::J u;
    FolField f;
    f.rc = FolInterp::run(pr.words, 1, pr.len, x, y, u, stk, lane, P);
    const bool ok = f.rc == RUN_OK && finite_(u.c[0]) && finite_(u.c[ji(1, 0)]) && finite_(u.c[ji(0, 1)]);
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    f.a = ok ? u.c[ji(1, 0)] : nan;
    f.b = ok ? u.c[ji(0, 1)] : nan;
    f.fin = ok;
    return f;
}

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

// ---------------------------------------------------------------- the registry's pair scan (host + device)
// The leader store of a registry is chunk-major: chunk c (64 sample points) of leader l is the
// 128 doubles at fol_store_at(cap, c, l) -- u_rho of points 64 c .. 64 c + 63, then u_z -- so the
// first chunk of consecutive leaders, which decides almost every non-matching pair, is one
// contiguous run, and the later chunks are touched only by the pairs that survive it.  Points
// past m^2 in the last chunk hold NaN.
constexpr int kFolChunk = 64;
constexpr int kFolAssignTile = 32;   // leaders per LDS tile of fol_assign_kernel (T)
constexpr int kFolRegChunks = 4;     // chunks of a row held in registers: m <= 16
constexpr int kFolEdgeMin = 64;      // pairs the link pass's edge buffer holds at least (it grows by doubling)
PD_HD int64_t fol_store_at(int64_t cap, int chunk, int64_t leader) {
    return ((int64_t)chunk * cap + leader) * (2 * kFolChunk);
}
// One chunk of a (row, leader) pair: this lane's point added to the pair's wave-uniform counts
// by fol_point_test and a ballot each (one lane under PD_HOST_SIM).  A pair is left at the first
// chunk with nb != 0; it matches iff nu >= min_points and nb == 0 after its last chunk.
struct FolCount {
    int nu, nb;
};
template <bool AXIS = false>
__device__ __forceinline__ void fol_chunk_test(double a, double b, double c, double d, bool active, double tau,
                                               FolCount& n) {
    const FolPoint t = fol_point_test<AXIS>(a, b, c, d, tau);
    n.nu += count_lanes(active && t.used);
    n.nb += count_lanes(active && t.bad);
}

// ---------------------------------------------------------------- the kind of a field (host + device)
// Whether a field is that of a function of one coordinate (fol_kind_kernel): over its finite
// points -- u_rho and u_z both finite -- kind 1 (rho-axis) iff u_z == 0 at every one and u_rho != 0
// at >= min_points of them, kind 2 (z-axis) the mirror image, 0 otherwise.  The two exclude
// each other.  This lane's point is added to the row's wave-uniform counts by a ballot each (one
// lane under PD_HOST_SIM).
struct FolKindCount {
    int a_nz, b_nz;   // finite points with u_rho != 0, with u_z != 0
    int a_ax, b_ax;   // finite points with u_z == 0 and u_rho != 0, with u_rho == 0 and u_z != 0
};
__device__ __forceinline__ void fol_kind_chunk(double a, double b, bool active, FolKindCount& n) {
    const bool fin = active && finite_(a) && finite_(b);
    const bool anz = fin && a != 0.0, bnz = fin && b != 0.0;
    n.a_nz += count_lanes(anz);
    n.b_nz += count_lanes(bnz);
    n.a_ax += count_lanes(anz && !bnz);
    n.b_ax += count_lanes(bnz && !anz);
}
PD_HD int fol_kind_of(const FolKindCount& n, int min_points) {
    if (n.b_nz == 0 && n.a_ax >= min_points) return 1;
    if (n.a_nz == 0 && n.b_ax >= min_points) return 2;
    return 0;
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
    // optional (pdeval_foliation_classes: the unassigned subset of a round, its first rows the
    // probes): row r's field is rows[idx[r]], probe k's is probes[pidx[k]]; NULL = r, k
    const int64_t* idx;
    const int64_t* pidx;
    uint32_t flags;            // PDEVAL_FOL_AXIS selects the kernel's AXIS instantiation
};
void launch_fol_match(const FolMatchArgs& a, hipStream_t s);

struct FolFieldArgs {
    const int32_t* ops;
    int64_t n_words;
    const int64_t* offsets;
    int64_t n;
    const int64_t* list;       // optional: row -> candidate index (NULL = identity)
    int64_t n_list;
    int n_chunk;               // ceil(m^2 / 64)
    FolGrid grid;
    PrmTab<double> prm;        // default (all 0): force-free programs carry no problem constants
    double* field;             // [n_list][2][m^2]
    int32_t* n_finite;         // optional, n_list, zeroed by the caller
};
void launch_fol_field(const FolFieldArgs& a, hipStream_t s);

// The pair scan of a registry (pdeval_fol_registry.hip, fol_scan): rows of fields against the
// resident leaders.  What both of its modes take.
struct FolScanArgs {
    const double* rows;        // row fields, [n_rows][2][mm]
    int64_t n_rows;
    const double* store;       // the leader store, chunk-major (fol_store_at)
    int64_t cap, L;            // its capacity and the leaders it holds
    int mm, n_chunk;
    double tau;
    int min_points;
    uint32_t flags;            // PDEVAL_FOL_AXIS selects the kernels' AXIS instantiations
};
// Stage A: first[row] = the smallest leader index the row matches, -1 if none (or
// n_finite[row] < min_points, when given)
struct FolAssignArgs : FolScanArgs {
    const int32_t* n_finite;   // optional, n_rows
    int64_t* first;            // n_rows
};
void launch_fol_assign(const FolAssignArgs& a, hipStream_t s);
// The link pass (DESIGN.md §14 "Links and components"): for every leader l < lim[row],
// l != cls[row], that the row matches, the pair (cls[row], l) is appended to edges.  A row with
// cls[row] < 0 yields none.
struct FolLinkArgs : FolScanArgs {
    const int32_t* cls;        // n_rows, each -1 or in [0, L) (checked by the host before the launch)
    const int32_t* lim;        // n_rows, each in [0, L] (likewise)
    int32_t* edges;            // [ecap][2]
    int64_t ecap;
    unsigned long long* count; // edges found, zeroed by the caller; those past ecap are counted, not stored
};
void launch_fol_link(const FolLinkArgs& a, hipStream_t s);

// rows of [.][2][mm] fields into the store (append, load) or the store's leaders out to
// [L][2][mm] (leaders): one wave per (leader, chunk)
struct FolMoveArgs {
    double* store;
    int64_t cap, base;         // leader k of the call is store leader base + k
    int64_t n_lead;
    double* fields;            // [n_rows][2][mm]
    int64_t n_rows;
    const int64_t* idx;        // optional: leader k's field is fields[idx[k]] (checked against n_rows)
    int mm, n_chunk;
    int to_store;              // 1: fields -> store, 0: store -> fields
};
void launch_fol_move(const FolMoveArgs& a, hipStream_t s);
// n_finite[row] = the points of the row with a finite u_rho (fields the caller holds)
void launch_fol_nfinite(const double* fields, int64_t n_rows, int mm, int32_t* n_finite, hipStream_t s);

// kind[row] of fol_kind_of: rows of [n_rows][2][mm] fields (cap == 0), or the leaders 0 .. n_rows-1
// of a chunk-major store of capacity cap (fol_store_at).  One wave per row.
struct FolKindArgs {
    const double* fields;
    int64_t n_rows;
    int64_t cap;
    int mm, n_chunk;
    int min_points;
    uint8_t* kind;             // n_rows
};
void launch_fol_kind(const FolKindArgs& a, hipStream_t s);

// ---------------------------------------------------------------- host side
// what the entry points (pdeval_foliation.hip, pdeval_fol_registry.hip) need of a context (pdeval.hip)
struct FolCtx {
    int problem, device;
    hipStream_t stream;
    double grid[8];   // {x_lo, x_hi, nx, y_lo, y_hi, ny, x_phase, y_phase} (pdeval_create)
};
void fol_ctx(pdeval_ctx* c, FolCtx* out);
// records msg as the context's pdeval_last_error text (the thread's when c is NULL); returns rc
int fol_fail(pdeval_ctx* c, int rc, const char* msg);

// shared by the entry points of pdeval_foliation.hip and pdeval_fol_registry.hip
// the checks of the program entry points; fills prm and the context view
int fol_check(pdeval_ctx* c, const char* fn, const int32_t* d_ops, int64_t n_words, const int64_t* d_offsets,
              int64_t n, int64_t n_list, const pdeval_fol_params* params, FolCtx* v, pdeval_fol_params* prm);
int fol_hip_fail(pdeval_ctx* c, const char* what, hipError_t e);
// zeroes d_n_finite (if given) and launches the field kernel on s
int fol_fields_launch(pdeval_ctx* c, const FolCtx& v, const pdeval_fol_params& prm, const int32_t* d_ops,
                      int64_t n_words, const int64_t* d_offsets, int64_t n, const int64_t* d_list, int64_t n_list,
                      double* d_field, int32_t* d_n_finite, hipStream_t s);
// The rounds: groups the rows `un` (indices into d_field's rows, in list order; emptied) with
// fol_match_kernel and fol_round, d_idx / d_mask holding un.size() entries each.  leader[row]
// receives list[leader row] (the row itself without a list).  Synchronizes s once per round.
int fol_rounds(pdeval_ctx* c, const double* d_field, int mm, const pdeval_fol_params& prm, std::vector<int64_t>& un,
               const int64_t* list, int64_t* leader, int64_t* d_idx, uint32_t* d_mask, hipStream_t s,
               int64_t* classes, int32_t* rounds);
#endif  // PD_HOST_SIM

}  // namespace pd

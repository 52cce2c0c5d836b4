// pdeval_fol_reduce_multi.hip -- the reduction kinds of each listed program at several Omega^2 in
// one pass (DESIGN.md §14 "Reduction kinds at several rotation rates"): the entry point
// pdeval_fol_reduce_multi, fol_reduce_multi_kernel and fol_reduce_multi_cplx_kernel.  Its own
// unit and its own argument block: pdeval_fol_reduce, its kernels and their argument layouts do
// not depend on anything here.
//
// The order-3 jet of u does not depend on Omega; only the epilogue red_point does, through
// w = Omega^2.  So a (row, point) is interpreted once and the rule is applied at each of the
// n_omega <= PDEVAL_RED_MAX_OMEGA values from the ten coefficients the lane already holds.  Slice
// k of every output is, bit for bit, what pdeval_fol_reduce writes at omega2[k]: red_point and
// red_point_cplx are called unchanged (contraction off inside them), the counts are sums of the
// same ballots and the maxima fold the same doubles (max does not depend on the order).
// The first Omega is peeled out of the Omega loop (step(0), then the loop from 1) on purpose: the
// interpreter is inlined into each kernel with FMA contraction on, and which product of a sum of
// two products (the jet square, the complex product) becomes the fma follows the operand order the
// optimiser gives that sum, which follows the code around the interpreter.  With the loop alone
// the jet square paired the other way than in fol_reduce_kernel and functions of a full 2-D jet
// squared differed in the last bits; with the peeled step the code after Interp::run is that of
// fol_reduce_kernel and the pairings are the same (the test compares bytes).
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/pdeval.h"
#include "pdeval_point.h"
#include "pdeval_fol_reduce.h"

namespace pd {

// One block for both kernels; the Omega^2 values travel in it (scalar loads from the kernel
// arguments, indexed by the wave-uniform k).
struct FolReduceMultiArgs {
    const int32_t* ops;
    int64_t n_words;
    const int64_t* offsets;
    int64_t n;
    const int64_t* list;       // optional: row -> candidate index (NULL = identity)
    int64_t n_list;
    int n_chunk;               // ceil(m^2 / 64)
    int n_omega;               // 1 .. PDEVAL_RED_MAX_OMEGA
    FolGrid grid;
    PrmTab<double> prm;        // default (all 0)
    double omega2[PDEVAL_RED_MAX_OMEGA];
    double tau;
    int min_points;
    uint8_t* kind;             // [n_omega][n_list]
    int32_t* counts;           // optional, [n_omega][n_list][4]
    double* qmax;              // optional, [n_omega][n_list][3]
    double* table;             // optional, [n_omega][n_list][3][m^2]: u, kappa, G (real pass only)
};

// The per-Omega state of a row.
//   counts  four per Omega, each a sum of wave-uniform ballot counts.  All 4 n_omega <= 32 of
//           them live in ONE vector register: lane 4 k + i holds counter i of Omega k.  A chunk
//           adds its four counts with two selects and a masked add; the end reads them back with
//           readlane.  No array indexed by k, hence no scratch and no unrolling of the Omega loop.
//   qmax    three running maxima per Omega and lane.  24 doubles per lane would take 48 VGPRs and
//           the shallow body's occupancy, so they sit in LDS behind the operand stack as
//           [k][3][lane]: a lane touches only its own words (no barrier), 64 consecutive doubles
//           are conflict-free.  The block is dynamic LDS of n_omega x 1,536 bytes, so a call pays
//           occupancy only for the slices it asked for.  The maxima are folded whether or not
//           d_qmax is given: the pointer is then read at the end only, not in the chunk loop.
__device__ __forceinline__ int red_multi_count(int cnt, int lane, int k, int n_fin, const int* bad) {
    const int sel = (lane & 2) ? ((lane & 1) ? bad[2] : bad[1]) : ((lane & 1) ? bad[0] : n_fin);
    return cnt + ((lane >> 2) == k ? sel : 0);
}
__device__ __forceinline__ RedCount red_multi_counts(int cnt, int k) {
    return {__builtin_amdgcn_readlane(cnt, 4 * k),
            {__builtin_amdgcn_readlane(cnt, 4 * k + 1), __builtin_amdgcn_readlane(cnt, 4 * k + 2),
             __builtin_amdgcn_readlane(cnt, 4 * k + 3)}};
}
// lane 0 stores slice k of a row: the kind, the counts and the maxima (folded over the wave here)
__device__ __forceinline__ void red_multi_store(const FolReduceMultiArgs& a, int64_t row, int lane, int k, int kind,
                                                const RedCount& n, const double* acc) {
    double q[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) q[j] = wave_max(acc[(k * 3 + j) * 64 + lane]);
    if (lane == 0) {
        const int64_t o = (int64_t)k * a.n_list + row;
        a.kind[o] = (uint8_t)kind;
        if (a.counts) {
            a.counts[o * 4] = n.n_fin;
#pragma unroll
            for (int j = 0; j < 3; ++j) a.counts[o * 4 + 1 + j] = n.bad[j];
        }
        if (a.qmax) {
#pragma unroll
            for (int j = 0; j < 3; ++j) a.qmax[o * 3 + j] = q[j];
        }
    }
}

// The work split of fol_reduce_kernel: one wave per list row, one wave per block; lanes are sample
// points and the wave loops over the row's ceil(m^2 / 64) chunks; the program is read
// wave-uniformly and run in order-3 jets on the operand stack in LDS as [slot][coef][lane]; the
// same two instantiations, each launch covering the whole list, a wave leaving before it reads any
// program word but the header unless the row is its own, and the shallow launch writing the rows
// that no instantiation runs (kind 0, zero counts, a NaN table) -- here in every slice.
// After Interp::run the lane holds the ten coefficients; the Omega loop applies red_point to them
// and folds the per-Omega state above.  Lanes past m^2 evaluate the last point again; they store
// nothing and count nothing.
template <int MAXD>
__global__ __launch_bounds__(64) void fol_reduce_multi_kernel(FolReduceMultiArgs a) {
    using I = Interp<double, 3, MAXD>;
    __shared__ double red_lds[red_stack_doubles<MAXD>()];
    extern __shared__ double red_acc[];      // [n_omega][3][lane]
    constexpr bool kShallow = MAXD == kRedShallowD;
    const int lane = threadIdx.x;
    const int64_t row = blockIdx.x;
    if (row >= a.n_list) return;
    const FolProg pr = fol_program(a.ops, a.n_words, a.offsets, a.n, a.list, row);
    // (pr.ok: the header word was read and names a stack <= kFolMaxD)
    const int depth = pr.ok ? (int)((rd_word(pr.words) >> 8) & 0xffu) : 0;
    if (pr.ok && (depth <= kRedShallowD) != kShallow) return;
    if (!pr.ok && !kShallow) return;
    const int mm = a.grid.m * a.grid.m;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    int cnt = 0;
    for (int i = 0; i < 3 * a.n_omega; ++i) red_acc[i * 64 + lane] = 0.0;
    bool run_ok = pr.ok;
    for (int c = 0; c < a.n_chunk; ++c) {
        const int p = c * kFolChunk + lane;
        const bool active = p < mm;
        double x = 0.0, y = 0.0;
        typename I::J u;
        if (run_ok) {
            fol_point_xy(a.grid, active ? p : mm - 1, x, y);
            run_ok = I::run(pr.words, 1, pr.len, x, y, u, red_lds, lane, a.prm) == RUN_OK;
        }
        const auto step = [&](int k) {
            double tu = nan, tk = nan, tg = nan;
            if (run_ok) {
                const RedPoint r = red_point(u.c, x, a.omega2[k], a.tau);
                const bool fin = active && r.fin;
                int bad[3];
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    bad[j] = count_lanes(active && r.bad[j]);
                    if (fin) {
                        double* q = red_acc + (k * 3 + j) * 64 + lane;
                        *q = fmax(*q, red_q(r, j));
                    }
                }
                cnt = red_multi_count(cnt, lane, k, count_lanes(fin), bad);
                if (a.table) {
                    red_coefs(r, tk, tg);
                    tu = r.fin ? u.c[0] : nan;
                }
            }
            if (a.table && active) {
                double* tab = a.table + ((int64_t)k * a.n_list + row) * 3 * (int64_t)mm;
                tab[p] = tu;
                tab[mm + p] = tk;
                tab[2 * mm + p] = tg;
            }
        };
        step(0);
        for (int k = 1; k < a.n_omega; ++k) step(k);
    }
    // a run that does not return RUN_OK (wave-uniform: it depends on the program alone) fails at
    // the first chunk: nothing was counted
    for (int k = 0; k < a.n_omega; ++k) {
        const RedCount n = red_multi_counts(cnt, k);
        red_multi_store(a, row, lane, k, run_ok ? red_kind_of(n, a.min_points) : PDEVAL_RED_NONE, n, red_acc);
    }
}

// The complex pass at several Omega^2 (PDEVAL_FOL_CPLX), after the real launches on the same
// stream: fol_reduce_cplx_kernel's selection, arithmetic and two stack bodies (shallow: two LDS
// slots of cplx; deep: PrivVStack under ValInterp), with the Omega loop around red_point_cplx and
// the per-Omega state of the real kernel.
// Selection: a slice is rewritten iff the real pass wrote PDEVAL_RED_NONE into it and
// fol_program_cplx accepts the row.  The NONE conditions of the real pass -- a declined program,
// too few finite jets -- do not depend on Omega, so a row is NONE in every slice or in none; only
// the finiteness of the forms themselves enters n_finite with w, at an Omega^2 large enough to
// overflow them.  The wave therefore reads the row's kind in every slice (n_omega bytes) and
// keeps the set of NONE slices as a mask, which costs nothing when the slices agree and follows
// pdeval_fol_reduce slice by slice when they do not.  A run the interpreter declines leaves
// before any store.  The table is never written: its rows stay NaN in every slice.
template <int MAXD>
__global__ __launch_bounds__(64) void fol_reduce_multi_cplx_kernel(FolReduceMultiArgs a) {
    constexpr bool kShallow = MAXD == kRedShallowD;
    using I = Interp<cplx, 3, MAXD>;
    using VI = ValInterp<cplx, 3, MAXD, double>;
    using STK = PrivVStack<cplx, nc(3), MAXD - 1>;
    extern __shared__ double red_acc[];      // [n_omega][3][lane]
    const int lane = threadIdx.x;
    const int64_t row = blockIdx.x;
    if (row >= a.n_list) return;
    unsigned take = 0u;
    for (int k = 0; k < a.n_omega; ++k) {
        if (__builtin_amdgcn_readfirstlane((int)a.kind[(int64_t)k * a.n_list + row]) == PDEVAL_RED_NONE) take |= 1u << k;
    }
    if (!take) return;
    const FolCplxProg pr = fol_program_cplx(a.ops, a.n_words, a.offsets, a.n, a.list, row);
    if (!pr.ok) return;
    if (((int)((rd_word(pr.words) >> 8) & 0xffu) <= kRedShallowD) != kShallow) return;
    const int mm = a.grid.m * a.grid.m;
    int cnt = 0;
    for (int i = 0; i < 3 * a.n_omega; ++i) red_acc[i * 64 + lane] = 0.0;
    for (int c = 0; c < a.n_chunk; ++c) {
        const int p = c * kFolChunk + lane;
        const bool active = p < mm;
        double x, y;
        fol_point_xy(a.grid, active ? p : mm - 1, x, y);
        typename I::J u;
        int rc;
        if constexpr (kShallow) {
            __shared__ __align__(16) cplx red_clds[red_cplx_stack_words<MAXD>()];
            rc = I::run(pr.words, 1, pr.len, x, y, u, red_clds, lane, a.prm);
        } else {
            STK stk;
            rc = VI::template run<STK, false>(pr.words, 1, pr.len, x, y, u, stk, a.prm);
        }
        if (rc != RUN_OK) return;
        const auto step = [&](int k) {
            if (!((take >> k) & 1u)) return;
            const RedPointCplx r = red_point_cplx(u.c, x, a.omega2[k], a.tau);
            const bool fin = active && r.fin;
            int bad[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                bad[j] = count_lanes(active && r.bad[j]);
                if (fin) {
                    double* q = red_acc + (k * 3 + j) * 64 + lane;
                    *q = fmax(*q, red_q(r, j));
                }
            }
            cnt = red_multi_count(cnt, lane, k, count_lanes(fin), bad);
        };
        step(0);
        for (int k = 1; k < a.n_omega; ++k) step(k);
    }
    for (int k = 0; k < a.n_omega; ++k) {
        if (!((take >> k) & 1u)) continue;
        const RedCount n = red_multi_counts(cnt, k);
        red_multi_store(a, row, lane, k, red_kind_of(n, a.min_points), n, red_acc);
    }
}

}  // namespace pd

using namespace pd;

extern "C" int pdeval_fol_reduce_multi(pdeval_ctx* c, const int32_t* d_ops, int64_t n_words, const int64_t* d_offsets,
                                       int64_t n, const int64_t* d_list, int64_t n_list,
                                       const pdeval_fol_params* params, const double* omega2s, int n_omega,
                                       uint8_t* d_kind, int32_t* d_counts, double* d_qmax, double* d_table,
                                       void* stream) {
    FolCtx v;
    pdeval_fol_params prm;
    const int rc = fol_check(c, "pdeval_fol_reduce_multi", d_ops, n_words, d_offsets, n, n_list, params, &v, &prm);
    if (rc != PDEVAL_OK) return rc;
    if (!omega2s || n_omega < 1 || n_omega > PDEVAL_RED_MAX_OMEGA)
        return fol_fail(c, PDEVAL_ERR_ARG, "pdeval_fol_reduce_multi: omega2s must hold 1 .. PDEVAL_RED_MAX_OMEGA values");
    for (int k = 0; k < n_omega; ++k) {
        if (!(omega2s[k] >= 0.0) || !std::isfinite(omega2s[k]))
            return fol_fail(c, PDEVAL_ERR_ARG, "pdeval_fol_reduce_multi: every omega2 must be finite and >= 0");
    }
    if (n_list > 0 && !d_kind) return fol_fail(c, PDEVAL_ERR_ARG, "pdeval_fol_reduce_multi: bad argument");
    if (n_list == 0) return PDEVAL_OK;
    hipError_t e = hipSetDevice(v.device);
    if (e != hipSuccess) return fol_hip_fail(c, "hipSetDevice", e);
    // (n_list <= PDEVAL_MAX_BATCH, fol_check: n_list one-wave blocks are one launch)
    FolReduceMultiArgs a{};
    a.ops = d_ops;
    a.n_words = n_words;
    a.offsets = d_offsets;
    a.n = n;
    a.list = d_list;
    a.n_list = n_list;
    a.n_chunk = (prm.m * prm.m + kFolChunk - 1) / kFolChunk;
    a.n_omega = n_omega;
    a.grid = fol_grid(v.grid, prm.m);
    for (int k = 0; k < n_omega; ++k) a.omega2[k] = omega2s[k];
    a.tau = prm.tau;
    a.min_points = prm.min_points;
    a.kind = d_kind;
    a.counts = d_counts;
    a.qmax = d_qmax;
    a.table = d_table;
    const hipStream_t s = stream ? (hipStream_t)stream : v.stream;
    const dim3 grid((unsigned)n_list), block(64);
    const size_t acc = (size_t)n_omega * 3 * 64 * sizeof(double);   // the maxima, behind the stack
    hipLaunchKernelGGL(fol_reduce_multi_kernel<kRedShallowD>, grid, block, acc, s, a);
    hipLaunchKernelGGL(fol_reduce_multi_kernel<kFolMaxD>, grid, block, acc, s, a);
    if ((e = hipGetLastError()) != hipSuccess) return fol_hip_fail(c, "fol_reduce_multi_kernel", e);
    if (prm.flags & PDEVAL_FOL_CPLX) {
        hipLaunchKernelGGL(fol_reduce_multi_cplx_kernel<kRedShallowD>, grid, block, acc, s, a);
        hipLaunchKernelGGL(fol_reduce_multi_cplx_kernel<kFolMaxD>, grid, block, acc, s, a);
        if ((e = hipGetLastError()) != hipSuccess) return fol_hip_fail(c, "fol_reduce_multi_cplx_kernel", e);
    }
    return PDEVAL_OK;
}

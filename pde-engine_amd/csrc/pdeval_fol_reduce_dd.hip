// pdeval_fol_reduce_dd.hip -- the settle tier of the reduction kinds (DESIGN.md §14 "Settled in
// double-double"): fol_reduce_dd_kernel and the entry point pdeval_fol_reduce_dd.  Its own unit:
// fol_reduce_kernel's code does not depend on anything here.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/pdeval.h"
#include "pdeval_point.h"
#include "pdeval_fol_reduce.h"

namespace pd {

// counts and qmax are the accumulators of the rows' waves: cleared by a kernel, not a memset
// (DESIGN.md §3 "Robustness": a memset node does not belong in a captured graph)
__global__ __launch_bounds__(256) void fol_reduce_dd_clear_kernel(FolReduceArgs a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < a.n_list * 4) a.counts[i] = 0;
    if (i < a.n_list * 3) a.qmax[i] = 0.0;
}

// The list is short -- the few rows the fp64 rule leaves in the band -- so the parallelism comes
// from the sample points: one one-wave block per (row, chunk of 64 points), blockIdx.x the row,
// blockIdx.y the chunk, lanes are points.  The program is wave-uniform and is read through the
// constant address space (ValInterp's VEC = false: scalar loads), run once in order-3 jets of
// double-doubles at the lane's point, which enters as an exact dd; the rule is red_point_dd.
// The wave adds its four counts (a ballot each) to the row's with atomicAdd and folds its three
// maxima of |X| / S_X into the row's with an integer atomicMax on the bit pattern (non-negative
// doubles order as their bits).  Sums and maxima do not depend on the order of arrival, stream
// order puts the clearing kernel before and the finishing kernel after: no tickets, no fences.
// The operand stack below the accumulator, as the fp64 kernel in two instantiations:
//   MAXD = kRedShallowD  two slots in LDS as 16-byte words, [slot][coef][lane] of dd (LdsVStack):
//                        a lane's hi and lo travel together in one ds_read_b128 / ds_write_b128,
//                        half the LDS instructions of split hi / lo planes, and 64 consecutive
//                        16-byte words are conflict-free; each lane touches only its own words,
//                        no barrier; 20,480 bytes per block;
//   MAXD = kFolMaxD      seven slots would be 71,680 bytes, more than a block may have: private
//                        memory (PrivVStack), as dd_point_kernel's deep instantiation.
// Each launch covers the whole list and a wave leaves after the header word unless the row is
// its own.  A row whose program fails fol_program's checks, is complex-valued or does not run
// (wave-uniform: it depends on the program alone) adds nothing: zero counts, kind 0.
// Lanes past m^2 evaluate the last point again and count nothing.
template <int MAXD>
__global__ __launch_bounds__(64) void fol_reduce_dd_kernel(FolReduceArgs a) {
    constexpr bool kShallow = MAXD == kRedShallowD;
    using VI = ValInterp<dd, 3, MAXD, dd>;
    using STK = typename std::conditional<kShallow, LdsVStack<dd, nc(3)>, PrivVStack<dd, nc(3), MAXD - 1>>::type;
    const int lane = threadIdx.x;
    const int64_t row = blockIdx.x;
    const int mm = a.grid.m * a.grid.m;
    const int p = (int)blockIdx.y * kFolChunk + lane;
    if (row >= a.n_list || (int)blockIdx.y >= a.n_chunk) return;
    const FolProg pr = fol_program(a.ops, a.n_words, a.offsets, a.n, a.list, row);
    if (!pr.ok) return;
    if (((int)((rd_word(pr.words) >> 8) & 0xffu) <= kRedShallowD) != kShallow) return;
    STK stk;
    if constexpr (kShallow) {
        __shared__ __align__(16) dd red_dd_lds[red_dd_stack_words<MAXD>()];
        stk = STK{red_dd_lds, lane};
    }
    const bool active = p < mm;
    double x, y;
    fol_point_xy(a.grid, active ? p : mm - 1, x, y);
    const PrmTab<dd> prm{};   // (force-free programs carry no problem constants)
    typename VI::J u;
    if (VI::template run<STK, false>(pr.words, 1, pr.len, dd_from(x), dd_from(y), u, stk, prm) != RUN_OK) return;
    const RedPointDD r = red_point_dd(u.c, x, a.omega2, a.tau);
    const bool fin = active && r.fin;
    int n[4];
    double q[3];
    n[0] = count_lanes(fin);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        n[1 + k] = count_lanes(active && r.bad[k]);
        q[k] = wave_max(fin ? red_q(r, k) : 0.0);
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (n[k]) atomicAdd(a.counts + row * 4 + k, n[k]);
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (q[k] > 0.0)
                atomicMax(reinterpret_cast<unsigned long long*>(a.qmax + row * 3 + k),
                          (unsigned long long)__double_as_longlong(q[k]));
    }
}

// one lane per row: the kind from the row's finished counts
__global__ __launch_bounds__(64) void fol_reduce_dd_finish_kernel(FolReduceArgs a) {
    const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= a.n_list) return;
    const int32_t* c = a.counts + row * 4;
    // (a row that did not run has zero counts, and min_points >= 1: kind 0)
    a.kind[row] = (uint8_t)red_kind_of(RedCount{c[0], {c[1], c[2], c[3]}}, a.min_points);
}

void launch_fol_reduce_dd(const FolReduceArgs& a, hipStream_t s) {
    const dim3 grid((unsigned)a.n_list, (unsigned)a.n_chunk), block(64);
    hipLaunchKernelGGL(fol_reduce_dd_clear_kernel, dim3((unsigned)((a.n_list * 4 + 255) / 256)), dim3(256), 0, s, a);
    hipLaunchKernelGGL(fol_reduce_dd_kernel<kRedShallowD>, grid, block, 0, s, a);
    hipLaunchKernelGGL(fol_reduce_dd_kernel<kFolMaxD>, grid, block, 0, s, a);
    hipLaunchKernelGGL(fol_reduce_dd_finish_kernel, dim3((unsigned)((a.n_list + 63) / 64)), block, 0, s, a);
}

}  // namespace pd

using namespace pd;

extern "C" int pdeval_fol_reduce_dd(pdeval_ctx* c, const int32_t* d_ops, int64_t n_words, const int64_t* d_offsets,
                                    int64_t n, const int64_t* d_list, int64_t n_list, const pdeval_fol_params* params,
                                    double omega2, uint8_t* d_kind, int32_t* d_counts, double* d_qmax, void* stream) {
    FolCtx v;
    pdeval_fol_params prm;
    const int rc = fol_check(c, "pdeval_fol_reduce_dd", d_ops, n_words, d_offsets, n, n_list, params, &v, &prm);
    if (rc != PDEVAL_OK) return rc;
    if (!(omega2 >= 0.0) || !std::isfinite(omega2))
        return fol_fail(c, PDEVAL_ERR_ARG, "pdeval_fol_reduce_dd: omega2 must be finite and >= 0");
    if (n_list > 0 && (!d_kind || !d_counts || !d_qmax))
        return fol_fail(c, PDEVAL_ERR_ARG,
                        "pdeval_fol_reduce_dd: d_kind, d_counts and d_qmax are required (the rows' accumulators)");
    if (n_list == 0) return PDEVAL_OK;
    hipError_t e = hipSetDevice(v.device);
    if (e != hipSuccess) return fol_hip_fail(c, "hipSetDevice", e);
    FolReduceArgs a{};
    a.ops = d_ops;
    a.n_words = n_words;
    a.offsets = d_offsets;
    a.n = n;
    a.list = d_list;
    a.n_list = n_list;
    a.n_chunk = (prm.m * prm.m + kFolChunk - 1) / kFolChunk;   // (m <= 64, fol_check: at most 64 chunks)
    a.grid = fol_grid(v.grid, prm.m);
    a.omega2 = omega2;
    a.tau = prm.tau;
    a.min_points = prm.min_points;
    a.kind = d_kind;
    a.counts = d_counts;
    a.qmax = d_qmax;
    launch_fol_reduce_dd(a, stream ? (hipStream_t)stream : v.stream);
    if ((e = hipGetLastError()) != hipSuccess) return fol_hip_fail(c, "fol_reduce_dd_kernel", e);
    return PDEVAL_OK;
}

// pdeval_fol_reduce_cplx.hip -- the reduction kind of the complex-valued rows (PDEVAL_FOL_CPLX;
// DESIGN.md §14 "Reduction kinds of complex-valued rows"): fol_reduce_cplx_kernel and its
// launcher, called by pdeval_fol_reduce after the two fp64 launches.  Its own unit:
// fol_reduce_kernel's code does not depend on anything here.
#include <hip/hip_runtime.h>

#include "../../include/pdeval.h"
#include "pdeval_point.h"
#include "pdeval_fol_reduce.h"

namespace pd {

// One wave per list row, one wave per block, as fol_field_cplx_kernel and fol_reduce_kernel;
// lanes are sample points and the wave loops over the row's ceil(m^2 / 64) chunks, running the
// program again at each.  The four counts are wave-uniform counters fed by a ballot each and the
// three maxima of |X| / S_X are folded with wave_max at the end, so lane 0 stores everything:
// no atomics, no accumulators, no second pass.
// Selection, wave-uniform and before anything is written: the wave reads kind[row] once and
// leaves unless the real pass wrote PDEVAL_RED_NONE there and fol_program_cplx accepts the row
// (entry and offsets in range, a header first, stack <= kFolMaxD; no program word of a declined
// row is read).  That takes the programs with PDEVAL_FLAG_COMPLEX and the unflagged rows that
// are real at fewer than min_points points -- the rows the complex field pass takes -- and a row
// the real pass decided keeps every bit.
// A taken row is run in order-3 complex jets, JetOps<cplx, 3> under Interp<cplx, 3, MAXD> -- the
// arithmetic of the validator's complex passes, so the branches of sqrt, pow and log are those
// the verdict was reached with -- the program read wave-uniformly through the constant address
// space, and red_point_cplx gives the point's verdict.  The operand stack below the accumulator,
// in the two instantiations of the other reduce kernels (a wave whose row belongs to the other
// one leaves after the header word):
//   MAXD = kRedShallowD  two slots in LDS as 16-byte words, [slot][coef][lane] of cplx: a lane's
//                        real and imaginary words travel in one 128-bit LDS access, 64
//                        consecutive 16-byte words are conflict-free, each lane touches only its
//                        own words, no barrier; 2 x 10 x 64 x 16 = 20,480 bytes per block;
//   MAXD = kFolMaxD      seven slots would be 71,680 bytes, more than a block may have: private
//                        memory (PrivVStack), as the dd tier's deep body; ValInterp with V =
//                        double drives the same JetOps and Interp<cplx, 3, MAXD>::binop.
// A run that does not return RUN_OK (wave-uniform: it depends on the program alone) fails at the
// first chunk, before any store: the row stays as the real pass wrote it.  The table is never
// written: kappa and G of a complex u are complex.  Lanes past m^2 evaluate the last point
// again and count nothing.
template <int MAXD>
__global__ __launch_bounds__(64) void fol_reduce_cplx_kernel(FolReduceCplxArgs a) {
    constexpr bool kShallow = MAXD == kRedShallowD;
    using I = Interp<cplx, 3, MAXD>;
    using VI = ValInterp<cplx, 3, MAXD, double>;
    using STK = PrivVStack<cplx, nc(3), MAXD - 1>;
    const int lane = threadIdx.x;
    const int64_t row = blockIdx.x;
    if (row >= a.n_list) return;
    if (__builtin_amdgcn_readfirstlane((int)a.kind[row]) != PDEVAL_RED_NONE) return;
    const FolCplxProg pr = fol_program_cplx(a.ops, a.n_words, a.offsets, a.n, a.list, row);
    if (!pr.ok) return;
    if (((int)((rd_word(pr.words) >> 8) & 0xffu) <= kRedShallowD) != kShallow) return;
    const int mm = a.grid.m * a.grid.m;
    RedCount n{0, {0, 0, 0}};
    double q[3] = {0.0, 0.0, 0.0};
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
        const RedPointCplx r = red_point_cplx(u.c, x, a.omega2, a.tau);
        const bool fin = active && r.fin;
        n.n_fin += count_lanes(fin);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            n.bad[k] += count_lanes(active && r.bad[k]);
            if (a.qmax && fin) q[k] = fmax(q[k], red_q(r, k));
        }
    }
    if (a.qmax) {
#pragma unroll
        for (int k = 0; k < 3; ++k) q[k] = wave_max(q[k]);
    }
    if (lane == 0) {
        a.kind[row] = (uint8_t)red_kind_of(n, a.min_points);
        if (a.counts) {
            a.counts[row * 4] = n.n_fin;
#pragma unroll
            for (int k = 0; k < 3; ++k) a.counts[row * 4 + 1 + k] = n.bad[k];
        }
        if (a.qmax) {
#pragma unroll
            for (int k = 0; k < 3; ++k) a.qmax[row * 3 + k] = q[k];
        }
    }
}

void launch_fol_reduce_cplx(const FolReduceCplxArgs& a, hipStream_t s) {
    const dim3 grid((unsigned)a.n_list), block(64);
    hipLaunchKernelGGL(fol_reduce_cplx_kernel<kRedShallowD>, grid, block, 0, s, a);
    hipLaunchKernelGGL(fol_reduce_cplx_kernel<kFolMaxD>, grid, block, 0, s, a);
}

}  // namespace pd

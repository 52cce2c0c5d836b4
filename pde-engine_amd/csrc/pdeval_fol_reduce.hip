// pdeval_fol_reduce.hip -- the reduction kind of each listed program (DESIGN.md §14 "Reduction
// kinds"): fol_reduce_kernel and the entry point pdeval_fol_reduce.  Its own unit beside the
// foliation kernels: nothing of the validation or the class path depends on it.  With
// PDEVAL_FOL_CPLX the entry point then launches the complex pass (pdeval_fol_reduce_cplx.hip).
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/pdeval.h"
#include "pdeval_fol_reduce.h"

namespace pd {

// One wave per list row, one wave per block; lanes are sample points and the wave loops over the
// row's ceil(m^2 / 64) chunks, running the program again at each.  The kind needs the row's four
// counts together: they are wave-uniform counters fed by a ballot each, so there is no atomic and
// no second pass, and lane 0 stores the kind, the counts and the row maxima of |X| / S_X.
// The program is read wave-uniformly (scalar loads) and run in order-3 jets, the operand stack
// below the accumulator in LDS as [slot][coef][lane]: each lane touches only its own words, no
// barrier.  The stack decides the occupancy -- 7 slots are 35,840 bytes, four one-wave blocks per
// CU -- so the kernel exists twice: MAXD = kRedShallowD (2 slots, 10,240 bytes: the registers
// bind first) takes the rows whose header names a stack of at most kRedShallowD, MAXD = kFolMaxD
// the deeper ones.  Each launch covers the whole list and a wave leaves at once, before it reads
// any program word but the header, unless the row is its own; the shallow launch also writes
// the rows that no instantiation runs (kind 0, zero counts, a NaN table).
// Lanes past m^2 evaluate the last point again; they store nothing and count nothing.
template <int MAXD>
__global__ __launch_bounds__(64) void fol_reduce_kernel(FolReduceArgs a) {
    using I = Interp<double, 3, MAXD>;
    __shared__ double red_lds[red_stack_doubles<MAXD>()];
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
    double* tab = a.table ? a.table + row * 3 * (int64_t)mm : nullptr;
    RedCount n{0, {0, 0, 0}};
    double q[3] = {0.0, 0.0, 0.0};
    bool run_ok = pr.ok;
    for (int c = 0; c < a.n_chunk; ++c) {
        const int p = c * kFolChunk + lane;
        const bool active = p < mm;
        double tu = nan, tk = nan, tg = nan;
        if (run_ok) {
            double x, y;
            fol_point_xy(a.grid, active ? p : mm - 1, x, y);
            typename I::J u;
            run_ok = I::run(pr.words, 1, pr.len, x, y, u, red_lds, lane, a.prm) == RUN_OK;
            if (run_ok) {
                const RedPoint r = red_point(u.c, x, a.omega2, a.tau);
                const bool fin = active && r.fin;
                n.n_fin += count_lanes(fin);
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    n.bad[k] += count_lanes(active && r.bad[k]);
                    if (a.qmax && fin) q[k] = fmax(q[k], red_q(r, k));
                }
                if (tab) {
                    red_coefs(r, tk, tg);
                    tu = r.fin ? u.c[0] : nan;
                }
            }
        }
        if (tab && active) {
            tab[p] = tu;
            tab[mm + p] = tk;
            tab[2 * mm + p] = tg;
        }
    }
    // a run that does not return RUN_OK (wave-uniform: it depends on the program alone) fails at
    // the first chunk: nothing was counted
    if (a.qmax) {
#pragma unroll
        for (int k = 0; k < 3; ++k) q[k] = wave_max(q[k]);
    }
    if (lane == 0) {
        a.kind[row] = (uint8_t)(run_ok ? red_kind_of(n, a.min_points) : PDEVAL_RED_NONE);
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

void launch_fol_reduce(const FolReduceArgs& a, hipStream_t s) {
    const dim3 grid((unsigned)a.n_list), block(64);
    hipLaunchKernelGGL(fol_reduce_kernel<kRedShallowD>, grid, block, 0, s, a);
    hipLaunchKernelGGL(fol_reduce_kernel<kFolMaxD>, grid, block, 0, s, a);
}

}  // namespace pd

using namespace pd;

extern "C" int pdeval_fol_reduce(pdeval_ctx* c, const int32_t* d_ops, int64_t n_words, const int64_t* d_offsets,
                                 int64_t n, const int64_t* d_list, int64_t n_list, const pdeval_fol_params* params,
                                 double omega2, uint8_t* d_kind, int32_t* d_counts, double* d_qmax, double* d_table,
                                 void* stream) {
    FolCtx v;
    pdeval_fol_params prm;
    const int rc = fol_check(c, "pdeval_fol_reduce", d_ops, n_words, d_offsets, n, n_list, params, &v, &prm);
    if (rc != PDEVAL_OK) return rc;
    if (!(omega2 >= 0.0) || !std::isfinite(omega2))
        return fol_fail(c, PDEVAL_ERR_ARG, "pdeval_fol_reduce: omega2 must be finite and >= 0");
    if (n_list > 0 && !d_kind) return fol_fail(c, PDEVAL_ERR_ARG, "pdeval_fol_reduce: bad argument");
    if (n_list == 0) return PDEVAL_OK;
    hipError_t e = hipSetDevice(v.device);
    if (e != hipSuccess) return fol_hip_fail(c, "hipSetDevice", e);
    // (n_list <= PDEVAL_MAX_BATCH, fol_check: n_list one-wave blocks are one launch)
    FolReduceArgs a{};
    a.ops = d_ops;
    a.n_words = n_words;
    a.offsets = d_offsets;
    a.n = n;
    a.list = d_list;
    a.n_list = n_list;
    a.n_chunk = (prm.m * prm.m + kFolChunk - 1) / kFolChunk;
    a.grid = fol_grid(v.grid, prm.m);
    a.omega2 = omega2;
    a.tau = prm.tau;
    a.min_points = prm.min_points;
    a.kind = d_kind;
    a.counts = d_counts;
    a.qmax = d_qmax;
    a.table = d_table;
    launch_fol_reduce(a, stream ? (hipStream_t)stream : v.stream);
    if ((e = hipGetLastError()) != hipSuccess) return fol_hip_fail(c, "fol_reduce_kernel", e);
    if (prm.flags & PDEVAL_FOL_CPLX) {
        // the rows the real pass left at PDEVAL_RED_NONE, in complex jets (pdeval_fol_reduce_cplx.hip)
        FolReduceCplxArgs ca{};
        ca.ops = a.ops;
        ca.n_words = a.n_words;
        ca.offsets = a.offsets;
        ca.n = a.n;
        ca.list = a.list;
        ca.n_list = a.n_list;
        ca.n_chunk = a.n_chunk;
        ca.grid = a.grid;
        ca.omega2 = a.omega2;
        ca.tau = a.tau;
        ca.min_points = a.min_points;
        ca.kind = a.kind;
        ca.counts = a.counts;
        ca.qmax = a.qmax;
        launch_fol_reduce_cplx(ca, stream ? (hipStream_t)stream : v.stream);
        if ((e = hipGetLastError()) != hipSuccess) return fol_hip_fail(c, "fol_reduce_cplx_kernel", e);
    }
    return PDEVAL_OK;
}

// pdeval_fol_profile.hip -- psi(u) and the current along each foliation (DESIGN.md §14 "Profiles:
// psi(u) and the current"): the entry point pdeval_fol_profile and fol_profile_kernel.  Its own
// unit and its own argument block; it reads the table pdeval_fol_reduce / pdeval_fol_reduce_multi
// write and touches nothing of theirs.
//
// A table row holds u, kappa = -L_T A / L_T B and G = W / L_T B at the m x m sample points.  The
// reduced equations psi'' = kappa(u) psi' and I I'(psi) = G(u) psi' are ordinary differential
// equations in u, so the row is sorted by u and integrated by the trapezoid rule (include/pdeval.h
// states the rule).  A sort and three prefix sums do not fit the interpreter kernels' "one wave per
// row, lanes are points": here ONE BLOCK takes one row, sized by N = the power of two >= max(m^2, 64).
//
//   E = N / T elements per thread: 1 at N = 64, 2 at 128 .. 2048 (T = N / 2 = 64 .. 1024 threads),
//   4 at N = 4096 (T = 1024, sixteen waves).
//
//   LDS   key[N] (uint64) and idx[N] (uint16): 10 N bytes, 40 KB at N = 4096, dynamic -- a block pays
//         for its own N.  The key is the double u + 0.0 mapped to an unsigned integer of the same
//         order (negative: all bits flipped; otherwise: the sign bit set), so -0.0 and +0.0 are one
//         key and a negative u sorts below a positive one; an invalid point and the padding carry
//         ~0, which no finite double maps to and which sorts last.  The order is (key, idx), a
//         total order: the result does not depend on the network.
//
//   sort  a bitonic network, one compare-exchange per (thread, E / 2 comparators) and step.  Wave w
//         owns comparators [64 R w, 64 R (w + 1)), R = max(E / 2, 1), which at a stride j <= 64 R
//         touch only elements [128 R w, 128 R (w + 1)): those steps exchange through the wave's own
//         LDS words and are separated by a wave-level fence, not by a block barrier.  A block
//         barrier stands only where a step with a larger stride begins or ends: log2(N / (64 R))
//         runs of them.  N <= 128 is one wave and has none after the load.
//
//   n     the valid points are the keys below ~0, a prefix of the sorted row: the one thread that
//         sees the last of them stores n (no counting, no atomics).
//
//   sums  thread t then owns the E consecutive elements from t E, holds their u, kappa and G (gathered
//         from the row through idx: p < m^2 is checked, the row is L2-resident) in registers, and the
//         key storage is reused for the one value per thread its right neighbour needs -- the last
//         kappa, later the last psi' and G psi'^2.  P is a block-wide inclusive scan (sequential in the
//         thread, shuffles in the wave, wave totals through LDS, fix-up); psi' = exp(P) with the
//         device library's exp; psi and Q are scanned together, after it.
//
// Vector stores, plain C++, no inline assembly, no atomics, one launch.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/pdeval.h"
#include "pdeval_foliation.h"

namespace pd {

struct FolProfileArgs {
    const double* table;   // [n_rows][3][mm]: u, kappa, G
    int64_t n_rows;
    int mm;                // m^2
    int N;                 // the power of two >= max(mm, 64)
    int min_points;
    double* profile;       // [n_rows][4][mm]: u, psi', psi, Q
    int32_t* perm;         // optional, [n_rows][mm]
    int32_t* n;            // optional, [n_rows]
};

constexpr uint64_t kProfLast = ~0ull;     // the key of an invalid point and of the padding
constexpr int kProfMaxWaves = 16;

__device__ __forceinline__ uint64_t prof_key(double u) {
    const uint64_t b = (uint64_t)__double_as_longlong(u + 0.0);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double prof_u(uint64_t k) {
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}
__device__ __forceinline__ bool prof_finite(double v) { return fabs(v) < __builtin_huge_val(); }

// orders the LDS accesses of one wave: its lanes' stores before, their loads after
__device__ __forceinline__ void prof_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// K block-wide inclusive scans at once over the block's T E elements, thread t holding elements
// t E .. t E + E - 1 of each in v[k]: sequential in the thread, shuffles over the threads' totals in
// the wave, the waves' totals through wtot ([K][kProfMaxWaves]), then element = own prefix +
// (waves before + lanes before).  Ends with a barrier: wtot may be reused at once.
template <int E, int K>
__device__ __forceinline__ void prof_scan(double (&v)[K][E], double* wtot, int t) {
    const int lane = t & 63, w = t >> 6;
    double before[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
#pragma unroll
        for (int e = 1; e < E; ++e) v[k][e] += v[k][e - 1];
        double inc = v[k][E - 1];
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const double y = __shfl_up(inc, o, 64);
            if (lane >= o) inc += y;
        }
        if (lane == 63) wtot[k * kProfMaxWaves + w] = inc;
        const double ex = __shfl_up(inc, 1, 64);
        before[k] = lane ? ex : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double off = 0.0;
        for (int x = 0; x < w; ++x) off += wtot[k * kProfMaxWaves + x];
        off += before[k];
#pragma unroll
        for (int e = 0; e < E; ++e) v[k][e] += off;
    }
    __syncthreads();
}

template <int E>
__global__ __launch_bounds__(1024) void fol_profile_kernel(FolProfileArgs a) {
    constexpr int R = E >= 2 ? E / 2 : 1;          // comparators per thread and step
    constexpr int kLocal = 64 * R;                 // strides up to here stay inside the wave's elements
    extern __shared__ uint64_t prof_lds[];
    __shared__ double wtot[2 * kProfMaxWaves];
    __shared__ int n_sh;
    const int N = a.N, mm = a.mm, T = blockDim.x, t = threadIdx.x;
    uint64_t* key = prof_lds;                                 // [N]
    uint16_t* idx = reinterpret_cast<uint16_t*>(key + N);     // [N]
    double* nb = reinterpret_cast<double*>(key);              // [2 T] after the sort (2 T <= N, or E == 1 below)
    const int64_t row = blockIdx.x;
    if (row >= a.n_rows) return;
    const double* tab = a.table + row * 3 * (int64_t)mm;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);

    // ---- load: coalesced, element i = point i
    for (int i = t; i < N; i += T) {
        uint64_t k = kProfLast;
        if (i < mm) {
            const double u = tab[i], kap = tab[mm + i], g = tab[2 * mm + i];
            if (prof_finite(u) && prof_finite(kap) && prof_finite(g)) k = prof_key(u);
        }
        key[i] = k;
        idx[i] = (uint16_t)i;
    }

    // ---- sort ascending by (key, idx)
    int prev = 2 * N;                               // (the load is not wave-local: a block barrier first)
    for (int k = 2; k <= N; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            if (j > kLocal || prev > kLocal) __syncthreads();
            else prof_wave_sync();
            prev = j;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int c = (t >> 6) * (64 * R) + r * 64 + (t & 63);
                if (c < (N >> 1)) {
                    const int lo = ((c & ~(j - 1)) << 1) | (c & (j - 1)), hi = lo + j;
                    const uint64_t ka = key[lo], kb = key[hi];
                    const uint16_t ia = idx[lo], ib = idx[hi];
                    const bool gt = ka > kb || (ka == kb && ia > ib);
                    if (gt == ((lo & k) == 0)) {
                        key[lo] = kb; key[hi] = ka;
                        idx[lo] = ib; idx[hi] = ia;
                    }
                }
            }
        }
    }
    __syncthreads();

    // ---- own elements to registers; n = the length of the prefix of valid keys
    const int base = t * E;
    double u[E];
    int p[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int i = base + e;                     // (T E == N: in range)
        const uint64_t k = key[i];
        const bool ok = k != kProfLast;
        u[e] = prof_u(k);
        p[e] = idx[i];
        if (ok && (i + 1 == N || key[i + 1] == kProfLast)) n_sh = i + 1;
        if (i == 0 && !ok) n_sh = 0;
    }
    const double u_left = base ? prof_u(key[base - 1]) : 0.0;
    __syncthreads();
    const int n = n_sh;
    if (t == 0 && a.n) a.n[row] = n;
    const bool fill = n < a.min_points;            // block-uniform: such a row is NaN / -1 throughout
    double dp[E], sq[2][E];                         // psi'; psi and Q
    if (!fill) {
        // ---- kappa and G through the permutation; the increments of P
        double kap[E], g[E], d[E];
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const bool ok = base + e < n && p[e] < mm;
            kap[e] = ok ? tab[mm + p[e]] : 0.0;
            g[e] = ok ? tab[2 * mm + p[e]] : 0.0;
        }
        nb[t] = kap[E - 1];
        __syncthreads();
        const double kap_left = t ? nb[t - 1] : 0.0;
        double s[1][E];
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const int i = base + e;
            d[e] = (i >= 1 && i < n) ? u[e] - (e ? u[e - 1] : u_left) : 0.0;
            s[0][e] = 0.5 * (kap[e] + (e ? kap[e - 1] : kap_left)) * d[e];
        }
        prof_scan<E, 1>(s, wtot, t);                // (its barriers also order nb's reads before the next stores)
        // ---- psi' = exp(P); the increments of psi and Q
        double gq[E];
#pragma unroll
        for (int e = 0; e < E; ++e) {
            dp[e] = exp(s[0][e]);
            gq[e] = g[e] * dp[e] * dp[e];
        }
        if constexpr (E == 1) {                     // N == T == 64: one value at a time
            nb[t] = dp[0];
            __syncthreads();
            const double dp_left = t ? nb[t - 1] : 0.0;
            __syncthreads();
            nb[t] = gq[0];
            __syncthreads();
            const double gq_left = t ? nb[t - 1] : 0.0;
            sq[0][0] = 0.5 * (dp[0] + dp_left) * d[0];
            sq[1][0] = 0.5 * (gq[0] + gq_left) * d[0];
        } else {
            nb[t] = dp[E - 1];
            nb[T + t] = gq[E - 1];
            __syncthreads();
            const double dp_left = t ? nb[t - 1] : 0.0, gq_left = t ? nb[T + t - 1] : 0.0;
#pragma unroll
            for (int e = 0; e < E; ++e) {
                sq[0][e] = 0.5 * (dp[e] + (e ? dp[e - 1] : dp_left)) * d[e];
                sq[1][e] = 0.5 * (gq[e] + (e ? gq[e - 1] : gq_left)) * d[e];
            }
        }
        prof_scan<E, 2>(sq, wtot, t);
    }

    // ---- store: position i of the sorted row
    double* prof = a.profile + row * 4 * (int64_t)mm;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int i = base + e;
        if (i >= mm) continue;
        const bool ok = !fill && i < n;
        prof[i] = ok ? u[e] : nan;
        prof[mm + i] = ok ? dp[e] : nan;
        prof[2 * mm + i] = ok ? sq[0][e] : nan;
        prof[3 * mm + i] = ok ? sq[1][e] : nan;
        if (a.perm) a.perm[row * (int64_t)mm + i] = ok ? p[e] : -1;
    }
}

}  // namespace pd

using namespace pd;

extern "C" int pdeval_fol_profile(pdeval_ctx* c, const double* d_table, int64_t n_rows, const pdeval_fol_params* params,
                                  double* d_profile, int32_t* d_perm, int32_t* d_n, void* stream) {
    if (!c) return fol_fail(nullptr, PDEVAL_ERR_ARG, "pdeval_fol_profile: null context");
    FolCtx v;
    fol_ctx(c, &v);
    if (v.problem != PDEVAL_PROBLEM_FORCE_FREE)
        return fol_fail(c, PDEVAL_ERR_ARG, "pdeval_fol_profile: the reduction on a foliation is a force-free notion");
    pdeval_fol_params prm;
    if (params) prm = *params;
    else pdeval_default_fol_params(&prm);
    if (prm.m < 4 || prm.m > 64 || prm.min_points < 1)
        return fol_fail(c, PDEVAL_ERR_ARG, "pdeval_fol_profile: bad parameters (4 <= m <= 64, min_points >= 1)");
    if (n_rows < 0 || n_rows > PDEVAL_MAX_BATCH || (n_rows > 0 && (!d_table || !d_profile)))
        return fol_fail(c, PDEVAL_ERR_ARG, "pdeval_fol_profile: bad argument");
    if (n_rows == 0) return PDEVAL_OK;
    hipError_t e = hipSetDevice(v.device);
    if (e != hipSuccess) return fol_hip_fail(c, "hipSetDevice", e);
    FolProfileArgs a{};
    a.table = d_table;
    a.n_rows = n_rows;
    a.mm = prm.m * prm.m;
    a.N = 64;
    while (a.N < a.mm) a.N <<= 1;
    a.min_points = prm.min_points;
    a.profile = d_profile;
    a.perm = d_perm;
    a.n = d_n;
    const hipStream_t s = stream ? (hipStream_t)stream : v.stream;
    // (n_rows <= PDEVAL_MAX_BATCH: n_rows blocks are one launch)
    const dim3 grid((unsigned)n_rows);
    const size_t lds = (size_t)a.N * (sizeof(uint64_t) + sizeof(uint16_t));
    if (a.N == 64) hipLaunchKernelGGL(fol_profile_kernel<1>, grid, dim3(64), lds, s, a);
    else if (a.N <= 2048) hipLaunchKernelGGL(fol_profile_kernel<2>, grid, dim3(a.N / 2), lds, s, a);
    else hipLaunchKernelGGL(fol_profile_kernel<4>, grid, dim3(1024), lds, s, a);
    if ((e = hipGetLastError()) != hipSuccess) return fol_hip_fail(c, "fol_profile_kernel", e);
    return PDEVAL_OK;
}

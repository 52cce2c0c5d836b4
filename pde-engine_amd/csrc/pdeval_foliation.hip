// pdeval_foliation.hip -- the Jacobian match kernel of the foliation classes and its entry
// point pdeval_jacobian_match.  Its own unit: the kernel is small and none of
// the validation path depends on it.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "../../include/pdeval.h"
#include "pdeval_foliation.h"

namespace pd {

// One wave per row, four rows per block.  For each probe the wave walks the m^2 points (lanes are
// points), counts the usable and the bad points with ballots (wave-uniform counters in SGPRs)
// and, if asked, keeps the running maximum of q per lane, reduced with wave_max at the end.
// The probe fields are re-read by every row: they are read straight from global memory and
// live in L2 (32 probes x 2 m^2 doubles: 128 KiB at m = 16, 2 MiB at m = 64 -- more than a CU's
// LDS holds -- against 4 MiB of L2 per XCD); every wave reads them in the same order, coalesced.
// The row's own field (4 KiB at m = 16) is re-read once per probe and stays in the CU's L1.
// Without the diagnostics a probe is left at its first bad point: the mask is decided.
__global__ __launch_bounds__(256) void fol_match_kernel(FolMatchArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (row >= a.n_rows) return;
    const int mm = a.mm;
    const double* ra = a.rows + row * 2 * (int64_t)mm;
    const bool diag = a.n_used || a.qmax;
    uint32_t mask = 0u;
    for (int k = 0; k < a.n_probe; ++k) {
        const double* pa = a.probes + (int64_t)k * 2 * mm;
        int nu = 0, nb = 0;
        double q = 0.0;
        for (int p0 = 0; p0 < mm; p0 += 64) {
            const int p = p0 + lane;
            const bool active = p < mm;
            const int pc = active ? p : mm - 1;   // (lanes past m^2 re-read the last point, uncounted)
            const FolPoint t = fol_point_test(ra[pc], ra[mm + pc], pa[pc], pa[mm + pc], a.tau);
            nu += count_lanes(active && t.used);
            nb += count_lanes(active && t.bad);
            if (a.qmax && active && t.used) q = fmax(q, fol_q(t));
            if (!diag && nb) break;
        }
        if (nu >= a.min_points && nb == 0) mask |= 1u << k;
        if (a.qmax) q = wave_max(q);
        if (lane == 0) {
            if (a.n_used) a.n_used[row * a.n_probe + k] = nu;
            if (a.qmax) a.qmax[row * a.n_probe + k] = q;
        }
    }
    if (lane == 0) a.mask[row] = mask;
}

void launch_fol_match(const FolMatchArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(fol_match_kernel, dim3((unsigned)((a.n_rows + 3) / 4)), dim3(256), 0, s, a);
}

}  // namespace pd

using namespace pd;

extern "C" int pdeval_default_fol_params(pdeval_fol_params* p) {
    if (!p) return PDEVAL_ERR_ARG;
    p->tau = 1e-7;   // the grid stage's tau_grid (pdeval_default_params)
    p->m = 16;
    p->min_points = 16;
    p->reserved = 0;
    return PDEVAL_OK;
}

extern "C" int pdeval_jacobian_match(pdeval_ctx* c, const double* d_rows_field, int64_t n_rows,
                                     const double* d_probe_field, int n_probe, const pdeval_fol_params* params,
                                     uint32_t* d_mask, int32_t* d_n_used, double* d_qmax, void* stream) {
    if (!c) return fol_fail(nullptr, PDEVAL_ERR_ARG, "pdeval_jacobian_match: null context");
    FolCtx v;
    fol_ctx(c, &v);
    if (v.problem != PDEVAL_PROBLEM_FORCE_FREE)
        return fol_fail(c, PDEVAL_ERR_ARG,
                        "pdeval_jacobian_match: foliation classes are a force-free notion (the Kerr equation is "
                        "linear: u -> f(u) is no symmetry of it)");
    pdeval_fol_params prm;
    if (params) prm = *params;
    else pdeval_default_fol_params(&prm);
    if (prm.m < 4 || prm.m > 64 || prm.min_points < 1 || !(prm.tau >= 0.0) || !std::isfinite(prm.tau))
        return fol_fail(c, PDEVAL_ERR_ARG,
                        "pdeval_jacobian_match: bad parameters (4 <= m <= 64, min_points >= 1, tau >= 0 finite)");
    if (n_probe > PDEVAL_FOL_MAX_PROBES)
        return fol_fail(c, PDEVAL_ERR_ARG, "pdeval_jacobian_match: more than PDEVAL_FOL_MAX_PROBES probes");
    if (n_rows < 0 || n_probe < 0 || n_rows > PDEVAL_MAX_BATCH ||
        (n_rows > 0 && (!d_rows_field || !d_mask || (n_probe > 0 && !d_probe_field))))
        return fol_fail(c, PDEVAL_ERR_ARG, "pdeval_jacobian_match: bad argument");
    if (n_rows == 0) return PDEVAL_OK;
    hipError_t e = hipSetDevice(v.device);
    if (e != hipSuccess) return fol_fail(c, PDEVAL_ERR_HIP, (std::string("hipSetDevice: ") + hipGetErrorString(e)).c_str());
    FolMatchArgs a{};
    a.rows = d_rows_field;
    a.n_rows = n_rows;
    a.probes = d_probe_field;
    a.n_probe = n_probe;
    a.mm = prm.m * prm.m;
    a.tau = prm.tau;
    a.min_points = prm.min_points;
    a.mask = d_mask;
    a.n_used = d_n_used;
    a.qmax = d_qmax;
    launch_fol_match(a, stream ? (hipStream_t)stream : v.stream);
    e = hipGetLastError();
    if (e != hipSuccess) return fol_fail(c, PDEVAL_ERR_HIP, (std::string("fol_match_kernel: ") + hipGetErrorString(e)).c_str());
    return PDEVAL_OK;
}

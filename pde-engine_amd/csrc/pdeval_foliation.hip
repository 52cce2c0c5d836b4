// pdeval_foliation.hip -- the foliation classes: the gradient field kernel, the
// Jacobian match kernel and the entry points pdeval_gradient_fields, pdeval_jacobian_match and
// pdeval_foliation_classes.  Its own unit: the kernels are small and none of the validation path
// depends on them.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

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
// AXIS: the point test with the axis rule (PDEVAL_FOL_AXIS); AXIS = false is the kernel as it was.
template <bool AXIS>
__global__ __launch_bounds__(256) void fol_match_kernel(FolMatchArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (row >= a.n_rows) return;
    const int mm = a.mm;
    // (with an index the row's field is rows[idx[row]]: the unassigned subset of a round)
    const int64_t rsrc = a.idx ? a.idx[row] : row;
    const double* ra = a.rows + rsrc * 2 * (int64_t)mm;
    const bool diag = a.n_used || a.qmax;
    uint32_t mask = 0u;
    for (int k = 0; k < a.n_probe; ++k) {
        const double* pa = a.probes + (a.pidx ? a.pidx[k] : (int64_t)k) * 2 * mm;
        int nu = 0, nb = 0;
        double q = 0.0;
        for (int p0 = 0; p0 < mm; p0 += 64) {
            const int p = p0 + lane;
            const bool active = p < mm;
            const int pc = active ? p : mm - 1;   // (lanes past m^2 re-read the last point, uncounted)
            const FolPoint t = fol_point_test<AXIS>(ra[pc], ra[mm + pc], pa[pc], pa[mm + pc], a.tau);
            nu += count_lanes(active && t.used);
            nb += count_lanes(active && t.bad);
            if (a.qmax && active && t.used) q = fmax(q, fol_q<AXIS>(t));
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
    const dim3 grid((unsigned)((a.n_rows + 3) / 4)), block(256);
    if (a.flags & PDEVAL_FOL_AXIS) hipLaunchKernelGGL(fol_match_kernel<true>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(fol_match_kernel<false>, grid, block, 0, s, a);
}

// One wave per row, four rows per block; lanes are sample points.  The row's finite points are
// sorted into the four counts of fol_kind_chunk with a ballot each (wave-uniform counters in
// SGPRs) and lane 0 stores the row's kind as one byte.  The row is read from [n_rows][2][mm]
// fields, or (cap > 0) from leader `row` of a chunk-major store, whose points past m^2 hold NaN.
// The only index read is row < n_rows.
__global__ __launch_bounds__(256) void fol_kind_kernel(FolKindArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (row >= a.n_rows) return;
    const int mm = a.mm;
    FolKindCount n{0, 0, 0, 0};
    for (int c = 0; c < a.n_chunk; ++c) {
        const int p = c * kFolChunk + lane;
        const bool active = p < mm;
        double u, v;
        if (a.cap > 0) {
            const double* q = a.fields + fol_store_at(a.cap, c, row);
            u = q[lane];
            v = q[kFolChunk + lane];
        } else {
            const double* ra = a.fields + row * 2 * (int64_t)mm;
            const int pc = active ? p : mm - 1;   // (lanes past m^2 re-read the last point, uncounted)
            u = ra[pc];
            v = ra[mm + pc];
        }
        fol_kind_chunk(u, v, active, n);
    }
    if (lane == 0) a.kind[row] = (uint8_t)fol_kind_of(n, a.min_points);
}

void launch_fol_kind(const FolKindArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(fol_kind_kernel, dim3((unsigned)((a.n_rows + 3) / 4)), dim3(256), 0, s, a);
}

// One wave per (list row, 64-point chunk), four waves per block; lanes are sample points.  The
// program is read wave-uniformly (scalar loads) and run in order-1 jets, the operand stack
// below the accumulator in LDS (kFolStackDoubles per wave).  Lanes past m^2 compute the last
// point again and store nothing.  A row that fol_program declines, or whose run does not
// return RUN_OK (wave-uniform: it depends on the program alone), is NaN throughout.  The
// row's finite points are counted with a ballot per chunk and added to n_finite[row], which the
// caller has zeroed.
__global__ __launch_bounds__(256) void fol_field_kernel(FolFieldArgs a) {
    __shared__ double fol_lds[4 * kFolStackDoubles];
    const int lane = threadIdx.x & 63;
    const int wib = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t item = (int64_t)blockIdx.x * 4 + wib;
    const int64_t row = item / a.n_chunk;
    if (row >= a.n_list) return;
    const int chunk = (int)(item - row * a.n_chunk);
    const int mm = a.grid.m * a.grid.m;
    const int p = chunk * 64 + lane;
    const bool active = p < mm;
    const FolProg pr = fol_program(a.ops, a.n_words, a.offsets, a.n, a.list, row);
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    FolField f{nan, nan, false, RUN_BAD};
    if (pr.ok) {
        f = fol_field_point(pr, a.grid, active ? p : mm - 1, fol_lds + (size_t)wib * kFolStackDoubles, lane,
                            a.prm);
        if (f.rc != RUN_OK) f = FolField{nan, nan, false, f.rc};
    }
    if (active) {
        double* out = a.field + row * 2 * (int64_t)mm;
        out[p] = f.a;
        out[mm + p] = f.b;
    }
    const int nf = count_lanes(active && f.fin);
    if (a.n_finite && lane == 0 && nf) atomicAdd(a.n_finite + row, nf);
}

void launch_fol_field(const FolFieldArgs& a, hipStream_t s) {
    const int64_t items = a.n_list * a.n_chunk;
    hipLaunchKernelGGL(fol_field_kernel, dim3((unsigned)((items + 3) / 4)), dim3(256), 0, s, a);
}

}  // namespace pd

using namespace pd;

extern "C" int pdeval_default_fol_params(pdeval_fol_params* p) {
    if (!p) return PDEVAL_ERR_ARG;
    p->tau = 1e-7;   // the grid stage's tau_grid (pdeval_default_params)
    p->m = 16;
    p->min_points = 16;
    p->flags = 0;
    return PDEVAL_OK;
}

extern "C" int pdeval_jacobian_match(pdeval_ctx* c, const double* d_rows_field, int64_t n_rows,
                                     const double* d_probe_field, int n_probe, const pdeval_fol_params* params,
                                     uint32_t* d_mask, int32_t* d_n_used, double* d_qmax, void* stream) {
    FolCtx v;
    pdeval_fol_params prm;
    const int rc = fol_check(c, "pdeval_jacobian_match", nullptr, 0, nullptr, 0, 0, params, &v, &prm);
    if (rc != PDEVAL_OK) return rc;
    if (n_probe > PDEVAL_FOL_MAX_PROBES)
        return fol_fail(c, PDEVAL_ERR_ARG, "pdeval_jacobian_match: more than PDEVAL_FOL_MAX_PROBES probes");
    if (n_rows < 0 || n_probe < 0 || n_rows > PDEVAL_MAX_BATCH ||
        (n_rows > 0 && (!d_rows_field || !d_mask || (n_probe > 0 && !d_probe_field))))
        return fol_fail(c, PDEVAL_ERR_ARG, "pdeval_jacobian_match: bad argument");
    if (n_rows == 0) return PDEVAL_OK;
    hipError_t e = hipSetDevice(v.device);
    if (e != hipSuccess) return fol_hip_fail(c, "hipSetDevice", e);
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
    a.flags = (uint32_t)prm.flags;
    launch_fol_match(a, stream ? (hipStream_t)stream : v.stream);
    e = hipGetLastError();
    if (e != hipSuccess) return fol_hip_fail(c, "fol_match_kernel", e);
    return PDEVAL_OK;
}

namespace pd {
// the checks the program entry points share; fills prm and the context view
int fol_check(pdeval_ctx* c, const char* fn, const int32_t* d_ops, int64_t n_words, const int64_t* d_offsets,
              int64_t n, int64_t n_list, const pdeval_fol_params* params, FolCtx* v, pdeval_fol_params* prm) {
    const std::string f(fn);
    if (!c) return fol_fail(nullptr, PDEVAL_ERR_ARG, (f + ": null context").c_str());
    fol_ctx(c, v);
    if (v->problem != PDEVAL_PROBLEM_FORCE_FREE)
        return fol_fail(c, PDEVAL_ERR_ARG,
                        (f + ": foliation classes are a force-free notion (the Kerr equation is linear: u -> f(u) "
                             "is no symmetry of it)").c_str());
    if (params) *prm = *params;
    else pdeval_default_fol_params(prm);
    if (prm->m < 4 || prm->m > 64 || prm->min_points < 1 || !(prm->tau >= 0.0) || !std::isfinite(prm->tau))
        return fol_fail(c, PDEVAL_ERR_ARG,
                        (f + ": bad parameters (4 <= m <= 64, min_points >= 1, tau >= 0 finite)").c_str());
    if (n_list < 0 || n < 0 || n_words < 0 || n > PDEVAL_MAX_BATCH || n_list > PDEVAL_MAX_BATCH ||
        (n_list > 0 && (!d_ops || !d_offsets)))
        return fol_fail(c, PDEVAL_ERR_ARG, (f + ": bad argument").c_str());
    return PDEVAL_OK;
}

int fol_hip_fail(pdeval_ctx* c, const char* what, hipError_t e) {
    return fol_fail(c, PDEVAL_ERR_HIP, (std::string(what) + ": " + hipGetErrorString(e)).c_str());
}

// zeroes d_n_finite (if given) and launches the field kernel on s
int fol_fields_launch(pdeval_ctx* c, const FolCtx& v, const pdeval_fol_params& prm, const int32_t* d_ops,
                      int64_t n_words, const int64_t* d_offsets, int64_t n, const int64_t* d_list, int64_t n_list,
                      double* d_field, int32_t* d_n_finite, hipStream_t s) {
    FolFieldArgs a{};
    a.ops = d_ops;
    a.n_words = n_words;
    a.offsets = d_offsets;
    a.n = n;
    a.list = d_list;
    a.n_list = n_list;
    a.n_chunk = (prm.m * prm.m + 63) / 64;
    a.grid = fol_grid(v.grid, prm.m);
    a.field = d_field;
    a.n_finite = d_n_finite;
    if ((a.n_list * a.n_chunk + 3) / 4 > 0x7fffffffll)
        return fol_fail(c, PDEVAL_ERR_ARG, "fol_field_kernel: n_list x chunks exceeds one launch");
    hipError_t e;
    if (d_n_finite && (e = hipMemsetAsync(d_n_finite, 0, (size_t)n_list * sizeof(int32_t), s)) != hipSuccess)
        return fol_hip_fail(c, "hipMemsetAsync", e);
    launch_fol_field(a, s);
    if ((e = hipGetLastError()) != hipSuccess) return fol_hip_fail(c, "fol_field_kernel", e);
    return PDEVAL_OK;
}

// the rounds of pdeval_foliation_classes and of a registry's Stage B
int fol_rounds(pdeval_ctx* c, const double* d_field, int mm, const pdeval_fol_params& prm, std::vector<int64_t>& un,
               const int64_t* list, int64_t* leader, int64_t* d_idx, uint32_t* d_mask, hipStream_t s,
               int64_t* classes, int32_t* rounds) {
    hipError_t e;
    std::vector<int64_t> next;
    std::vector<uint32_t> mask;
    while (!un.empty()) {
        const int64_t nu = (int64_t)un.size();
        const int np = (int)std::min<int64_t>(PDEVAL_FOL_MAX_PROBES, nu);
        mask.resize((size_t)nu);
        if ((e = hipMemcpyAsync(d_idx, un.data(), (size_t)nu * sizeof(int64_t), hipMemcpyHostToDevice, s)) != hipSuccess)
            return fol_hip_fail(c, "hipMemcpyAsync", e);
        FolMatchArgs a{};
        a.rows = d_field;
        a.n_rows = nu;
        a.probes = d_field;
        a.n_probe = np;
        a.mm = mm;
        a.tau = prm.tau;
        a.min_points = prm.min_points;
        a.mask = d_mask;
        a.idx = d_idx;
        a.pidx = d_idx;   // the round's probes: its first np rows
        a.flags = (uint32_t)prm.flags;
        launch_fol_match(a, s);
        if ((e = hipGetLastError()) != hipSuccess) return fol_hip_fail(c, "fol_match_kernel", e);
        if ((e = hipMemcpyAsync(mask.data(), d_mask, (size_t)nu * sizeof(uint32_t), hipMemcpyDeviceToHost, s)) != hipSuccess)
            return fol_hip_fail(c, "hipMemcpyAsync", e);
        // (un is read by the upload above until the stream has passed it: synchronize before fol_round swaps it)
        if ((e = hipStreamSynchronize(s)) != hipSuccess) return fol_hip_fail(c, "fol_match_kernel", e);
        *classes += fol_round(mask.data(), un.data(), nu, np, list, leader, next);
        un.swap(next);
        ++*rounds;
    }
    return PDEVAL_OK;
}
}  // namespace pd

extern "C" int pdeval_gradient_fields(pdeval_ctx* c, const int32_t* d_ops, int64_t n_words, const int64_t* d_offsets,
                                      int64_t n, const int64_t* d_list, int64_t n_list,
                                      const pdeval_fol_params* params, double* d_field, int32_t* d_n_finite,
                                      void* stream) {
    FolCtx v;
    pdeval_fol_params prm;
    const int rc = fol_check(c, "pdeval_gradient_fields", d_ops, n_words, d_offsets, n, n_list, params, &v, &prm);
    if (rc != PDEVAL_OK) return rc;
    if (n_list > 0 && !d_field) return fol_fail(c, PDEVAL_ERR_ARG, "pdeval_gradient_fields: bad argument");
    if (n_list == 0) return PDEVAL_OK;
    hipError_t e = hipSetDevice(v.device);
    if (e != hipSuccess) return fol_hip_fail(c, "hipSetDevice", e);
    return fol_fields_launch(c, v, prm, d_ops, n_words, d_offsets, n, d_list, n_list, d_field, d_n_finite,
                             stream ? (hipStream_t)stream : v.stream);
}

extern "C" int pdeval_field_kinds(pdeval_ctx* c, const double* d_fields, int64_t n_rows,
                                  const pdeval_fol_params* params, uint8_t* d_kind, void* stream) {
    FolCtx v;
    pdeval_fol_params prm;
    const int rc = fol_check(c, "pdeval_field_kinds", nullptr, 0, nullptr, 0, 0, params, &v, &prm);
    if (rc != PDEVAL_OK) return rc;
    if (n_rows < 0 || n_rows > PDEVAL_MAX_BATCH || (n_rows > 0 && (!d_fields || !d_kind)))
        return fol_fail(c, PDEVAL_ERR_ARG, "pdeval_field_kinds: bad argument");
    if (n_rows == 0) return PDEVAL_OK;
    hipError_t e = hipSetDevice(v.device);
    if (e != hipSuccess) return fol_hip_fail(c, "hipSetDevice", e);
    FolKindArgs a{};
    a.fields = d_fields;
    a.n_rows = n_rows;
    a.cap = 0;
    a.mm = prm.m * prm.m;
    a.n_chunk = (a.mm + kFolChunk - 1) / kFolChunk;
    a.min_points = prm.min_points;
    a.kind = d_kind;
    launch_fol_kind(a, stream ? (hipStream_t)stream : v.stream);
    if ((e = hipGetLastError()) != hipSuccess) return fol_hip_fail(c, "fol_kind_kernel", e);
    return PDEVAL_OK;
}

extern "C" int pdeval_foliation_classes(pdeval_ctx* c, const int32_t* d_ops, int64_t n_words,
                                        const int64_t* d_offsets, int64_t n, const int64_t* d_list, int64_t n_list,
                                        const pdeval_fol_params* params, int64_t* leader, int64_t* n_classes,
                                        int32_t* n_rounds) {
    FolCtx v;
    pdeval_fol_params prm;
    int rc = fol_check(c, "pdeval_foliation_classes", d_ops, n_words, d_offsets, n, n_list, params, &v, &prm);
    if (rc != PDEVAL_OK) return rc;
    if (n_list > 0 && !leader) return fol_fail(c, PDEVAL_ERR_ARG, "pdeval_foliation_classes: bad argument");
    if (n_classes) *n_classes = 0;
    if (n_rounds) *n_rounds = 0;
    if (n_list == 0) return PDEVAL_OK;
    hipError_t e = hipSetDevice(v.device);
    if (e != hipSuccess) return fol_hip_fail(c, "hipSetDevice", e);
    const hipStream_t s = v.stream;
    const int mm = prm.m * prm.m;
    // device buffers: the fields of the whole list (never copied to the host), the finite
    // counts, the round's row indices and its masks; freed when the call returns
    DevBuf<double> d_field;
    DevBuf<int32_t> d_nfin;
    DevBuf<int64_t> d_idx;
    DevBuf<uint32_t> d_mask;
    const int64_t field_doubles = n_list * 2 * (int64_t)mm;
    if (!d_field.reserve(field_doubles))
        return fol_fail(c, PDEVAL_ERR_ALLOC,
                        ("pdeval_foliation_classes: cannot allocate " + std::to_string((size_t)field_doubles * sizeof(double)) +
                         " bytes of gradient fields (n_list x 2 m^2 x 8): classify a shorter list or a smaller m")
                            .c_str());
    if (!d_nfin.reserve(n_list) || !d_idx.reserve(n_list) || !d_mask.reserve(n_list))
        return fol_fail(c, PDEVAL_ERR_ALLOC, "pdeval_foliation_classes: cannot allocate the round buffers");
    rc = fol_fields_launch(c, v, prm, d_ops, n_words, d_offsets, n, d_list, n_list, d_field.p, d_nfin.p, s);
    if (rc != PDEVAL_OK) return rc;
    std::vector<int32_t> nfin((size_t)n_list);
    std::vector<int64_t> list;
    if (d_list) {
        list.resize((size_t)n_list);
        if ((e = hipMemcpyAsync(list.data(), d_list, (size_t)n_list * sizeof(int64_t), hipMemcpyDeviceToHost, s)) != hipSuccess)
            return fol_hip_fail(c, "hipMemcpyAsync", e);
    }
    if ((e = hipMemcpyAsync(nfin.data(), d_nfin.p, (size_t)n_list * sizeof(int32_t), hipMemcpyDeviceToHost, s)) != hipSuccess)
        return fol_hip_fail(c, "hipMemcpyAsync", e);
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return fol_hip_fail(c, "fol_field_kernel", e);
    // rows with too few finite points are unclassified; the others wait for a round
    std::vector<int64_t> un;
    for (int64_t r = 0; r < n_list; ++r) {
        leader[r] = -1;
        if (nfin[(size_t)r] >= prm.min_points) un.push_back(r);
    }
    int64_t classes = 0;
    int32_t rounds = 0;
    rc = fol_rounds(c, d_field.p, mm, prm, un, d_list ? list.data() : nullptr, leader, d_idx.p, d_mask.p, s, &classes, &rounds);
    if (rc != PDEVAL_OK) return rc;
    if (n_classes) *n_classes = classes;
    if (n_rounds) *n_rounds = rounds;
    return PDEVAL_OK;
}

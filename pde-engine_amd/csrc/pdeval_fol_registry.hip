// pdeval_fol_registry.hip -- the foliation class registry (DESIGN.md §14 "Registry"): the leaders'
// gradient fields resident on the device across batches and the one pair scan over them,
// fol_scan, in its two modes: Stage A (fol_assign_kernel: each row's first match, in one launch)
// and the link pass (fol_link_kernel: every other leader a row matches, "Links and components");
// the store's append / export kernel and the pdeval_fol_registry_* entry points.  Stage B and the
// fields reuse pdeval_foliation.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <memory>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/pdeval.h"
#include "pdeval_fol_book.h"
#include "pdeval_foliation.h"

namespace pd {

// The pair scan.  One wave per row, four rows per 256-thread block; lanes are sample points.  The
// leaders are walked in creation order in tiles of T = kFolAssignTile: the block copies the
// tile's first chunks (T x 1 KiB, contiguous in the chunk-major store) into LDS, the next tile
// travelling in registers meanwhile, and each of its waves tests its row against them from
// there, so a leader's screening chunk leaves L2 once per four rows.  A pair is left at its
// first chunk with a bad point -- almost always the first -- and only a pair that survives
// reads the leader's later chunks, straight from global memory.  REG (m <= 16): the row's whole
// field, at most 4 chunks x 2 doubles per lane, stays in registers for the scan; otherwise
// only its first chunk does and the later ones are re-read per surviving pair.  Counts are
// ballots into wave-uniform counters.  AXIS: the chunk test with the axis rule (PDEVAL_FOL_AXIS).
// The mode supplies what differs, each under an `if constexpr (LINK)` below:
//                     Stage A                              link pass
//   the row scans     [0, L)                               [0, lim[row]) without cls[row]
//   it scans nothing  n_finite[row] < min_points           cls[row] < 0
//   the block walks   the tiles below L                    below the largest lim of its four rows
//                                                          (one LDS word per wave and a barrier)
//   on a match        first[row] = the leader, the row     lane 0 appends (cls[row], leader), the slot
//                     is done                              taken by an atomic add on a device counter;
//                                                          past ecap the edge is counted, not stored
//                                                          (the host grows the buffer and repeats)
//   the block ends    when its four rows are done          after its last tile
// The only indices read are row < n_rows and leader < L (Stage A), leader < max lim <= L and
// cls[row] in [-1, L) (link pass; the host checks lim and cls before the launch).  Edge order is
// whatever the atomics give; the components do not depend on it.
enum class FolMode { StageA, Link };
template <FolMode MODE>
using FolModeArgs = std::conditional_t<MODE == FolMode::Link, FolLinkArgs, FolAssignArgs>;

template <FolMode MODE, bool REG, bool AXIS>
__device__ __forceinline__ void fol_scan(const FolModeArgs<MODE>& a) {
    constexpr bool LINK = MODE == FolMode::Link;
    constexpr int T = kFolAssignTile, NR = REG ? kFolRegChunks : 1;
    constexpr int kPf = T * 2 * kFolChunk / 2 / 256;   // double2 per thread and tile
    __shared__ double2 tile2[T * kFolChunk];
    const double* tile = (const double*)tile2;
    const int lane = threadIdx.x & 63;
    const int wib = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t row = (int64_t)blockIdx.x * 4 + wib;
    const int mm = a.mm;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    const bool in_batch = row < a.n_rows;
    const double* ra = a.rows + (in_batch ? row : 0) * 2 * (int64_t)mm;
    // the row scans the leaders [0, lim) other than `own`; done: it scans nothing (more)
    int64_t lim = a.L;
    [[maybe_unused]] int own = -1;
    bool done = !in_batch;
    if constexpr (LINK) {
        if (in_batch) own = __builtin_amdgcn_readfirstlane(a.cls[row]);
        done = own < 0;
        lim = done ? 0 : __builtin_amdgcn_readfirstlane(a.lim[row]);
    } else {
        // (a row with fewer finite points than a match needs usable ones matches nothing)
        if (in_batch && a.n_finite) done = __builtin_amdgcn_readfirstlane((int)(a.n_finite[row] < a.min_points)) != 0;
    }
    double fa[NR], fb[NR];
#pragma unroll
    for (int c = 0; c < NR; ++c) {
        const int p = c * kFolChunk + lane;
        const int pc = p < mm ? p : mm - 1;
        fa[c] = p < mm ? ra[pc] : nan;
        fb[c] = p < mm ? ra[mm + pc] : nan;
    }
    int64_t top = a.L;   // block-uniform: the leaders the block walks
    if constexpr (LINK) {
        __shared__ int s_lim[4];
        if (lane == 0) s_lim[wib] = (int)lim;
        __syncthreads();
        top = max(max(s_lim[0], s_lim[1]), max(s_lim[2], s_lim[3]));   // <= L
    }
    double2 pf[kPf];
    auto fetch = [&](int64_t t0) {
        const int n2 = (top - t0 < T ? (int)(top - t0) : T) * kFolChunk;   // double2 of the tile's leaders
        const double2* src = (const double2*)(a.store + fol_store_at(a.cap, 0, t0));
#pragma unroll
        for (int i = 0; i < kPf; ++i) {
            const int j = (int)threadIdx.x + 256 * i;
            pf[i] = j < n2 ? src[j] : double2{nan, nan};
        }
    };
    [[maybe_unused]] int64_t first = -1;
    if (top > 0) fetch(0);
    for (int64_t t0 = 0; t0 < top; t0 += T) {
#pragma unroll
        for (int i = 0; i < kPf; ++i) tile2[(int)threadIdx.x + 256 * i] = pf[i];
        __syncthreads();
        if (t0 + T < top) fetch(t0 + T);
        if (!done) {
            const int tn = lim - t0 < T ? (int)(lim - t0) : T;   // (<= 0 for a row whose leaders end before this tile)
            for (int k = 0; k < tn; ++k) {
                const int64_t l = t0 + k;
                if constexpr (LINK)
                    if (l == own) continue;
                const double* q0 = tile + k * 2 * kFolChunk;
                FolCount n{0, 0};
                fol_chunk_test<AXIS>(fa[0], fb[0], q0[lane], q0[kFolChunk + lane], lane < mm, a.tau, n);
                if (n.nb) continue;
                if constexpr (REG) {
#pragma unroll
                    for (int c = 1; c < NR; ++c)
                        if (c < a.n_chunk && !n.nb) {
                            const double* q = a.store + fol_store_at(a.cap, c, l);
                            fol_chunk_test<AXIS>(fa[c], fb[c], q[lane], q[kFolChunk + lane], c * kFolChunk + lane < mm,
                                                 a.tau, n);
                        }
                } else {
                    for (int c = 1; c < a.n_chunk && !n.nb; ++c) {
                        const double* q = a.store + fol_store_at(a.cap, c, l);
                        const int p = c * kFolChunk + lane;
                        const int pc = p < mm ? p : mm - 1;
                        fol_chunk_test<AXIS>(ra[pc], ra[mm + pc], q[lane], q[kFolChunk + lane], p < mm, a.tau, n);
                    }
                }
                if (n.nu >= a.min_points && n.nb == 0) {
                    if constexpr (LINK) {
                        if (lane == 0) {
                            const unsigned long long slot = atomicAdd(a.count, 1ull);
                            if (slot < (unsigned long long)a.ecap) {
                                a.edges[2 * slot] = own;
                                a.edges[2 * slot + 1] = (int32_t)l;
                            }
                        }
                    } else {
                        first = l;
                        done = true;
                        break;
                    }
                }
            }
        }
        // (every exit is also the barrier between this tile's readers and the next tile's writers)
        if constexpr (LINK) __syncthreads();
        else if (__syncthreads_and(done)) break;
    }
    if constexpr (!LINK)
        if (lane == 0 && in_batch) a.first[row] = first;
}

template <bool REG, bool AXIS>
__global__ __launch_bounds__(256) void fol_assign_kernel(FolAssignArgs a) {
    fol_scan<FolMode::StageA, REG, AXIS>(a);
}
template <bool REG, bool AXIS>
__global__ __launch_bounds__(256) void fol_link_kernel(FolLinkArgs a) {
    fol_scan<FolMode::Link, REG, AXIS>(a);
}

// launches k[REG + 2 AXIS], the instantiation the arguments select
template <class Args>
void launch_fol_scan(void (*const (&k)[4])(Args), const Args& a, hipStream_t s) {
    const int v = (a.n_chunk <= kFolRegChunks ? 1 : 0) + ((a.flags & PDEVAL_FOL_AXIS) ? 2 : 0);
    hipLaunchKernelGGL(k[v], dim3((unsigned)((a.n_rows + 3) / 4)), dim3(256), 0, s, a);
}
void launch_fol_assign(const FolAssignArgs& a, hipStream_t s) {
    static void (*const k[4])(FolAssignArgs) = {fol_assign_kernel<false, false>, fol_assign_kernel<true, false>,
                                                fol_assign_kernel<false, true>, fol_assign_kernel<true, true>};
    launch_fol_scan(k, a, s);
}
void launch_fol_link(const FolLinkArgs& a, hipStream_t s) {
    static void (*const k[4])(FolLinkArgs) = {fol_link_kernel<false, false>, fol_link_kernel<true, false>,
                                              fol_link_kernel<false, true>, fol_link_kernel<true, true>};
    launch_fol_scan(k, a, s);
}

// One wave per (leader, chunk) of the call.  to_store: leader k's field, fields[idx[k]] (or
// fields[k]), becomes store leader base + k, NaN at the points past m^2 and throughout for an
// index outside [0, n_rows); otherwise store leader base + k is written out to fields[k].
__global__ __launch_bounds__(256) void fol_move_kernel(FolMoveArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t item = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t k = item / a.n_chunk;
    if (k >= a.n_lead) return;
    const int c = (int)(item - k * a.n_chunk);
    const int64_t src = a.idx ? a.idx[k] : k;
    const bool ok = src >= 0 && src < a.n_rows;
    const int p = c * kFolChunk + lane;
    const bool active = ok && p < a.mm;
    double* f = a.fields + (ok ? src : 0) * 2 * (int64_t)a.mm;
    double* st = a.store + fol_store_at(a.cap, c, a.base + k);
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    if (a.to_store) {
        st[lane] = active ? f[p] : nan;
        st[kFolChunk + lane] = active ? f[a.mm + p] : nan;
    } else if (active) {
        f[p] = st[lane];
        f[a.mm + p] = st[kFolChunk + lane];
    }
}

void launch_fol_move(const FolMoveArgs& a, hipStream_t s) {
    const int64_t items = a.n_lead * a.n_chunk;
    hipLaunchKernelGGL(fol_move_kernel, dim3((unsigned)((items + 3) / 4)), dim3(256), 0, s, a);
}

// One wave per row: the points with a finite u_rho, as fol_field_kernel counts them (it stores
// both components NaN unless u, u_rho and u_z are all finite).
__global__ __launch_bounds__(256) void fol_nfinite_kernel(const double* fields, int64_t n_rows, int mm,
                                                          int32_t* n_finite) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (row >= n_rows) return;
    const double* ra = fields + row * 2 * (int64_t)mm;
    int nf = 0;
    for (int p0 = 0; p0 < mm; p0 += kFolChunk) {
        const int p = p0 + lane;
        nf += count_lanes(p < mm && finite_(ra[p < mm ? p : mm - 1]));
    }
    if (lane == 0) n_finite[row] = nf;
}

void launch_fol_nfinite(const double* fields, int64_t n_rows, int mm, int32_t* n_finite, hipStream_t s) {
    hipLaunchKernelGGL(fol_nfinite_kernel, dim3((unsigned)((n_rows + 3) / 4)), dim3(256), 0, s, fields, n_rows, mm,
                       n_finite);
}

}  // namespace pd

using namespace pd;

// The four timing events of a registry: all of them or none.
struct FolEvents {
    hipEvent_t e[4] = {};
    FolEvents() = default;
    FolEvents(const FolEvents&) = delete;
    FolEvents& operator=(const FolEvents&) = delete;
    ~FolEvents() { clear(); }
    void clear() {
        for (hipEvent_t& x : e) {
            if (x) (void)hipEventDestroy(x);
            x = nullptr;
        }
    }
    hipError_t create() {
        for (hipEvent_t& x : e) {
            const hipError_t err = hipEventCreate(&x);
            if (err != hipSuccess) {
                x = nullptr;
                clear();
                return err;
            }
        }
        return hipSuccess;
    }
};

// A registry: bound to one context and one parameter set.  The leader store and the scratch of
// a batch belong to it and are reused between calls; each buffer knows its own capacity.
struct pdeval_fol_registry {
    pdeval_ctx* ctx = nullptr;
    FolCtx v{};
    pdeval_fol_params prm{};
    int mm = 0, n_chunk = 0;
    DevBuf<double> d_store;   // chunk-major, cap() leaders (fol_store_at)
    FolBook book;
    // scratch of a batch: Stage A's first[], the finite counts, Stage B's indices and masks
    DevBuf<int64_t> d_first, d_idx;
    DevBuf<int32_t> d_nfin;
    DevBuf<uint32_t> d_mask;
    DevBuf<double> d_field;   // the fields of a batch of programs (pdeval_fol_registry_assign)
    FolEvents ev;             // e[0], e[1] around Stage A's launch; e[2], e[3] around each launch of the link kernel
    bool timed = false;
    // the link pass (PDEVAL_FOL_LINK, pdeval_fol_registry_link_fields): the rows' classes and scan
    // limits, the edge buffer (edge_cap() pairs) and its counter; allocated at first use
    int64_t edge_hint = 0;
    DevBuf<int32_t> d_cls, d_lim, d_edges;
    DevBuf<unsigned long long> d_count;
    double link_ms = 0.0;     // the link kernel's launches of the most recent call, summed
    std::vector<int32_t> cls32, lim32, edges;
    std::vector<FolBook::Link> merged, fresh;
    // host buffers of a batch, reused
    std::vector<int64_t> first, leader_b, un, new_rows, ids;
    std::vector<int32_t> nfin;

    int64_t leader_doubles() const { return (int64_t)n_chunk * 2 * kFolChunk; }
    int64_t cap() const { return d_store.cap / leader_doubles(); }
    int64_t edge_cap() const { return d_edges.cap / 2; }
};

namespace {
// the store holds `need` leaders: doubling, outside any kernel (new allocation, one
// device-to-device copy per chunk plane, free); on failure nothing has changed
int reg_reserve(pdeval_fol_registry* r, int64_t need) {
    if (need <= r->cap()) return PDEVAL_OK;
    const int64_t cap = fol_next_capacity(r->cap(), need);
    DevBuf<double> grown;
    if (!grown.reserve(cap * r->leader_doubles()))
        return fol_fail(r->ctx, PDEVAL_ERR_ALLOC,
                        ("pdeval_fol_registry: cannot allocate " +
                         std::to_string((size_t)cap * (size_t)r->leader_doubles() * sizeof(double)) +
                         " bytes of leader fields (capacity x chunks x 1 KiB)").c_str());
    const int64_t L = r->book.n_classes();
    hipError_t e = hipSuccess;
    for (int c = 0; c < r->n_chunk && L > 0 && e == hipSuccess; ++c)
        e = hipMemcpyAsync(grown.p + fol_store_at(cap, c, 0), r->d_store.p + fol_store_at(r->cap(), c, 0),
                           (size_t)L * 2 * kFolChunk * sizeof(double), hipMemcpyDeviceToDevice, r->v.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(r->v.stream);
    if (e != hipSuccess) return fol_hip_fail(r->ctx, "hipMemcpyAsync", e);
    r->d_store.swap(grown);
    return PDEVAL_OK;
}

// the scratch of a batch of n rows (and, with_field, its fields): a buffer is reallocated only
// when a batch outgrows it
int reg_scratch(pdeval_fol_registry* r, int64_t n, bool with_field) {
    if (!r->d_first.reserve(n) || !r->d_nfin.reserve(n) || !r->d_idx.reserve(n) || !r->d_mask.reserve(n))
        return fol_fail(r->ctx, PDEVAL_ERR_ALLOC, "pdeval_fol_registry: cannot allocate the batch buffers");
    const int64_t doubles = n * 2 * (int64_t)r->mm;
    if (with_field && !r->d_field.reserve(doubles))
        return fol_fail(r->ctx, PDEVAL_ERR_ALLOC,
                        ("pdeval_fol_registry_assign: cannot allocate " + std::to_string((size_t)doubles * sizeof(double)) +
                         " bytes of gradient fields (n_list x 2 m^2 x 8): assign a shorter list or a smaller m")
                            .c_str());
    return PDEVAL_OK;
}

// the registry and the context of a call
int reg_check(pdeval_ctx* c, pdeval_fol_registry* r, const char* fn) {
    const std::string f(fn);
    if (!c) return fol_fail(nullptr, PDEVAL_ERR_ARG, (f + ": null context").c_str());
    if (!r) return fol_fail(c, PDEVAL_ERR_ARG, (f + ": null registry").c_str());
    if (r->ctx != c)
        return fol_fail(c, PDEVAL_ERR_ARG, (f + ": the registry belongs to another context").c_str());
    return PDEVAL_OK;
}

// what both modes of the scan take: the rows d_fields against the store's leaders [0, L)
FolScanArgs reg_scan_args(const pdeval_fol_registry* r, const double* d_fields, int64_t n, int64_t L) {
    return {d_fields, n, r->d_store.p, r->cap(), L, r->mm, r->n_chunk, r->prm.tau, r->prm.min_points,
            (uint32_t)r->prm.flags};
}

// fol_move_kernel between the store's leaders base .. base + n_lead - 1 and `fields` (n_rows rows,
// leader k's at idx[k], or at k without idx), waited for
int reg_move(pdeval_fol_registry* r, int64_t base, int64_t n_lead, double* fields, int64_t n_rows, const int64_t* idx,
             bool to_store) {
    const FolMoveArgs m{r->d_store.p, r->cap(), base, n_lead, fields, n_rows, idx, r->mm, r->n_chunk, to_store ? 1 : 0};
    launch_fol_move(m, r->v.stream);
    hipError_t e;
    if ((e = hipGetLastError()) != hipSuccess || (e = hipStreamSynchronize(r->v.stream)) != hipSuccess)
        return fol_hip_fail(r->ctx, "fol_move_kernel", e);
    return PDEVAL_OK;
}

// the buffers of a link pass over n rows; the edge buffer holds at least `edges` pairs
int reg_link_scratch(pdeval_fol_registry* r, int64_t n, int64_t edges) {
    if (!r->d_cls.reserve(n) || !r->d_lim.reserve(n))
        return fol_fail(r->ctx, PDEVAL_ERR_ALLOC, "pdeval_fol_registry: cannot allocate the link pass's row buffers");
    if (!r->d_count.reserve(1))
        return fol_fail(r->ctx, PDEVAL_ERR_ALLOC, "pdeval_fol_registry: cannot allocate the edge counter");
    if (edges > r->edge_cap()) {
        const int64_t cap = fol_next_capacity(r->edge_cap(), edges);
        if (!r->d_edges.reserve(2 * cap))
            return fol_fail(r->ctx, PDEVAL_ERR_ALLOC,
                            ("pdeval_fol_registry: cannot allocate an edge buffer of " + std::to_string(cap) + " pairs").c_str());
    }
    return PDEVAL_OK;
}

// The link pass over the rows d_fields with the classes r->cls32 and the limits r->lim32 against
// the store's leaders [0, L) (the book may still hold fewer: a batch is linked before it is
// committed, so that a failure here leaves classes and components as they were).  Leaves the
// planned links in r->merged / r->fresh; nothing of the book has changed.
int reg_link(pdeval_fol_registry* r, const double* d_fields, int64_t n, int64_t L) {
    pdeval_ctx* c = r->ctx;
    const hipStream_t s = r->v.stream;
    r->link_ms = 0.0;
    r->edges.clear();
    if (L > INT32_MAX) return fol_fail(c, PDEVAL_ERR_ARG, "pdeval_fol_registry: the link pass holds class ids in 32 bits");
    if (!FolBook::link_rows_ok(r->cls32.data(), r->lim32.data(), n, L))
        return fol_fail(c, PDEVAL_ERR_ARG, "pdeval_fol_registry: a class id or a scan limit of the link pass outside the registry");
    if (n > 0 && L > 1) {
        int rc = reg_link_scratch(r, n, std::max<int64_t>(r->edge_hint, 1));
        if (rc != PDEVAL_OK) return rc;
        hipError_t e;
        if ((e = hipMemcpyAsync(r->d_cls.p, r->cls32.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, s)) != hipSuccess ||
            (e = hipMemcpyAsync(r->d_lim.p, r->lim32.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, s)) != hipSuccess)
            return fol_hip_fail(c, "hipMemcpyAsync", e);
        // at most two launches: the second with a buffer that holds what the first counted
        for (int pass = 0; pass < 2; ++pass) {
            const FolLinkArgs a{reg_scan_args(r, d_fields, n, L), r->d_cls.p, r->d_lim.p, r->d_edges.p, r->edge_cap(),
                                r->d_count.p};
            if ((e = hipMemsetAsync(r->d_count.p, 0, sizeof(unsigned long long), s)) != hipSuccess)
                return fol_hip_fail(c, "hipMemsetAsync", e);
            (void)hipEventRecord(r->ev.e[2], s);
            launch_fol_link(a, s);
            if ((e = hipGetLastError()) != hipSuccess) return fol_hip_fail(c, "fol_link_kernel", e);
            (void)hipEventRecord(r->ev.e[3], s);
            unsigned long long count = 0;
            if ((e = hipMemcpyAsync(&count, r->d_count.p, sizeof(count), hipMemcpyDeviceToHost, s)) != hipSuccess)
                return fol_hip_fail(c, "hipMemcpyAsync", e);
            if ((e = hipStreamSynchronize(s)) != hipSuccess) return fol_hip_fail(c, "fol_link_kernel", e);
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, r->ev.e[2], r->ev.e[3]) != hipSuccess) (void)hipGetLastError();
            else r->link_ms += ms;
            // (a row yields at most one edge per leader other than its own)
            if (count > (unsigned long long)n * (unsigned long long)(L - 1))
                return fol_fail(c, PDEVAL_ERR_HIP, "pdeval_fol_registry: fol_link_kernel counted more edges than pairs");
            if ((int64_t)count > r->edge_cap()) {
                if (pass == 1)
                    return fol_fail(c, PDEVAL_ERR_HIP, "pdeval_fol_registry: fol_link_kernel counted more edges the second time");
                if ((rc = reg_link_scratch(r, n, (int64_t)count)) != PDEVAL_OK) return rc;
                continue;
            }
            try {
                r->edges.resize((size_t)count * 2);
            } catch (const std::bad_alloc&) {
                return fol_fail(c, PDEVAL_ERR_ALLOC, "pdeval_fol_registry: cannot allocate the host copy of the edges");
            }
            if (count > 0) {
                if ((e = hipMemcpyAsync(r->edges.data(), r->d_edges.p, (size_t)count * 2 * sizeof(int32_t), hipMemcpyDeviceToHost, s)) != hipSuccess)
                    return fol_hip_fail(c, "hipMemcpyAsync", e);
                if ((e = hipStreamSynchronize(s)) != hipSuccess) return fol_hip_fail(c, "hipMemcpyAsync", e);
            }
            break;
        }
    }
    try {
        if (!r->book.plan_links(r->edges.data(), (int64_t)r->edges.size() / 2, L, r->merged, r->fresh))
            return fol_fail(c, PDEVAL_ERR_HIP, "pdeval_fol_registry: fol_link_kernel returned an edge outside the registry");
    } catch (const std::bad_alloc&) {
        return fol_fail(c, PDEVAL_ERR_ALLOC, "pdeval_fol_registry: cannot allocate the links");
    }
    return PDEVAL_OK;
}

// edges of a caller (load_links, merge_links) planned and committed; bad: the text of PDEVAL_ERR_ARG
int reg_add_links(pdeval_fol_registry* r, const int64_t* edges, int64_t n, const char* bad) {
    try {
        if (!r->book.plan_links(edges, n, r->book.n_classes(), r->merged, r->fresh))
            return fol_fail(r->ctx, PDEVAL_ERR_ARG, bad);
    } catch (const std::bad_alloc&) {
        return fol_fail(r->ctx, PDEVAL_ERR_ALLOC, "pdeval_fol_registry: cannot allocate the links");
    }
    r->book.commit_links(r->merged, r->fresh);
    return PDEVAL_OK;
}

// Stage A, Stage B and the append on the fields of a batch; d_nfin: their finite counts
int reg_assign(pdeval_fol_registry* r, const double* d_fields, const int32_t* d_nfin, int64_t n, const int64_t* keys,
               int64_t* class_id, int64_t* n_new) {
    pdeval_ctx* c = r->ctx;
    const hipStream_t s = r->v.stream;
    const int64_t L = r->book.n_classes();
    hipError_t e;
    r->first.assign((size_t)n, -1);
    r->nfin.resize((size_t)n);
    r->timed = false;
    if (L > 0) {   // Stage A: one launch and one download whatever L is
        const FolAssignArgs a{reg_scan_args(r, d_fields, n, L), d_nfin, r->d_first.p};
        (void)hipEventRecord(r->ev.e[0], s);
        launch_fol_assign(a, s);
        if ((e = hipGetLastError()) != hipSuccess) return fol_hip_fail(c, "fol_assign_kernel", e);
        (void)hipEventRecord(r->ev.e[1], s);
        r->timed = true;
        if ((e = hipMemcpyAsync(r->first.data(), r->d_first.p, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToHost, s)) != hipSuccess)
            return fol_hip_fail(c, "hipMemcpyAsync", e);
    }
    if ((e = hipMemcpyAsync(r->nfin.data(), d_nfin, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, s)) != hipSuccess)
        return fol_hip_fail(c, "hipMemcpyAsync", e);
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return fol_hip_fail(c, "fol_assign_kernel", e);
    if (!FolBook::first_ok(r->first.data(), n, L))
        return fol_fail(c, PDEVAL_ERR_HIP, "pdeval_fol_registry: fol_assign_kernel returned a leader outside the registry");
    // Stage B: the unmatched rows among themselves, by the rounds of pdeval_foliation_classes
    FolBook::stage_b_rows(r->first.data(), r->nfin.data(), n, r->prm.min_points, r->un);
    r->leader_b.assign((size_t)n, -1);
    int64_t classes = 0;
    int32_t rounds = 0;
    int rc = fol_rounds(c, d_fields, r->mm, r->prm, r->un, nullptr, r->leader_b.data(), r->d_idx.p, r->d_mask.p, s,
                        &classes, &rounds);
    if (rc != PDEVAL_OK) return rc;
    r->ids.resize((size_t)n);
    if (!r->book.plan(r->first.data(), r->leader_b.data(), n, r->ids.data(), r->new_rows) ||
        (int64_t)r->new_rows.size() != classes)
        return fol_fail(c, PDEVAL_ERR_HIP, "pdeval_fol_registry: the rounds returned a leader outside the batch");
    // the append: room first (a failure leaves the registry as it was), then the new leaders' fields
    if (classes > 0) {
        if ((rc = reg_reserve(r, L + classes)) != PDEVAL_OK) return rc;
        if ((e = hipMemcpyAsync(r->d_idx.p, r->new_rows.data(), (size_t)classes * sizeof(int64_t), hipMemcpyHostToDevice, s)) != hipSuccess)
            return fol_hip_fail(c, "hipMemcpyAsync", e);
        if ((rc = reg_move(r, L, classes, const_cast<double*>(d_fields), n, r->d_idx.p, true)) != PDEVAL_OK) return rc;
    }
    // the link pass (PDEVAL_FOL_LINK): the batch's rows, by the arrival rule, against the store as
    // the batch leaves it; planned before the commit, committed with it
    const bool link = (r->prm.flags & PDEVAL_FOL_LINK) != 0;
    if (link) {
        FolBook::arrival_limits(r->ids.data(), n, L, r->new_rows, r->cls32, r->lim32);
        if ((rc = reg_link(r, d_fields, n, L + classes)) != PDEVAL_OK) return rc;
    }
    r->book.commit(r->ids.data(), n, keys, r->new_rows);
    if (link) r->book.commit_links(r->merged, r->fresh);
    std::copy(r->ids.begin(), r->ids.end(), class_id);
    if (n_new) *n_new = classes;
    return PDEVAL_OK;
}
}  // namespace

extern "C" int pdeval_fol_registry_create(pdeval_ctx* c, const pdeval_fol_params* params, int64_t capacity_hint,
                                          pdeval_fol_registry** out) {
    FolCtx v;
    pdeval_fol_params prm;
    int rc = fol_check(c, "pdeval_fol_registry_create", nullptr, 0, nullptr, 0, 0, params, &v, &prm);
    if (rc != PDEVAL_OK) return rc;
    if (!out || capacity_hint < 0 || capacity_hint > PDEVAL_MAX_BATCH)
        return fol_fail(c, PDEVAL_ERR_ARG, "pdeval_fol_registry_create: bad argument");
    hipError_t e = hipSetDevice(v.device);
    if (e != hipSuccess) return fol_hip_fail(c, "hipSetDevice", e);
    std::unique_ptr<pdeval_fol_registry> r(new pdeval_fol_registry);   // (a failure below frees what it holds)
    r->ctx = c;
    r->v = v;
    r->prm = prm;
    r->mm = prm.m * prm.m;
    r->n_chunk = (r->mm + kFolChunk - 1) / kFolChunk;
    r->edge_hint = std::max<int64_t>(capacity_hint, kFolEdgeMin);
    if ((e = r->ev.create()) != hipSuccess) return fol_hip_fail(c, "hipEventCreate", e);
    if ((rc = reg_reserve(r.get(), std::max<int64_t>(capacity_hint, 1))) != PDEVAL_OK) return rc;
    *out = r.release();
    return PDEVAL_OK;
}

extern "C" int pdeval_fol_registry_destroy(pdeval_fol_registry* r) {
    if (!r) return PDEVAL_OK;
    (void)hipSetDevice(r->v.device);
    delete r;   // its buffers and events with it
    return PDEVAL_OK;
}

extern "C" int pdeval_fol_registry_assign_fields(pdeval_ctx* c, pdeval_fol_registry* r, const double* d_fields,
                                                 const int32_t* d_n_finite, int64_t n_rows, const int64_t* keys,
                                                 int64_t* class_id, int64_t* n_new) {
    int rc = reg_check(c, r, "pdeval_fol_registry_assign_fields");
    if (rc != PDEVAL_OK) return rc;
    if (n_new) *n_new = 0;
    if (n_rows < 0 || n_rows > PDEVAL_MAX_BATCH || (n_rows > 0 && (!d_fields || !class_id)))
        return fol_fail(c, PDEVAL_ERR_ARG, "pdeval_fol_registry_assign_fields: bad argument");
    if (n_rows == 0) return PDEVAL_OK;
    hipError_t e = hipSetDevice(r->v.device);
    if (e != hipSuccess) return fol_hip_fail(c, "hipSetDevice", e);
    if ((rc = reg_scratch(r, n_rows, false)) != PDEVAL_OK) return rc;
    if (!d_n_finite) {
        launch_fol_nfinite(d_fields, n_rows, r->mm, r->d_nfin.p, r->v.stream);
        if ((e = hipGetLastError()) != hipSuccess) return fol_hip_fail(c, "fol_nfinite_kernel", e);
        d_n_finite = r->d_nfin.p;
    }
    return reg_assign(r, d_fields, d_n_finite, n_rows, keys, class_id, n_new);
}

extern "C" int pdeval_fol_registry_assign(pdeval_ctx* c, pdeval_fol_registry* r, const int32_t* d_ops, int64_t n_words,
                                          const int64_t* d_offsets, int64_t n, const int64_t* d_list, int64_t n_list,
                                          const int64_t* keys, int64_t* class_id, int64_t* n_new) {
    int rc = reg_check(c, r, "pdeval_fol_registry_assign");
    if (rc != PDEVAL_OK) return rc;
    FolCtx v;
    pdeval_fol_params prm;
    rc = fol_check(c, "pdeval_fol_registry_assign", d_ops, n_words, d_offsets, n, n_list, &r->prm, &v, &prm);
    if (rc != PDEVAL_OK) return rc;
    if (n_new) *n_new = 0;
    if (n_list > 0 && !class_id) return fol_fail(c, PDEVAL_ERR_ARG, "pdeval_fol_registry_assign: bad argument");
    if (n_list == 0) return PDEVAL_OK;
    hipError_t e = hipSetDevice(r->v.device);
    if (e != hipSuccess) return fol_hip_fail(c, "hipSetDevice", e);
    if ((rc = reg_scratch(r, n_list, true)) != PDEVAL_OK) return rc;
    rc = fol_fields_launch(c, r->v, r->prm, d_ops, n_words, d_offsets, n, d_list, n_list, r->d_field.p, r->d_nfin.p,
                           r->v.stream);
    if (rc != PDEVAL_OK) return rc;
    return reg_assign(r, r->d_field.p, r->d_nfin.p, n_list, keys, class_id, n_new);
}

extern "C" int pdeval_fol_registry_size(pdeval_fol_registry* r, int64_t* n_classes, int64_t* n_rows_seen) {
    if (!r) return fol_fail(nullptr, PDEVAL_ERR_ARG, "pdeval_fol_registry_size: null registry");
    if (n_classes) *n_classes = r->book.n_classes();
    if (n_rows_seen) *n_rows_seen = r->book.rows_seen;
    return PDEVAL_OK;
}

extern "C" int pdeval_fol_registry_info(pdeval_fol_registry* r, pdeval_fol_params* params, double* grid,
                                        double* stage_a_ms) {
    if (!r) return fol_fail(nullptr, PDEVAL_ERR_ARG, "pdeval_fol_registry_info: null registry");
    if (params) *params = r->prm;
    if (grid) std::copy(r->v.grid, r->v.grid + 8, grid);
    if (stage_a_ms) {
        float ms = 0.f;
        if (r->timed && hipEventElapsedTime(&ms, r->ev.e[0], r->ev.e[1]) != hipSuccess) {
            (void)hipGetLastError();
            ms = 0.f;
        }
        *stage_a_ms = ms;
    }
    return PDEVAL_OK;
}

extern "C" int pdeval_fol_registry_leaders(pdeval_fol_registry* r, double* d_fields, int64_t* leader_keys,
                                           int64_t* sizes) {
    if (!r) return fol_fail(nullptr, PDEVAL_ERR_ARG, "pdeval_fol_registry_leaders: null registry");
    const int64_t L = r->book.n_classes();
    if (leader_keys) std::copy(r->book.keys.begin(), r->book.keys.end(), leader_keys);
    if (sizes) std::copy(r->book.sizes.begin(), r->book.sizes.end(), sizes);
    if (!d_fields || L == 0) return PDEVAL_OK;
    hipError_t e = hipSetDevice(r->v.device);
    if (e != hipSuccess) return fol_hip_fail(r->ctx, "hipSetDevice", e);
    return reg_move(r, 0, L, d_fields, L, nullptr, false);
}

extern "C" int pdeval_fol_registry_kinds(pdeval_fol_registry* r, uint8_t* kinds) {
    if (!r) return fol_fail(nullptr, PDEVAL_ERR_ARG, "pdeval_fol_registry_kinds: null registry");
    pdeval_ctx* c = r->ctx;
    const int64_t L = r->book.n_classes();
    if (L == 0) return PDEVAL_OK;
    if (!kinds) return fol_fail(c, PDEVAL_ERR_ARG, "pdeval_fol_registry_kinds: bad argument");
    hipError_t e = hipSetDevice(r->v.device);
    if (e != hipSuccess) return fol_hip_fail(c, "hipSetDevice", e);
    DevBuf<uint8_t> d_kind;
    if (!d_kind.reserve(L))
        return fol_fail(c, PDEVAL_ERR_ALLOC, "pdeval_fol_registry_kinds: cannot allocate the kinds");
    FolKindArgs a{};
    a.fields = r->d_store.p;   // the leaders where they are: chunk-major (fol_store_at)
    a.n_rows = L;
    a.cap = r->cap();
    a.mm = r->mm;
    a.n_chunk = r->n_chunk;
    a.min_points = r->prm.min_points;
    a.kind = d_kind.p;
    launch_fol_kind(a, r->v.stream);
    if ((e = hipGetLastError()) == hipSuccess)
        e = hipMemcpyAsync(kinds, d_kind.p, (size_t)L, hipMemcpyDeviceToHost, r->v.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(r->v.stream);
    if (e != hipSuccess) return fol_hip_fail(c, "fol_kind_kernel", e);
    return PDEVAL_OK;
}

extern "C" int pdeval_fol_registry_load(pdeval_ctx* c, pdeval_fol_registry* r, const double* d_fields,
                                        const int64_t* leader_keys, const int64_t* sizes, int64_t n_classes) {
    int rc = reg_check(c, r, "pdeval_fol_registry_load");
    if (rc != PDEVAL_OK) return rc;
    if (r->book.n_classes() != 0 || r->book.rows_seen != 0)
        return fol_fail(c, PDEVAL_ERR_ARG, "pdeval_fol_registry_load: the registry is not empty");
    if (n_classes < 0 || n_classes > PDEVAL_MAX_BATCH || (n_classes > 0 && (!d_fields || !leader_keys || !sizes)))
        return fol_fail(c, PDEVAL_ERR_ARG, "pdeval_fol_registry_load: bad argument");
    for (int64_t k = 0; k < n_classes; ++k)
        if (sizes[k] < 0) return fol_fail(c, PDEVAL_ERR_ARG, "pdeval_fol_registry_load: a negative class size");
    if (n_classes == 0) return PDEVAL_OK;
    hipError_t e = hipSetDevice(r->v.device);
    if (e != hipSuccess) return fol_hip_fail(c, "hipSetDevice", e);
    if ((rc = reg_reserve(r, n_classes)) != PDEVAL_OK) return rc;
    if ((rc = reg_move(r, 0, n_classes, const_cast<double*>(d_fields), n_classes, nullptr, true)) != PDEVAL_OK) return rc;
    r->book.load(leader_keys, sizes, n_classes);
    return PDEVAL_OK;
}

extern "C" int pdeval_fol_registry_add_sizes(pdeval_fol_registry* r, const int64_t* class_id, const int64_t* count,
                                             int64_t n) {
    if (!r) return fol_fail(nullptr, PDEVAL_ERR_ARG, "pdeval_fol_registry_add_sizes: null registry");
    if (n < 0 || (n > 0 && (!class_id || !count)) || !r->book.add_sizes(class_id, count, n))
        return fol_fail(r->ctx, PDEVAL_ERR_ARG, "pdeval_fol_registry_add_sizes: bad argument (a class outside the registry or a negative count)");
    return PDEVAL_OK;
}

extern "C" int pdeval_fol_registry_link_fields(pdeval_ctx* c, pdeval_fol_registry* r, const double* d_fields,
                                               const int64_t* class_id, int64_t n_rows, int64_t* n_new_links) {
    int rc = reg_check(c, r, "pdeval_fol_registry_link_fields");
    if (rc != PDEVAL_OK) return rc;
    if (n_new_links) *n_new_links = 0;
    if (n_rows < 0 || n_rows > PDEVAL_MAX_BATCH || (n_rows > 0 && (!d_fields || !class_id)))
        return fol_fail(c, PDEVAL_ERR_ARG, "pdeval_fol_registry_link_fields: bad argument");
    const int64_t L = r->book.n_classes();
    for (int64_t k = 0; k < n_rows; ++k)
        if (class_id[k] < -1 || class_id[k] >= L)
            return fol_fail(c, PDEVAL_ERR_ARG, "pdeval_fol_registry_link_fields: a class id outside [-1, n_classes)");
    if (n_rows == 0) return PDEVAL_OK;
    hipError_t e = hipSetDevice(r->v.device);
    if (e != hipSuccess) return fol_hip_fail(c, "hipSetDevice", e);
    r->cls32.resize((size_t)n_rows);
    r->lim32.resize((size_t)n_rows);
    for (int64_t k = 0; k < n_rows; ++k) {
        r->cls32[(size_t)k] = (int32_t)class_id[k];
        r->lim32[(size_t)k] = class_id[k] < 0 ? 0 : (int32_t)std::min<int64_t>(L, INT32_MAX);
    }
    if ((rc = reg_link(r, d_fields, n_rows, L)) != PDEVAL_OK) return rc;
    if (n_new_links) *n_new_links = (int64_t)r->fresh.size();
    r->book.commit_links(r->merged, r->fresh);
    return PDEVAL_OK;
}

extern "C" int pdeval_fol_registry_components(pdeval_fol_registry* r, int64_t* component, int64_t* n_components,
                                              int64_t* n_links) {
    if (!r) return fol_fail(nullptr, PDEVAL_ERR_ARG, "pdeval_fol_registry_components: null registry");
    const int64_t L = r->book.n_classes();
    for (int64_t k = 0; component && k < L; ++k) component[k] = r->book.component(k);
    if (n_components) *n_components = r->book.n_components();
    if (n_links) *n_links = (int64_t)r->book.links.size();
    return PDEVAL_OK;
}

extern "C" int pdeval_fol_registry_links(pdeval_fol_registry* r, int64_t* edges) {
    if (!r) return fol_fail(nullptr, PDEVAL_ERR_ARG, "pdeval_fol_registry_links: null registry");
    if (!edges && !r->book.links.empty())
        return fol_fail(r->ctx, PDEVAL_ERR_ARG, "pdeval_fol_registry_links: bad argument");
    for (size_t k = 0; k < r->book.links.size(); ++k) {
        edges[2 * k] = r->book.links[k].first;
        edges[2 * k + 1] = r->book.links[k].second;
    }
    return PDEVAL_OK;
}

extern "C" int pdeval_fol_registry_load_links(pdeval_fol_registry* r, const int64_t* edges, int64_t n) {
    if (!r) return fol_fail(nullptr, PDEVAL_ERR_ARG, "pdeval_fol_registry_load_links: null registry");
    if (n < 0 || (n > 0 && !edges)) return fol_fail(r->ctx, PDEVAL_ERR_ARG, "pdeval_fol_registry_load_links: bad argument");
    return reg_add_links(r, edges, n,
                         "pdeval_fol_registry_load_links: an edge with an end outside [0, n_classes) or with equal ends");
}

extern "C" int pdeval_fol_registry_merge_links(pdeval_fol_registry* r, const int64_t* edges, int64_t n,
                                               const int64_t* id_map, int64_t n_map) {
    if (!r) return fol_fail(nullptr, PDEVAL_ERR_ARG, "pdeval_fol_registry_merge_links: null registry");
    if (n < 0 || n_map < 0 || (n > 0 && (!edges || !id_map)))
        return fol_fail(r->ctx, PDEVAL_ERR_ARG, "pdeval_fol_registry_merge_links: bad argument");
    std::vector<int64_t> mapped;
    try {
        if (!FolBook::map_links(edges, n, id_map, n_map, mapped))
            return fol_fail(r->ctx, PDEVAL_ERR_ARG,
                            "pdeval_fol_registry_merge_links: an edge with an end outside [0, n_map) or with equal ends");
    } catch (const std::bad_alloc&) {
        return fol_fail(r->ctx, PDEVAL_ERR_ALLOC, "pdeval_fol_registry: cannot allocate the links");
    }
    return reg_add_links(r, mapped.data(), (int64_t)mapped.size() / 2,
                         "pdeval_fol_registry_merge_links: the id map names a class outside [0, n_classes)");
}

extern "C" int pdeval_fol_registry_link_ms(pdeval_fol_registry* r, double* link_ms) {
    if (!r) return fol_fail(nullptr, PDEVAL_ERR_ARG, "pdeval_fol_registry_link_ms: null registry");
    if (link_ms) *link_ms = r->link_ms;
    return PDEVAL_OK;
}

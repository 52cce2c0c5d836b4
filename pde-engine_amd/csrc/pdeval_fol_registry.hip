// pdeval_fol_registry.hip -- the foliation class registry (DESIGN.md §14 "Registry"): the leaders'
// gradient fields resident on the device across batches, fol_assign_kernel (Stage A: each row's
// first match among them in one launch), fol_link_kernel (the link pass: every other leader a
// row matches, "Links and components"), the store's append / export kernel and the
// pdeval_fol_registry_* entry points.  Stage B and the fields reuse pdeval_foliation.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <new>
#include <string>
#include <vector>

#include "../../include/pdeval.h"
#include "pdeval_fol_book.h"
#include "pdeval_foliation.h"

namespace pd {

// Stage A.  One wave per row, four rows per 256-thread block; lanes are sample points.  The
// leaders are walked in creation order in tiles of T = kFolAssignTile: the block copies the
// tile's first chunks (T x 1 KiB, contiguous in the chunk-major store) into LDS, the next tile
// travelling in registers meanwhile, and each of its waves tests its row against them from
// there, so a leader's screening chunk leaves L2 once per four rows.  A pair is left at its
// first chunk with a bad point -- almost always the first -- and only a pair that survives
// reads the leader's later chunks, straight from global memory.  REG (m <= 16): the row's whole
// field, at most 4 chunks x 2 doubles per lane, stays in registers for the scan; otherwise
// only its first chunk does and the later ones are re-read per surviving pair.  Counts are
// ballots into wave-uniform counters; a row is finished at its first match and a block when
// its four rows are.  The only indices read are row < n_rows and leader < L, both loop bounds.
// AXIS: the chunk test with the axis rule (PDEVAL_FOL_AXIS); AXIS = false is the kernel as it was.
template <bool REG, bool AXIS>
__global__ __launch_bounds__(256) void fol_assign_kernel(FolAssignArgs a) {
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
    // (a row with fewer finite points than a match needs usable ones matches nothing)
    bool done = !in_batch;
    if (in_batch && a.n_finite) done = __builtin_amdgcn_readfirstlane((int)(a.n_finite[row] < a.min_points)) != 0;
    double fa[NR], fb[NR];
#pragma unroll
    for (int c = 0; c < NR; ++c) {
        const int p = c * kFolChunk + lane;
        const int pc = p < mm ? p : mm - 1;
        fa[c] = p < mm ? ra[pc] : nan;
        fb[c] = p < mm ? ra[mm + pc] : nan;
    }
    const int64_t L = a.L;
    double2 pf[kPf];
    auto fetch = [&](int64_t t0) {
        const int64_t n2 = (L - t0 < T ? L - t0 : T) * kFolChunk;   // double2 of the tile's leaders
        const double2* src = (const double2*)(a.store + fol_store_at(a.cap, 0, t0));
#pragma unroll
        for (int i = 0; i < kPf; ++i) {
            const int j = (int)threadIdx.x + 256 * i;
            pf[i] = j < n2 ? src[j] : double2{nan, nan};
        }
    };
    int64_t first = -1;
    if (L > 0) fetch(0);
    for (int64_t t0 = 0; t0 < L; t0 += T) {
#pragma unroll
        for (int i = 0; i < kPf; ++i) tile2[(int)threadIdx.x + 256 * i] = pf[i];
        __syncthreads();
        if (t0 + T < L) fetch(t0 + T);
        if (!done) {
            const int tn = L - t0 < T ? (int)(L - t0) : T;
            for (int k = 0; k < tn; ++k) {
                const double* q0 = tile + k * 2 * kFolChunk;
                FolCount n{0, 0};
                fol_chunk_test<AXIS>(fa[0], fb[0], q0[lane], q0[kFolChunk + lane], lane < mm, a.tau, n);
                if (n.nb) continue;
                const int64_t l = t0 + k;
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
                    first = l;
                    done = true;
                    break;
                }
            }
        }
        // (also the barrier between this tile's readers and the next tile's writers)
        if (__syncthreads_and(done)) break;
    }
    if (lane == 0 && in_batch) a.first[row] = first;
}

void launch_fol_assign(const FolAssignArgs& a, hipStream_t s) {
    const dim3 grid((unsigned)((a.n_rows + 3) / 4)), block(256);
    const bool reg = a.n_chunk <= kFolRegChunks, axis = (a.flags & PDEVAL_FOL_AXIS) != 0;
    if (reg && !axis) hipLaunchKernelGGL((fol_assign_kernel<true, false>), grid, block, 0, s, a);
    else if (!reg && !axis) hipLaunchKernelGGL((fol_assign_kernel<false, false>), grid, block, 0, s, a);
    else if (reg) hipLaunchKernelGGL((fol_assign_kernel<true, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((fol_assign_kernel<false, true>), grid, block, 0, s, a);
}

// The link pass (DESIGN.md §14 "Links and components").  The shape of Stage A -- one wave per
// row, four rows per block, the leaders' first chunks in LDS tiles of T, REG at m <= 16, a pair
// left at its first bad chunk -- with these differences: a row does not stop at a match, it scans
// the leaders [0, lim[row]) and skips its own class cls[row], and for every match lane 0 appends
// the pair (cls[row], leader) to the edge buffer, the slot taken by an atomic add on a device
// counter; an edge past the buffer's capacity is counted and not stored (the host grows the
// buffer and repeats the launch).  A row with cls[row] < 0 scans nothing.  The block walks the
// tiles below the largest lim of its four rows, so the only indices read are row < n_rows and
// leader < max lim <= L; the host checks lim and cls before the launch.  Edge order is
// whatever the atomics give; the components do not depend on it.
template <bool REG, bool AXIS>
__global__ __launch_bounds__(256) void fol_link_kernel(FolLinkArgs a) {
    constexpr int T = kFolAssignTile, NR = REG ? kFolRegChunks : 1;
    constexpr int kPf = T * 2 * kFolChunk / 2 / 256;   // double2 per thread and tile
    __shared__ double2 tile2[T * kFolChunk];
    __shared__ int s_lim[4];
    const double* tile = (const double*)tile2;
    const int lane = threadIdx.x & 63;
    const int wib = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t row = (int64_t)blockIdx.x * 4 + wib;
    const int mm = a.mm;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    const bool in_batch = row < a.n_rows;
    const double* ra = a.rows + (in_batch ? row : 0) * 2 * (int64_t)mm;
    const int own = in_batch ? __builtin_amdgcn_readfirstlane(a.cls[row]) : -1;
    const int lim = own >= 0 ? __builtin_amdgcn_readfirstlane(a.lim[row]) : 0;
    if (lane == 0) s_lim[wib] = lim;
    double fa[NR], fb[NR];
#pragma unroll
    for (int c = 0; c < NR; ++c) {
        const int p = c * kFolChunk + lane;
        const int pc = p < mm ? p : mm - 1;
        fa[c] = p < mm ? ra[pc] : nan;
        fb[c] = p < mm ? ra[mm + pc] : nan;
    }
    __syncthreads();
    const int top = max(max(s_lim[0], s_lim[1]), max(s_lim[2], s_lim[3]));   // block-uniform, <= L
    double2 pf[kPf];
    auto fetch = [&](int t0) {
        const int n2 = (top - t0 < T ? top - t0 : T) * kFolChunk;   // double2 of the tile's leaders
        const double2* src = (const double2*)(a.store + fol_store_at(a.cap, 0, t0));
#pragma unroll
        for (int i = 0; i < kPf; ++i) {
            const int j = (int)threadIdx.x + 256 * i;
            pf[i] = j < n2 ? src[j] : double2{nan, nan};
        }
    };
    if (top > 0) fetch(0);
    for (int t0 = 0; t0 < top; t0 += T) {
#pragma unroll
        for (int i = 0; i < kPf; ++i) tile2[(int)threadIdx.x + 256 * i] = pf[i];
        __syncthreads();
        if (t0 + T < top) fetch(t0 + T);
        const int tn = lim - t0 < T ? lim - t0 : T;   // (<= 0 for a row whose leaders end before this tile)
        for (int k = 0; k < tn; ++k) {
            const int l = t0 + k;
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
            if (n.nu >= a.min_points && n.nb == 0 && lane == 0) {
                const unsigned long long slot = atomicAdd(a.count, 1ull);
                if (slot < (unsigned long long)a.ecap) {
                    a.edges[2 * slot] = own;
                    a.edges[2 * slot + 1] = l;
                }
            }
        }
        __syncthreads();   // this tile's readers before the next tile's writers
    }
}

void launch_fol_link(const FolLinkArgs& a, hipStream_t s) {
    const dim3 grid((unsigned)((a.n_rows + 3) / 4)), block(256);
    const bool reg = a.n_chunk <= kFolRegChunks, axis = (a.flags & PDEVAL_FOL_AXIS) != 0;
    if (reg && !axis) hipLaunchKernelGGL((fol_link_kernel<true, false>), grid, block, 0, s, a);
    else if (!reg && !axis) hipLaunchKernelGGL((fol_link_kernel<false, false>), grid, block, 0, s, a);
    else if (reg) hipLaunchKernelGGL((fol_link_kernel<true, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((fol_link_kernel<false, true>), grid, block, 0, s, a);
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

// A registry: bound to one context and one parameter set.  The leader store and the scratch of
// a batch belong to it and are reused between calls.
struct pdeval_fol_registry {
    pdeval_ctx* ctx = nullptr;
    FolCtx v{};
    pdeval_fol_params prm{};
    int mm = 0, n_chunk = 0;
    double* d_store = nullptr;   // chunk-major, cap leaders (fol_store_at)
    int64_t cap = 0;
    FolBook book;
    // scratch of a batch, batch_cap rows: Stage A's first[], the finite counts, Stage B's indices and masks
    int64_t batch_cap = 0;
    int64_t* d_first = nullptr;
    int32_t* d_nfin = nullptr;
    int64_t* d_idx = nullptr;
    uint32_t* d_mask = nullptr;
    // the fields of a batch of programs, field_cap rows (pdeval_fol_registry_assign)
    int64_t field_cap = 0;
    double* d_field = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;   // around Stage A's launch
    bool timed = false;
    // the link pass (PDEVAL_FOL_LINK, pdeval_fol_registry_link_fields): the rows' classes and scan
    // limits, link_cap rows; the edge buffer, edge_cap pairs, and its counter; allocated at first use
    int64_t link_cap = 0, edge_cap = 0, edge_hint = 0;
    int32_t* d_cls = nullptr;
    int32_t* d_lim = nullptr;
    int32_t* d_edges = nullptr;
    unsigned long long* d_count = nullptr;
    hipEvent_t e2 = nullptr, e3 = nullptr;   // around each launch of the link kernel
    double link_ms = 0.0;                    // their sum over the most recent call
    std::vector<int32_t> cls32, lim32, edges;
    std::vector<FolBook::Link> merged, fresh;
    // host buffers of a batch, reused
    std::vector<int64_t> first, leader_b, un, new_rows, ids;
    std::vector<int32_t> nfin;
};

namespace {
size_t store_bytes(const pdeval_fol_registry* r, int64_t cap) {
    return (size_t)cap * (size_t)r->n_chunk * 2 * kFolChunk * sizeof(double);
}

// the store holds `need` leaders: doubling, outside any kernel (new allocation, one
// device-to-device copy per chunk plane, free); on failure nothing has changed
int reg_reserve(pdeval_fol_registry* r, int64_t need) {
    if (need <= r->cap) return PDEVAL_OK;
    const int64_t cap = fol_next_capacity(r->cap, need);
    double* d_new = nullptr;
    if (hipMalloc((void**)&d_new, store_bytes(r, cap)) != hipSuccess) {
        (void)hipGetLastError();
        return fol_fail(r->ctx, PDEVAL_ERR_ALLOC,
                        ("pdeval_fol_registry: cannot allocate " + std::to_string(store_bytes(r, cap)) +
                         " bytes of leader fields (capacity x chunks x 1 KiB)").c_str());
    }
    const int64_t L = r->book.n_classes();
    hipError_t e = hipSuccess;
    for (int c = 0; c < r->n_chunk && L > 0 && e == hipSuccess; ++c)
        e = hipMemcpyAsync(d_new + fol_store_at(cap, c, 0), r->d_store + fol_store_at(r->cap, c, 0),
                           (size_t)L * 2 * kFolChunk * sizeof(double), hipMemcpyDeviceToDevice, r->v.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(r->v.stream);
    if (e != hipSuccess) {
        (void)hipFree(d_new);
        return fol_hip_fail(r->ctx, "hipMemcpyAsync", e);
    }
    (void)hipFree(r->d_store);
    r->d_store = d_new;
    r->cap = cap;
    return PDEVAL_OK;
}

// the scratch of a batch of n rows (and, with_field, its fields): hipMalloc only when a batch
// outgrows what is there
int reg_scratch(pdeval_fol_registry* r, int64_t n, bool with_field) {
    if (n > r->batch_cap) {
        int64_t* d_first = nullptr;
        int32_t* d_nfin = nullptr;
        int64_t* d_idx = nullptr;
        uint32_t* d_mask = nullptr;
        if (hipMalloc((void**)&d_first, (size_t)n * sizeof(int64_t)) != hipSuccess ||
            hipMalloc((void**)&d_nfin, (size_t)n * sizeof(int32_t)) != hipSuccess ||
            hipMalloc((void**)&d_idx, (size_t)n * sizeof(int64_t)) != hipSuccess ||
            hipMalloc((void**)&d_mask, (size_t)n * sizeof(uint32_t)) != hipSuccess) {
            (void)hipGetLastError();
            (void)hipFree(d_first);
            (void)hipFree(d_nfin);
            (void)hipFree(d_idx);
            (void)hipFree(d_mask);
            return fol_fail(r->ctx, PDEVAL_ERR_ALLOC, "pdeval_fol_registry: cannot allocate the batch buffers");
        }
        (void)hipFree(r->d_first);
        (void)hipFree(r->d_nfin);
        (void)hipFree(r->d_idx);
        (void)hipFree(r->d_mask);
        r->d_first = d_first;
        r->d_nfin = d_nfin;
        r->d_idx = d_idx;
        r->d_mask = d_mask;
        r->batch_cap = n;
    }
    if (with_field && n > r->field_cap) {
        double* d_field = nullptr;
        const size_t bytes = (size_t)n * 2 * (size_t)r->mm * sizeof(double);
        if (hipMalloc((void**)&d_field, bytes) != hipSuccess) {
            (void)hipGetLastError();
            return fol_fail(r->ctx, PDEVAL_ERR_ALLOC,
                            ("pdeval_fol_registry_assign: cannot allocate " + std::to_string(bytes) +
                             " bytes of gradient fields (n_list x 2 m^2 x 8): assign a shorter list or a smaller m")
                                .c_str());
        }
        (void)hipFree(r->d_field);
        r->d_field = d_field;
        r->field_cap = n;
    }
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

void reg_move_args(const pdeval_fol_registry* r, FolMoveArgs* a) {
    a->store = r->d_store;
    a->cap = r->cap;
    a->mm = r->mm;
    a->n_chunk = r->n_chunk;
}

// the buffers of a link pass over n rows; the edge buffer holds at least `edges` pairs
int reg_link_scratch(pdeval_fol_registry* r, int64_t n, int64_t edges) {
    if (n > r->link_cap) {
        int32_t* d_cls = nullptr;
        int32_t* d_lim = nullptr;
        if (hipMalloc((void**)&d_cls, (size_t)n * sizeof(int32_t)) != hipSuccess ||
            hipMalloc((void**)&d_lim, (size_t)n * sizeof(int32_t)) != hipSuccess) {
            (void)hipGetLastError();
            (void)hipFree(d_cls);
            return fol_fail(r->ctx, PDEVAL_ERR_ALLOC, "pdeval_fol_registry: cannot allocate the link pass's row buffers");
        }
        (void)hipFree(r->d_cls);
        (void)hipFree(r->d_lim);
        r->d_cls = d_cls;
        r->d_lim = d_lim;
        r->link_cap = n;
    }
    if (!r->d_count && hipMalloc((void**)&r->d_count, sizeof(unsigned long long)) != hipSuccess) {
        (void)hipGetLastError();
        r->d_count = nullptr;
        return fol_fail(r->ctx, PDEVAL_ERR_ALLOC, "pdeval_fol_registry: cannot allocate the edge counter");
    }
    if (edges > r->edge_cap) {
        const int64_t cap = fol_next_capacity(r->edge_cap, edges);
        int32_t* d_edges = nullptr;
        if (hipMalloc((void**)&d_edges, (size_t)cap * 2 * sizeof(int32_t)) != hipSuccess) {
            (void)hipGetLastError();
            return fol_fail(r->ctx, PDEVAL_ERR_ALLOC,
                            ("pdeval_fol_registry: cannot allocate an edge buffer of " + std::to_string(cap) + " pairs").c_str());
        }
        (void)hipFree(r->d_edges);
        r->d_edges = d_edges;
        r->edge_cap = cap;
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
        if ((e = hipMemcpyAsync(r->d_cls, r->cls32.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, s)) != hipSuccess ||
            (e = hipMemcpyAsync(r->d_lim, r->lim32.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, s)) != hipSuccess)
            return fol_hip_fail(c, "hipMemcpyAsync", e);
        // at most two launches: the second with a buffer that holds what the first counted
        for (int pass = 0; pass < 2; ++pass) {
            FolLinkArgs a{};
            a.rows = d_fields;
            a.n_rows = n;
            a.cls = r->d_cls;
            a.lim = r->d_lim;
            a.store = r->d_store;
            a.cap = r->cap;
            a.L = L;
            a.mm = r->mm;
            a.n_chunk = r->n_chunk;
            a.tau = r->prm.tau;
            a.min_points = r->prm.min_points;
            a.edges = r->d_edges;
            a.ecap = r->edge_cap;
            a.count = r->d_count;
            a.flags = (uint32_t)r->prm.flags;
            if ((e = hipMemsetAsync(r->d_count, 0, sizeof(unsigned long long), s)) != hipSuccess)
                return fol_hip_fail(c, "hipMemsetAsync", e);
            (void)hipEventRecord(r->e2, s);
            launch_fol_link(a, s);
            if ((e = hipGetLastError()) != hipSuccess) return fol_hip_fail(c, "fol_link_kernel", e);
            (void)hipEventRecord(r->e3, s);
            unsigned long long count = 0;
            if ((e = hipMemcpyAsync(&count, r->d_count, sizeof(count), hipMemcpyDeviceToHost, s)) != hipSuccess)
                return fol_hip_fail(c, "hipMemcpyAsync", e);
            if ((e = hipStreamSynchronize(s)) != hipSuccess) return fol_hip_fail(c, "fol_link_kernel", e);
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, r->e2, r->e3) != hipSuccess) (void)hipGetLastError();
            else r->link_ms += ms;
            // (a row yields at most one edge per leader other than its own)
            if (count > (unsigned long long)n * (unsigned long long)(L - 1))
                return fol_fail(c, PDEVAL_ERR_HIP, "pdeval_fol_registry: fol_link_kernel counted more edges than pairs");
            if ((int64_t)count > r->edge_cap) {
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
                if ((e = hipMemcpyAsync(r->edges.data(), r->d_edges, (size_t)count * 2 * sizeof(int32_t), hipMemcpyDeviceToHost, s)) != hipSuccess)
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
        FolAssignArgs a{};
        a.rows = d_fields;
        a.n_rows = n;
        a.n_finite = d_nfin;
        a.store = r->d_store;
        a.cap = r->cap;
        a.L = L;
        a.mm = r->mm;
        a.n_chunk = r->n_chunk;
        a.tau = r->prm.tau;
        a.min_points = r->prm.min_points;
        a.first = r->d_first;
        a.flags = (uint32_t)r->prm.flags;
        (void)hipEventRecord(r->e0, s);
        launch_fol_assign(a, s);
        if ((e = hipGetLastError()) != hipSuccess) return fol_hip_fail(c, "fol_assign_kernel", e);
        (void)hipEventRecord(r->e1, s);
        r->timed = true;
        if ((e = hipMemcpyAsync(r->first.data(), r->d_first, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToHost, s)) != hipSuccess)
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
    int rc = fol_rounds(c, d_fields, r->mm, r->prm, r->un, nullptr, r->leader_b.data(), r->d_idx, r->d_mask, s,
                        &classes, &rounds);
    if (rc != PDEVAL_OK) return rc;
    r->ids.resize((size_t)n);
    if (!r->book.plan(r->first.data(), r->leader_b.data(), n, r->ids.data(), r->new_rows) ||
        (int64_t)r->new_rows.size() != classes)
        return fol_fail(c, PDEVAL_ERR_HIP, "pdeval_fol_registry: the rounds returned a leader outside the batch");
    // the append: room first (a failure leaves the registry as it was), then the new leaders' fields
    if (classes > 0) {
        if ((rc = reg_reserve(r, L + classes)) != PDEVAL_OK) return rc;
        if ((e = hipMemcpyAsync(r->d_idx, r->new_rows.data(), (size_t)classes * sizeof(int64_t), hipMemcpyHostToDevice, s)) != hipSuccess)
            return fol_hip_fail(c, "hipMemcpyAsync", e);
        FolMoveArgs m{};
        reg_move_args(r, &m);
        m.base = L;
        m.n_lead = classes;
        m.fields = const_cast<double*>(d_fields);
        m.n_rows = n;
        m.idx = r->d_idx;
        m.to_store = 1;
        launch_fol_move(m, s);
        if ((e = hipGetLastError()) != hipSuccess) return fol_hip_fail(c, "fol_move_kernel", e);
        if ((e = hipStreamSynchronize(s)) != hipSuccess) return fol_hip_fail(c, "fol_move_kernel", e);
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
    pdeval_fol_registry* r = new pdeval_fol_registry;
    r->ctx = c;
    r->v = v;
    r->prm = prm;
    r->mm = prm.m * prm.m;
    r->n_chunk = (r->mm + kFolChunk - 1) / kFolChunk;
    r->edge_hint = std::max<int64_t>(capacity_hint, kFolEdgeMin);
    if ((e = hipEventCreate(&r->e0)) != hipSuccess || (e = hipEventCreate(&r->e1)) != hipSuccess ||
        (e = hipEventCreate(&r->e2)) != hipSuccess || (e = hipEventCreate(&r->e3)) != hipSuccess) {
        if (r->e0) (void)hipEventDestroy(r->e0);
        if (r->e1) (void)hipEventDestroy(r->e1);
        if (r->e2) (void)hipEventDestroy(r->e2);
        delete r;
        return fol_hip_fail(c, "hipEventCreate", e);
    }
    if ((rc = reg_reserve(r, std::max<int64_t>(capacity_hint, 1))) != PDEVAL_OK) {
        (void)hipEventDestroy(r->e0);
        (void)hipEventDestroy(r->e1);
        (void)hipEventDestroy(r->e2);
        (void)hipEventDestroy(r->e3);
        delete r;
        return rc;
    }
    *out = r;
    return PDEVAL_OK;
}

extern "C" int pdeval_fol_registry_destroy(pdeval_fol_registry* r) {
    if (!r) return PDEVAL_OK;
    (void)hipSetDevice(r->v.device);
    (void)hipFree(r->d_store);
    (void)hipFree(r->d_first);
    (void)hipFree(r->d_nfin);
    (void)hipFree(r->d_idx);
    (void)hipFree(r->d_mask);
    (void)hipFree(r->d_field);
    (void)hipFree(r->d_cls);
    (void)hipFree(r->d_lim);
    (void)hipFree(r->d_edges);
    (void)hipFree(r->d_count);
    (void)hipEventDestroy(r->e0);
    (void)hipEventDestroy(r->e1);
    (void)hipEventDestroy(r->e2);
    (void)hipEventDestroy(r->e3);
    delete r;
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
        launch_fol_nfinite(d_fields, n_rows, r->mm, r->d_nfin, r->v.stream);
        if ((e = hipGetLastError()) != hipSuccess) return fol_hip_fail(c, "fol_nfinite_kernel", e);
        d_n_finite = r->d_nfin;
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
    rc = fol_fields_launch(c, r->v, r->prm, d_ops, n_words, d_offsets, n, d_list, n_list, r->d_field, r->d_nfin,
                           r->v.stream);
    if (rc != PDEVAL_OK) return rc;
    return reg_assign(r, r->d_field, r->d_nfin, n_list, keys, class_id, n_new);
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
        if (r->timed && hipEventElapsedTime(&ms, r->e0, r->e1) != hipSuccess) {
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
    pdeval_ctx* c = r->ctx;
    const int64_t L = r->book.n_classes();
    if (leader_keys) std::copy(r->book.keys.begin(), r->book.keys.end(), leader_keys);
    if (sizes) std::copy(r->book.sizes.begin(), r->book.sizes.end(), sizes);
    if (!d_fields || L == 0) return PDEVAL_OK;
    hipError_t e = hipSetDevice(r->v.device);
    if (e != hipSuccess) return fol_hip_fail(c, "hipSetDevice", e);
    FolMoveArgs m{};
    reg_move_args(r, &m);
    m.base = 0;
    m.n_lead = L;
    m.fields = d_fields;
    m.n_rows = L;
    m.to_store = 0;
    launch_fol_move(m, r->v.stream);
    if ((e = hipGetLastError()) != hipSuccess) return fol_hip_fail(c, "fol_move_kernel", e);
    if ((e = hipStreamSynchronize(r->v.stream)) != hipSuccess) return fol_hip_fail(c, "fol_move_kernel", e);
    return PDEVAL_OK;
}

extern "C" int pdeval_fol_registry_kinds(pdeval_fol_registry* r, uint8_t* kinds) {
    if (!r) return fol_fail(nullptr, PDEVAL_ERR_ARG, "pdeval_fol_registry_kinds: null registry");
    pdeval_ctx* c = r->ctx;
    const int64_t L = r->book.n_classes();
    if (L == 0) return PDEVAL_OK;
    if (!kinds) return fol_fail(c, PDEVAL_ERR_ARG, "pdeval_fol_registry_kinds: bad argument");
    hipError_t e = hipSetDevice(r->v.device);
    if (e != hipSuccess) return fol_hip_fail(c, "hipSetDevice", e);
    uint8_t* d_kind = nullptr;
    if (hipMalloc((void**)&d_kind, (size_t)L) != hipSuccess) {
        (void)hipGetLastError();
        return fol_fail(c, PDEVAL_ERR_ALLOC, "pdeval_fol_registry_kinds: cannot allocate the kinds");
    }
    FolKindArgs a{};
    a.fields = r->d_store;   // the leaders where they are: chunk-major (fol_store_at)
    a.n_rows = L;
    a.cap = r->cap;
    a.mm = r->mm;
    a.n_chunk = r->n_chunk;
    a.min_points = r->prm.min_points;
    a.kind = d_kind;
    launch_fol_kind(a, r->v.stream);
    if ((e = hipGetLastError()) == hipSuccess)
        e = hipMemcpyAsync(kinds, d_kind, (size_t)L, hipMemcpyDeviceToHost, r->v.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(r->v.stream);
    (void)hipFree(d_kind);
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
    FolMoveArgs m{};
    reg_move_args(r, &m);
    m.base = 0;
    m.n_lead = n_classes;
    m.fields = const_cast<double*>(d_fields);
    m.n_rows = n_classes;
    m.to_store = 1;
    launch_fol_move(m, r->v.stream);
    if ((e = hipGetLastError()) != hipSuccess) return fol_hip_fail(c, "fol_move_kernel", e);
    if ((e = hipStreamSynchronize(r->v.stream)) != hipSuccess) return fol_hip_fail(c, "fol_move_kernel", e);
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

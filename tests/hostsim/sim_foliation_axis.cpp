// tests/hostsim/sim_foliation_axis.cpp -- the per-point code of the foliation kernels with the
// axis rule (pdeval_foliation.h: fol_point_test<AXIS>, fol_q<AXIS>, fol_chunk_test<AXIS>,
// fol_kind_chunk / fol_kind_of) built for the CPU, one lane: the match kernel's counts, the
// leader rounds, a registry streamed through the chunk-major store (fol_store_at, FolBook) and
// the kind of a field.  `axis` selects the instantiation as the launchers do.  Test
// infrastructure only (tests/test_foliation_axis_host.py); the product is built by hipcc for
// gfx950.
#include <algorithm>
#include <vector>
#include "../../include/pdeval.h"
#include "../../pde-engine_amd/csrc/pdeval_foliation.h"
#include "../../pde-engine_amd/csrc/pdeval_fol_book.h"
using namespace pd;

static double sim_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

// One row field against one probe field (2 mm doubles each), as fol_match_kernel<AXIS> counts.
template <bool AXIS>
static int match_t(const double* row, const double* probe, int mm, double tau, int min_points, int* n_used, int* n_bad,
                   double* qmax) {
    int nu = 0, nb = 0;
    double q = 0.0;
    for (int p = 0; p < mm; ++p) {
        const FolPoint t = fol_point_test<AXIS>(row[p], row[mm + p], probe[p], probe[mm + p], tau);
        nu += t.used;
        nb += t.bad;
        if (t.used) q = fmax(q, fol_q<AXIS>(t));
    }
    if (n_used) *n_used = nu;
    if (n_bad) *n_bad = nb;
    if (qmax) *qmax = q;
    return nu >= min_points && nb == 0;
}

// Returns 1 on a match.
extern "C" int sim_axis_match(const double* row, const double* probe, int mm, double tau, int min_points, int flags,
                              int* n_used, int* n_bad, double* qmax) {
    return (flags & PDEVAL_FOL_AXIS) ? match_t<true>(row, probe, mm, tau, min_points, n_used, n_bad, qmax)
                                     : match_t<false>(row, probe, mm, tau, min_points, n_used, n_bad, qmax);
}

static int sim_nfinite(const double* f, int mm) {
    int nf = 0;
    for (int p = 0; p < mm; ++p) nf += finite_(f[p]);
    return nf;
}

// The grouping on host fields: rounds of up to 32 probes, fol_round assigning.  leader[i]: the
// leader's row, or -1 with fewer than min_points finite points.  Returns the number of classes.
extern "C" int sim_axis_classes(const double* fields, int n, int mm, double tau, int min_points, int flags,
                                int64_t* leader, int* rounds) {
    std::vector<int64_t> un, next;
    for (int i = 0; i < n; ++i) {
        leader[i] = -1;
        if (sim_nfinite(fields + (size_t)i * 2 * mm, mm) >= min_points) un.push_back(i);
    }
    int classes = 0, nr = 0;
    std::vector<uint32_t> mask;
    while (!un.empty()) {
        const int64_t nu = (int64_t)un.size();
        const int np = (int)std::min<int64_t>(PDEVAL_FOL_MAX_PROBES, nu);
        mask.assign((size_t)nu, 0u);
        for (int64_t r = 0; r < nu; ++r)
            for (int k = 0; k < np; ++k)
                if (sim_axis_match(fields + (size_t)un[r] * 2 * mm, fields + (size_t)un[k] * 2 * mm, mm, tau, min_points,
                                   flags, nullptr, nullptr, nullptr))
                    mask[(size_t)r] |= 1u << k;
        classes += fol_round(mask.data(), un.data(), nu, np, nullptr, leader, next);
        un.swap(next);
        ++nr;
    }
    if (rounds) *rounds = nr;
    return classes;
}

// ---- a registry on the chunk-major store, as pdeval_fol_registry.hip keeps it
struct AxisReg {
    int mm, n_chunk, min_points, flags;
    double tau;
    int64_t cap;
    std::vector<double> store;
    FolBook book;
};

static void reg_reserve(AxisReg* r, int64_t need) {
    if (need <= r->cap) return;
    const int64_t cap = fol_next_capacity(r->cap, need), L = r->book.n_classes();
    std::vector<double> s((size_t)cap * r->n_chunk * 2 * kFolChunk, sim_nan());
    for (int c = 0; c < r->n_chunk; ++c)
        std::copy(r->store.begin() + fol_store_at(r->cap, c, 0), r->store.begin() + fol_store_at(r->cap, c, L),
                  s.begin() + fol_store_at(cap, c, 0));
    r->store.swap(s);
    r->cap = cap;
}

static void reg_put(AxisReg* r, int64_t l, const double* f) {
    for (int c = 0; c < r->n_chunk; ++c)
        for (int lane = 0; lane < kFolChunk; ++lane) {
            const int p = c * kFolChunk + lane;
            double* st = r->store.data() + fol_store_at(r->cap, c, l);
            st[lane] = p < r->mm ? f[p] : sim_nan();
            st[kFolChunk + lane] = p < r->mm ? f[r->mm + p] : sim_nan();
        }
}

// one row field against store leader l, chunk by chunk, left at the first chunk with a bad point
template <bool AXIS>
static bool reg_pair_t(const AxisReg* r, const double* f, int64_t l) {
    FolCount n{0, 0};
    for (int c = 0; c < r->n_chunk && !n.nb; ++c) {
        const double* q = r->store.data() + fol_store_at(r->cap, c, l);
        for (int lane = 0; lane < kFolChunk; ++lane) {
            const int p = c * kFolChunk + lane;
            const bool active = p < r->mm;
            fol_chunk_test<AXIS>(active ? f[p] : sim_nan(), active ? f[r->mm + p] : sim_nan(), q[lane],
                                 q[kFolChunk + lane], active, r->tau, n);
        }
    }
    return n.nu >= r->min_points && n.nb == 0;
}
static bool reg_pair(const AxisReg* r, const double* f, int64_t l) {
    return (r->flags & PDEVAL_FOL_AXIS) ? reg_pair_t<true>(r, f, l) : reg_pair_t<false>(r, f, l);
}

// one batch: Stage A, Stage B by rounds, the append and the bookkeeping; false if the plan fails
static bool reg_assign(AxisReg* r, const double* fields, int64_t n, int64_t* class_id) {
    const int64_t L = r->book.n_classes();
    const int mm = r->mm;
    std::vector<int64_t> first((size_t)n, -1), leader_b((size_t)n, -1), un, next, new_rows, ids((size_t)n);
    std::vector<int32_t> nfin((size_t)n);
    for (int64_t row = 0; row < n; ++row) {
        const double* f = fields + row * 2 * (int64_t)mm;
        nfin[(size_t)row] = sim_nfinite(f, mm);
        if (nfin[(size_t)row] < r->min_points) continue;
        for (int64_t l = 0; l < L; ++l)
            if (reg_pair(r, f, l)) {
                first[(size_t)row] = l;
                break;
            }
    }
    FolBook::stage_b_rows(first.data(), nfin.data(), n, r->min_points, un);
    std::vector<uint32_t> mask;
    int64_t classes = 0;
    while (!un.empty()) {
        const int64_t nu = (int64_t)un.size();
        const int np = (int)std::min<int64_t>(PDEVAL_FOL_MAX_PROBES, nu);
        AxisReg probes{mm, r->n_chunk, r->min_points, r->flags, r->tau, 0, {}, {}};
        reg_reserve(&probes, np);
        for (int k = 0; k < np; ++k) reg_put(&probes, k, fields + un[(size_t)k] * 2 * (int64_t)mm);
        mask.assign((size_t)nu, 0u);
        for (int64_t q = 0; q < nu; ++q)
            for (int k = 0; k < np; ++k)
                if (reg_pair(&probes, fields + un[(size_t)q] * 2 * (int64_t)mm, k)) mask[(size_t)q] |= 1u << k;
        classes += fol_round(mask.data(), un.data(), nu, np, nullptr, leader_b.data(), next);
        un.swap(next);
    }
    if (!r->book.plan(first.data(), leader_b.data(), n, ids.data(), new_rows) || (int64_t)new_rows.size() != classes)
        return false;
    reg_reserve(r, L + classes);
    for (size_t k = 0; k < new_rows.size(); ++k) reg_put(r, L + (int64_t)k, fields + new_rows[k] * 2 * (int64_t)mm);
    r->book.commit(ids.data(), n, nullptr, new_rows);
    std::copy(ids.begin(), ids.end(), class_id);
    return true;
}

// `fields` (n rows) assigned to a fresh registry in the consecutive batches that the n_cuts cut
// positions delimit.  class_id (n): the rows' ids; kinds (n, may be NULL): the kinds of the
// leaders, read from the store chunk by chunk as fol_kind_kernel does, first n_classes entries.
// Returns the number of classes, or -1.
extern "C" int64_t sim_axis_stream(const double* fields, int64_t n, int mm, double tau, int min_points, int flags,
                                   const int64_t* cuts, int n_cuts, int64_t* class_id, uint8_t* kinds) {
    AxisReg r{mm, (mm + kFolChunk - 1) / kFolChunk, min_points, flags, tau, 0, {}, {}};
    reg_reserve(&r, 1);
    int64_t a = 0;
    for (int k = 0; k <= n_cuts; ++k) {
        const int64_t b = k < n_cuts ? cuts[k] : n;
        if (b < a || b > n) return -1;
        if (b > a && !reg_assign(&r, fields + a * 2 * (int64_t)mm, b - a, class_id + a)) return -1;
        a = b;
    }
    const int64_t L = r.book.n_classes();
    for (int64_t l = 0; kinds && l < L; ++l) {
        FolKindCount cnt{0, 0, 0, 0};
        for (int c = 0; c < r.n_chunk; ++c) {
            const double* q = r.store.data() + fol_store_at(r.cap, c, l);
            for (int lane = 0; lane < kFolChunk; ++lane)
                fol_kind_chunk(q[lane], q[kFolChunk + lane], c * kFolChunk + lane < mm, cnt);
        }
        kinds[l] = (uint8_t)fol_kind_of(cnt, min_points);
    }
    return L;
}

// kind[row] of rows of [n][2][mm] fields, as fol_kind_kernel counts them
extern "C" void sim_axis_kinds(const double* fields, int64_t n, int mm, int min_points, uint8_t* kind) {
    for (int64_t row = 0; row < n; ++row) {
        const double* f = fields + row * 2 * (int64_t)mm;
        FolKindCount cnt{0, 0, 0, 0};
        for (int p = 0; p < mm; ++p) fol_kind_chunk(f[p], f[mm + p], true, cnt);
        kind[row] = (uint8_t)fol_kind_of(cnt, min_points);
    }
}

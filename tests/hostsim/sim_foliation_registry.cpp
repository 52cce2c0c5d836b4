// tests/hostsim/sim_foliation_registry.cpp -- the foliation class registry on the CPU: the pair
// scan of fol_assign_kernel (pdeval_foliation.h: fol_chunk_test on the chunk-major store of
// fol_store_at, one lane at a time), the rounds of Stage B (fol_round) and the host bookkeeping
// the product uses (pdeval_fol_book.h: FolBook, fol_next_capacity).  Test infrastructure only
// (tests/test_foliation_registry_host.py, guard_fol_registry.cpp); the product is built by hipcc
// for gfx950.
#include <algorithm>
#include <vector>
#include "../../include/pdeval.h"
#include "../../pde-engine_amd/csrc/pdeval_foliation.h"
#include "../../pde-engine_amd/csrc/pdeval_fol_book.h"
using namespace pd;

struct SimReg {
    int mm, n_chunk, min_points;
    double tau;
    int64_t cap;
    std::vector<double> store;   // chunk-major, cap leaders
    FolBook book;
};

static double sim_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

// the store holds `need` leaders: doubling, one copy per chunk plane (as reg_reserve)
static void sim_reserve(SimReg* r, int64_t need) {
    if (need <= r->cap) return;
    const int64_t cap = fol_next_capacity(r->cap, need), L = r->book.n_classes();
    std::vector<double> s((size_t)cap * r->n_chunk * 2 * kFolChunk, sim_nan());
    for (int c = 0; c < r->n_chunk; ++c)
        std::copy(r->store.begin() + fol_store_at(r->cap, c, 0), r->store.begin() + fol_store_at(r->cap, c, L),
                  s.begin() + fol_store_at(cap, c, 0));
    r->store.swap(s);
    r->cap = cap;
}

// field [2][mm] -> store leader l (as fol_move_kernel: NaN past m^2)
static void sim_put(SimReg* r, int64_t l, const double* f) {
    for (int c = 0; c < r->n_chunk; ++c)
        for (int lane = 0; lane < kFolChunk; ++lane) {
            const int p = c * kFolChunk + lane;
            double* st = r->store.data() + fol_store_at(r->cap, c, l);
            st[lane] = p < r->mm ? f[p] : sim_nan();
            st[kFolChunk + lane] = p < r->mm ? f[r->mm + p] : sim_nan();
        }
}

// one row field against store leader l, chunk by chunk, left at the first chunk with a bad point
static bool sim_pair(const SimReg* r, const double* f, int64_t l) {
    FolCount n{0, 0};
    for (int c = 0; c < r->n_chunk && !n.nb; ++c) {
        const double* q = r->store.data() + fol_store_at(r->cap, c, l);
        for (int lane = 0; lane < kFolChunk; ++lane) {
            const int p = c * kFolChunk + lane;
            const bool active = p < r->mm;
            fol_chunk_test(active ? f[p] : sim_nan(), active ? f[r->mm + p] : sim_nan(), q[lane], q[kFolChunk + lane],
                           active, r->tau, n);
        }
    }
    return n.nu >= r->min_points && n.nb == 0;
}

static int sim_nfinite(const double* f, int mm) {
    int nf = 0;
    for (int p = 0; p < mm; ++p) nf += finite_(f[p]);
    return nf;
}

extern "C" void* sim_reg_create(int mm, double tau, int min_points, int64_t capacity_hint) {
    SimReg* r = new SimReg{mm, (mm + kFolChunk - 1) / kFolChunk, min_points, tau, 0, {}, {}};
    sim_reserve(r, std::max<int64_t>(capacity_hint, 1));
    return r;
}
extern "C" void sim_reg_destroy(void* h) { delete (SimReg*)h; }
extern "C" int64_t sim_reg_capacity(void* h) { return ((SimReg*)h)->cap; }

// Stage A: first[row] = the smallest leader index the row matches, -1 if none
extern "C" void sim_reg_first(void* h, const double* fields, int64_t n, int64_t* first) {
    const SimReg* r = (const SimReg*)h;
    const int64_t L = r->book.n_classes();
    for (int64_t row = 0; row < n; ++row) {
        const double* f = fields + row * 2 * (int64_t)r->mm;
        first[row] = -1;
        if (sim_nfinite(f, r->mm) < r->min_points) continue;
        for (int64_t l = 0; l < L; ++l)
            if (sim_pair(r, f, l)) {
                first[row] = l;
                break;
            }
    }
}

// One batch: Stage A (first_in != NULL: taken from the caller instead, as a download would
// deliver it), Stage B by rounds, the append and the bookkeeping.  Returns the number of new
// leaders, or -1 -- the registry unchanged -- when first_in or the rounds point outside.
extern "C" int64_t sim_reg_assign(void* h, const double* fields, int64_t n, const int64_t* keys, const int64_t* first_in,
                                  int64_t* class_id) {
    SimReg* r = (SimReg*)h;
    const int64_t L = r->book.n_classes();
    const int mm = r->mm;
    std::vector<int64_t> first((size_t)n, -1), leader_b((size_t)n, -1), un, next, new_rows, ids((size_t)n);
    std::vector<int32_t> nfin((size_t)n);
    for (int64_t row = 0; row < n; ++row) nfin[(size_t)row] = sim_nfinite(fields + row * 2 * (int64_t)mm, mm);
    if (first_in) first.assign(first_in, first_in + n);
    else sim_reg_first(h, fields, n, first.data());
    if (!FolBook::first_ok(first.data(), n, L)) return -1;
    FolBook::stage_b_rows(first.data(), nfin.data(), n, r->min_points, un);
    // Stage B on the batch's own fields: each round's probes go into a scratch store, so that the
    // rows meet them through the same chunk test
    std::vector<uint32_t> mask;
    int64_t classes = 0;
    while (!un.empty()) {
        const int64_t nu = (int64_t)un.size();
        const int np = (int)std::min<int64_t>(PDEVAL_FOL_MAX_PROBES, nu);
        SimReg probes{mm, r->n_chunk, r->min_points, r->tau, 0, {}, {}};
        sim_reserve(&probes, np);
        for (int k = 0; k < np; ++k) sim_put(&probes, k, fields + un[(size_t)k] * 2 * (int64_t)mm);
        mask.assign((size_t)nu, 0u);
        for (int64_t q = 0; q < nu; ++q)
            for (int k = 0; k < np; ++k)
                if (sim_pair(&probes, fields + un[(size_t)q] * 2 * (int64_t)mm, k)) mask[(size_t)q] |= 1u << k;
        classes += fol_round(mask.data(), un.data(), nu, np, nullptr, leader_b.data(), next);
        un.swap(next);
    }
    if (!r->book.plan(first.data(), leader_b.data(), n, ids.data(), new_rows) || (int64_t)new_rows.size() != classes)
        return -1;
    sim_reserve(r, L + classes);
    for (size_t k = 0; k < new_rows.size(); ++k) sim_put(r, L + (int64_t)k, fields + new_rows[k] * 2 * (int64_t)mm);
    r->book.commit(ids.data(), n, keys, new_rows);
    std::copy(ids.begin(), ids.end(), class_id);
    return classes;
}

extern "C" void sim_reg_size(void* h, int64_t* n_classes, int64_t* rows_seen) {
    const SimReg* r = (const SimReg*)h;
    *n_classes = r->book.n_classes();
    *rows_seen = r->book.rows_seen;
}

// fields [L][2][mm] (may be NULL), keys and sizes of the leaders
extern "C" void sim_reg_leaders(void* h, double* fields, int64_t* keys, int64_t* sizes) {
    const SimReg* r = (const SimReg*)h;
    const int64_t L = r->book.n_classes();
    std::copy(r->book.keys.begin(), r->book.keys.end(), keys);
    std::copy(r->book.sizes.begin(), r->book.sizes.end(), sizes);
    if (!fields) return;
    for (int64_t l = 0; l < L; ++l)
        for (int p = 0; p < r->mm; ++p) {
            const double* st = r->store.data() + fol_store_at(r->cap, p / kFolChunk, l);
            fields[l * 2 * (int64_t)r->mm + p] = st[p % kFolChunk];
            fields[l * 2 * (int64_t)r->mm + r->mm + p] = st[kFolChunk + p % kFolChunk];
        }
}

// saved leaders into an empty registry; returns 0, or -1 (nothing changed) if it is not empty
extern "C" int sim_reg_load(void* h, const double* fields, const int64_t* keys, const int64_t* sizes, int64_t n) {
    SimReg* r = (SimReg*)h;
    if (r->book.n_classes() != 0 || r->book.rows_seen != 0 || n < 0) return -1;
    sim_reserve(r, n);
    for (int64_t l = 0; l < n; ++l) sim_put(r, l, fields + l * 2 * (int64_t)r->mm);
    return r->book.load(keys, sizes, n) ? 0 : -1;
}

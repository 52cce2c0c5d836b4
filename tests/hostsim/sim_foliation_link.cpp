// tests/hostsim/sim_foliation_link.cpp -- the link pass of the foliation class registry built for
// the CPU, one lane (DESIGN.md §14 "Links and components"): the pair scan of fol_link_kernel on
// the chunk-major store (fol_chunk_test<AXIS>, fol_store_at; a row scans the leaders below its
// limit, skips its own class and does not stop at a match), its capped edge buffer with the
// counter that runs past the capacity and the host's grow-and-repeat, and the product's host
// bookkeeping of links and components (pdeval_fol_book.h: arrival_limits, link_rows_ok,
// plan_links / commit_links, map_links, the union-find).  The classes themselves are built by
// sim_foliation_axis.cpp's registry.  Test infrastructure only (tests/test_foliation_link_host.py,
// guard_fol_links.cpp); the product is built by hipcc for gfx950.
#include "sim_foliation_axis.cpp"

struct LinkReg {
    AxisReg r;
    int64_t edge_cap;
    int launches;   // of the most recent pass
};

// the scan of one row, as a wave of fol_link_kernel runs it; count runs on past the capacity
static void link_row(const LinkReg* g, const double* f, int own, int lim, std::vector<int32_t>& edges, int64_t ecap,
                     unsigned long long& count) {
    if (own < 0) lim = 0;
    for (int l = 0; l < lim; ++l) {
        if (l == own) continue;
        if (!reg_pair(&g->r, f, l)) continue;
        const unsigned long long slot = count++;
        if (slot < (unsigned long long)ecap) {
            edges[2 * slot] = own;
            edges[2 * slot + 1] = l;
        }
    }
}

// The pass over n rows against the store's leaders [0, L): at most two launches, the second with a
// buffer that holds what the first counted.  The planned links are left in merged / fresh.
static bool link_pass(LinkReg* g, const double* fields, int64_t n, const std::vector<int32_t>& cls,
                      const std::vector<int32_t>& lim, int64_t L, std::vector<FolBook::Link>& merged,
                      std::vector<FolBook::Link>& fresh) {
    g->launches = 0;
    if (!FolBook::link_rows_ok(cls.data(), lim.data(), n, L)) return false;
    std::vector<int32_t> edges;
    unsigned long long count = 0;
    for (int pass = 0; pass < 2 && n > 0 && L > 1; ++pass) {
        edges.assign((size_t)g->edge_cap * 2, -9);
        count = 0;
        ++g->launches;
        for (int64_t row = 0; row < n; ++row)
            link_row(g, fields + row * 2 * (int64_t)g->r.mm, cls[(size_t)row], lim[(size_t)row], edges, g->edge_cap, count);
        if ((int64_t)count <= g->edge_cap) break;
        if (pass == 1) return false;
        g->edge_cap = fol_next_capacity(g->edge_cap, (int64_t)count);
    }
    edges.resize((size_t)count * 2);
    return g->r.book.plan_links(edges.data(), (int64_t)count, L, merged, fresh);
}

extern "C" void* sim_link_create(int mm, double tau, int min_points, int flags, int64_t edge_cap) {
    LinkReg* g = new LinkReg{{mm, (mm + kFolChunk - 1) / kFolChunk, min_points, flags, tau, 0, {}, {}},
                             edge_cap > 0 ? edge_cap : 1, 0};
    reg_reserve(&g->r, 1);
    return g;
}
extern "C" void sim_link_destroy(void* h) { delete (LinkReg*)h; }

// One batch: the classes by sim_foliation_axis.cpp's registry, then (PDEVAL_FOL_LINK) the link
// pass by the arrival rule.  Returns the number of new links, or -1.
extern "C" int64_t sim_link_assign(void* h, const double* fields, int64_t n, int64_t* class_id) {
    LinkReg* g = (LinkReg*)h;
    const int64_t L0 = g->r.book.n_classes();
    if (!reg_assign(&g->r, fields, n, class_id)) return -1;
    if (!(g->r.flags & PDEVAL_FOL_LINK)) return 0;
    // the rows that became leaders: ids are dense in order of creation, a leader is its class's first row
    std::vector<int64_t> new_rows;
    for (int64_t row = 0; row < n; ++row)
        if (class_id[row] == L0 + (int64_t)new_rows.size()) new_rows.push_back(row);
    std::vector<int32_t> cls, lim;
    FolBook::arrival_limits(class_id, n, L0, new_rows, cls, lim);
    std::vector<FolBook::Link> merged, fresh;
    if (!link_pass(g, fields, n, cls, lim, g->r.book.n_classes(), merged, fresh)) return -1;
    g->r.book.commit_links(merged, fresh);
    return (int64_t)fresh.size();
}

// pdeval_fol_registry_link_fields: rows with their class ids against all current leaders
extern "C" int64_t sim_link_fields(void* h, const double* fields, const int64_t* class_id, int64_t n) {
    LinkReg* g = (LinkReg*)h;
    const int64_t L = g->r.book.n_classes();
    std::vector<int32_t> cls((size_t)n), lim((size_t)n);
    for (int64_t k = 0; k < n; ++k) {
        if (class_id[k] < -1 || class_id[k] >= L) return -1;
        cls[(size_t)k] = (int32_t)class_id[k];
        lim[(size_t)k] = class_id[k] < 0 ? 0 : (int32_t)L;
    }
    std::vector<FolBook::Link> merged, fresh;
    if (!link_pass(g, fields, n, cls, lim, L, merged, fresh)) return -1;
    g->r.book.commit_links(merged, fresh);
    return (int64_t)fresh.size();
}

// component (L, may be NULL), sizes (L, may be NULL); returns L
extern "C" int64_t sim_link_components(void* h, int64_t* component, int64_t* sizes, int64_t* n_components,
                                       int64_t* n_links) {
    LinkReg* g = (LinkReg*)h;
    const int64_t L = g->r.book.n_classes();
    for (int64_t c = 0; component && c < L; ++c) component[c] = g->r.book.component(c);
    if (sizes) std::copy(g->r.book.sizes.begin(), g->r.book.sizes.end(), sizes);
    if (n_components) *n_components = g->r.book.n_components();
    if (n_links) *n_links = (int64_t)g->r.book.links.size();
    return L;
}
extern "C" void sim_link_links(void* h, int64_t* edges) {
    LinkReg* g = (LinkReg*)h;
    for (size_t k = 0; k < g->r.book.links.size(); ++k) {
        edges[2 * k] = g->r.book.links[k].first;
        edges[2 * k + 1] = g->r.book.links[k].second;
    }
}
extern "C" int sim_link_launches(void* h) { return ((LinkReg*)h)->launches; }
extern "C" int64_t sim_link_edge_cap(void* h) { return ((LinkReg*)h)->edge_cap; }

// pdeval_fol_registry_load_links; -1 for a bad edge, nothing added
extern "C" int sim_link_load_links(void* h, const int64_t* edges, int64_t n) {
    LinkReg* g = (LinkReg*)h;
    std::vector<FolBook::Link> merged, fresh;
    if (!g->r.book.plan_links(edges, n, g->r.book.n_classes(), merged, fresh)) return -1;
    g->r.book.commit_links(merged, fresh);
    return 0;
}

// FoliationRegistry.merge: other's leaders assigned here in their order, its sizes added, its
// links mapped through the id map (id_map: other's L entries).  Returns other's L, or -1.
extern "C" int64_t sim_link_merge(void* h, void* other, int64_t* id_map) {
    LinkReg* g = (LinkReg*)h;
    const LinkReg* o = (const LinkReg*)other;
    const int64_t Lo = o->r.book.n_classes();
    const int mm = g->r.mm;
    if (o->r.mm != mm) return -1;
    std::vector<double> f((size_t)Lo * 2 * mm);
    for (int64_t l = 0; l < Lo; ++l)
        for (int p = 0; p < mm; ++p) {
            const double* st = o->r.store.data() + fol_store_at(o->r.cap, p / kFolChunk, l);
            f[(size_t)l * 2 * mm + p] = st[p % kFolChunk];
            f[(size_t)l * 2 * mm + mm + p] = st[kFolChunk + p % kFolChunk];
        }
    if (Lo > 0 && sim_link_assign(h, f.data(), Lo, id_map) < 0) return -1;
    std::vector<int64_t> extra((size_t)Lo), flat, mapped;
    for (int64_t l = 0; l < Lo; ++l) extra[(size_t)l] = o->r.book.sizes[(size_t)l] - 1;
    if (!g->r.book.add_sizes(id_map, extra.data(), Lo)) return -1;
    for (const FolBook::Link& e : o->r.book.links) {
        flat.push_back(e.first);
        flat.push_back(e.second);
    }
    if (!FolBook::map_links(flat.data(), (int64_t)flat.size() / 2, id_map, Lo, mapped)) return -1;
    return sim_link_load_links(h, mapped.data(), (int64_t)mapped.size() / 2) == 0 ? Lo : -1;
}

// tests/hostsim/guard_fol_links.cpp -- a stand-alone check of the registry's link bookkeeping
// (pdeval_fol_book.h: plan_links / commit_links, the union-find, map_links, arrival_limits,
// link_rows_ok) and of the link pass's capped edge buffer, built with
// -fsanitize=address,undefined by tests/test_foliation_link_host.py and run directly: every array
// is a heap block of its exact size, so an index followed outside one ends the run.  Edge
// validation with out-of-range and self edges, growth with the registry, the merge mapping and a
// failed plan that leaves classes and components as they were.  Test infrastructure only.
#include <cmath>
#include <cstdio>
#include <memory>

#include "sim_foliation_link.cpp"

static int failures = 0;
static void expect(bool ok, const char* what) {
    if (!ok) {
        std::printf("FAILED: %s\n", what);
        ++failures;
    }
}

// n constant fields (cos t, sin t) at angles t = 0.3 + 0.03 (first + k) < pi, none along an axis:
// distinct foliations, each matching itself; `keep` (may be NULL) masks the points to NaN
static std::unique_ptr<double[]> rows(int first, int n, int mm, const bool* keep = nullptr) {
    std::unique_ptr<double[]> f(new double[(size_t)n * 2 * mm]);
    for (int k = 0; k < n; ++k)
        for (int p = 0; p < mm; ++p) {
            const bool on = !keep || keep[p];
            f[(size_t)k * 2 * mm + p] = on ? std::cos(0.3 + 0.03 * (first + k)) : NAN;
            f[(size_t)k * 2 * mm + mm + p] = on ? std::sin(0.3 + 0.03 * (first + k)) : NAN;
        }
    return f;
}

static std::unique_ptr<int64_t[]> comps(void* reg, int64_t L, int64_t* nc, int64_t* nl) {
    std::unique_ptr<int64_t[]> c(new int64_t[L > 0 ? L : 1]);
    expect(sim_link_components(reg, c.get(), nullptr, nc, nl) == L, "n_classes");
    return c;
}

int main() {
    const int m = 9, mm = m * m;   // two chunks, the second partial
    // ---- the union-find alone: 70 classes, a chain built from its far end, labels = smallest id
    {
        FolBook book;
        std::unique_ptr<int64_t[]> k(new int64_t[70]), s(new int64_t[70]);
        for (int i = 0; i < 70; ++i) {
            k[i] = i;
            s[i] = 1;
        }
        expect(book.load(k.get(), s.get(), 70), "load 70");
        std::vector<FolBook::Link> merged, fresh;
        for (int i = 68; i >= 40; --i) {
            const int64_t e[2] = {i + 1, i};
            expect(book.plan_links(e, 1, 70, merged, fresh) && fresh.size() == 1, "a new link");
            book.commit_links(merged, fresh);
        }
        expect(book.component(69) == 40 && book.component(40) == 40 && book.component(39) == 39, "chain root 40");
        expect(book.n_components() == 41 && book.links.size() == 29, "41 components, 29 links");
        // repeats and both orientations: nothing new
        const int64_t rep[6] = {41, 40, 40, 41, 69, 68};
        expect(book.plan_links(rep, 3, 70, merged, fresh) && fresh.empty() && merged.size() == 29, "known links");
        book.commit_links(merged, fresh);
        // out-of-range and self edges: errors of the call, never indices; the book is unchanged
        const int64_t bad[6][2] = {{0, 70}, {70, 0}, {-1, 3}, {3, INT64_MIN}, {5, 5}, {(int64_t)1 << 40, 1}};
        for (int b = 0; b < 6; ++b) {
            const int64_t e[4] = {0, 1, bad[b][0], bad[b][1]};   // a good edge first: not added either
            expect(!book.plan_links(e, 2, 70, merged, fresh), "bad edge rejected");
        }
        expect(book.n_components() == 41 && book.links.size() == 29 && book.component(1) == 1, "unchanged after bad edges");
        const int32_t bad32[2] = {0, INT32_MIN};
        expect(!book.plan_links(bad32, 1, 70, merged, fresh), "bad 32-bit edge rejected");
        // the classes an edge may name are those of its batch: L = 40 excludes the chain
        const int64_t e40[2] = {39, 40};
        expect(!book.plan_links(e40, 1, 40, merged, fresh) && book.plan_links(e40, 1, 41, merged, fresh), "L bounds the ends");
        book.commit_links(merged, fresh);
        expect(book.component(69) == 39 && book.n_components() == 40, "components only merge");
        // cls / lim of a launch
        const int32_t cls[3] = {-1, 0, 69}, lim[3] = {0, 70, 1};
        const int32_t cls_bad[3] = {-2, INT32_MIN, 70}, lim_bad[3] = {0, 71, -1};
        expect(FolBook::link_rows_ok(cls, lim, 3, 70), "rows ok");
        for (int i = 0; i < 3; ++i) {
            int32_t c2[3] = {cls[0], cls[1], cls[2]}, l2[3] = {lim[0], lim[1], lim[2]};
            c2[i] = cls_bad[i];
            expect(!FolBook::link_rows_ok(c2, lim, 3, 70), "bad cls");
            l2[i] = i == 0 ? 71 : lim_bad[i];
            expect(!FolBook::link_rows_ok(cls, l2, 3, 70), "bad lim");
        }
    }
    // ---- growth with the registry: leaders on disjoint halves, bridged by full rows, over calls
    std::unique_ptr<bool[]> left(new bool[mm]), right(new bool[mm]);
    for (int p = 0; p < mm; ++p) {
        left[p] = p < mm / 2;
        right[p] = !left[p];
    }
    void* reg = sim_link_create(mm, 1e-7, 16, PDEVAL_FOL_LINK, 1);
    int64_t nc = 0, nl = 0;
    {
        // 35 foliations: left halves (classes 0 .. 34), then right halves (35 .. 69): no links yet
        std::unique_ptr<int64_t[]> ids(new int64_t[35]);
        auto fl = rows(0, 35, mm, left.get());
        expect(sim_link_assign(reg, fl.get(), 35, ids.get()) == 0, "left halves: no links");
        auto fr = rows(0, 35, mm, right.get());
        expect(sim_link_assign(reg, fr.get(), 35, ids.get()) == 0 && ids[34] == 69, "right halves: no links");
        auto c = comps(reg, 70, &nc, &nl);
        expect(nc == 70 && nl == 0, "70 components");
        // the full rows: each joins its left half and links it to its right half; the edge buffer
        // of one pair overflows, grows and the pass is repeated
        auto ff = rows(0, 35, mm);
        expect(sim_link_assign(reg, ff.get(), 35, ids.get()) == 35, "35 links");
        expect(sim_link_launches(reg) == 2 && sim_link_edge_cap(reg) == 64, "edge buffer grown to 64");
        for (int k = 0; k < 35; ++k) expect(ids[k] == k, "full rows join the left halves");
        c = comps(reg, 70, &nc, &nl);
        expect(nc == 35 && nl == 35, "35 components");
        for (int k = 0; k < 70; ++k) expect(c[k] == k % 35, "component = the smaller id");
        // 10 new foliations in one batch, each as left half, right half, full row: the arrival rule
        // inside a batch, classes appended past 70 with their components
        std::unique_ptr<double[]> mix(new double[(size_t)30 * 2 * mm]);
        for (int k = 0; k < 10; ++k) {
            auto a = rows(40 + k, 1, mm, left.get()), b = rows(40 + k, 1, mm, right.get()), f = rows(40 + k, 1, mm);
            std::copy(a.get(), a.get() + 2 * mm, mix.get() + (size_t)(3 * k) * 2 * mm);
            std::copy(b.get(), b.get() + 2 * mm, mix.get() + (size_t)(3 * k + 1) * 2 * mm);
            std::copy(f.get(), f.get() + 2 * mm, mix.get() + (size_t)(3 * k + 2) * 2 * mm);
        }
        std::unique_ptr<int64_t[]> ids30(new int64_t[30]);
        expect(sim_link_assign(reg, mix.get(), 30, ids30.get()) == 10, "10 links inside one batch");
        c = comps(reg, 90, &nc, &nl);
        expect(nc == 45 && nl == 45, "45 components");
        for (int k = 0; k < 10; ++k)
            expect(ids30[3 * k] == 70 + 2 * k && ids30[3 * k + 1] == 71 + 2 * k && ids30[3 * k + 2] == 70 + 2 * k &&
                       c[71 + 2 * k] == 70 + 2 * k,
                   "in-batch leaders link");
    }
    // ---- a failed plan leaves classes and components as they were
    {
        std::unique_ptr<int64_t[]> ids(new int64_t[2]);
        auto f = rows(0, 2, mm);
        ids[0] = 0;
        ids[1] = 90;   // outside [-1, L)
        expect(sim_link_fields(reg, f.get(), ids.get(), 2) == -1, "link_fields: bad class id");
        const int64_t e[4] = {0, 1, 90, 2};
        expect(sim_link_load_links(reg, e, 2) == -1, "load_links: bad edge");
        auto c = comps(reg, 90, &nc, &nl);
        expect(nc == 45 && nl == 45 && c[1] == 1, "unchanged after the failed calls");
        ids[1] = -1;   // skipped
        expect(sim_link_fields(reg, f.get(), ids.get(), 2) == 0, "link_fields: nothing new");
    }
    // ---- merge mapping: a second registry with the right halves first; its links land on ours
    {
        void* other = sim_link_create(mm, 1e-7, 16, PDEVAL_FOL_LINK, 0);
        std::unique_ptr<int64_t[]> ids(new int64_t[5]), map(new int64_t[15]);
        auto fr = rows(0, 5, mm, right.get()), fl = rows(30, 5, mm, left.get()), ff = rows(100, 5, mm);
        expect(sim_link_assign(other, fr.get(), 5, ids.get()) == 0, "other: right halves");
        expect(sim_link_assign(other, fl.get(), 5, ids.get()) == 0, "other: left halves");
        expect(sim_link_assign(other, ff.get(), 5, ids.get()) == 0, "other: unrelated");
        const int64_t e[6] = {0, 5, 1, 12, 3, 4};   // links of its own, to be mapped
        expect(sim_link_load_links(other, e, 3) == 0, "other: links");
        expect(sim_link_merge(reg, other, map.get()) == 15, "merge");
        for (int k = 0; k < 5; ++k)
            expect(map[k] == 35 + k && map[5 + k] == 30 + k && map[10 + k] == 90 + k, "id map");
        auto c = comps(reg, 95, &nc, &nl);
        // {0,5} -> {35,30}: joins components 0 and 30; {1,12} -> {36,92}: 92 joins 1; {3,4} -> {38,39}: joins 3 and 4
        expect(c[30] == 0 && c[65] == 0 && c[92] == 1 && c[4] == 3 && c[39] == 3 && c[38] == 3, "mapped links");
        expect(nl == 48 && nc == 45 + 5 - 3, "48 links, 47 components");
        // an edge of the other registry whose ends land in one class here links nothing
        const int64_t same_map[2] = {7, 7}, one[2] = {0, 1};
        std::vector<int64_t> mapped;
        expect(FolBook::map_links(one, 1, same_map, 2, mapped) && mapped.empty(), "ends in one class: dropped");
        expect(!FolBook::map_links(one, 1, same_map, 1, mapped), "edge outside the map");
        const int64_t self[2] = {1, 1};
        expect(!FolBook::map_links(self, 1, same_map, 2, mapped), "self edge in the other registry");
        sim_link_destroy(other);
    }
    sim_link_destroy(reg);
    std::printf("guard: %d failures\n", failures);
    return failures ? 1 : 0;
}

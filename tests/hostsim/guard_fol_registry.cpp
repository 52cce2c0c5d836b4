// tests/hostsim/guard_fol_registry.cpp -- a stand-alone check of the registry's host bookkeeping
// (pdeval_fol_book.h) and store layout (fol_store_at), built with -fsanitize=address,undefined by
// tests/test_foliation_registry_host.py and run directly: every array is a heap block of its
// exact size, so an index followed outside one ends the run.  Growth from capacity 1 through 70
// leaders, load into an empty and into a non-empty registry, keys absent and present, and a
// Stage A result that points outside [0, L).  Test infrastructure only.
#include <cmath>
#include <cstdio>
#include <memory>

#include "sim_foliation_registry.cpp"

static int failures = 0;
static void expect(bool ok, const char* what) {
    if (!ok) {
        std::printf("FAILED: %s\n", what);
        ++failures;
    }
}

// n constant fields (cos t, sin t) at angles t = 0.3 + 0.03 (first + k) < pi, none along an axis:
// distinct foliations, each matching itself
static std::unique_ptr<double[]> rows(int first, int n, int mm) {
    std::unique_ptr<double[]> f(new double[(size_t)n * 2 * mm]);
    for (int k = 0; k < n; ++k)
        for (int p = 0; p < mm; ++p) {
            f[(size_t)k * 2 * mm + p] = std::cos(0.3 + 0.03 * (first + k));
            f[(size_t)k * 2 * mm + mm + p] = std::sin(0.3 + 0.03 * (first + k));
        }
    return f;
}

int main() {
    const int m = 9, mm = m * m;   // two chunks, the second partial
    void* reg = sim_reg_create(mm, 1e-7, 16, 1);
    expect(sim_reg_capacity(reg) == 1, "capacity hint 1");
    // growth: 70 distinct leaders over three calls (1, 33, 36 rows), keys absent / present / absent
    const int part[3] = {1, 33, 36};
    int done = 0;
    for (int c = 0; c < 3; ++c) {
        const int n = part[c];
        auto f = rows(done, n, mm);
        std::unique_ptr<int64_t[]> ids(new int64_t[n]), keys(new int64_t[n]);
        for (int k = 0; k < n; ++k) keys[k] = 1000 + done + k;
        const int64_t n_new = sim_reg_assign(reg, f.get(), n, c == 1 ? keys.get() : nullptr, nullptr, ids.get());
        expect(n_new == n, "every row a new leader");
        for (int k = 0; k < n; ++k) expect(ids[k] == done + k, "ids dense in order of creation");
        done += n;
    }
    expect(sim_reg_capacity(reg) == 128, "capacity doubled to 128");
    int64_t L = 0, seen = 0;
    sim_reg_size(reg, &L, &seen);
    expect(L == 70 && seen == 70, "70 classes, 70 rows");
    // the same 70 rows again, in one call: each joins its own class, nothing is appended
    {
        auto f = rows(0, 70, mm);
        std::unique_ptr<int64_t[]> ids(new int64_t[70]);
        expect(sim_reg_assign(reg, f.get(), 70, nullptr, nullptr, ids.get()) == 0, "no new leader");
        for (int k = 0; k < 70; ++k) expect(ids[k] == k, "stable ids");
    }
    std::unique_ptr<double[]> lf(new double[(size_t)70 * 2 * mm]);
    std::unique_ptr<int64_t[]> lk(new int64_t[70]), ls(new int64_t[70]);
    sim_reg_leaders(reg, lf.get(), lk.get(), ls.get());
    {
        auto f = rows(0, 70, mm);
        bool same = true;
        for (size_t i = 0; i < (size_t)70 * 2 * mm; ++i) same = same && lf[i] == f[i];
        expect(same, "leader fields survive the growth bit for bit");
    }
    for (int k = 0; k < 70; ++k) {
        // keys: row numbers 0 and 34 .. 69 (absent), 1001 .. 1033 (present)
        expect(lk[k] == (k >= 1 && k < 34 ? 1000 + k : k), "keys");
        expect(ls[k] == 2, "sizes");
    }
    // a Stage A result outside [0, L): rejected, not followed; the registry is unchanged
    {
        auto f = rows(0, 3, mm);
        std::unique_ptr<int64_t[]> ids(new int64_t[3]), first(new int64_t[3]);
        const int64_t bad[4] = {70, -2, (int64_t)1 << 40, INT64_MIN};
        for (int b = 0; b < 4; ++b) {
            first[0] = 0;
            first[1] = bad[b];
            first[2] = 2;
            expect(sim_reg_assign(reg, f.get(), 3, nullptr, first.get(), ids.get()) == -1, "bad first[] rejected");
        }
        sim_reg_size(reg, &L, &seen);
        expect(L == 70 && seen == 140, "unchanged after the rejected calls");
        first[1] = 69;   // (inside: followed as it is)
        expect(sim_reg_assign(reg, f.get(), 3, nullptr, first.get(), ids.get()) == 0 && ids[1] == 69, "first[] inside");
    }
    // load: into an empty registry (ids preserved), into a non-empty one (refused)
    void* reg2 = sim_reg_create(mm, 1e-7, 16, 0);
    expect(sim_reg_load(reg2, lf.get(), lk.get(), ls.get(), 70) == 0, "load into an empty registry");
    expect(sim_reg_load(reg2, lf.get(), lk.get(), ls.get(), 70) == -1, "load into a non-empty registry");
    expect(sim_reg_load(reg, lf.get(), lk.get(), ls.get(), 70) == -1, "load into a used registry");
    {
        auto f = rows(60, 20, mm);   // 10 known, 10 new
        std::unique_ptr<int64_t[]> ids(new int64_t[20]);
        expect(sim_reg_assign(reg2, f.get(), 20, nullptr, nullptr, ids.get()) == 10, "10 new after load");
        for (int k = 0; k < 20; ++k) expect(ids[k] == 60 + k, "ids continue after load");
        sim_reg_size(reg2, &L, &seen);
        expect(L == 80 && seen == 160, "sizes after load");
    }
    sim_reg_destroy(reg);
    sim_reg_destroy(reg2);
    std::printf("guard: %d failures\n", failures);
    return failures ? 1 : 0;
}

// tests/hostsim/guard_ctx_scratch.cpp -- a stand-alone check of the validator context's scratch
// owner (pdeval_scratch.h, pdeval_devbuf.h) under failing allocations, built with
// -fsanitize=address,undefined by tests/test_ctx_scratch_host.py and run directly.  The HIP calls
// the two headers use are stand-ins over malloc whose k-th allocating call (hipMalloc or
// hipMemset) fails once.  For every combination of the hoist / hoist_slots / tier2_mask switches,
// the scratch goes through reserve(1), reserve(1025), reserve(5000) -- the 1,024-candidate and
// 4,096-word minimums, one growth past each -- and at each stage every k is made to fail: the
// call reports it, the capacity reads 0, the hoist pair is both-or-neither, the epoch moved if a
// pointer did, and the retry leaves every buffer large enough to be written to its full extent
// (an undersized block ends the run; a leaked one fails it at exit).  Test infrastructure only.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

typedef int hipError_t;
enum { hipSuccess = 0, hipErrorOutOfMemory = 2 };
static int g_calls = 0, g_fail_at = 0, g_injected = 0, g_pending = 0;
static bool fail_now() {
    if (++g_calls != g_fail_at) return false;
    ++g_injected;
    g_pending = 1;
    return true;
}
static hipError_t hipMalloc(void** p, size_t bytes) { return fail_now() ? hipErrorOutOfMemory : (*p = std::malloc(bytes), hipSuccess); }
static hipError_t hipFree(void* p) { return std::free(p), hipSuccess; }
static hipError_t hipMemset(void* p, int v, size_t bytes) { return fail_now() ? hipErrorOutOfMemory : (std::memset(p, v, bytes), hipSuccess); }
static hipError_t hipGetLastError() { const int e = g_pending ? hipErrorOutOfMemory : hipSuccess; return g_pending = 0, e; }

#define PD_HOST_SIM
#include "../../pde-engine_amd/csrc/pdeval_scratch.h"

using pd::Scratch;
using pd::ScratchCfg;

static int failures = 0;
static void expect(bool ok, const char* what, int combo, int stage, int k) {
    if (ok) return;
    std::printf("FAILED: %s (switches %d, stage %d, failing call %d)\n", what, combo, stage, k);
    ++failures;
}

static size_t sort_bytes(int64_t cap) { return cap < 2000 ? 0 : (size_t)cap * 3 + 1; }   // (0: the 16-byte minimum)

// every buffer of the scratch: pointer, bytes it holds, bytes a batch of (n, n_words) needs of it
// (restated here from the sizes pdeval.hip's ensure_scratch and ensure_dec used), kept zero or not
struct Buf {
    void* p;
    int64_t have, need;
    bool zero;
};
static std::vector<Buf> bufs(const Scratch& s, const ScratchCfg& g, int64_t n, int64_t n_words) {
    const int64_t c = n < 1024 ? 1024 : n, w = n_words < 4096 ? 4096 : n_words;
    const int64_t pool = g.hoist_pool_slots, slots = g.hoist_slots ? pool : c > pool ? c : pool;
    const int64_t st = (int64_t)sort_bytes(c);
    std::vector<Buf> b;
    auto add = [&](auto& d, int64_t count, bool zero = false) { b.push_back({d.p, d.cap * (int64_t)sizeof(*d.p), count * (int64_t)sizeof(*d.p), zero}); };
    for (const auto& l : s.list) add(l, c);
    add(s.pstate, c), add(s.ddps, c), add(s.dd_res, 4 * c), add(s.dd_q, c);
    add(s.hoist, g.hoist ? slots * g.hoist_stride : 0);
    add(s.hoist_own, g.hoist && g.hoist_slots ? pool : 0, true);
    add(s.hseg, g.hoist ? 4 * c : 0);
    add(s.fmask, g.tier2_mask ? c * g.fmask_words : 0), add(s.fsum, g.tier2_mask ? c : 0);
    add(s.status, c), add(s.noise, 4 * c), add(s.t2acc, c * g.t2acc_bytes, true);
    add(s.skeys, 2 * c), add(s.sidx, 2 * c), add(s.stemp, st ? st : 16), add(s.dec, w + 4);
    return b;
}

// after a reserve(n, n_words) that succeeded
static void check_full(Scratch& s, const ScratchCfg& g, int64_t n, int64_t n_words, int combo, int stage, int k) {
    expect(s.cap >= n && s.cap >= 1024 && s.dec_cap >= n_words && s.dec_cap >= 4096, "capacity after success", combo, stage, k);
    expect(s.stemp_bytes == sort_bytes(s.cap), "sort scratch size", combo, stage, k);
    for (const Buf& b : bufs(s, g, n, n_words)) {
        expect(b.need ? b.p && b.have >= b.need : !b.p, "a buffer holds what the batch needs (or is absent)", combo, stage, k);
        if (!b.p || b.have < b.need) continue;
        for (int64_t i = 0; b.zero && i < b.need; ++i)
            if (((const char*)b.p)[i]) return expect(false, "zeroed block", combo, stage, k);
        std::memset(b.p, b.zero ? 0 : 0x5a, (size_t)b.need);   // the full extent
    }
}

int main() {
    const int64_t ns[3] = {1, 1025, 5000};
    for (int combo = 0; combo < 8; ++combo) {
        ScratchCfg g;
        g.hoist = combo & 1, g.hoist_slots = combo & 2, g.tier2_mask = combo & 4;
        g.hoist_pool_slots = 2000, g.hoist_stride = 24, g.fmask_words = 3, g.t2acc_bytes = 40;
        g.sort_temp_bytes = sort_bytes;
        for (int stage = 0; stage < 3; ++stage) {
            int n_calls = 1;
            for (int k = 0; k <= n_calls; ++k) {   // k = 0: no failure, counts the stage's allocating calls
                Scratch s;
                uint64_t epoch = 0;
                g_fail_at = 0;
                for (int t = 0; t < stage; ++t) {
                    expect(s.reserve(ns[t], 4 * ns[t], g, epoch) == hipSuccess, "earlier stage", combo, t, k);
                    check_full(s, g, ns[t], 4 * ns[t], combo, t, k);
                }
                const int64_t n = ns[stage], n_words = 4 * n;
                std::vector<Buf> before = bufs(s, g, n, n_words);
                const uint64_t epoch0 = epoch;
                g_calls = g_injected = 0;
                g_fail_at = k;
                const hipError_t e = s.reserve(n, n_words, g, epoch);
                g_fail_at = 0;
                {
                    std::vector<Buf> now = bufs(s, g, n, n_words);
                    bool moved = false;
                    for (size_t i = 0; i < now.size(); ++i) moved = moved || now[i].p != before[i].p;
                    expect(!moved || epoch != epoch0, "the epoch moves with a pointer", combo, stage, k);
                }
                if (k == 0) {
                    n_calls = g_calls;
                    expect(e == hipSuccess && n_calls > 0, "the stage allocates", combo, stage, k);
                } else {
                    if (g_injected != 1) {
                        std::printf("no failure injected (switches %d, stage %d, call %d of %d)\n", combo, stage, k, n_calls);
                        return 2;
                    }
                    expect(e != hipSuccess, "reserve reports the failure", combo, stage, k);
                    expect(s.cap == 0 && s.dec_cap == 0, "capacity 0 after a failure", combo, stage, k);
                    expect(!s.hoist_own.p || s.hoist.p, "owner words without slots", combo, stage, k);
                    expect(!g.hoist_slots || !s.hoist.p || s.hoist_own.p, "slots without owner words", combo, stage, k);
                    expect(hipGetLastError() == hipSuccess, "no HIP error left pending", combo, stage, k);
                    expect(s.reserve(n, n_words, g, epoch) == hipSuccess, "the retry succeeds", combo, stage, k);
                }
                check_full(s, g, n, n_words, combo, stage, k);
                for (int t = stage + 1; t < 3; ++t) {   // and it grows on from the recovered state
                    expect(s.reserve(ns[t], 4 * ns[t], g, epoch) == hipSuccess, "later stage", combo, t, k);
                    check_full(s, g, ns[t], 4 * ns[t], combo, t, k);
                }
            }
        }
    }
    std::printf("guard: %d failures\n", failures);
    return failures ? 1 : 0;
}

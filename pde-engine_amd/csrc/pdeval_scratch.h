// pdeval_scratch.h -- the batch-sized device scratch of a validator context (pdeval.hip): the
// work lists between the passes, the per-candidate state of the point stage and tier 2, the
// decoded programs and hoisted prefixes of the lean passes, the shape sort's buffers.  Host code
// only (it compiles for the CPU, tests/hostsim/guard_ctx_scratch.cpp): what depends on kernel
// types comes in as the plain numbers of ScratchCfg.
#pragma once
#include "pdeval_devbuf.h"

namespace pd {

constexpr int kScratchLists = 20;         // PD_N_LISTS of pdeval.hip
constexpr int64_t kScratchMinCap = 1024;   // candidates the scratch holds at least
constexpr int64_t kScratchMinDec = 4096;   // decoded words it holds at least

// filled once, at pdeval_create
struct ScratchCfg {
    // the context's A/B switches: env PDEVAL_HOIST=0 no hoisted prefixes, PDEVAL_HOIST_SLOTS=0 one
    // hoist slot per candidate, PDEVAL_TIER2_MASK=0 tier 2 re-checks the whole grid
    bool hoist = true, hoist_slots = true, tier2_mask = true;
    int64_t hoist_pool_slots = 0;   // 8 * kHoistPool: one pool per XCD (pdeval_grid.h hoist_acquire)
    int64_t hoist_stride = 0;       // doubles per slot, pd::hoist_stride(K)
    int64_t fmask_words = 0;        // failing-lane words per candidate, nx * (ny / 64)
    int64_t t2acc_bytes = 0;        // sizeof(T2Acc)
    size_t (*sort_temp_bytes)(int64_t cap) = nullptr;   // the shape sort's scratch for cap candidates
};

struct Scratch {
    // What every buffer below holds room for: cap candidates and dec_cap decoded words.  Both
    // are 0 unless every buffer does -- a reserve() that fails anywhere leaves them 0, and the
    // next call allocates whatever is missing.
    int64_t cap = 0, dec_cap = 0;
    DevBuf<int64_t> list[kScratchLists];   // the work lists, cap entries each
    DevBuf<uint8_t> pstate, ddps;          // point-stage state; the early double-double tier's classes
    DevBuf<double> dd_res, dd_q;           // speculative provisional passes' outputs (cap * 4, cap)
    // The hoisted prefixes / segments of the lean passes (pdeval_grid.h PD_HOIST).  hoist_slots:
    // hoist_pool_slots slots and their owner words (zero = free), whatever the batch size; the
    // two are present only together, after both allocations and the zeroing succeeded.  The
    // kernels read a missing hoist_own as the other layout, one slot per candidate (A/B).
    DevBuf<double> hoist;
    DevBuf<uint32_t> hoist_own;
    DevBuf<int32_t> hseg;                  // the decoder's hoisted segments, cap x 4 words
    DevBuf<uint64_t> fmask, fsum;          // tier 2's failing lanes (cap x fmask_words) and stored chunks
    DevBuf<uint8_t> status;                // classes when the caller asks for no status output
    DevBuf<double> noise;                  // fp64 noise bounds at the reference points, cap * 4
    DevBuf<uint8_t> t2acc;                 // cap T2Acc entries, zero between launches (tier 2 leaves them so)
    DevBuf<uint64_t> skeys;                // shape sort (pdeval_sort.hip): keys 2 x cap,
    DevBuf<int32_t> sidx;                  // permutation 2 x cap,
    DevBuf<uint8_t> stemp;                 // scratch of stemp_bytes (the block holds at least 16)
    size_t stemp_bytes = 0;
    DevBuf<int32_t> dec;                   // decoded programs of the lean grid passes, dec_cap words + 4

    // Room for a batch of n candidates and n_words program words; never called inside a sized
    // hot call.  `epoch` advances with every pointer that changes (DevBuf::replace).
    hipError_t reserve(int64_t n, int64_t n_words, const ScratchCfg& g, uint64_t& epoch) {
        if (n <= cap && n_words <= dec_cap) return hipSuccess;
        const int64_t c = n <= cap ? cap : n < kScratchMinCap ? kScratchMinCap : n;
        const int64_t w = n_words <= dec_cap ? dec_cap : n_words < kScratchMinDec ? kScratchMinDec : n_words;
        cap = dec_cap = 0;
        hipError_t e = hipSuccess;
        auto ok = [&e](hipError_t r) { return (e = r) == hipSuccess; };
        for (DevBuf<int64_t>& l : list)
            if (!ok(l.replace(c, epoch))) return e;
        if (!ok(pstate.replace(c, epoch)) || !ok(ddps.replace(c, epoch)) ||
            !ok(dd_res.replace(c * 4, epoch)) || !ok(dd_q.replace(c, epoch)))   // (n_ref <= 4)
            return e;
        if (g.hoist && g.hoist_slots && !hoist.p) {   // allocated once, it does not grow with the batch
            if (!ok(hoist.replace(g.hoist_pool_slots * g.hoist_stride, epoch)) ||
                !ok(hoist_own.replace(g.hoist_pool_slots, epoch, true))) {
                hoist.release(epoch);
                return e;
            }
        } else if (g.hoist && !g.hoist_slots) {
            if (!ok(hoist.replace((c > g.hoist_pool_slots ? c : g.hoist_pool_slots) * g.hoist_stride, epoch))) return e;
        }
        if (g.hoist && !ok(hseg.replace(c * 4, epoch))) return e;
        if (g.tier2_mask && (!ok(fmask.replace(c * g.fmask_words, epoch)) || !ok(fsum.replace(c, epoch)))) return e;
        if (!ok(status.replace(c, epoch)) || !ok(noise.replace(c * 4, epoch)) ||
            !ok(t2acc.replace(c * g.t2acc_bytes, epoch, true)) || !ok(skeys.replace(2 * c, epoch)) ||
            !ok(sidx.replace(2 * c, epoch)))
            return e;
        stemp_bytes = g.sort_temp_bytes(c);
        if (!ok(stemp.replace(stemp_bytes ? (int64_t)stemp_bytes : 16, epoch))) return e;
        // + 4 words: the lean interpreter reads an opcode word with the two after it (pdeval_grid.h)
        if (!ok(dec.replace(w + 4, epoch))) return e;
        cap = c;
        dec_cap = w;
        return hipSuccess;
    }
};

}  // namespace pd

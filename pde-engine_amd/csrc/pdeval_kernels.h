// pdeval_kernels.h -- the gfx950 candidate-validation kernel.
//
// One wavefront validates one candidate.  Its 64 lanes are 64 sample points; the wave walks
// the candidate's postfix program (wave-uniform, read with scalar loads, so the interpreter
// never diverges), evaluating it in jet arithmetic (jet.h) with a register-resident operand
// stack, then applies the problem's residual operator in an epilogue:
//   force-free  det[[L_T A, L_T B], [L_T^2 A, L_T^2 B]]   (problems/force_free/validator.py:323-347)
//   Kerr        d_r[G/(1-x^2) d_r u] + d_x[G/Delta d_x u]  (problems/kerr_magnetosphere/validator.py:77-91)
// and a scaled zero test q = |residual| / S, S = the same epilogue evaluated on magnitudes
// (DESIGN.md "Zero test").  Chunk 0 carries the reference point(s) in its first lanes, so the
// reference's point stage (validator.py:349-402 / kerr :163-192) is decided first; the grid
// chunks then play the role of the symbolic stage (validator.py:404-427 / kerr :283-315).
// Per-lane statistics are reduced across the wave with DPP/shuffles; lane 0 writes the
// per-candidate outputs and sets the verdict bit with one atomicOr.
#pragma once
#include <stdint.h>

#include <type_traits>

#include "../../include/pdeval.h"
#include "jet.h"

namespace pd {

// The problem's constants for one stage (Kerr M and a, PDEVAL_IMM_PRM): {M, a, 1/M, 1/a, M^2,
// a^2, 1/M^2, 1/a^2} as the coordinate type V (double, or dd in the double-double point tier).  The point stage gets the
// validator's M_value, a_value; the constant test and the grid stage the stand-ins of the
// symbols (pdeval_kerr_constants).  Passed by value: 4 wave-uniform values, scalar selects.
template <class V> struct PrmTab {
    V v[8];
};
template <class V> PD_HD V prm_value(const PrmTab<V>& t, uint32_t d) {
    const uint32_t k = d & 7u;
    const V lo = (k & 1u) ? ((k & 2u) ? t.v[3] : t.v[1]) : ((k & 2u) ? t.v[2] : t.v[0]);
    const V hi = (k & 1u) ? ((k & 2u) ? t.v[7] : t.v[5]) : ((k & 2u) ? t.v[6] : t.v[4]);
    const V v = (k & 4u) ? hi : lo;
    return (d & PDEVAL_PRM_NEG) ? -v : v;
}

struct KernelArgs {
    const int32_t* ops;
    const int64_t* offsets;
    int64_t n_words;            // size of ops[] (programs are bounds-checked against it)
    int64_t n;                  // candidates in the batch
    const int64_t* list;        // optional: wave -> candidate index (NULL = identity)
    const int32_t* list_count;  // optional device count for list (persistent passes)
    int64_t list_cap;
    // sample points: chunk 0 holds the reference points (lanes < n_ref), chunk c >= 1 the grid
    // row x = gx[(c-1) / (ny/64)] (one x per chunk: a scalar), y = gy[.. + lane]
    double ref_x[4], ref_y[4];
    dd ref_xd[4], ref_yd[4];    // the same reference points as double-doubles (exact rationals)
    dd kc_ref[16];              // Kerr: operator coefficients at the reference points, dd
    const double* gx;           // nx grid abscissae
    const double* gy;           // ny grid ordinates (ny % 64 == 0)
    int nx, ny;
    const double* kc;           // Kerr: 4 operator coefficients per point (NULL for FF)
    const double* kc2;          // Kerr: the same with the first two doubled (lean grid passes)
    // coordinate-power tables of the lean grid passes (pdeval_grid.h ptab_kernel, built once per
    // context), or NULL: the jets C(n,k) v^(n-k), k <= K, of v**n for 0 <= n <= 16 at every
    // grid abscissa ([n][row][k], wave-uniform) and ordinate ([n][k][j], lane j)
    const double* ptab;
    int n_ref;
    int n_pts;                  // n_ref + nx * ny
    int fp_pts[PDEVAL_FP_N];    // point indices whose u value is the fingerprint
    pdeval_params prm;
    pdeval_outputs out;
    int64_t* defer_list;        // candidates this variant cannot take (deeper stack)
    int32_t* defer_count;
    int64_t* cplx_list;         // FF candidates non-finite at the reference point
    int32_t* cplx_count;
    int64_t list_capacity;      // capacity of defer_list and cplx_list (appends beyond are dropped)
    int64_t* esc_list;          // tier-2 escalations: cand | ESC_* flags << 48
    int32_t* esc_count;
    uint8_t* pstate;            // point-stage state per candidate (P0_*), or NULL
    uint8_t* ddps;              // the early double-double tier's result per candidate (dd_point_kernel<DEFER>)
    // (PD_DD_SPEC) the provisional point passes (P0_PROV) evaluated speculatively in the early
    // tier: their res_ref / q_ref go to these side arrays (n * n_ref, n; a NaN sentinel where
    // not written) and dd_apply_kernel copies them out only if the final class calls for the
    // double-double value -- the rule the late tier applied after the grid
    double* dd_res;
    double* dd_q;
    int dd_spec;
    int64_t* pdeep_list;        // real programs deeper than pass 0's stack: the deep point pass
    int32_t* pdeep_count;
    double* noise_ref;          // n * n_ref fp64 noise bounds at the reference points (point stage)
    struct T2Acc* t2acc;        // tier 2: one accumulator per list entry (pdeval_tier2.h), zeroed
    const int32_t* perm;        // order of pass 0 and the tier-B collect pass (pdeval_sort.hip), or NULL
    int32_t* dec;               // n_words: the programs pre-decoded for the lean grid passes
    uint64_t* fmask;            // lean passes: per candidate and 64-point grid chunk, the lanes
                                // that failed the tier-1 test (what tier 2 re-checks); NULL = none
    uint64_t* fsum;             // ... per candidate, the chunks whose fmask word was written (bit
                                // per chunk, <= 64 chunks; ~0 = every word): the lean passes store
                                // only the non-zero words
    int32_t* hseg;              // decoder: per candidate {original word, start, end, y?} of its
                                // hoisted segment (start 0: none; pdeval_grid.h PD_HOIST_SUB)
    double* hoist;              // lean passes: per slot (hoist_stride doubles), the pure
                                // coefficients of a candidate's hoisted prefix at every grid row
                                // or lane and, Kerr, its hoisted segment's jets (pdeval_grid.h
                                // PD_HOIST); NULL = nothing hoisted
    uint32_t* hoist_own;        // one owner word per slot (0 = free): a running wave holds the
                                // slot of its candidate (pdeval_grid.h hoist_acquire)
    int hoist_pool;             // slots per XCD (8 pools); a split launch indexes by candidate
    int64_t* one_list;          // decoder: the force-free candidates of one coordinate alone, which
    int32_t* one_count;         // grid_one_kernel evaluates at 64 points (pdeval_grid.h PD_ONECOORD);
                                // NULL = none (every candidate takes pass 1)
    // the problem's constants per stage (PDEVAL_IMM_PRM; Kerr M, a): point stage (fp64 and
    // double-double) and the constant test / grid stage
    PrmTab<double> prm_pt, prm_grid;
    PrmTab<dd> prm_pt_dd, prm_grid_dd;
    // Kerr constant test (pdeval_point.h): points where u's gradient must be rounding noise
    double ct_x[8], ct_y[8];
    int n_ct;
    // device error word (d_counts[PD_N_LISTS], zeroed with the counters at every launch chain):
    // bit k = a work-list entry outside [0, n) met by kernel family k (checked_cand), which is
    // then skipped; the host turns a non-zero word into an error of the call
    uint32_t* errw;
    // persistent list kernels: the head of their work queue (a zeroed counter per launch), or
    // NULL for the static schedule (item blockIdx.x, then + gridDim.x)
    uint32_t* qhead;
    int qchunk;                 // items per grab of the work queue
};

// The work items of a persistent one-wave block: the static schedule (item blockIdx.x, then
// + gridDim.x), or -- when the launch has a queue head -- chunks of a.qchunk consecutive items
// taken with one atomic each (a wave that finishes early takes the next chunk).
#ifndef PD_QUEUE
#define PD_QUEUE 1
#endif
struct WorkQueue {
    int64_t end = 0;   // end of the current chunk (queue mode)
    __device__ __forceinline__ int64_t grab(const KernelArgs& a) {
        uint32_t v = 0;
        if ((threadIdx.x & 63) == 0) v = atomicAdd(a.qhead, (uint32_t)a.qchunk);
        const int64_t b = (int64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)v);
        end = b + a.qchunk;
        return b;
    }
    __device__ __forceinline__ int64_t first(const KernelArgs& a) { return PD_QUEUE && a.qhead ? grab(a) : (int64_t)blockIdx.x; }
    __device__ __forceinline__ int64_t next(const KernelArgs& a, int64_t wp) {
        if (!PD_QUEUE || !a.qhead) return wp + gridDim.x;
        return wp + 1 < end ? wp + 1 : grab(a);
    }
};

// A candidate index read from a work list or the shape permutation, checked: an entry outside
// [0, n) -- a list read before its write completed, or a corrupt list -- is recorded in the
// error word (bit `code`) and the caller skips it, instead of indexing the batch with it.
enum : uint32_t {
    ERRW_PERM = 1u, ERRW_GRID_LIST = 2u, ERRW_GENERIC = 4u, ERRW_POINT_LIST = 8u, ERRW_DD = 16u,
    ERRW_DD_APPLY = 32u, ERRW_TIER2 = 64u, ERRW_CPLX = 128u, ERRW_HOIST = 256u, ERRW_ONE = 512u
};
#ifndef PD_CHECK_LISTS
#define PD_CHECK_LISTS 1
#endif
__device__ __forceinline__ int64_t checked_cand(const KernelArgs& a, int64_t cand, uint32_t code) {
    if (!PD_CHECK_LISTS || (cand >= 0 && cand < a.n)) return cand;
    if (a.errw) atomicOr(a.errw, code);
    return -1;
}

// Partial grid counts of one tier-2 list entry whose grid is split over several waves.
struct T2Acc {
    int32_t nb1, nb2, nfin, nnonfin;
    unsigned long long qmax_bits;   // max of non-negative doubles = max of their bit patterns
    uint32_t grad;
    int32_t done;                   // parts merged so far
};

// doubles per candidate of the hoist buffer (pdeval_grid.h PD_HOIST): the prefix's K + 1 pure
// coefficients and, Kerr (K = 2) only, the segment's nc(K) coefficients, 64 rows (or lanes) each
// (force-free hoists no segments: 2.5 KiB per candidate instead of 10)
PD_HD constexpr size_t hoist_stride(int K) { return (size_t)(K + 1 + (K == 4 ? 0 : (K + 1) * (K + 2) / 2)) * 64; }
// slots of the hoist buffer per XCD: more than the waves one XCD holds at once (32 CUs x 4
// SIMDs x <= 6 waves/SIMD in pass 1 = 768), so a wave finds a free slot within a few probes;
// 8 x 1536 slots = 30 MiB force-free, 54 MiB Kerr, whatever the batch size
constexpr int kHoistPool = 1536;

// Escalation flags (bits 48.. of a tier-2 list entry; the candidate index is the low 48 bits).
enum : uint32_t {
    ESC_POINT = 1,      // the point stage failed its scaled test (tier 1)
    ESC_GRID_EVAL = 2,  // the grid was evaluated in tier 1 (full_grid, or the point passed)
    ESC_GRID_FAIL = 4,  // ... and had more than max_bad failing points
    ESC_ANY_GRAD = 8,   // tier 1 saw a finite point with a non-zero gradient
    ESC_NFIN = 16,      // tier 1 saw at least one finite grid point
    ESC_MASK = 32,      // ... and recorded its failing points in a.fmask (the lean passes)
};
// Point-stage state per candidate (pdeval_point.h).  Bits 0-1: P0_NONE (not decided: malformed
// program, the grid pass runs its own chunk 0), P0_PASS, P0_REJECT (final).  Flags:
//   P0_CPLX  not real at the reference point: the complex passes take the candidate
//   P0_PROV  passed provisionally (|res| within kappa x fp64 noise): if the grid accepts or
//            rejects, the double-double tier re-decides the point stage (it may be a REJECT_POINT)
//   P0_GRAD  a reference point has a non-zero gradient
//   P0_DD    undecided in fp64 (value too close to its noise or to a threshold): treated as
//            PASS by the grid passes, decided by the double-double tier at the end
//   P0_CONST (Kerr) u is constant: at every reference point its gradient lies within the
//            error bound of its rounding (kerr validator.py:231-240 drops u when simplify(u) has
//            neither r nor x; a constant's computed gradient is rounding noise, never exactly 0)
//   P0_NZ    a reference point's residual is CERTAINLY non-zero (beyond kappa x its noise bound)
//            yet below the point stage's threshold: the residual is not identically zero, so the
//            reference's symbolic stage cannot reduce it to 0 (force-free validator.py:404-427,
//            Kerr :283-315) and a grid ACCEPT becomes REJECT_GRID (dd_collect / dd_point)
enum : uint8_t { P0_NONE = 0, P0_PASS = 1, P0_REJECT = 2, P0_CPLX = 4, P0_PROV = 8, P0_GRAD = 16,
                 P0_DD = 32, P0_CONST = 64, P0_NZ = 128 };

// The one-candidate-per-lane interpreters (ValInterp::run of the double-double point tier,
// ErrInterp::run_s of the point / tier-2 stages) are force-inlined: as calls, the complex and
// double-double instances kept their arguments and the by-value kernel arguments they referenced
// in scratch (dd_point_kernel<0,dd,2>: 2,036 -> 144 B per lane; tier-2 complex 1,744 -> 656 B).
// PD_DD_INLINE=0 / PD_T2_INLINE=0 give the compiler back the choice (A/B variants).
#ifndef PD_DD_INLINE
#define PD_DD_INLINE 1
#endif
#ifndef PD_T2_INLINE
#define PD_T2_INLINE 1
#endif
#if PD_DD_INLINE
#define PD_DD_INLINE_ATTR __forceinline__
#else
#define PD_DD_INLINE_ATTR
#endif
#if PD_T2_INLINE
#define PD_T2_INLINE_ATTR __forceinline__
#else
#define PD_T2_INLINE_ATTR
#endif

#define PD_ESC_SHIFT 48
#define PD_ESC_CAND_MASK ((1ll << PD_ESC_SHIFT) - 1)

// Append a candidate to a device work list (lane 0 only).  Returns false when the list is
// full -- impossible when capacity >= n, which the host guarantees; checked anyway so a bad
// call can never write out of bounds.
__device__ __forceinline__ bool list_append(int64_t* list, int32_t* count, int64_t cap, int64_t cand) {
    const int slot = atomicAdd(count, 1);
    if (slot >= cap) return false;
    list[slot] = cand;
    return true;
}

template <class T> struct Real;
template <> struct Real<double> { static constexpr bool cplx_pass = false; };
template <> struct Real<cplx> { static constexpr bool cplx_pass = true; };
template <> struct Real<dd> { static constexpr bool cplx_pass = false; };
template <> struct Real<cdd> { static constexpr bool cplx_pass = true; };
template <class T> PD_HD T imag_unit();
template <> PD_HD cplx imag_unit<cplx>() { return {0.0, 1.0}; }
template <> PD_HD cdd imag_unit<cdd>() { return {{0.0, 0.0}, {1.0, 0.0}}; }

// Program words are wave-uniform: read them through the constant address space so they
// become scalar loads (s_load_dword, served by the scalar cache) instead of vector loads +
// readfirstlane -- one such dependent load per opcode per chunk was a large share of the
// interpreter's time.
#ifndef PD_HOST_SIM
typedef const __attribute__((address_space(4))) uint32_t* cword_ptr;
#else
typedef const uint32_t* cword_ptr;   // tests/hostsim: the interpreter on the CPU, one lane
#endif
__device__ __forceinline__ uint32_t rd_word(const int32_t* p) {
    return *(cword_ptr)(p);
}
__device__ __forceinline__ double rd_imm(const int32_t* p) {
    // the two words following an opcode hold the f64 immediate, low word first
    const uint32_t lo = *(cword_ptr)(p);
    const uint32_t hi = *(cword_ptr)(p + 1);
    return __hiloint2double((int)hi, (int)lo);
}
// a wave-uniform double (grid abscissa) through the scalar cache
__device__ __forceinline__ double rd_sf64(const double* p) {
#ifndef PD_HOST_SIM
    return *(const __attribute__((address_space(4))) double*)(p);
#else
    return *p;
#endif
}
// a value the caller knows to be the same in every lane, moved into scalar registers (a row's
// powers of 1/x: held in VGPRs they cost the interpreter 4 of its registers)
__device__ __forceinline__ double uniform_f64(double v) {
#ifndef PD_HOST_SIM
    return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)),
                            __builtin_amdgcn_readfirstlane(__double2loint(v)));
#else
    return v;
#endif
}
// a value the optimizer must treat as unknown from here on (no rematerialization, no
// rewriting of expressions that use it)
__device__ __forceinline__ void pin_f64(double& v) {
#ifndef PD_HOST_SIM
    asm volatile("" : "+v"(v));
#else
    (void)v;
#endif
}
// an immediate that may be one of the problem's constants (PDEVAL_IMM_PRM)
__device__ __forceinline__ double rd_immp(const int32_t* p, uint32_t w, const PrmTab<double>& P) {
    if (w & PDEVAL_IMM_PRM) return prm_value(P, rd_word(p));
    return rd_imm(p);
}
__device__ __forceinline__ bool op_has_imm(uint32_t op) {
    return op == PDOP_PUSH_C || op == PDOP_ADDC || op == PDOP_MULC || op == PDOP_RDIVC ||
           op == PDOP_POW;
}

template <class T, int K> struct JetOps {
    static constexpr int NC = nc(K);
    struct J { T c[NC]; };

    static PD_HD void set_const(J& t, T v) {
        t.c[0] = v;
#pragma unroll
        for (int i = 1; i < NC; ++i) t.c[i] = zero<T>();
    }
    // coordinate operations take the coordinate as V = double, or dd in the double-double tier
    template <class V> static PD_HD void set_var(J& t, V v, int axis) {
        set_const(t, cvt<T>(v));
        t.c[axis == 0 ? ji(1, 0) : ji(0, 1)] = from_real<T>(1.0);
    }
    static PD_HD void add(const J& a, J& t) {
#pragma unroll
        for (int i = 0; i < NC; ++i) t.c[i] = a.c[i] + t.c[i];
    }
    static PD_HD void sub(const J& a, J& t) {  // t = a - t
#pragma unroll
        for (int i = 0; i < NC; ++i) t.c[i] = a.c[i] - t.c[i];
    }
    static PD_HD void rsub(const J& a, J& t) {  // t = t - a
#pragma unroll
        for (int i = 0; i < NC; ++i) t.c[i] = t.c[i] - a.c[i];
    }
    // t = a * t in place: outputs in decreasing total degree; c_ij reads t_kl only for
    // (k,l) <= (i,j), and no other output of degree i+j reads t_ij, so overwriting is safe
    // (saves a jet of registers against a separate result)
#ifndef PD_MUL_TMP
#define PD_MUL_TMP 0
#endif
    static PD_HD void mul(const J& a, J& t) {
        if constexpr (PD_MUL_TMP) {   // (codegen variant: the product into a temporary, then copied)
            J r;
            jmul<T, K, K, K>(a.c, t.c, r.c);
            t = r;
            return;
        }
#pragma unroll
        for (int d = K; d >= 0; --d) {
#pragma unroll
            for (int j = 0; j <= d; ++j) {
                const int i = d - j;
                T s = a.c[0] * t.c[ji(i, j)];
#pragma unroll
                for (int d1 = 1; d1 <= d; ++d1)
#pragma unroll
                    for (int j1 = 0; j1 <= d1; ++j1) {
                        const int i1 = d1 - j1, i2 = i - i1, j2 = j - j1;
                        if (i2 < 0 || j2 < 0) continue;
                        s = fmac(a.c[ji(i1, j1)], t.c[ji(i2, j2)], s);
                    }
                t.c[ji(i, j)] = s;
            }
        }
    }
    static PD_HD void div(const J& a, J& t) {  // t = a / t
        J r;
        jdiv<T, K>(a.c, t.c, r.c);
        t = r;
    }
    // t = t / a in place: outputs in increasing degree; c_dj needs t_dj (read before it is
    // overwritten) and outputs of lower degree (already in t)
    static PD_HD void rdiv(const J& a, J& t) {
        const T inv = recip(a.c[0]);
#pragma unroll
        for (int d = 0; d <= K; ++d) {
#pragma unroll
            for (int j = 0; j <= d; ++j) {
                const int i = d - j;
                T s = t.c[ji(i, j)];
#pragma unroll
                for (int d1 = 1; d1 <= d; ++d1)
#pragma unroll
                    for (int j1 = 0; j1 <= d1; ++j1) {
                        const int i1 = d1 - j1, i2 = i - i1, j2 = j - j1;
                        if (i2 < 0 || j2 < 0) continue;
                        s = fmac(-a.c[ji(i1, j1)], t.c[ji(i2, j2)], s);
                    }
                t.c[ji(i, j)] = qdiv(s, a.c[0], inv);
            }
        }
    }
    static PD_HD void scale(J& t, T s) {
#pragma unroll
        for (int i = 0; i < NC; ++i) t.c[i] = t.c[i] * s;
    }
    // t *= (v + d_axis)
    template <class V> static PD_HD void mul_var(J& t, V v, int axis) {
        const T vv = cvt<T>(v);
#pragma unroll
        for (int d = K; d >= 0; --d) {
#pragma unroll
            for (int j = 0; j <= d; ++j) {
                const int i = d - j;
                T s = t.c[ji(i, j)] * vv;
                if (axis == 0 && i > 0) s = s + t.c[ji(i - 1, j)];
                if (axis == 1 && j > 0) s = s + t.c[ji(i, j - 1)];
                t.c[ji(i, j)] = s;
            }
        }
    }
    // t /= (v + d_axis)
    template <class V> static PD_HD void div_var(J& t, V v, int axis) {
        const T vv = cvt<T>(v);
        const T inv = cvt<T>(rcp(v));
#pragma unroll
        for (int d = 0; d <= K; ++d) {
#pragma unroll
            for (int j = 0; j <= d; ++j) {
                const int i = d - j;
                T s = t.c[ji(i, j)];
                if (axis == 0 && i > 0) s = s - t.c[ji(i - 1, j)];
                if (axis == 1 && j > 0) s = s - t.c[ji(i, j - 1)];
                t.c[ji(i, j)] = qdiv(s, vv, inv);
            }
        }
    }
    // ---- coordinate powers p = v^n along an axis (PDOP_*_P): p_k = C(n,k) v^(n-k), k <= K.
    // Every index below is a compile-time constant after unrolling (axis is a template
    // parameter, n enters only through values), so the jets stay in registers.
    template <int N, class V> static PD_HD void pco_small(V v, V* pk) {   // N < K
        V vp[N + 1];
        vp[0] = vone<V>();
#pragma unroll
        for (int k = 1; k <= N; ++k) vp[k] = vp[k - 1] * v;
        double b = 1.0;
#pragma unroll
        for (int k = 0; k <= K; ++k) {
            pk[k] = k <= N ? vp[k <= N ? N - k : 0] * b : vzero<V>();
            b = b * (double)(N - k) / (double)(k + 1);
        }
    }
    template <class V> static PD_HD void pcoefs(V v, int n, V* pk) {
        if constexpr (K > 2) {
            if (n == 2) { pco_small<2>(v, pk); return; }
        }
        if constexpr (K > 3) {
            if (n == 3) { pco_small<3>(v, pk); return; }
        }
        V base = vone<V>();                 // v^(n-K), n >= K here
        for (int e = 0; e < n - K; ++e) base = base * v;
        V pw[K + 1];
        pw[K] = base;
#pragma unroll
        for (int k = K - 1; k >= 0; --k) pw[k] = pw[k + 1] * v;
        double b = 1.0;
#pragma unroll
        for (int k = 0; k <= K; ++k) {
            pk[k] = pw[k] * b;
            b = b * (double)(n - k) / (double)(k + 1);
        }
    }
    template <int AX> static PD_HD constexpr int pidx(int k, int other) { return AX == 0 ? ji(k, other) : ji(other, k); }
    template <int AX, class V> static PD_HD void set_p(J& t, const V* pk) {
        set_const(t, cvt<T>(pk[0]));
#pragma unroll
        for (int k = 1; k <= K; ++k) t.c[pidx<AX>(k, 0)] = cvt<T>(pk[k]);
    }
    template <int AX, class V> static PD_HD void add_p(J& t, const V* pk, double sg) {
#pragma unroll
        for (int k = 0; k <= K; ++k) t.c[pidx<AX>(k, 0)] = t.c[pidx<AX>(k, 0)] + cvt<T>(pk[k] * sg);
    }
    // t *= p in place (decreasing degree: c_ij reads t at lower orders along the axis)
    template <int AX, class V> static PD_HD void mul_p(J& t, const V* pk) {
#pragma unroll
        for (int d = K; d >= 0; --d) {
#pragma unroll
            for (int j = 0; j <= d; ++j) {
                const int i = d - j;
                const int ia = AX == 0 ? i : j, io = AX == 0 ? j : i;
                T s = t.c[ji(i, j)] * pk[0];
#pragma unroll
                for (int k = 1; k <= K; ++k)
                    if (k <= ia) s = fmac(t.c[pidx<AX>(ia - k, io)], cvt<T>(pk[k]), s);
                t.c[ji(i, j)] = s;
            }
        }
    }
    // t /= p in place (increasing degree)
    template <int AX, class V> static PD_HD void div_p(J& t, const V* pk) {
        const T b0 = cvt<T>(pk[0]);
        const T inv = cvt<T>(rcp(pk[0]));
#pragma unroll
        for (int d = 0; d <= K; ++d) {
#pragma unroll
            for (int j = 0; j <= d; ++j) {
                const int i = d - j;
                const int ia = AX == 0 ? i : j, io = AX == 0 ? j : i;
                T s = t.c[ji(i, j)];
#pragma unroll
                for (int k = 1; k <= K; ++k)
                    if (k <= ia) s = fmac(t.c[pidx<AX>(ia - k, io)], cvt<T>(-pk[k]), s);
                t.c[ji(i, j)] = qdiv(s, b0, inv);
            }
        }
    }
    // the opcode's action on the top of stack for a fixed axis
    template <int AX, class V> static PD_HD void p_op(uint32_t op, J& t, const V* pk) {
        if (op == PDOP_ADD_P) add_p<AX>(t, pk, 1.0);
        else if (op == PDOP_SUB_P) add_p<AX>(t, pk, -1.0);
        else if (op == PDOP_MUL_P) mul_p<AX>(t, pk);
        else if (op == PDOP_DIV_P) div_p<AX>(t, pk);
        else {  // RDIV_P: t = p / t
            J p;
            set_p<AX>(p, pk);
            div(p, t);
        }
    }
    static PD_HD void rdivc(J& t, T c) {  // t = c / t
        J a;
        set_const(a, c);
        div(a, t);
    }
    // t = t*t with the symmetric half of the products (into a temporary: computing it in place
    // was measured to raise pass 1's scratch from 64 to 80 bytes per lane)
    static PD_HD void square(J& t) {
        J r;
#pragma unroll
        for (int d = K; d >= 0; --d) {
#pragma unroll
            for (int j = 0; j <= d; ++j) {
                T s = zero<T>();
                bool first = true;
                // pairs (k, d-k) of degrees with k <= d-k; the (i1,j1) x (i2,j2) terms with
                // (i1,j1) < (i2,j2) lexicographically are doubled
#pragma unroll
                for (int d1 = 0; d1 <= d; ++d1) {
#pragma unroll
                    for (int j1 = 0; j1 <= d1; ++j1) {
                        const int i1 = d1 - j1, i = d - j, i2 = i - i1, j2 = j - j1;
                        if (i2 < 0 || j2 < 0) continue;
                        const int k1 = ji(i1, j1), k2 = ji(i2, j2);
                        if (k1 > k2) continue;
                        const T prod = (k1 == k2) ? t.c[k1] * t.c[k2] : (t.c[k1] + t.c[k1]) * t.c[k2];
                        s = first ? prod : s + prod;
                        first = false;
                    }
                }
                r.c[ji(d - j, j)] = s;
            }
        }
        t = r;
    }
    static PD_HD void pown(J& t, int n) {  // 2 <= n <= 16
        if (n == 2) {
            square(t);
            return;
        }
        J base = t;
        if (n == 3) {
            square(t);
            mul(base, t);
            return;
        }
        if (n == 4) {
            square(t);
            square(t);
            return;
        }
        // general: t = base^n by repeated multiplication (rare exponents)
        for (int k = 1; k < n; ++k) mul(base, t);
    }
    static PD_HD void powa(J& t, double alpha) {
        T f[K + 1];
        coef_pow<T, K>(t.c[0], alpha, pow_real_exp(t.c[0], alpha), f);
        jcompose<T, K>(t.c, f);
    }
    static PD_HD void sqrtj(J& t) {
        T f[K + 1];
        coef_pow<T, K>(t.c[0], 0.5, sqrt_(t.c[0]), f);
        jcompose<T, K>(t.c, f);
    }
    static PD_HD void expj(J& t) {
        T f[K + 1];
        f[0] = exp_(t.c[0]);
#pragma unroll
        for (int k = 1; k <= K; ++k) f[k] = divk(f[k - 1], 1.0, k);
        jcompose<T, K>(t.c, f);
    }
    static PD_HD void logj(J& t) {
        T f[K + 1];
        const T r = recip(t.c[0]);
        f[0] = log_(t.c[0]);
        T rk = r;
#pragma unroll
        for (int k = 1; k <= K; ++k) {
            f[k] = divk(rk, (k & 1) ? 1.0 : -1.0, k);
            rk = rk * r;
        }
        jcompose<T, K>(t.c, f);
    }
};

// |x| of a jet: sign(x0) * x away from the kink; at x0 == 0 (or non-real x0) undefined.
template <int K> __device__ __forceinline__ void absj(typename JetOps<double, K>::J& t) {
    const double s = t.c[0] > 0.0 ? 1.0 : (t.c[0] < 0.0 ? -1.0 : NAN);
    JetOps<double, K>::scale(t, s);
}
template <int K> __device__ __forceinline__ void absj(typename JetOps<cplx, K>::J& t) {
    // Abs of a complex value is not holomorphic: only real arguments are meaningful
    const double s = (t.c[0].im == 0.0) ? (t.c[0].re > 0.0 ? 1.0 : (t.c[0].re < 0.0 ? -1.0 : NAN)) : NAN;
    JetOps<cplx, K>::scale(t, from_real<cplx>(s));
}
template <int K> __device__ __forceinline__ void absj(typename JetOps<dd, K>::J& t) {
    const double s = t.c[0].hi > 0.0 ? 1.0 : (t.c[0].hi < 0.0 ? -1.0 : NAN);
    JetOps<dd, K>::scale(t, from_real<dd>(s));
}
template <int K> __device__ __forceinline__ void absj(typename JetOps<cdd, K>::J& t) {
    const double s = is_zero(t.c[0].im) ? (t.c[0].re.hi > 0.0 ? 1.0 : (t.c[0].re.hi < 0.0 ? -1.0 : NAN)) : NAN;
    JetOps<cdd, K>::scale(t, from_real<cdd>(s));
}

// ------------------------------------------------------------------ residual epilogues
// A sample point counts as finite only if every Taylor coefficient of u is below 2^160: the
// residual is then free of intermediate overflow in any evaluation order (force-free S is of
// degree 6 in the coefficients), so the device and the oracle agree on which points exist.
constexpr double kHugeJet = 0x1p160;
// Kerr reference points: a jet whose every coefficient AND every rounding bound is below 2^-900
// (or a bound that is not finite: 0 * inf in the bound of an underflowed base) has underflowed,
// e.g. exp_neg(exp(r/a**2)) at a = 1/10.  The reference's N(lhs, 40) has no exponent limit and
// finds |lhs| astronomically small there, so such a point PASSES the fast point check
// (kerr validator.py:163-192) and is no evidence of a constant (the constant test, :231-240, is
// structural: exp(-exp(r/a**2)) has r).  A u that cancels exactly (-x/(1 - x) - 1 + 1/(1 - x))
// has zero coefficients too, but rounding bounds of the size of its terms: not an underflow.
constexpr double kTinyJet = 0x1p-900;
// The fingerprint value of u at a point: u itself, or Re u + sqrt(2) Im u for a complex u -- a
// complex constant has a flat fingerprint, a purely imaginary non-constant one does not (the
// host's zero-gradient re-check looks only at flat fingerprints, pdeval/batch.py)
constexpr double kFpIm = 0x1.6a09e667f3bcdp+0;
__device__ __forceinline__ double fp_value(double v) { return v; }
__device__ __forceinline__ double fp_value(cplx v) { return v.re + kFpIm * v.im; }
template <class T, int NC> __device__ __forceinline__ bool underflowed(const double* m, const double* e) {
    bool t = true;
#pragma unroll
    for (int i = 0; i < NC; ++i) t = t && m[i] < kTinyJet && !(e[i] >= kTinyJet);
    return t;
}
__device__ __forceinline__ bool jet_coef_ok(double v) { return fabs(v) < kHugeJet; }
__device__ __forceinline__ bool jet_coef_ok(cplx v) { return fabs(v.re) < kHugeJet && fabs(v.im) < kHugeJet; }
struct PointResult {
    double res_re, res_im;  // residual (complex pass: both parts)
    double res_abs;         // |residual|
    double scale;           // S
    bool grad_zero;         // u_x == u_y == 0 exactly
    bool finite;
    uint64_t fin_lanes;     // the wave's lanes where `finite` holds (grid passes; PD_BALLOT_SPLIT)
};
// The grid passes count finite points with a ballot of `finite`.  `finite` is an AND of several
// compares, and a ballot of such an AND is lowered as a select of 0/1 into a VGPR and a compare
// of it (2 VALU per ballot, twice per point); a ballot of one compare is the compare's own lane
// mask.  So the lean epilogues form fin_lanes as the AND of the ballots of the individual
// compares (the same lanes), and grid_body ballots only the zero test's compare beside it.
#ifndef PD_BALLOT_SPLIT
#define PD_BALLOT_SPLIT 1
#endif
// isfinite as a plain compare (|x| <= DBL_MAX: false for an infinity and for NaN), so that its
// ballot folds: isfinite itself lowers to v_cmp_class, which the ballot combine does not match
__device__ __forceinline__ bool finite_cmp(double x) { return fabs(x) <= 0x1.fffffffffffffp+1023; }
__device__ __forceinline__ uint64_t ballot64(bool b) {
#ifndef PD_HOST_SIM
    return __builtin_amdgcn_ballot_w64(b);
#else
    return __ballot(b);
#endif
}

// Force-free foliation determinant from the order-4 jet of u.
// p = u_rho, q = u_z (order 3);  A = p_rho + q_z - p/rho,  B = p^2 + q^2 (order 2);
// LA = q A_rho - p A_z, LB = q B_rho - p B_z (order 1);  L2A = q LA_rho - p LA_z (order 0);
// det = LA * L2B - LB * L2A.   (validator.py:323-347; Omega = 0 on the problem path)
// Rotating field lines, a constant Omega (validator.py:326-329, om2 = Omega^2 != 0):
// A = (1 - rho^2 om2)(u_rr + u_zz) - (1 + rho^2 om2)/rho u_r = A_0 - om2 (rho^2 (u_rr + u_zz) + rho u_r)
// and B = (1 - rho^2 om2) B_0: corrections of A_0 and B_0 in ff_rotate_A / _B, out of line
// behind a uniform branch, so the Omega = 0 epilogue is the same code as before.
// MAG = true evaluates the same expression on magnitudes with every difference turned into
// a sum: S >= sum of |monomials| of the fully expanded determinant.
#ifndef PD_BSYM
#define PD_BSYM 1
#endif
// the force-free finiteness guards as one maximum of the coefficient magnitudes (ff_epilogue_p)
#ifndef PD_FF_GUARD_MAX
#define PD_FF_GUARD_MAX 1
#endif
__device__ __forceinline__ double max_abs(double a, double b);
#ifndef PD_AFMA
#define PD_AFMA 1
#endif
PD_HD bool om2_nz(double w) { return w != 0.0; }
PD_HD bool om2_nz(dd w) { return w.hi != 0.0; }

template <class T, bool MAG> struct FFEpi {
    // Everything is read straight from u's Taylor coefficients (no materialized copies of
    // p = u_rho, q = u_z), and each intermediate dies as soon as its Lie derivative is
    // formed: this keeps the epilogue's live set small enough for more waves per SIMD.
    static PD_HD T sgn(T a) { return MAG ? a : -a; }
    // MAG: read |c_ij| (a free source modifier on the VALU), so no copy of u is made
    static PD_HD T rd(const T* u, int k) {
        if constexpr (MAG) return fabs(u[k]);
        else return u[k];
    }
    static PD_HD T U(const T* u, int i, int j) { return rd(u, ji(i, j)); }
    // p_ij = (i+1) c_{i+1,j},  q_ij = (j+1) c_{i,j+1}
    static PD_HD T P(const T* u, int i, int j) { return rd(u, ji(i + 1, j)) * (double)(i + 1); }
    static PD_HD T Q(const T* u, int i, int j) { return rd(u, ji(i, j + 1)) * (double)(j + 1); }

    // L_T f (order 1) = q f_rho - p f_z for f of order 2
    static PD_HD void lie1(const T* u, const T* f, T* out) {
        const T p00 = P(u, 0, 0), p10 = P(u, 1, 0), p01 = P(u, 0, 1);
        const T q00 = Q(u, 0, 0), q10 = Q(u, 1, 0), q01 = Q(u, 0, 1);
        // f is an intermediate (already a magnitude in the MAG evaluation)
        const T fr00 = f[ji(1, 0)], fr10 = f[ji(2, 0)] * 2.0, fr01 = f[ji(1, 1)];
        const T fz00 = f[ji(0, 1)], fz10 = f[ji(1, 1)], fz01 = f[ji(0, 2)] * 2.0;
        out[0] = q00 * fr00 + sgn(p00 * fz00);
        out[ji(1, 0)] = fmac(q00, fr10, q10 * fr00) + sgn(fmac(p00, fz10, p10 * fz00));
        out[ji(0, 1)] = fmac(q00, fr01, q01 * fr00) + sgn(fmac(p00, fz01, p01 * fz00));
    }

    // rho: R = double, or dd in the double-double point tier; r0 = rcp(rho) (the grid passes
    // pass their row's correctly rounded 1/x from the host table, the same value)
    // om2: Omega^2 as O = double, or dd in the double-double point tier (params.omega2_lo)
    template <class R, class O = double> static PD_HD T eval(const T* u, R rho, O om2 = O{}) { return eval_r(u, rcp(rho), rho, om2); }
    template <class R> static PD_HD T eval_r(const T* u, R r0) { return eval_r(u, r0, r0, 0.0); }
    template <class R, class O> static PD_HD T eval_r(const T* u, R r0, R rho, O om2) {
        const R r2 = r0 * r0;
        return eval_p(u, r0, r2, r2 * r0, rho, om2);
    }
    // r2 = r0 * r0, r3 = r2 * r0 (the lean grid passes hand in their row's wave-uniform copies)
    template <class R, class O> static PD_HD T eval_p(const T* u, R r0, R r2, R r3, R rho, O om2) {
        // 1/rho jet in the rho direction: (-1)^i / rho^(i+1)
        const R ri[3] = {r0, r2 * (MAG ? 1.0 : -1.0), r3};
        T LA[3], LB[3];
        {
            // A = p_rho + q_z - p / rho   (validator.py:323), order 2
            T A[6];
#pragma unroll
            for (int d = 0; d <= 2; ++d)
#pragma unroll
                for (int j = 0; j <= d; ++j) {
                    const int i = d - j;
                    T pr = P(u, i, j) * ri[0];
#pragma unroll
                    for (int i1 = 1; i1 <= i; ++i1) pr = fmac(P(u, i - i1, j), cvt<T>(ri[i1]), pr);
#if PD_AFMA
                    // u_rr + u_zz accumulated onto -p/rho: two FMAs, no separate add
                    T s = fmac(U(u, i, j + 2), from_real<T>((double)((j + 1) * (j + 2))), sgn(pr));
                    A[ji(i, j)] = fmac(U(u, i + 2, j), from_real<T>((double)((i + 1) * (i + 2))), s);
#else
                    T s = U(u, i + 2, j) * (double)((i + 1) * (i + 2));
                    s = fmac(U(u, i, j + 2), from_real<T>((double)((j + 1) * (j + 2))), s);
                    A[ji(i, j)] = s + sgn(pr);
#endif
                }
            if (om2_nz(om2)) rotate_A(A, u, rho, om2);
            lie1(u, A, LA);
        }
        {
            // B = p^2 + q^2   (validator.py:324), order 2
            T B[6];
#if PD_BSYM
            // the square of a jet: each cross product once, doubled (2 p_a p_b, a != b) --
            // 22 multiply-adds instead of 30
            {
                const T p00 = P(u, 0, 0), p10 = P(u, 1, 0), p01 = P(u, 0, 1);
                const T p20 = P(u, 2, 0), p11 = P(u, 1, 1), p02 = P(u, 0, 2);
                const T q00 = Q(u, 0, 0), q10 = Q(u, 1, 0), q01 = Q(u, 0, 1);
                const T q20 = Q(u, 2, 0), q11 = Q(u, 1, 1), q02 = Q(u, 0, 2);
                const T p00d = p00 + p00, q00d = q00 + q00, p10d = p10 + p10, q10d = q10 + q10;
                B[ji(0, 0)] = fmac(p00, p00, q00 * q00);
                B[ji(1, 0)] = fmac(p00d, p10, q00d * q10);
                B[ji(0, 1)] = fmac(p00d, p01, q00d * q01);
                B[ji(2, 0)] = fmac(p10, p10, fmac(q10, q10, fmac(p00d, p20, q00d * q20)));
                B[ji(1, 1)] = fmac(p10d, p01, fmac(q10d, q01, fmac(p00d, p11, q00d * q11)));
                B[ji(0, 2)] = fmac(p01, p01, fmac(q01, q01, fmac(p00d, p02, q00d * q02)));
            }
#else
#pragma unroll
            for (int d = 0; d <= 2; ++d)
#pragma unroll
                for (int j = 0; j <= d; ++j) {
                    const int i = d - j;
                    T s = zero<T>();
#pragma unroll
                    for (int d1 = 0; d1 <= d; ++d1)
#pragma unroll
                        for (int j1 = 0; j1 <= d1; ++j1) {
                            const int i1 = d1 - j1, i2 = i - i1, j2 = j - j1;
                            if (i2 < 0 || j2 < 0) continue;
                            s = fmac(P(u, i1, j1), P(u, i2, j2), s);
                            s = fmac(Q(u, i1, j1), Q(u, i2, j2), s);
                        }
                    B[ji(i, j)] = s;
                }
#endif
            if (om2_nz(om2)) rotate_B(B, rho, om2);
            lie1(u, B, LB);
        }
        // L_T^2 f (order 0) = q (L_T f)_rho - p (L_T f)_z
        const T p00 = P(u, 0, 0), q00 = Q(u, 0, 0);
        const T L2A = q00 * LA[ji(1, 0)] + sgn(p00 * LA[ji(0, 1)]);
        const T L2B = q00 * LB[ji(1, 0)] + sgn(p00 * LB[ji(0, 1)]);
        // det[[L_T A, L_T B], [L_T^2 A, L_T^2 B]]   (validator.py:347)
        return LA[0] * L2B + sgn(LB[0] * L2A);
    }

    // A -= om2 C, C = rho^2 (u_rr + u_zz) + rho u_r, order 2 in (rho, z); the rho^k factors as
    // jets in the rho direction: rho = (x, 1), rho^2 = (x^2, 2x, 1)
    template <class R, class O> static PD_HD void rotate_A(T* A, const T* u, R x, O om2) {
        T PQ[6];
#pragma unroll
        for (int d = 0; d <= 2; ++d)
#pragma unroll
            for (int j = 0; j <= d; ++j) {
                const int i = d - j;
                PQ[ji(i, j)] = fmac(U(u, i, j + 2), from_real<T>((double)((j + 1) * (j + 2))),
                                    U(u, i + 2, j) * (double)((i + 1) * (i + 2)));
            }
        const T x1 = cvt<T>(x), x2 = cvt<T>(x * x), x2t = cvt<T>(x + x);
#pragma unroll
        for (int d = 0; d <= 2; ++d)
#pragma unroll
            for (int j = 0; j <= d; ++j) {
                const int i = d - j;
                T c = x2 * PQ[ji(i, j)];
                c = fmac(x1, P(u, i, j), c);
                if (i >= 1) c = c + fmac(x2t, PQ[ji(i - 1, j)], P(u, i - 1, j));
                if (i >= 2) c = c + PQ[ji(i - 2, j)];
                A[ji(i, j)] = A[ji(i, j)] + sgn(c * om2);
            }
    }
    // B (1 - om2 rho^2)
    template <class R, class O> static PD_HD void rotate_B(T* B, R x, O om2) {
        T B0[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) B0[k] = B[k];
        const T x2 = cvt<T>(x * x), x2t = cvt<T>(x + x);
#pragma unroll
        for (int d = 0; d <= 2; ++d)
#pragma unroll
            for (int j = 0; j <= d; ++j) {
                const int i = d - j;
                T c = x2 * B0[ji(i, j)];
                if (i >= 1) c = fmac(x2t, B0[ji(i - 1, j)], c);
                if (i >= 2) c = c + B0[ji(i - 2, j)];
                B[ji(i, j)] = B0[ji(i, j)] + sgn(c * om2);
            }
    }
};

// (inv_rho = rcp(rho): the lean grid passes read it from the grid's reciprocal table instead of
// dividing once per row; ff_epilogue below divides)
template <class T> __device__ __forceinline__ PointResult ff_epilogue_p(const T* u, double inv_rho, double r2, double r3,
                                                                       double rho, double om2) {
    PointResult r;
#ifdef PD_VAR_NO_EPI   // timing variant: no determinant at all (verdicts meaningless)
    {
        r.res_abs = mag(u[1] * u[2]);
        r.res_re = r.res_abs;
        r.res_im = 0.0;
        r.scale = 1.0;
        r.grad_zero = false;
        r.finite = true;
        return r;
    }
#endif
    const T det = FFEpi<T, false>::eval_p(u, inv_rho, r2, r3, rho, om2);
    // keep the signed and the magnitude evaluations apart: interleaved, the scheduler keeps
    // both sets of intermediates live
    __builtin_amdgcn_sched_barrier(0);
    double S;
#ifdef PD_VAR_NO_MAG   // timing variant: no magnitude shadow (verdicts meaningless)
    S = 1.0;
#else
    if constexpr (Real<T>::cplx_pass) {
        double m[15];
#pragma unroll
        for (int i = 0; i < 15; ++i) m[i] = mag(u[i]);
        S = FFEpi<double, true>::eval_p(m, inv_rho, r2, r3, rho, om2);
    } else {
        S = FFEpi<double, true>::eval_p(u, inv_rho, r2, r3, rho, om2);
    }
#endif
    r.res_abs = mag(det);
    if constexpr (Real<T>::cplx_pass) {
        r.res_re = ((const cplx*)&det)->re;
        r.res_im = ((const cplx*)&det)->im;
    } else {
        r.res_re = *(const double*)&det;
        r.res_im = 0.0;
    }
    r.scale = S;
    r.grad_zero = is_zero(u[ji(1, 0)]) && is_zero(u[ji(0, 1)]);
    bool fin = finite_(det) & isfinite(S);
    if constexpr (std::is_same<T, double>::value && PD_FF_GUARD_MAX) {
        // the 15 coefficient guards as one maximum (PD_FF_GUARD_MAX): max |c| < 2^160 over the
        // 14 derivative coefficients, and u itself tested on its own.  The same result: a NaN
        // that v_max drops is in S already -- every derivative coefficient is read by the
        // magnitude evaluation (A reads c10..c04 but c01, lie1 reads c01), where it makes S
        // NaN -- and an infinite coefficient wins the maximum.
        const double* c = reinterpret_cast<const double*>(u);
        double m = max_abs(max_abs(max_abs(c[1], c[2]), max_abs(c[3], c[4])), max_abs(max_abs(c[5], c[6]), max_abs(c[7], c[8])));
        m = max_abs(m, max_abs(max_abs(max_abs(c[9], c[10]), max_abs(c[11], c[12])), max_abs(c[13], c[14])));
        const double d0 = *reinterpret_cast<const double*>(&det);
        if constexpr (PD_BALLOT_SPLIT)
            r.fin_lanes = ballot64(finite_cmp(d0)) & ballot64(finite_cmp(S)) & ballot64(m < kHugeJet) & ballot64(jet_coef_ok(c[0]));
        fin = fin & (m < kHugeJet) & jet_coef_ok(u[0]);
        r.finite = fin;
        if constexpr (!PD_BALLOT_SPLIT) r.fin_lanes = ballot64(fin);
        return r;
    } else {
#pragma unroll
        for (int i = 0; i < 15; ++i) fin = fin & jet_coef_ok(u[i]);
    }
    r.finite = fin;
    r.fin_lanes = ballot64(fin);
    return r;
}

template <class T> __device__ __forceinline__ PointResult ff_epilogue_r(const T* u, double inv_rho, double rho = 0.0,
                                                                       double om2 = 0.0) {
    const double r2 = inv_rho * inv_rho;
    return ff_epilogue_p<T>(u, inv_rho, r2, r2 * inv_rho, rho, om2);
}

template <class T> __device__ __forceinline__ PointResult ff_epilogue(const T* u, double rho, double om2 = 0.0) {
    return ff_epilogue_r<T>(u, rcp(rho), rho, om2);
}

// Kerr surrogate: L[u] = k1 u_rr + k2 u_xx + k3 u_r + k4 u_x, coefficients per point.
template <class T> __device__ __forceinline__ PointResult kerr_epilogue(const T* u, const double* k) {
    PointResult r;
    const T t1 = u[ji(2, 0)] * (2.0 * k[0]);
    const T t2 = u[ji(0, 2)] * (2.0 * k[1]);
    const T t3 = u[ji(1, 0)] * k[2];
    const T t4 = u[ji(0, 1)] * k[3];
    const T L = (t1 + t2) + (t3 + t4);
    r.scale = (mag(t1) + mag(t2)) + (mag(t3) + mag(t4));
    r.res_abs = mag(L);
    if constexpr (Real<T>::cplx_pass) {
        r.res_re = ((const cplx*)&L)->re;
        r.res_im = ((const cplx*)&L)->im;
    } else {
        r.res_re = *(const double*)&L;
        r.res_im = 0.0;
    }
    r.grad_zero = is_zero(u[ji(1, 0)]) && is_zero(u[ji(0, 1)]);
    bool fin = finite_(L) && isfinite(r.scale);
    // (fin_lanes below) a jet that is exactly 0 to second order carries no information: u underflowed there
    // (exp_neg(E*exp(r**2)*..) is 0 in fp64 on most of the grid), as an analytic u that is not
    // identically 0 cannot vanish with its derivatives at a sample point
    // (u_rx, coefficient ji(1, 1), is not in the operator -- no mixed term, kerr validator.py
    // :77-91 -- so it is neither tested nor, in the lean grid passes, computed: kKerrMixed)
    bool allz = true;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        if (i == ji(1, 1)) continue;
        fin = fin && jet_coef_ok(u[i]);
        allz = allz && is_zero(u[i]);
    }
    r.finite = fin && !allz;
    r.fin_lanes = ballot64(r.finite);
    return r;
}

// max(|a|, |b|) in one v_max_f64 with both source modifiers.  The compiler's fmax first
// canonicalizes each operand (one more v_max per operand) to quiet a signalling NaN; the one
// caller below gives a NaN no meaning, so the bare instruction is enough.
__device__ __forceinline__ double max_abs(double a, double b) {
#ifndef PD_HOST_SIM
    double r;
    asm volatile("v_max_f64 %0, |%1|, |%2|" : "=v"(r) : "v"(a), "v"(b));
    return r;
#else
    return fmax(fabs(a), fabs(b));
#endif
}

// kerr_epilogue for the lean grid passes (real jets): k2 = {2 k1, 2 k2, k3, k4} (the doubled
// table, kc2), and the coefficient tests folded into one maximum -- the same PointResult,
// bit for bit:
//  * every t_i finite <=> S finite, and then |L| <= S (rounding is monotone), so L is finite;
//  * m = max |c| over the five coefficients: all zero <=> m == 0, all below kHugeJet <=>
//    m < kHugeJet, unless a coefficient is NaN (v_max drops a quiet NaN) -- a NaN in u_r, u_x,
//    u_rr or u_xx makes S NaN, and u itself is tested on its own; with a NaN "finite" is false
//    whatever m says.
template <class T> __device__ __forceinline__ PointResult kerr_epilogue_lean(const T* u, const double* k2) {
    static_assert(!Real<T>::cplx_pass, "real jets only");
    PointResult r;
    const double t1 = u[ji(2, 0)] * k2[0];
    const double t2 = u[ji(0, 2)] * k2[1];
    const double t3 = u[ji(1, 0)] * k2[2];
    const double t4 = u[ji(0, 1)] * k2[3];
    const double L = (t1 + t2) + (t3 + t4);
    r.scale = (fabs(t1) + fabs(t2)) + (fabs(t3) + fabs(t4));
    r.res_abs = fabs(L);
    r.res_re = L;
    r.res_im = 0.0;
    r.grad_zero = u[ji(1, 0)] == 0.0 && u[ji(0, 1)] == 0.0;
    const double m = max_abs(max_abs(max_abs(u[ji(0, 0)], u[ji(1, 0)]), max_abs(u[ji(0, 1)], u[ji(2, 0)])),
                             u[ji(0, 2)]);
    // (bitwise: && would make the compiler branch around the later tests)
    r.finite = isfinite(r.scale) & !isnan(u[ji(0, 0)]) & (m < kHugeJet) & (m != 0.0);
    if constexpr (PD_BALLOT_SPLIT)
        r.fin_lanes = ballot64(finite_cmp(r.scale)) & ballot64(u[ji(0, 0)] == u[ji(0, 0)]) & ballot64(m < kHugeJet) & ballot64(m != 0.0);
    else
        r.fin_lanes = ballot64(r.finite);
    return r;
}

__device__ __forceinline__ double scaled(double res_abs, double S) {
    if (S > 0.0) return res_abs / S;
    return res_abs == 0.0 ? 0.0 : INFINITY;
}

// scaled() as a select: the division runs in every lane (a lane with S <= 0 or NaN discards
// it), so the per-point test has no divergent branch and no exec-mask bookkeeping; same value
__device__ __forceinline__ double scaled_sel(double res_abs, double S) {
    const double q = res_abs / S;
    const double alt = res_abs == 0.0 ? 0.0 : INFINITY;
    return S > 0.0 ? q : alt;
}

// scaled() for the lean grid passes' per-point test: res_abs * 1/S with the hardware
// reciprocal and two Newton steps (5 VALU against the 10 of the IEEE division sequence, which
// the Kerr epilogue pays per point beside ~20 others).  Relative error ~2^-52 -- far below the
// jets' own rounding, which the grid threshold and tier 2 already absorb; the exact division
// for S outside [2^-1000, 2^1000] and for S == 0.
__device__ __forceinline__ double scaled_fast(double res_abs, double S) {
    if (S > 0x1p-1000 && S < 0x1p1000) {
        double r = __builtin_amdgcn_rcp(S);
        r = fma(r, fma(-S, r, 1.0), r);
        r = fma(r, fma(-S, r, 1.0), r);
        return res_abs * r;
    }
    return scaled(res_abs, S);
}

// The grid's zero test without a division: a finite point fails tier 1 iff |res| > tau * S
// (S >= 0 finite).  It equals fl(|res| / S) > tau except where |res| / S lies within a rounding
// of tau (a tolerance either way); S == 0 fails iff res != 0, as scaled() gives inf there.  The
// oracle (oracle/jet_oracle.c grid_fails) applies the same rule.
__device__ __forceinline__ bool grid_fails(double res_abs, double S, double tau) { return res_abs > tau * S; }

// a fast estimate of res / S (hardware reciprocal, no refinement): only ORDERS the grid points
// of a lane for the running maximum of q (GridMax); the reported q is the IEEE quotient of the
// point it chose
__device__ __forceinline__ double q_estimate(double res_abs, double S) {
#ifndef PD_HOST_SIM
    return res_abs * __builtin_amdgcn_rcp(S);
#else
    return res_abs * (1.0 / S);
#endif
}

// Per-lane running maximum of the scaled residual q = |res| / S over the finite grid points
// without a division per point.  EXACT (Kerr, whose grid-reject text prints q_grid): the point
// with the largest estimate is kept as the pair (|res|, S) and divided once at the end (q() is
// scaled(), so q_grid is that point's IEEE quotient -- the old value wherever the estimates order
// the points as the quotients do, i.e. unless two quotients of a lane agree to the estimate's
// accuracy).  res == 0 with S == 0 (estimate NaN) never wins, as q = 0 there; S == 0 with
// res > 0 (estimate inf) wins, q = inf.  !EXACT (force-free, whose q_grid no reason text
// reads): the maximum of the estimates themselves, in one register pair instead of three.
template <bool EXACT> struct GridMax {
    double r = 0.0, s = 1.0, e = 0.0;
    __device__ __forceinline__ void add(bool finite, double res_abs, double S) {
        const double est = q_estimate(res_abs, S);
        const bool take = finite & (est > e);
        if constexpr (EXACT) {
            r = take ? res_abs : r;
            s = take ? S : s;
        }
        e = take ? est : e;
    }
    __device__ __forceinline__ double q() const {
        if constexpr (EXACT) return scaled(r, s);
        else return e;
    }
};

// ------------------------------------------------------------------ wave reductions
// the lanes where b holds (one s_and with exec of the compare's lane mask; HIP's __ballot(int)
// first turns the bool into an int in a VGPR and compares it again: 2 VALU more per count)
__device__ __forceinline__ uint64_t lane_mask(bool b) {
#ifndef PD_HOST_SIM
    return __builtin_amdgcn_ballot_w64(b);
#else
    return __ballot(b);
#endif
}
__device__ __forceinline__ int count_lanes(bool b) {
#ifndef PD_HOST_SIM
    return (int)__popcll(__builtin_amdgcn_ballot_w64(b));
#else
    return (int)__popcll(__ballot(b));
#endif
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ------------------------------------------------------------------ the interpreter
// Result codes of run_program (wave-uniform).
enum { RUN_OK = 0, RUN_UNSUPPORTED = 1, RUN_BAD = 2 };

template <class T, int K, int MAXD> struct Interp {
    using O = JetOps<T, K>;
    using J = typename O::J;

    static __device__ __forceinline__ void binop(uint32_t op, const J& a, J& t) {
        switch (op) {
            case PDOP_ADD: O::add(a, t); break;
            case PDOP_SUB: O::sub(a, t); break;
            case PDOP_RSUB: O::rsub(a, t); break;
            case PDOP_MUL: O::mul(a, t); break;
            case PDOP_DIV: O::div(a, t); break;
            default: O::rdiv(a, t); break;
        }
    }
    // t = S[d-2] (op) t for the slot just below the top; d uniform.
    template <int I> static __device__ __forceinline__ void below(J* S, int d, uint32_t op, J& t) {
        if constexpr (I < MAXD - 1) {
            if (d == I + 2) {
                binop(op, S[I], t);
                return;
            }
            below<I + 1>(S, d, op, t);
        }
    }
    template <int I> static __device__ __forceinline__ void push_down(J* S, int d, const J& t) {
        if constexpr (I < MAXD - 1) {
            if (d == I + 1) {
                S[I] = t;
                return;
            }
            push_down<I + 1>(S, d, t);
        }
    }

    // Operand stack below the top-of-stack jet: kept in LDS, not VGPRs, so the registers
    // hold one jet (the accumulator) plus the op's temporaries -- more waves per SIMD.
    // Layout per wave: [slot][coefficient][lane] -> each lane touches only its own doubles and
    // consecutive lanes hit consecutive 8-byte words (no bank conflicts, no barriers needed).
    static constexpr int NCJ = nc(K);
    static __device__ __forceinline__ void lds_store(T* base, int slot, int lane, const J& t) {
#pragma unroll
        for (int c = 0; c < NCJ; ++c) base[(slot * NCJ + c) * 64 + lane] = t.c[c];
    }
    static __device__ __forceinline__ void lds_load(const T* base, int slot, int lane, J& t) {
#pragma unroll
        for (int c = 0; c < NCJ; ++c) t.c[c] = base[(slot * NCJ + c) * 64 + lane];
    }

    // Evaluate program words [pc, end) at point (x, y); result jet in T.
    static __device__ __forceinline__ int run(const int32_t* ops, int pc, int end, double x, double y,
                                              J& acc, T* stk, int lane, const PrmTab<double>& P) {
        int d = 0;
        if (pc >= end) return RUN_BAD;
        uint32_t w = rd_word(ops + pc);
        for (;;) {
            const uint32_t op = w & 0xffu;
            // immediate and next opcode word are fetched before this op's jet arithmetic, so
            // their scalar-load latency hides under it
            double imm = 0.0;
            int npc = pc + 1;
            if (op_has_imm(op)) {
                npc = pc + ((w & PDEVAL_IMM_DD) ? 5 : 3);   // (the double-double low part is skipped)
                if (npc > end) return RUN_BAD;
                imm = rd_immp(ops + pc + 1, w, P);
            }
            const uint32_t wn = (npc < end) ? rd_word(ops + npc) : 0u;
            switch (op) {
                case PDOP_PUSH_P: {
                    if (d > 0 && d < MAXD) lds_store(stk, d - 1, lane, acc);
                    double pk[K + 1];
                    if ((w >> 16) & 1) {
                        O::pcoefs(y, (int)((w >> 8) & 0xffu), pk);
                        O::template set_p<1>(acc, pk);
                    } else {
                        O::pcoefs(x, (int)((w >> 8) & 0xffu), pk);
                        O::template set_p<0>(acc, pk);
                    }
                    ++d;
                    break;
                }
                case PDOP_ADD_P: case PDOP_SUB_P: case PDOP_MUL_P: case PDOP_DIV_P: case PDOP_RDIV_P: {
                    double pk[K + 1];
                    if ((w >> 16) & 1) {
                        O::pcoefs(y, (int)((w >> 8) & 0xffu), pk);
                        O::template p_op<1>(op, acc, pk);
                    } else {
                        O::pcoefs(x, (int)((w >> 8) & 0xffu), pk);
                        O::template p_op<0>(op, acc, pk);
                    }
                    break;
                }
                case PDOP_PUSH_X:
                case PDOP_PUSH_Y:
                case PDOP_PUSH_C:
                case PDOP_PUSH_I: {
                    if (d > 0 && d < MAXD) lds_store(stk, d - 1, lane, acc);
                    if (op == PDOP_PUSH_X) O::set_var(acc, x, 0);
                    else if (op == PDOP_PUSH_Y) O::set_var(acc, y, 1);
                    else if (op == PDOP_PUSH_C) {
                        O::set_const(acc, from_real<T>(imm));
                    } else {
                        if constexpr (Real<T>::cplx_pass) O::set_const(acc, cplx{0.0, 1.0});
                        else return RUN_UNSUPPORTED;
                    }
                    ++d;
                    break;
                }
                case PDOP_ADD: case PDOP_SUB: case PDOP_RSUB:
                case PDOP_MUL: case PDOP_DIV: case PDOP_RDIV: {
                    if (d >= 2 && d <= MAXD) {
                        J lhs;
                        lds_load(stk, d - 2, lane, lhs);
                        binop(op, lhs, acc);
                    }
                    --d;
                    break;
                }
                case PDOP_ADDC: case PDOP_MULC: case PDOP_RDIVC: {
                    const double c = imm;
                    if (op == PDOP_ADDC) acc.c[0] = acc.c[0] + from_real<T>(c);
                    else if (op == PDOP_MULC) O::scale(acc, from_real<T>(c));
                    else O::rdivc(acc, from_real<T>(c));
                    break;
                }
                case PDOP_NEG:
#ifdef PD_VAR_NEG_XOR   // sign flips as integer XORs of the high words (exact, like * -1)
                    if constexpr (std::is_same<T, double>::value) {
#pragma unroll
                        for (int i = 0; i < NCJ; ++i)
                            acc.c[i] = __hiloint2double(__double2hiint(acc.c[i]) ^ (int)0x80000000,
                                                        __double2loint(acc.c[i]));
                        break;
                    }
#endif
                    O::scale(acc, from_real<T>(-1.0));
                    break;
                case PDOP_ADD_X: case PDOP_ADD_Y: case PDOP_SUB_X: case PDOP_SUB_Y: {
                    const bool isx = (op == PDOP_ADD_X || op == PDOP_SUB_X);
                    const double sg = (op == PDOP_ADD_X || op == PDOP_ADD_Y) ? 1.0 : -1.0;
                    acc.c[0] = acc.c[0] + from_real<T>(sg * (isx ? x : y));
                    const int idx = isx ? ji(1, 0) : ji(0, 1);
                    acc.c[idx] = acc.c[idx] + from_real<T>(sg);
                    break;
                }
                case PDOP_MUL_X: O::mul_var(acc, x, 0); break;
                case PDOP_MUL_Y: O::mul_var(acc, y, 1); break;
                case PDOP_DIV_X: O::div_var(acc, x, 0); break;
                case PDOP_DIV_Y: O::div_var(acc, y, 1); break;
                case PDOP_POWN:
                    O::pown(acc, (int)((w >> 8) & 0xffu));
                    break;
                case PDOP_POW: {
                    O::powa(acc, imm);
                    break;
                }
                case PDOP_SQRT: O::sqrtj(acc); break;
                case PDOP_EXP: O::expj(acc); break;
                case PDOP_LOG: O::logj(acc); break;
                case PDOP_ABS: absj<K>(acc); break;
                default: return RUN_UNSUPPORTED;
            }
            if (npc >= end) break;
            pc = npc;
            w = wn;
        }
        return d == 1 ? RUN_OK : RUN_BAD;
    }
};

// ------------------------------------------------------------------ the kernel
#ifndef PD_DEEP_PARTS
#define PD_DEEP_PARTS 16
#endif
// PROB: PDEVAL_PROBLEM_FORCE_FREE (K = 4) or PDEVAL_PROBLEM_KERR (K = 2).
// PARTS > 1 (the persistent deep-list passes): a candidate whose point stage pass 0 decided has
// its grid chunks split over PARTS waves (contiguous ranges); each part adds its counts into the
// list entry's accumulator (a.t2acc, zero between launches) and the part that completes the
// entry writes the outputs -- the stack-8 lists hold a few dozen to a few hundred candidates, and
// one wave each left the chip idle (Kerr pass 3: 2.95 ms for 98 candidates).  Sums, maxima and
// ORs do not depend on the split.  Any other candidate is taken by part 0 alone.
template <int PROB, class T, int MAXD, bool PERSISTENT, int PARTS = 1>
#ifndef PD_WAVES_PER_SIMD
#define PD_WAVES_PER_SIMD 4
#endif
#ifndef PD_CPLX_WAVES_PER_SIMD
#define PD_CPLX_WAVES_PER_SIMD 2
#endif
// real passes: 128 VGPRs, 4 waves per SIMD; the complex passes need more registers (their
// jets are twice as wide) and run at 2 waves per SIMD without spilling (12.5 vs 30 ms)
__global__ __launch_bounds__(256, Real<T>::cplx_pass ? PD_CPLX_WAVES_PER_SIMD : PD_WAVES_PER_SIMD)
void validate_kernel(KernelArgs a) {
    constexpr int K = (PROB == PDEVAL_PROBLEM_FORCE_FREE) ? 4 : 2;
    using I = Interp<T, K, MAXD>;
    using J = typename I::J;
    const int lane = threadIdx.x & 63;
    const int wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
#ifndef PD_HOST_SIM
    extern __shared__ __align__(16) unsigned char pd_lds[];
#else
    static unsigned char pd_lds[1];
#endif
    T* stk = reinterpret_cast<T*>(pd_lds) + (size_t)wib * (MAXD - 1) * nc(K) * 64;
    // (An XCD-contiguous block renumbering was measured here and rejected: pass 1 went from
    // 132.9 to 134.9 ms and its write traffic is dominated by scratch, not by partial lines of
    // the per-candidate outputs -- DESIGN.md §7.)
    const int64_t wave0 = (int64_t)blockIdx.x * (blockDim.x >> 6) + wib;
    // persistent variants stride over a device work list; the first pass is one wave per
    // candidate (a single iteration)
    const int64_t wstride = (int64_t)gridDim.x * (blockDim.x >> 6);
    int64_t nwork = a.list_count ? (int64_t)(*a.list_count) : (a.list ? a.list_cap : a.n);
    if (a.list && nwork > a.list_capacity) nwork = a.list_capacity;

    for (int64_t wp = wave0; wp < nwork * PARTS; wp = PERSISTENT ? wp + wstride : nwork * PARTS) {
        const int64_t wi = wp / PARTS;
        const int part = (int)(wp - wi * PARTS);
        const int64_t cand = a.list ? checked_cand(a, (int64_t)__builtin_amdgcn_readfirstlane((int)a.list[wi]), ERRW_GENERIC) : wi;
        if (cand < 0) continue;
        int64_t beg = a.offsets[cand], end = a.offsets[cand + 1];
        // programs are addressed relative to their first word with 32-bit offsets
        const bool in_bounds = beg >= 0 && end > beg && end <= a.n_words && end - beg < (1 << 24);
        if (!in_bounds) beg = end = 0;
        const int32_t* prog = a.ops + beg;
        const int plen = __builtin_amdgcn_readfirstlane((int)(end - beg));
        // header word: opcode 0, depth in bits 8-15, flags above
        const uint32_t hdr = in_bounds ? rd_word(prog) : 0xffu;
        int status = -1;
        if ((hdr & 0xffu) != 0u) status = PDEVAL_CLS_BAD_PROGRAM;
        // pass 0 decided the point stage of most real candidates (P0_*)
        uint8_t ps = P0_NONE;
        if (a.pstate) ps = (uint8_t)__builtin_amdgcn_readfirstlane((int)a.pstate[cand]);
        if constexpr (!Real<T>::cplx_pass) {
            if (ps & P0_CPLX) continue;                            // the complex passes take it
        }
        if ((ps & 3) == P0_REJECT && !a.prm.full_grid) continue;  // final after the point stage
        const bool p0 = (ps & 3) != P0_NONE;
        if constexpr (!Real<T>::cplx_pass) {
            if (status < 0 && (hdr & PDEVAL_FLAG_COMPLEX)) {
                if constexpr (PROB == PDEVAL_PROBLEM_FORCE_FREE) {
                    // complex-valued program: straight to the complex pass
                    if (!p0) {
                        if (lane == 0 && a.cplx_list) list_append(a.cplx_list, a.cplx_count, a.list_capacity, cand);
                        status = PDEVAL_CLS_NONFINITE_REF;
                    }
                } else {
                    // Kerr: a non-real value at a test point rejects (kerr validator.py:179-180),
                    // final whether or not pass 0 saw it first: the real grid cannot evaluate it
                    status = PDEVAL_CLS_REJECT_POINT;
                }
            }
        }
        const int depth = (int)((hdr >> 8) & 0xffu);
        if (status < 0 && depth > MAXD) {
            if (a.defer_list) {
                if (lane == 0) list_append(a.defer_list, a.defer_count, a.list_capacity, cand);
                continue;
            }
            status = PDEVAL_CLS_UNSUPPORTED;  // deeper than the last variant takes
        }
        // split over the parts only a grid whose point stage is decided (no chunk 0)
        const bool split = PARTS > 1 && p0 && status < 0 && a.t2acc;
        if (PARTS > 1 && !split && part != 0) continue;
        double q_ref = 0.0;        // FF: q*, Kerr: max |lhs| over reference points
        bool point_reject = (ps & 3) == P0_REJECT;
        bool point_final = p0;     // non-finite at a reference point, or decided by pass 0: no tier 2
        bool grid_eval = true;
        double qmax = 0.0;
        int nbad = 0, nnonfin = 0, nfin = 0;
        bool grad_nz = (ps & P0_GRAD) != 0;
        // chunk 0: the reference points; chunks 1..: one 64-point slice of a grid row each
        const int per_row = a.ny >> 6;
        const int nchunks = 1 + a.nx * per_row;
        const double y_lane = a.gy[lane];  // row slice 0; other slices reload below
        int ch_beg = p0 ? 1 : 0, ch_end = nchunks;
        if (split) {
            const int ng = nchunks - 1;
            ch_beg = 1 + (int)((int64_t)ng * part / PARTS);
            ch_end = 1 + (int)((int64_t)ng * (part + 1) / PARTS);
        }
        for (int ch = ch_beg; ch < ch_end && status < 0; ++ch) {
            bool active;
            int p;               // point index: reference points first, then the grid row-major
            double x, y;
            if (ch == 0) {
                active = lane < a.n_ref;
                p = lane;
                const int l = active ? lane : 0;
                x = l == 0 ? a.ref_x[0] : (l == 1 ? a.ref_x[1] : (l == 2 ? a.ref_x[2] : a.ref_x[3]));
                y = l == 0 ? a.ref_y[0] : (l == 1 ? a.ref_y[1] : (l == 2 ? a.ref_y[2] : a.ref_y[3]));
            } else {
                const int row = (ch - 1) / per_row, sl = (ch - 1) - row * per_row;
                active = true;
                p = a.n_ref + row * a.ny + sl * 64 + lane;
                x = rd_sf64(a.gx + row);   // scalar
                y = per_row == 1 ? y_lane : a.gy[sl * 64 + lane];
            }
            const int pp = p;
            J u;
            const int rc = I::run(prog, 1, plen, x, y, u, stk, lane, ch == 0 ? a.prm_pt : a.prm_grid);
            if (rc == RUN_UNSUPPORTED) { status = PDEVAL_CLS_UNSUPPORTED; break; }
            if (rc == RUN_BAD) { status = PDEVAL_CLS_BAD_PROGRAM; break; }
            PointResult r;
            if constexpr (PROB == PDEVAL_PROBLEM_FORCE_FREE) r = ff_epilogue<T>(u.c, x, a.prm.omega2);
            else r = kerr_epilogue<T>(u.c, a.kc + 4 * pp);
            const double qv = scaled(r.res_abs, r.scale);
            if (active) {
#pragma unroll
                for (int f = 0; f < PDEVAL_FP_N; ++f)
                    if (p == a.fp_pts[f] && a.out.fingerprint) {
                        a.out.fingerprint[cand * PDEVAL_FP_N + f] = fp_value(u.c[0]);
                    }
            }
            if (active && p < a.n_ref) {
                if (a.out.res_ref) a.out.res_ref[cand * a.n_ref + p] = r.res_re;
                if (r.finite && !r.grad_zero) grad_nz = true;
            } else if (active && r.finite) {
                qmax = fmax(qmax, qv);
                if (!r.grad_zero) grad_nz = true;
            }
            // grid counts are wave-uniform (ballot + popcount into SGPRs) rather than per-lane
            // counters reduced at the end: three fewer live VGPRs across the interpreter loop
            {
                const bool g = active && p >= a.n_ref;
                nfin += (int)__popcll(__ballot(g && r.finite));
                nbad += (int)__popcll(__ballot(g && r.finite && grid_fails(r.res_abs, r.scale, a.prm.tau_grid)));
                nnonfin += (int)__popcll(__ballot(g && !r.finite));
            }
            if (ch == 0) {
                // point stage: lanes 0..n_ref-1 hold the reference points
                double refv;
                if constexpr (PROB == PDEVAL_PROBLEM_FORCE_FREE) refv = (lane == 0) ? qv : 0.0;
                else refv = (lane < a.n_ref) ? r.res_abs : 0.0;
                q_ref = wave_max(refv);
                const bool nf = __any(active && p < a.n_ref && !r.finite);
                if constexpr (PROB == PDEVAL_PROBLEM_FORCE_FREE) {
                    if (nf) {
                        if constexpr (!Real<T>::cplx_pass) {
                            // not real at p*: the complex pass decides (SymPy evaluates the
                            // point exactly, in the complex field: validator.py:363-402)
                            status = PDEVAL_CLS_NONFINITE_REF;
                            if (lane == 0 && a.cplx_list)
                                list_append(a.cplx_list, a.cplx_count, a.list_capacity, cand);
                        } else {
                            point_reject = point_final = true;  // not finite even in the complex field
                        }
                    } else {
                        point_reject = !(q_ref <= a.prm.tau_point);
                    }
                } else {
                    // Kerr fast point check (kerr validator.py:163-192): non-real / NaN at a
                    // reference point rejects; otherwise reject iff max|lhs| >= 1e-10 (absolute)
                    point_final = nf;
                    point_reject = nf || !(q_ref < a.prm.kerr_abs_tol);
                }
                if (point_reject && !a.prm.full_grid) {
                    grid_eval = false;   // the reference's control flow: stop after the point stage
                    break;
                }
            }
        }
        // wave reductions
        qmax = wave_max(qmax);
        bool grad_w = __any(grad_nz);
        if (split) {
            // merge this part into the entry's accumulator; the last part carries on (a status
            // from the interpreter -- malformed, unsupported -- travels as bits of `grad`)
            int last = 0;
            if (lane == 0) {
                T2Acc* A = a.t2acc + wi;
                atomicAdd(&A->nb1, nbad);
                atomicAdd(&A->nfin, nfin);
                atomicAdd(&A->nnonfin, nnonfin);
                atomicMax(&A->qmax_bits, (unsigned long long)__double_as_longlong(qmax));   // qmax >= 0
                const uint32_t g = (grad_w ? 1u : 0u) | (status == PDEVAL_CLS_BAD_PROGRAM ? 2u : 0u) |
                                   (status == PDEVAL_CLS_UNSUPPORTED ? 4u : 0u);
                if (g) atomicOr(&A->grad, g);
                __threadfence();
                if (atomicAdd(&A->done, 1) == PARTS - 1) {
                    __threadfence();
                    nbad = atomicAdd(&A->nb1, 0);
                    nfin = atomicAdd(&A->nfin, 0);
                    nnonfin = atomicAdd(&A->nnonfin, 0);
                    qmax = __longlong_as_double((long long)atomicMax(&A->qmax_bits, 0ull));
                    const uint32_t gm = atomicOr(&A->grad, 0u);
                    grad_w = (gm & 1u) != 0u;
                    status = (gm & 2u) ? PDEVAL_CLS_BAD_PROGRAM : (gm & 4u) ? PDEVAL_CLS_UNSUPPORTED : -1;
                    A->nb1 = A->nb2 = A->nfin = A->nnonfin = A->done = 0;   // ready for the next use
                    A->grad = 0u;
                    A->qmax_bits = 0ull;
                    last = 1;
                }
            }
            if (!__builtin_amdgcn_readfirstlane(last)) continue;   // lane 0 is the first active lane
            status = __builtin_amdgcn_readfirstlane(status);
            nbad = __builtin_amdgcn_readfirstlane(nbad);
            nfin = __builtin_amdgcn_readfirstlane(nfin);
            nnonfin = __builtin_amdgcn_readfirstlane(nnonfin);
            grad_w = __builtin_amdgcn_readfirstlane((int)grad_w) != 0;
        }
        const bool any_grad = grad_w && !(ps & P0_CONST);
        if (lane == 0) {
            int cls = status;
            if (cls < 0) {
                // zero gradient: the reference exits only on a structurally zero gradient
                // (validator.py:309-312 compares the symbolic u_rho, u_z with 0), i.e. when u
                // references no coordinate; a numerically constant but structurally
                // non-constant u goes on and its det is identically 0.  Kerr excludes every
                // u that simplify() reduces to a constant (kerr validator.py:231-240).
                const bool structural = (PROB != PDEVAL_PROBLEM_FORCE_FREE) || (hdr & PDEVAL_FLAG_NOCOORD);
                uint32_t esc = 0;
                if (!any_grad && (nfin > 0 || (ps & P0_CONST)) && structural) cls = PDEVAL_CLS_ZERO_GRADIENT;
                else if (PROB != PDEVAL_PROBLEM_FORCE_FREE && !point_reject && grid_eval && nfin == 0)
                    cls = PDEVAL_CLS_REJECT_GRID;   // no finite grid point: nothing proves lhs == 0
                else if (point_reject) {
                    cls = PDEVAL_CLS_REJECT_POINT;
                    if (!point_final)
                        esc = ESC_POINT | (grid_eval ? ESC_GRID_EVAL : 0u) |
                              (grid_eval && nbad > a.prm.max_bad ? ESC_GRID_FAIL : 0u);
                } else if (nbad > a.prm.max_bad) {
                    cls = PDEVAL_CLS_REJECT_GRID;
                    esc = ESC_GRID_EVAL | ESC_GRID_FAIL;
                } else if (PROB == PDEVAL_PROBLEM_FORCE_FREE && a.prm.strict_symbolic &&
                           (hdr & (PDEVAL_FLAG_NONSMOOTH2D | PDEVAL_FLAG_UNPROVABLE))) {
                    cls = PDEVAL_CLS_REJECT_SYMBOLIC;
                } else {
                    cls = PDEVAL_CLS_ACCEPT;
                }
                // a tier-1 failure may be rounding noise: tier 2 re-decides it with error
                // bounds (tier2_kernel); the class written here is provisional
                if (esc && a.esc_list) {
                    esc |= (any_grad ? ESC_ANY_GRAD : 0u) | (nfin > 0 ? ESC_NFIN : 0u);
                    list_append(a.esc_list, a.esc_count, a.list_capacity,
                                cand | ((int64_t)esc << PD_ESC_SHIFT));
                }
            }
            if (a.out.status) a.out.status[cand] = (uint8_t)cls;
            if (a.out.q_ref && !p0) a.out.q_ref[cand] = q_ref;
            if (a.out.q_grid) a.out.q_grid[cand] = qmax;
            if (a.out.n_bad) a.out.n_bad[cand] = nbad;
            if (a.out.n_nonfinite) a.out.n_nonfinite[cand] = nnonfin;
            if (a.out.verdict_bits) {
                const uint32_t bit = 1u << (cand & 31);
                uint32_t* wp = (uint32_t*)a.out.verdict_bits + (cand >> 5);
                if (cls == PDEVAL_CLS_ACCEPT) atomicOr(wp, bit);
                else atomicAnd(wp, ~bit);
            }
        }
    }
}

}  // namespace pd

// tome_kernels.hip -- hand-written gfx950 (CDNA4, wave64) kernels of the ToMe merge path and the
// C ABI declared in include/tome_hip.h.  Built with: hipcc --offload-arch=gfx950 -O3
// -ffp-contract=off -shared -fPIC (csrc/build.py).  No torch, no CUDA, no portability layer.
//
// One translation unit: tome_common.h (types), tome_match.h, tome_ln_rows.h (the row statistics the forward LayerNorm
// kernels and k_ln_rows_bwd_amp share), tome_merge_slab.h (the row slab the merge family walks), tome_merge.h,
// tome_merge_ln_amp.h, tome_ln_fwd.h, tome_merge_bwd.h, tome_ln_bwd.h, tome_merge_ln_bwd.h, tome_merge_ln_bwd_amp.h,
// tome_gelu.h, tome_gelu_bwd.h, tome_token_mean.h, tome_short_attn_bwd.h, tome_traj_bwd.h and tome_partition.h (kernels), this file (host).
//
// Launch sequence of one matching (tome_match / tome_match_keys), kernels in tome_match.h:
//   k_unit_rows[_heads]  keys -> fp32 unit vectors, even/odd split, MFMA-fragment order (HBM bound)
//   k_scores_rowmax      A.B^T tile by tile on v_mfma_f32_32x32x2_f32, running row max/argmax in
//                        registers; the [T1,T2] score matrix never exists in memory      (MFMA bound)
//   k_rank_select        folds the j-parts, stable descending rank by counting, writes src/dst/unm
//   k_compact_unm        class-token case only: unm_idx in ascending row order (merge.py:71-73)
// and of one merge (tome_merge_wavg[_regrouped] / tome_merge / tome_drop / tome_unmerge), tome_merge.h:
//   k_merge_rows_fast    streaming waves (2-4 output rows each) + edge waves (rows that receive sources);
//                        <LN>: residual add in front and LayerNorm behind fused in (tome_merge_wavg_ln)
//   k_merge_rows / k_unmerge_rows   generic one-wave-per-row forms                        (HBM bound)
// and of the residual add + LayerNorm (tome_ln_fwd.h):
//   k_add_ln_rows        second residual + the next block's first LayerNorm (tome_add_layernorm; with fp32 weight /
//                        bias, a 16-bit y and a 16-bit or fp32 residual stream: tome_add_layernorm_amp)
//   k_add_ln_regroup     the same in the middle of TimeSformer's block, y written regrouped (tome_add_layernorm_regrouped)
// and of its backward (tome_merge_backward[_regrouped]), tome_merge_bwd.h:
//   k_merge_rows_bwd     gx[t] = gy[row of t] / out_div * in_mul, streaming gather             (HBM bound)
// and of the add + LayerNorm backward (tome_layernorm_backward), tome_ln_bwd.h:
//   k_ln_rows_bwd        gx = gx_in + rstd (gw - mean gw - xhat mean(gw xhat)), statistics recomputed from the stored
//                        rows with ln_rows' arithmetic (its own copy of the rounds); per-workgroup partial rows of
//                        dweight / dbias                                                        (HBM bound)
//   k_ln_param_grad      the partial rows summed in a fixed order
//   k_ln_rows_bwd<REGROUP>  the same behind TimeSformer's mid-block regrouping (tome_layernorm_backward_regrouped): the
//                        row map in front of gy, a class row's F gradients summed in fp32              (HBM bound)
// and of the fused residual add + merge + LayerNorm (tome_merge_ln_backward), tome_merge_ln_bwd.h:
//   k_merge_ln_rows_bwd  the two above as one pass: the LayerNorm term of row o(t) in fp32, scaled and rounded once
//                        per input token; parameter gradients over the merged rows, each counted once    (HBM bound)
// and their mixed-precision forms for a model under autocast with fp32 master weights (tome_merge_wavg_ln_amp /
// tome_drop_ln_amp, tome_layernorm_backward_amp, tome_merge_ln_backward_amp), tome_merge_ln_amp.h / tome_ln_bwd.h /
// tome_merge_ln_bwd_amp.h:
//   k_merge_rows_ln_amp  k_merge_rows_fast<LN> with fp32 weight / bias, a 16-bit y and a 16-bit or fp32 residual stream
//   k_ln_rows_bwd_amp    k_ln_rows_bwd on the forward's own rounds (tome_ln_rows.h) with a 16-bit gy, the stream's dtype
//                        for xs / gx_in / gx, fp32 partial rows summed into fp32 parameters, optionally gx rounded
//                        to 16 bits as a second output                                                   (HBM bound)
//   k_merge_ln_rows_bwd_amp  k_merge_ln_rows_bwd in those dtypes, on the same shared rounds: the backward of
//                        k_merge_rows_ln_amp as one pass                                                 (HBM bound)
// and of TimeSformer's temporal attention (tome_short_attention_backward), tome_short_attn_bwd.h:
//   k_short_attention_bwd  P recomputed, dq / dk / dv of sequences of <= 8 tokens in one pass, eight lanes per
//                        (sequence, head), dk / dv accumulated in registers                           (HBM bound)
// and of the MLP's backward between its two library GEMMs (tome_gelu_erf_backward / tome_gelu_tanh_backward),
// tome_gelu_bwd.h:
//   k_gelu_bwd           gh = ga gelu'(h) (erf or tanh form), the activation again with the forward's bits, per-workgroup
//                        partial rows of fc1's bias gradient (summed by k_ln_param_grad)        (HBM bound)
// and of the last block of a mean-pooling ViT (tome_token_mean), tome_token_mean.h:
//   k_token_mean         fp32 column mean over a clip's tokens, optionally of the exact-erf GELU's stored bits (HBM bound)
// and of the proportional attention's backward (tome_prop_attention_backward), tome_attn_bwd.h:
//   k_attn_bwd_dq        row statistics recomputed (two sweeps over the keys), dq, L and delta to the workspace
//   k_attn_bwd_dkv       dk and dv per block of keys over all queries                          (MFMA bound)
// the same two with a segment dimension for Motionformer's per-frame stage (tome_prop_attention_segments_backward): dq
// summed over the segments in registers, the segment one more grid factor of dk / dv;
// and of its temporal stage (tome_trajectory_mix_backward), tome_traj_bwd.h:
//   k_trajectory_mix_bwd   the F weights of a (token, head) recomputed, dq2 / dk2 / dval in one pass   (HBM bound)
// The partition matchings (kth_ / random_bipartite_soft_matching: arbitrary source / destination sets, every source
// merged) have their own sequence, written out at the top of tome_partition.h.
//
// The arithmetic contract (summation orders, tie rules) is the one written at the top of
// oracle/tome_oracle.c; the kernels reproduce it bit for bit.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <type_traits>

#include "../../include/tome_hip.h"
#include "tome_common.h"
#include "tome_match.h"
#include "tome_match_filter.h"
#include "tome_ln_rows.h"
#include "tome_merge_slab.h"
#include "tome_merge.h"
#include "tome_merge_ln_amp.h"
#include "tome_ln_fwd.h"
#include "tome_merge_bwd.h"
#include "tome_ln_bwd.h"
#include "tome_merge_ln_bwd.h"
#include "tome_merge_ln_bwd_amp.h"
#include "tome_gelu.h"
#include "tome_gelu_bwd.h"
#include "tome_token_mean.h"
#include "tome_partition.h"
#include "tome_attn.h"
#include "tome_attn_stream.h"
#include "tome_attn_resident.h"
#include "tome_attn_bwd.h"
#include "tome_short_attn_bwd.h"
#include "tome_traj_bwd.h"
#include "tome_embed.h"

// ------------------------------------------------------------------------------------------------
// host side: argument checks, workspace carving, launches
// ------------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";

static int fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

static int check_launch(const char *what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(TOME_ELAUNCH, "%s: %s", what, hipGetErrorString(e));
    return TOME_OK;
}

extern "C" int tome_abi_version(void) { return TOME_ABI_VERSION; }
extern "C" const char *tome_last_error(void) { return g_err; }

extern "C" int64_t tome_effective_r(int64_t T, int64_t r, int class_token, int distill_token) {
    int64_t prot = (class_token ? 1 : 0) + (distill_token ? 1 : 0);
    int64_t avail = T - prot;
    int64_t cap = avail >= 0 ? avail / 2 : -((-avail + 1) / 2);  // python floor division
    int64_t re = r < cap ? r : cap;
    return re < 0 ? 0 : re;
}

static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
static inline bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

// The dtype dispatch of every family: f(Dt<TX>{}) for token dtype code `dtype` (fp32 only where F32), otherwise
// bad() -- the entry point's own error.  Op<V>: a compile-time int handed to a launch site the same way.
template <typename T> struct Dt { using type = T; };
template <int V> using Op = std::integral_constant<int, V>;

template <bool F32, typename F, typename Bad>
static int dispatch_x(int dtype, F &&f, Bad &&bad) {
    switch (dtype) {
    case TOME_F32:
        if constexpr (F32) return f(Dt<float>{});
        break;
    case TOME_BF16: return f(Dt<bf16_t>{});
    case TOME_F16: return f(Dt<f16_t>{});
    }
    return bad();
}

// ... and f(Dt<TX>{}, Dt<TS>{}) for the (token, size) pairs of the weighted merges: sizes in the token dtype or fp32
template <bool F32, typename F, typename Bad>
static int dispatch_xs(int x_dtype, int size_dtype, F &&f, Bad &&bad) {
    return dispatch_x<F32>(x_dtype, [&](auto tx) {
        if (size_dtype == TOME_F32) return f(tx, Dt<float>{});
        if (size_dtype == x_dtype) return f(tx, tx);
        return bad();
    }, bad);
}

// The dtype test of the entries without an fp32 form: 0 for bf16 / f16, otherwise the error "<who>: 16-bit <what> only"
static int not_16bit(const char *who, int dtype, const char *what = "tokens") {
    if (dtype == TOME_BF16 || dtype == TOME_F16) return 0;
    return fail(TOME_EINVAL, "%s: 16-bit %s only", who, what);
}

// The vector width of the generic row kernels: f(Op<VEC>{}) with VEC = the elements of a 16-byte chunk when rows of C
// elements are whole chunks and both buffers are 16-byte aligned, otherwise f(Op<1>{})
template <typename TX, typename F>
static int with_vec(int64_t C, const void *in, const void *out, F &&f) {
    constexpr int VEC = 16 / sizeof(TX);
    if (C % VEC == 0 && aligned16(in) && aligned16(out)) return f(Op<VEC>{});
    return f(Op<1>{});
}

// Per-stage timing of tome_match for bench.py's roofline figures: MEASUREMENT BUILD ONLY (-DTOME_PROFILE_HOOKS ->
// lib/libtome_hip_prof.so, loaded by bench.py's stage-timing leg alone; csrc/build.py).  The product library carries
// neither the entry points nor the repeated launches.
#ifdef TOME_PROFILE_HOOKS
// Events are created when profiling is switched on, never inside a launch path.
#define PROF_EVENTS 4
static thread_local struct {
    bool on = false;
    bool valid = false;
    int reps = 1;  // each stage kernel is launched this many times between its two events (idempotent kernels)
    hipEvent_t ev[PROF_EVENTS];
} g_prof;

static inline void prof_mark(int i, hipStream_t st) {
    if (g_prof.on) (void)hipEventRecord(g_prof.ev[i], st);
}

extern "C" int tome_profile_enable(int on) {
    if (on && !g_prof.on) {
        for (int i = 0; i < PROF_EVENTS; ++i)
            if (hipEventCreate(&g_prof.ev[i]) != hipSuccess) return fail(TOME_ELAUNCH, "hipEventCreate failed");
        g_prof.on = true;
        g_prof.valid = false;
    }
    if (on) g_prof.reps = on;
    if (!on && g_prof.on) {
        for (int i = 0; i < PROF_EVENTS; ++i) (void)hipEventDestroy(g_prof.ev[i]);
        g_prof.on = false;
        g_prof.valid = false;
        g_prof.reps = 1;
    }
    return TOME_OK;
}

extern "C" int tome_profile_read(float *stage_ms, int max_stages) {
    if (!g_prof.on || !g_prof.valid || !stage_ms) return fail(TOME_EINVAL, "tome_profile_read: no profiled call");
    if (hipEventSynchronize(g_prof.ev[PROF_EVENTS - 1]) != hipSuccess)
        return fail(TOME_ELAUNCH, "tome_profile_read: event synchronize failed");
    for (int i = 0; i + 1 < PROF_EVENTS && i < max_stages; ++i) {
        if (hipEventElapsedTime(&stage_ms[i], g_prof.ev[i], g_prof.ev[i + 1]) != hipSuccess)
            return fail(TOME_ELAUNCH, "tome_profile_read: elapsed time failed");
        stage_ms[i] /= (float)g_prof.reps;
    }
    return TOME_OK;
}

static inline int prof_reps_now() { return g_prof.on ? g_prof.reps : 1; }
static inline void prof_done(int rc) { g_prof.valid = g_prof.on && rc == TOME_OK; }
#else
static inline void prof_mark(int, hipStream_t) {}
static inline int prof_reps_now() { return 1; }
static inline void prof_done(int) {}
#endif

#ifdef TOME_DIAG_CLOCK
// diagnostic build: in-kernel clock of the last k_scores_rowmax launch = sum(cycles) / sum(100 MHz ticks) over
// its waves, in GHz; also the mean wave duration in microseconds
extern "C" int tome_diag_clock(double *ghz, double *wave_us, int64_t *waves) {
    static unsigned long long host[TOME_DIAG_SLOTS * 2];
    if (hipMemcpyFromSymbol(host, HIP_SYMBOL(g_diag_stamps), sizeof(host)) != hipSuccess)
        return fail(TOME_ELAUNCH, "tome_diag_clock: copy failed");
    double cyc = 0, ticks = 0;
    int64_t nw = 0;
    for (int i = 0; i < TOME_DIAG_SLOTS; ++i)
        if (host[2 * i + 1] > 0) {
            cyc += (double)host[2 * i];
            ticks += (double)host[2 * i + 1];
            ++nw;
        }
    if (!nw) return fail(TOME_EINVAL, "tome_diag_clock: no stamps");
    *ghz = cyc / ticks * 0.1;
    *wave_us = ticks / nw * 0.01;
    *waves = nw;
    return TOME_OK;
}
#endif

// What the even/odd matching and the partition matching lay out alike at the head of their workspaces: the unit
// vectors of the two sets (Na / Nb rows in tiles of TILE_ROWS, nchunk chunks of 64 channels), the row maxima of
// k_scores_rowmax per j-part and the bad-row flags; the even/odd matching's rank array lies between them.
struct SetsWs {
    float *unitA, *unitB, *part_max;
    int *part_idx, *rank;
    uint8_t *badA, *badB;
    int ntA, ntB, nchunk;
    int64_t groupA_f4, groupB_f4;  // float4 per group of each unit set
    size_t bytes;
};

static SetsWs carve_sets(void *base, int64_t n, int64_t Na, int64_t Nb, int64_t D, bool ranked) {
    SetsWs w;
    w.nchunk = (int)((D + 63) / 64);
    w.ntA = (int)((Na + TILE_ROWS - 1) / TILE_ROWS);
    w.ntB = (int)((Nb + TILE_ROWS - 1) / TILE_ROWS);
    w.groupA_f4 = (int64_t)w.ntA * w.nchunk * 512;
    w.groupB_f4 = (int64_t)w.ntB * w.nchunk * 512;
    size_t off = 0;
    char *b = (char *)base;
    w.unitA = (float *)(b + off); off = align_up(off + 16 * (size_t)(n * w.groupA_f4), 256);
    w.unitB = (float *)(b + off); off = align_up(off + 16 * (size_t)(n * w.groupB_f4), 256);
    w.part_max = (float *)(b + off); off = align_up(off + sizeof(float) * (size_t)(n * MAX_WJ * Na), 256);
    w.part_idx = (int *)(b + off); off = align_up(off + sizeof(int) * (size_t)(n * MAX_WJ * Na), 256);
    w.rank = nullptr;
    if (ranked) { w.rank = (int *)(b + off); off = align_up(off + sizeof(int) * (size_t)(n * Na), 256); }
    w.badA = (uint8_t *)(b + off); off = align_up(off + (size_t)(n * Na), 256);
    w.badB = (uint8_t *)(b + off); off = align_up(off + (size_t)(n * (Nb > 0 ? Nb : 1)), 256);
    w.bytes = off;
    return w;
}

struct MatchWs : SetsWs {
    // the filter path (tome_match_filter.h; D <= 64): bf16 means in MFMA fragment order, norms, candidate lists
    uint4 *vA, *vB;
    float *normA, *normB, *invB, *node_max;
    int *node_idx;
    CandEntry *cand;
    uint8_t *cand_n, *tile_flag;
    int T2p;
};

static MatchWs carve(void *base, int64_t n, int64_t T, int64_t D) {
    const int64_t T1 = (T + 1) / 2, T2 = T / 2;
    MatchWs w;
    static_cast<SetsWs &>(w) = carve_sets(base, n, T1, T2, D, true);
    size_t off = w.bytes;
    char *b = (char *)base;
    w.T2p = w.ntB * TILE_ROWS;
    w.vA = w.vB = nullptr;
    if (w.nchunk == 1) {
        w.vA = (uint4 *)(b + off); off = align_up(off + 4096 * (size_t)(n * w.ntA), 256);
        w.vB = (uint4 *)(b + off); off = align_up(off + 4096 * (size_t)(n * (w.ntB > 0 ? w.ntB : 1)), 256);
        w.normA = (float *)(b + off); off = align_up(off + sizeof(float) * (size_t)(n * T1), 256);
        w.normB = (float *)(b + off); off = align_up(off + sizeof(float) * (size_t)(n * (T2 > 0 ? T2 : 1)), 256);
        w.invB = (float *)(b + off); off = align_up(off + sizeof(float) * (size_t)(n * (w.T2p > 0 ? w.T2p : 1)) + 64, 256);
        w.node_max = (float *)(b + off); off = align_up(off + sizeof(float) * (size_t)(n * T1), 256);
        w.node_idx = (int *)(b + off); off = align_up(off + sizeof(int) * (size_t)(n * T1), 256);
        w.cand = (CandEntry *)(b + off); off = align_up(off + sizeof(CandEntry) * 2 * FILT_KH * (size_t)(n * T1), 256);
        w.cand_n = (uint8_t *)(b + off); off = align_up(off + 2 * (size_t)(n * T1), 256);
        w.tile_flag = (uint8_t *)(b + off); off = align_up(off + (size_t)(n * w.ntA), 256);
    }
    w.bytes = off;
    return w;
}

extern "C" size_t tome_match_workspace_bytes(int64_t n, int64_t T, int64_t D) {
    if (n <= 0 || T <= 0 || D <= 0) return 0;
    return carve(nullptr, n, T, D).bytes;
}

// The workspace of the matching entries: at least `need` bytes, 256-byte aligned
static int check_workspace(const char *who, const void *workspace, size_t workspace_bytes, size_t need) {
    if (!workspace || workspace_bytes < need)
        return fail(TOME_EWORKSPACE, "%s: workspace %zu < %zu bytes", who, workspace_bytes, need);
    if (((uintptr_t)workspace & 255) != 0) return fail(TOME_EINVAL, "%s: workspace not 256-byte aligned", who);
    return TOME_OK;
}

// ... and in front of it the index buffers of an even/odd matching that merges `re` of T tokens: unm_idx may be
// absent when every even token is a source
static int check_match_buffers(const char *who, int64_t T, int64_t re, const int64_t *src_idx, const int64_t *dst_idx,
                               const int64_t *unm_idx, const void *workspace, size_t workspace_bytes, size_t need) {
    if (!src_idx || !dst_idx || (!unm_idx && (T + 1) / 2 > re)) return fail(TOME_EINVAL, "%s: null index buffer", who);
    return check_workspace(who, workspace, workspace_bytes, need);
}

// Can the unit-vector kernels read the rows of a [n, T, D] metric in 16-byte chunks?
static bool rows_16byte(const void *metric, int dtype, int64_t D, int64_t stride_n, int64_t stride_t) {
    const size_t es = dtype == TOME_F32 ? 4 : 2;
    return (D % 8 == 0) && (((uintptr_t)metric) % 16 == 0) && ((stride_n * es) % 16 == 0) && ((stride_t * es) % 16 == 0);
}

// Stage 1 of both matchings, the unit vectors: rows of whole 16-byte chunks (rows_16byte) whose chunk count of 64
// channels has an unrolled kernel take it -- fast(Dt<TY>{}, Op<NCH>{}) --, everything else generic(Dt<TY>{}).  The
// two callbacks launch; `who` names the entry in the error of an unknown dtype.
template <typename Fast, typename Generic>
static int launch_unit_rows(const char *who, int dtype, bool rows16, int nchunk, Fast &&fast, Generic &&generic) {
    return dispatch_x<true>(dtype, [&](auto ty) {
        switch (rows16 ? nchunk : 0) {
        case 1: fast(ty, Op<1>{}); break;
        case 2: fast(ty, Op<2>{}); break;
        case 3: fast(ty, Op<3>{}); break;
        case 4: fast(ty, Op<4>{}); break;
        case 6: fast(ty, Op<6>{}); break;
        case 8: fast(ty, Op<8>{}); break;
        case 12: fast(ty, Op<12>{}); break;
        case 16: fast(ty, Op<16>{}); break;
        default: generic(ty); break;
        }
        return TOME_OK;
    }, [&] { return fail(TOME_EINVAL, "%s: dtype %d", who, dtype); });
}

// Stage 2 of both matchings, similarity + row max / argmax of Na rows against Nb: one single-wave workgroup per
// (group, A tile, j-part); the B tiles are split into *parts parts so that the launch has >= ~6 waves per SIMD (1024
// SIMDs) whatever the batch (target measured on MI355X)
static int launch_scores_rowmax(const char *who, const SetsWs &w, int64_t n, int Na, int Nb, int distill_token,
                                hipStream_t st, int *parts) {
    const long target_waves = 6144L;
    int WJ = (int)((target_waves + n * w.ntA - 1) / (n * w.ntA));
    if (WJ > MAX_WJ) WJ = MAX_WJ;
    if (WJ > w.ntB) WJ = w.ntB;
    if (WJ < 1) WJ = 1;
    *parts = WJ;
    const int64_t nb2 = ((n + 7) / 8) * 8 * w.ntA * WJ;
    if (nb2 > 0x7fffffffLL) return fail(TOME_EINVAL, "%s: problem too large", who);
    auto launch = [&](auto one_chunk) {
        hipLaunchKernelGGL(k_scores_rowmax<decltype(one_chunk)::value != 0>, dim3((unsigned)nb2), dim3(64), 0, st,
                           (const f32x4 *)w.unitA, (const f32x4 *)w.unitB, (int)n, Na, Nb, w.nchunk, w.ntA, w.ntB, WJ,
                           w.groupA_f4, w.groupB_f4, distill_token, w.part_max, w.part_idx, nullptr);
        return check_launch("k_scores_rowmax");
    };
    return w.nchunk == 1 ? launch(Op<1>{}) : launch(Op<0>{});
}

static int launch_select(const SetsWs &w, int nparts, bool nan_flags, int64_t n, int64_t T, int64_t re, int class_token,
                         int distill_token, int64_t *src_idx, int64_t *dst_idx, int64_t *unm_idx,
                         float *node_max, int32_t *row_map, hipStream_t st) {
    const int T1 = (int)((T + 1) / 2);
    dim3 grid((T1 + 63) / 64, (unsigned)n);
    const int quarter = (((T1 + 3) >> 2) + 1) & ~1;
    const size_t lds = sizeof(unsigned long long) * (size_t)(4 * quarter);
    if (lds > 160 * 1024) return fail(TOME_EINVAL, "sequences of more than ~40000 tokens do not fit the ranking kernel's LDS");
    hipLaunchKernelGGL(k_rank_select, grid, dim3(256), lds, st, w.part_max, w.part_idx, nparts, (int)n, T1,
                       (int)(T / 2), nan_flags ? w.badA : nullptr, nan_flags ? w.badB : nullptr, (int)re, class_token,
                       distill_token, src_idx, dst_idx, unm_idx, node_max, w.rank, row_map);
    if (int rc = check_launch("k_rank_select")) return rc;
    if (class_token) {
        hipLaunchKernelGGL(k_compact_unm, dim3((unsigned)n), dim3(256), 0, st, w.rank, T1, (int)re,
                           distill_token, unm_idx, row_map);
        if (int rc = check_launch("k_compact_unm")) return rc;
    }
    return TOME_OK;
}

// The filter path (tome_match_filter.h) serves bf16 metrics of at most 64 channels when the launch has enough A tiles
// to fill the chip with one wave per tile; everything else keeps the fp32 pass.  TOME_SCORES_FILTER=0 switches it off
// (measurement switch, read per call).
static bool use_filter(const MatchWs &w, int dtype, int64_t n, int64_t D) {
    const char *e = getenv("TOME_SCORES_FILTER");
    if (e && e[0] == '0') return false;
    const int64_t min_tiles = (e && e[0] == '2') ? 1 : 1024;  // ("2": also for small launches -- the tests)
    return dtype == TOME_BF16 && w.nchunk == 1 && D % 8 == 0 && w.ntB > 0 && w.T2p <= FILT_MAX_T2P &&
           n * w.ntA >= min_tiles;
}

// shared tail of tome_match / tome_match_keys: stages 2 (similarity + row max) and 3 (rank + select)
static int match_tail(const char *who, const MatchWs &w, int64_t n, int64_t T, int64_t D, int64_t re, int class_token,
                      int distill_token, int64_t *src_idx, int64_t *dst_idx, int64_t *unm_idx, float *node_max,
                      int32_t *row_map, hipStream_t st, bool filtered) {
    const int T1 = (int)((T + 1) / 2), T2 = (int)(T / 2);
    const int prof_reps = prof_reps_now();
    int parts = 1;
    for (int rep = 0; rep < prof_reps; ++rep) {
        if (filtered) {
            // 2a. approximate scores on the bf16 matrix pipe, candidate columns per row (tome_match_filter.h)
            hipLaunchKernelGGL(k_scores_filter, dim3((unsigned)(((n + 7) / 8) * 8 * ((w.ntA + FILT_ATW - 1) / FILT_ATW))),
                               dim3(64), sizeof(float) * (size_t)w.T2p, st, w.vA, w.vB,
                               w.normA, w.invB, (int)n, T1, T2, w.T2p, w.ntA, w.ntB, distill_token, w.cand, w.cand_n,
                               w.tile_flag);
            if (int rc = check_launch("k_scores_filter")) return rc;
            // 2b. the exact score of every row's winner; the same launch carries one wave per A tile that takes the
            // fp32 pass when the filter flagged the tile (overflowed candidate list, norm out of range) and leaves at
            // once otherwise
            const int64_t exact_blocks = (n * T1 + 255) / 256, fb_blocks = (n * w.ntA + 3) / 4;
            hipLaunchKernelGGL(k_exact_rows, dim3((unsigned)(exact_blocks + fb_blocks)), dim3(256), 0, st, w.vA, w.vB,
                               w.normA, w.normB, (int)n, T1, T2, (int)D, w.ntA, w.ntB, w.cand, w.cand_n, w.tile_flag,
                               (int)exact_blocks, distill_token, w.node_max, w.node_idx);
            if (int rc = check_launch("k_exact_rows")) return rc;
            continue;
        }
        // 2. similarity + row max/argmax
        if (int rc = launch_scores_rowmax(who, w, n, T1, T2, distill_token, st, &parts)) return rc;
    }
    prof_mark(2, st);

    // 3. rank + select
    int rc = TOME_OK;
    SetsWs ws = w;
    if (filtered) {
        ws.part_max = w.node_max;
        ws.part_idx = w.node_idx;
    }
    for (int rep = 0; rep < prof_reps && rc == TOME_OK; ++rep)
        rc = launch_select(ws, parts, true, n, T, re, class_token, distill_token, src_idx, dst_idx, unm_idx, node_max, row_map, st);
    prof_mark(3, st);
    prof_done(rc);
    return rc;
}

extern "C" int tome_match(const void *metric, int dtype, int64_t n, int64_t T, int64_t D, int64_t stride_n,
                          int64_t stride_t, int64_t r, int class_token, int distill_token, int64_t *src_idx,
                          int64_t *dst_idx, int64_t *unm_idx, float *node_max, int32_t *row_map,
                          void *workspace, size_t workspace_bytes, tome_stream_t stream) {
    if (!metric || n <= 0 || T <= 0 || D <= 0) return fail(TOME_EINVAL, "tome_match: bad shape/pointer");
    if (n > 0x7fffffff / T || (int64_t)n * T * ((D + 63) / 64 * 64) > (int64_t)1 << 40)
        return fail(TOME_EINVAL, "tome_match: problem too large");
    const int64_t re = tome_effective_r(T, r, class_token, distill_token);
    if (re <= 0) return TOME_OK;
    if (int rc = check_match_buffers("tome_match", T, re, src_idx, dst_idx, unm_idx, workspace, workspace_bytes,
                                     tome_match_workspace_bytes(n, T, D)))
        return rc;
    hipStream_t st = (hipStream_t)stream;
    const MatchWs w = carve(workspace, n, T, D);
    // 1. unit vectors
    prof_mark(0, st);
    const bool rows16 = rows_16byte(metric, dtype, D, stride_n, stride_t);
    const bool filtered = rows16 && use_filter(w, dtype, n, D);
    const int prof_reps = prof_reps_now();
    for (int rep = 0; rep < prof_reps; ++rep) {
        if (filtered) {
            hipLaunchKernelGGL(k_unit_rows_f<false>, dim3((unsigned)((n * T + 31) / 32)), dim3(256), 0, st,
                               (const bf16_t *)metric, stride_n, 1, (int64_t)0, (int64_t)0, stride_t, (int)n, 1, (int)T, (int)D,
                               w.vA, w.vB, w.ntA, w.ntB, w.normA, w.normB, w.invB, w.T2p, w.badA, w.badB);
            continue;
        }
        const int rc = launch_unit_rows("tome_match", dtype, rows16, w.nchunk, [&](auto ty, auto nch) {
            using TY = typename decltype(ty)::type;
            hipLaunchKernelGGL((k_unit_rows<TY, decltype(nch)::value>), dim3((unsigned)((n * T + 31) / 32)), dim3(256), 0,
                               st, (const TY *)metric, stride_n, stride_t, (int)n, (int)T, (int)D, w.unitA, w.unitB,
                               w.groupA_f4, w.groupB_f4, w.badA, w.badB);
        }, [&](auto ty) {
            using TY = typename decltype(ty)::type;
            hipLaunchKernelGGL((k_unit_rows_generic<TY>), dim3((unsigned)((n * T + 255) / 256)), dim3(256), 0, st,
                               (const TY *)metric, stride_n, stride_t, (int)n, (int)T, (int)D, w.nchunk * 64, w.unitA,
                               w.unitB, w.groupA_f4, w.groupB_f4, w.badA, w.badB);
        });
        if (rc) return rc;
    }
    if (int rc = check_launch("k_unit_rows")) return rc;
    prof_mark(1, st);

    return match_tail("tome_match", w, n, T, D, re, class_token, distill_token, src_idx, dst_idx, unm_idx, node_max,
                      row_map, st, filtered);
}

extern "C" int tome_match_keys(const void *keys, int dtype, int64_t n, int64_t H, int64_t T, int64_t D,
                               int64_t stride_n, int64_t inner, int64_t stride_inner, int64_t stride_h,
                               int64_t stride_t, int64_t r, int class_token,
                               int distill_token, int64_t *src_idx, int64_t *dst_idx, int64_t *unm_idx,
                               float *node_max, int32_t *row_map, void *workspace, size_t workspace_bytes,
                               tome_stream_t stream) {
    if (!keys || n <= 0 || T <= 0 || H <= 0) return fail(TOME_EINVAL, "tome_match_keys: bad shape/pointer");
    if (D != 64) return fail(TOME_EINVAL, "tome_match_keys: head dimension %lld (only 64 is fused)", (long long)D);
    if (n > 0x7fffffff / T) return fail(TOME_EINVAL, "tome_match_keys: problem too large");
    const size_t es = dtype == TOME_F32 ? 4 : 2;
    auto bad_dtype = [&] { return fail(TOME_EINVAL, "tome_match_keys: dtype %d", dtype); };
    if (dtype < TOME_F32 || dtype > TOME_F16) return bad_dtype();
    if (((uintptr_t)keys) % 16 || (stride_n * es) % 16 || (stride_h * es) % 16 || (stride_t * es) % 16 ||
        (stride_inner * es) % 16)
        return fail(TOME_EINVAL, "tome_match_keys: keys must be 16-byte aligned in every stride");
    if (inner < 1 || n % inner) return fail(TOME_EINVAL, "tome_match_keys: %lld groups do not split into %lld per clip",
                                            (long long)n, (long long)inner);
    const int64_t re = tome_effective_r(T, r, class_token, distill_token);
    if (re <= 0) return TOME_OK;
    if (int rc = check_match_buffers("tome_match_keys", T, re, src_idx, dst_idx, unm_idx, workspace, workspace_bytes,
                                     tome_match_workspace_bytes(n, T, D)))
        return rc;
    hipStream_t st = (hipStream_t)stream;
    const MatchWs w = carve(workspace, n, T, D);
    prof_mark(0, st);
    const int prof_reps = prof_reps_now();
    const unsigned nb = (unsigned)((n * T + 31) / 32);
    const bool filtered = use_filter(w, dtype, n, D);
    for (int rep = 0; rep < prof_reps; ++rep) {
        if (filtered) {
            hipLaunchKernelGGL(k_unit_rows_f<true>, dim3(nb), dim3(256), 0, st, (const bf16_t *)keys, stride_n, (int)inner,
                               stride_inner, stride_h, stride_t, (int)n, (int)H, (int)T, (int)D, w.vA, w.vB, w.ntA, w.ntB,
                               w.normA, w.normB, w.invB, w.T2p, w.badA, w.badB);
            continue;
        }
        const int rc = dispatch_x<true>(dtype, [&](auto ty) {
            using TY = typename decltype(ty)::type;
            hipLaunchKernelGGL(k_unit_rows_heads<TY>, dim3(nb), dim3(256), 0, st, (const TY *)keys, stride_n, (int)inner,
                               stride_inner, stride_h, stride_t, (int)n, (int)H, (int)T, w.unitA, w.unitB, w.groupA_f4,
                               w.groupB_f4, w.badA, w.badB);
            return TOME_OK;
        }, bad_dtype);
        if (rc) return rc;
    }
    if (int rc = check_launch("k_unit_rows_heads")) return rc;
    prof_mark(1, st);
    return match_tail("tome_match_keys", w, n, T, D, re, class_token, distill_token, src_idx, dst_idx, unm_idx, node_max,
                      row_map, st, filtered);
}

extern "C" int tome_match_scores(const float *scores, int64_t n, int64_t T, int64_t r, int class_token,
                                 int distill_token, int64_t *src_idx, int64_t *dst_idx, int64_t *unm_idx,
                                 float *node_max, int32_t *row_map, void *workspace, size_t workspace_bytes,
                                 tome_stream_t stream) {
    if (!scores || n <= 0 || T <= 0) return fail(TOME_EINVAL, "tome_match_scores: bad shape/pointer");
    const int64_t re = tome_effective_r(T, r, class_token, distill_token);
    if (re <= 0) return TOME_OK;
    if (int rc = check_match_buffers("tome_match_scores", T, re, src_idx, dst_idx, unm_idx, workspace, workspace_bytes,
                                     tome_match_workspace_bytes(n, T, 1)))
        return rc;
    hipStream_t st = (hipStream_t)stream;
    const MatchWs w = carve(workspace, n, T, 1);
    const int T1 = (int)((T + 1) / 2), T2 = (int)(T / 2);
    const unsigned nb = (unsigned)((n * T1 + 3) / 4);
    hipLaunchKernelGGL(k_rowmax_given, dim3(nb), dim3(256), 0, st, scores, (int)n, T1, T2, class_token,
                       distill_token, w.part_max, w.part_idx);
    if (int rc = check_launch("k_rowmax_given")) return rc;
    return launch_select(w, 1, false, n, T, re, class_token, distill_token, src_idx, dst_idx, unm_idx, node_max, row_map,
                         st);
}

extern "C" int tome_edge_keep(const float *node_max, const int64_t *src_idx, int64_t n, int64_t T, int64_t r,
                              float threshold, uint8_t *edge_keep, tome_stream_t stream) {
    if (!node_max || !src_idx || !edge_keep || n <= 0 || r <= 0) return fail(TOME_EINVAL, "tome_edge_keep: bad args");
    const int T1 = (int)((T + 1) / 2);
    const unsigned nb = (unsigned)((n * r + 255) / 256);
    hipLaunchKernelGGL(k_edge_keep, dim3(nb), dim3(256), 0, (hipStream_t)stream, node_max, src_idx, (int)n, T1,
                       (int)r, threshold, edge_keep);
    return check_launch("k_edge_keep");
}

static TokLayout contiguous_layout(int64_t T, int64_t C) { return TokLayout{0, T * C, 0, C, 1}; }

// XCD-aware numbering of the workgroups (MergeSched, csrc/tome_merge.h) for the launches where many destinations
// receive sources (8 r >= T: TimeSformer / Motionformer frame groups at r = 32, late layers at r = 16) -- there the
// edge blocks at the end of every group otherwise land on the same XCDs in every group; measured per layer with
// tools/regroup_kernel_times.py: -4 ... -7 % at r = 32, +-1 % at r = 16, +3 % at r = 8 and +3.6 % on the
// benchmark's VideoMAE launches (598 vs 577 us), hence not there.
static MergeSched merge_sched(bool drop, int64_t T, int64_t r, int64_t bpg, int64_t ny) {
    const int64_t total = bpg * ny;
    MergeSched sch{(unsigned)bpg, (unsigned)total, 0u, 0, 0ull};
    if (!drop && r <= 64 && 8 * r >= T && total < (1ll << 28) && bpg < (1ll << 12) && total >= 64) {
        sch.per_xcd = (unsigned)((total + 7) / 8);
        sch.on = 1;
        sch.magic = ((1ull << 40) + (unsigned long long)bpg - 1ull) / (unsigned long long)bpg;
    }
    return sch;
}

// the template arguments of one k_merge_rows_fast form, handed to launch_merge_rows' launch site
template <int NIT, bool LN, bool EAGER> struct FastForm {
    static constexpr int nit = NIT;
    static constexpr bool ln = LN, eager = EAGER;
};

template <typename TX, typename TS, int OP>
static int launch_merge_rows(const void *x, const void *size, int64_t n, int64_t T, int64_t C, int64_t r,
                             const int64_t *src, const int64_t *dst, const int64_t *unm, int distill,
                             const uint8_t *keep, void *xout, void *sout, hipStream_t st,
                             const TokLayout *lin_p = nullptr, const TokLayout *lout_p = nullptr, int cls_rows = 0,
                             const LnArgs *ln_p = nullptr, void *lsout = nullptr) {
    constexpr int VEC = 16 / sizeof(TX);
    const int64_t To = T - r;
    const TokLayout lin = lin_p ? *lin_p : contiguous_layout(T, C);
    const TokLayout lout = lout_p ? *lout_p : contiguous_layout(To, C);
    const bool vec_ok = (C % VEC == 0) && aligned16(x) && aligned16(xout);
    const int64_t cpr = C / VEC;  // 16-byte chunks per row
    const LnArgs no_ln{nullptr, nullptr, nullptr, 0.0f, nullptr, 0, TokLayout{0, 0, 0, 0, 1}, nullptr, nullptr};
    if (vec_ok && cpr <= FAST_NIT * WAVE) {
        // rows per wave: measured on MI355X, NIT=6 (four 1536-byte rows per wave for 768-channel bf16 tokens)
        // beats NIT=3 by ~4 %; with the LayerNorm fused and the residual stream next to x 3 chunks per lane
        // (77 instead of 107 VGPRs, six instead of four waves per SIMD) measured 5 % faster (124 vs 131 us)
        const int nit = (cpr <= 3 * WAVE && ln_p && ln_p->addend) ? 3 : FAST_NIT;
        int R = (int)((nit * WAVE) / cpr);
        if (R > FAST_MAXR) R = FAST_MAXR;
        // grid.x = the blocks of one group (streaming waves, then the edge waves), (y, z) = group (+ rows of blocks
        // for the class tokens behind them)
        const int64_t bpg = ((To + R - 1) / R + (OP == OP_DROP ? 0 : r) + 3) / 4;
        const int64_t ny = n + (cls_rows ? (cls_rows + 4 * bpg - 1) / (4 * bpg) : 0);
        const int64_t gy = ny < 65535 ? ny : 65535, gz = (ny + gy - 1) / gy;
        if (gz > 65535) return fail(TOME_EINVAL, "merge: too many groups (%lld)", (long long)n);
        const MergeSched sch = merge_sched(OP == OP_DROP, T, r, bpg, ny);
        const dim3 grid = sch.on ? dim3(8u * sch.per_xcd, 1u, 1u) : dim3((unsigned)bpg, (unsigned)gy, (unsigned)gz);
        const LnArgs &ln = ln_p ? *ln_p : no_ln;
        auto launch = [&](auto form) {
            using F = decltype(form);
            hipLaunchKernelGGL((k_merge_rows_fast<TX, TS, OP, F::nit, F::ln, F::eager>), grid, dim3(256), 0, st,
                               (const TX *)x, (const TS *)size, (int)n, (int)T, (int)C, (int)r, R, (int)cpr,
                               (int)((To + R - 1) / R), src, dst, unm, distill, keep, (TX *)xout, (TS *)sout, lin, lout,
                               cls_rows, ln, (TS *)lsout, sch);
            return check_launch("k_merge_rows_fast");
        };
        if (ln_p) {
            if ((OP != OP_WAVG && OP != OP_DROP) || sizeof(TX) != 2 || cpr > 2 * WAVE || !aligned16(ln_p->y) ||
                !aligned16(ln_p->weight) || !aligned16(ln_p->bias))
                return fail(TOME_EINVAL, "fused LayerNorm needs 16-bit tokens with C <= 1024 and 16-byte aligned buffers");
            // drop: every kept row is a streamed row -- no edge waves, no EAGER form, merge_sched stays off
            if constexpr (OP == OP_DROP && sizeof(TX) == 2)
                return nit == 3 ? launch(FastForm<3, true, false>{}) : launch(FastForm<6, true, false>{});
            if constexpr (OP == OP_WAVG && sizeof(TX) == 2) {
                // many destinations receive sources: the streaming waves skip those rows (EAGER, csrc/tome_merge.h)
                if (r <= 64 && 8 * r >= T)
                    return nit == 3 ? launch(FastForm<3, true, true>{}) : launch(FastForm<6, true, true>{});
                return nit == 3 ? launch(FastForm<3, true, false>{}) : launch(FastForm<6, true, false>{});
            }
        }
        return launch(FastForm<FAST_NIT, false, false>{});
    }
    if (cls_rows || ln_p)
        return fail(TOME_EINVAL, "regrouped / LayerNorm-fused merge needs rows of whole 16-byte chunks (C=%lld)", (long long)C);
    const int64_t rows = n * To;
    const unsigned nb = (unsigned)((rows + 3) / 4);
    if (vec_ok)
        hipLaunchKernelGGL((k_merge_rows<TX, TS, VEC, OP>), dim3(nb), dim3(256), 0, st, (const TX *)x,
                           (const TS *)size, (int)n, (int)T, (int)C, (int)r, src, dst, unm, distill, keep, (TX *)xout,
                           (TS *)sout, lin, lout, (TS *)lsout);
    else
        hipLaunchKernelGGL((k_merge_rows<TX, TS, 1, OP>), dim3(nb), dim3(256), 0, st, (const TX *)x,
                           (const TS *)size, (int)n, (int)T, (int)C, (int)r, src, dst, unm, distill, keep, (TX *)xout,
                           (TS *)sout, lin, lout, (TS *)lsout);
    return check_launch("k_merge_rows");
}

static int check_merge_args(const char *who, const void *x, int64_t n, int64_t T, int64_t C, int64_t r,
                            const void *out) {
    if (!x || !out || n <= 0 || T <= 0 || C <= 0) return fail(TOME_EINVAL, "%s: bad shape/pointer", who);
    if (r <= 0 || r > T / 2) return fail(TOME_EINVAL, "%s: r=%lld outside (0, T/2]", who, (long long)r);
    if (n * (T - r) > 0x7fffffffLL * 4 || n * T > 0x7fffffffLL) return fail(TOME_EINVAL, "%s: too many rows", who);
    return TOME_OK;
}

extern "C" int tome_merge_wavg(const void *x, int x_dtype, const void *size, int size_dtype, int64_t n, int64_t T,
                               int64_t C, int64_t r, const int64_t *src_idx, const int64_t *dst_idx,
                               const int64_t *unm_idx, int distill_token, const uint8_t *edge_keep, void *x_out,
                               void *size_out, void *log_size_out, tome_stream_t stream) {
    if (int rc = check_merge_args("tome_merge_wavg", x, n, T, C, r, x_out)) return rc;
    if (!src_idx || !dst_idx || (!unm_idx && (T + 1) / 2 > r) || !size_out)
        return fail(TOME_EINVAL, "tome_merge_wavg: null buffer");
    return dispatch_xs<true>(x_dtype, size_dtype, [&](auto tx, auto ts) {
        return launch_merge_rows<typename decltype(tx)::type, typename decltype(ts)::type, OP_WAVG>(
            x, size, n, T, C, r, src_idx, dst_idx, unm_idx, distill_token, edge_keep, x_out, size_out,
            (hipStream_t)stream, nullptr, nullptr, 0, nullptr, log_size_out);
    }, [&] { return fail(TOME_EINVAL, "tome_merge_wavg: unsupported dtypes x=%d size=%d", x_dtype, size_dtype); });
}

extern "C" int tome_merge_wavg_ln(const void *x, int x_dtype, const void *size, int size_dtype, int64_t n, int64_t T,
                                  int64_t C, int64_t r, const int64_t *src_idx, const int64_t *dst_idx,
                                  const int64_t *unm_idx, int distill_token, const uint8_t *edge_keep,
                                  const void *ln_weight, const void *ln_bias, float eps, const void *addend,
                                  void *x_out, void *y_out, void *size_out, void *log_size_out,
                                  const void *x_out_bias, tome_stream_t stream) {
    if (int rc = check_merge_args("tome_merge_wavg_ln", x, n, T, C, r, x_out)) return rc;
    if (addend && !aligned16(addend)) return fail(TOME_EINVAL, "tome_merge_wavg_ln: addend not 16-byte aligned");
    if (x_out_bias && !aligned16(x_out_bias)) return fail(TOME_EINVAL, "tome_merge_wavg_ln: x_out_bias not 16-byte aligned");
    if (!src_idx || !dst_idx || (!unm_idx && (T + 1) / 2 > r) || !size_out || !y_out || !ln_weight || !ln_bias)
        return fail(TOME_EINVAL, "tome_merge_wavg_ln: null buffer");
    const LnArgs ln{ln_weight, ln_bias, y_out, eps, addend, 0, TokLayout{0, 0, 0, 0, 1}, nullptr, x_out_bias};
    return dispatch_xs<false>(x_dtype, size_dtype, [&](auto tx, auto ts) {
        return launch_merge_rows<typename decltype(tx)::type, typename decltype(ts)::type, OP_WAVG>(
            x, size, n, T, C, r, src_idx, dst_idx, unm_idx, distill_token, edge_keep, x_out, size_out,
            (hipStream_t)stream, nullptr, nullptr, 0, &ln, log_size_out);
    }, [&] { return fail(TOME_EINVAL, "tome_merge_wavg_ln: 16-bit tokens only (x=%d size=%d)", x_dtype, size_dtype); });
}

static int merge_wavg_regrouped_impl(const char *who, const void *x, int x_dtype, const void *size, int size_dtype,
                                     int64_t B, int64_t F, int64_t P, int64_t C, int64_t r, int has_cls,
                                     const int64_t *src_idx, const int64_t *dst_idx, const int64_t *unm_idx,
                                     const uint8_t *edge_keep, void *x_out, void *size_out, void *log_size_out,
                                     const LnArgs *ln, tome_stream_t stream) {
    if (B <= 0 || F <= 0) return fail(TOME_EINVAL, "%s: bad shape", who);
    const int64_t n = B * F;
    if (int rc = check_merge_args(who, x, n, P, C, r, x_out)) return rc;
    if (!src_idx || !dst_idx || (!unm_idx && (P + 1) / 2 > r) || !size_out) return fail(TOME_EINVAL, "%s: null buffer", who);
    const int cls = has_cls ? 1 : 0;
    const TokLayout lin{cls * C, (cls + P * F) * C, C, F * C, (int)F};
    const TokLayout lout{cls * C, (cls + (P - r) * F) * C, C, F * C, (int)F};
    return dispatch_xs<true>(x_dtype, size_dtype, [&](auto tx, auto ts) {
        return launch_merge_rows<typename decltype(tx)::type, typename decltype(ts)::type, OP_WAVG>(
            x, size, n, P, C, r, src_idx, dst_idx, unm_idx, 0, edge_keep, x_out, size_out, (hipStream_t)stream, &lin,
            &lout, cls ? (int)B : 0, ln, log_size_out);
    }, [&] { return fail(TOME_EINVAL, "%s: unsupported dtypes x=%d size=%d", who, x_dtype, size_dtype); });
}

extern "C" int tome_merge_wavg_regrouped(const void *x, int x_dtype, const void *size, int size_dtype, int64_t B,
                                         int64_t F, int64_t P, int64_t C, int64_t r, int has_cls,
                                         const int64_t *src_idx, const int64_t *dst_idx, const int64_t *unm_idx,
                                         const uint8_t *edge_keep, void *x_out, void *size_out,
                                         void *log_size_out, tome_stream_t stream) {
    return merge_wavg_regrouped_impl("tome_merge_wavg_regrouped", x, x_dtype, size, size_dtype, B, F, P, C, r, has_cls,
                                     src_idx, dst_idx, unm_idx, edge_keep, x_out, size_out, log_size_out, nullptr, stream);
}

extern "C" int tome_merge_wavg_regrouped_ln(const void *x, int x_dtype, const void *size, int size_dtype, int64_t B,
                                            int64_t F, int64_t P, int64_t C, int64_t r, int has_cls,
                                            const int64_t *src_idx, const int64_t *dst_idx,
                                            const int64_t *unm_idx, const uint8_t *edge_keep, const void *ln_weight,
                                            const void *ln_bias, float eps, const void *addend,
                                            int addend_grouped, const void *cls_addend, void *x_out,
                                            void *y_out, void *size_out, void *log_size_out,
                                            const void *x_out_bias, tome_stream_t stream) {
    if (x_out_bias && !aligned16(x_out_bias))
        return fail(TOME_EINVAL, "tome_merge_wavg_regrouped_ln: x_out_bias not 16-byte aligned");
    if (!y_out || !ln_weight || !ln_bias) return fail(TOME_EINVAL, "tome_merge_wavg_regrouped_ln: null buffer");
    if (x_dtype == TOME_F32) return fail(TOME_EINVAL, "tome_merge_wavg_regrouped_ln: 16-bit tokens only");
    if ((addend && !aligned16(addend)) || (cls_addend && !aligned16(cls_addend)))
        return fail(TOME_EINVAL, "tome_merge_wavg_regrouped_ln: addend alignment");
    if (addend_grouped && !addend) return fail(TOME_EINVAL, "tome_merge_wavg_regrouped_ln: addend_grouped without addend");
    LnArgs ln{ln_weight, ln_bias, y_out, eps, addend, 0, TokLayout{0, 0, 0, 0, 1}, nullptr, x_out_bias};
    if (addend_grouped) {  // addend [B*F, has_cls + P, C]: group g's token p at (g*(cls+P) + cls + p)*C
        const int64_t cls = has_cls ? 1 : 0;
        ln.a_own = 1;
        ln.la = TokLayout{cls * C, (cls + P) * C, 0, C, 1};
        ln.cls_addend = cls_addend;
    }
    return merge_wavg_regrouped_impl("tome_merge_wavg_regrouped_ln", x, x_dtype, size, size_dtype, B, F, P, C, r,
                                     has_cls, src_idx, dst_idx, unm_idx, edge_keep, x_out, size_out, log_size_out, &ln, stream);
}

// Rows per wave of the LayerNorm kernels: `nit` 16-byte chunks per lane, rows of `cpr` chunks, at most FAST_MAXR rows.
// The backward (ln_bwd_form) recomputes the statistics of the rows the forward normalised and must pick the forward's
// packing to reproduce its bits: every one of them asks here.
static inline int ln_rows_per_wave(int64_t cpr, int nit) {
    const int64_t R = (nit * WAVE) / cpr;
    return R > FAST_MAXR ? FAST_MAXR : (int)R;
}

// One launch of k_add_ln_rows (three slots per lane) for the 16-bit entries and the autocast entry alike.
template <typename TS, typename TA, typename TY, typename TP>
static int launch_add_ln_rows(const char *who, const void *x, const void *addend, int64_t rows, int64_t C,
                              const void *ln_weight, const void *ln_bias, float eps, int64_t y_group, void *x_out,
                              void *y_out, tome_stream_t stream) {
    const int64_t cpr = C / 8;
    const int R = ln_rows_per_wave(cpr, 3);  // 3 slots per lane: 100.6 us vs 105 us with 6 (batch 64)
    const int64_t waves = (rows + R - 1) / R;
    if ((waves + 3) / 4 > 0x7fffffffLL) return fail(TOME_EINVAL, "%s: too many rows", who);
    hipLaunchKernelGGL((k_add_ln_rows<TS, TA, TY, TP, 3>), dim3((unsigned)((waves + 3) / 4)), dim3(256), 0,
                       (hipStream_t)stream, (const TS *)x, (const TA *)addend, rows, (int)C, R, (int)cpr,
                       (const TP *)ln_weight, (const TP *)ln_bias, eps, (int)y_group, (TS *)x_out, (TY *)y_out);
    return check_launch("k_add_ln_rows");
}

static int add_layernorm_impl(const void *x, const void *addend, int dtype, int64_t rows, int64_t C,
                              const void *ln_weight, const void *ln_bias, float eps, void *x_out, void *y_out,
                              int64_t y_group, tome_stream_t stream) {
    // addend == NULL: LayerNorm only (y_out = LN(x)); x_out is then neither read nor written and may be NULL
    if (!x || !ln_weight || !ln_bias || (addend && !x_out) || !y_out || rows <= 0 || C <= 0)
        return fail(TOME_EINVAL, "tome_add_layernorm: bad shape/pointer");
    if (int rc = not_16bit("tome_add_layernorm", dtype)) return rc;
    if (C % 8 || C / 8 > 2 * WAVE || !aligned16(x) || !aligned16(addend) || (addend && !aligned16(x_out)) ||
        !aligned16(y_out) || !aligned16(ln_weight) || !aligned16(ln_bias))
        return fail(TOME_EINVAL, "tome_add_layernorm: C %% 8 == 0, C <= 1024 and 16-byte aligned buffers required");
    return dispatch_x<false>(dtype, [&](auto tx) {
        using TX = typename decltype(tx)::type;
        return launch_add_ln_rows<TX, TX, TX, TX>("tome_add_layernorm", x, addend, rows, C, ln_weight, ln_bias, eps,
                                                  y_group, x_out, y_out, stream);
    }, [&] { return not_16bit("tome_add_layernorm", dtype); });
}

extern "C" int tome_add_layernorm(const void *x, const void *addend, int dtype, int64_t rows, int64_t C,
                                  const void *ln_weight, const void *ln_bias, float eps, void *x_out, void *y_out,
                                  tome_stream_t stream) {
    return add_layernorm_impl(x, addend, dtype, rows, C, ln_weight, ln_bias, eps, x_out, y_out, 0, stream);
}

extern "C" int tome_add_layernorm_skip_first(const void *x, const void *addend, int dtype, int64_t groups,
                                             int64_t group_rows, int64_t C, const void *ln_weight,
                                             const void *ln_bias, float eps, void *x_out, void *y_out,
                                             tome_stream_t stream) {
    if (groups <= 0 || group_rows < 2 || group_rows > 0x7fffffffLL)
        return fail(TOME_EINVAL, "tome_add_layernorm_skip_first: groups of at least two rows required");
    return add_layernorm_impl(x, addend, dtype, groups * group_rows, C, ln_weight, ln_bias, eps, x_out, y_out, group_rows,
                              stream);
}

extern "C" int tome_add_layernorm_regrouped(const void *x, const void *addend, int dtype, int64_t B, int64_t F, int64_t P,
                                            int64_t C, const void *ln_weight, const void *ln_bias, float eps,
                                            void *x_out, void *y_out, tome_stream_t stream) {
    if (!x || !addend || !x_out || !y_out || !ln_weight || !ln_bias || B <= 0 || F <= 0 || P <= 0 || C <= 0)
        return fail(TOME_EINVAL, "tome_add_layernorm_regrouped: bad shape/pointer");
    if (int rc = not_16bit("tome_add_layernorm_regrouped", dtype)) return rc;
    const int64_t cpr = C / 8;
    if (C % 8 || cpr > 2 * WAVE || !aligned16(x) || !aligned16(addend) || !aligned16(x_out) || !aligned16(y_out) ||
        !aligned16(ln_weight) || !aligned16(ln_bias))
        return fail(TOME_EINVAL, "tome_add_layernorm_regrouped: C %% 8 == 0, C <= 1024 and 16-byte aligned buffers required");
    const int64_t rows = B * (1 + P * F);
    if (rows > 0x7fffffffLL) return fail(TOME_EINVAL, "tome_add_layernorm_regrouped: too many rows");
    const int R = ln_rows_per_wave(cpr, 3);
    if (R < 1) return fail(TOME_EINVAL, "tome_add_layernorm_regrouped: row too wide");
    const int64_t waves = (rows + R - 1) / R;
    const LnArgs ln{ln_weight, ln_bias, y_out, eps, nullptr, 0, TokLayout{0, 0, 0, 0, 1}, nullptr, nullptr};
    const dim3 grid((unsigned)((waves + 3) / 4));
    hipStream_t st = (hipStream_t)stream;
    return dispatch_x<false>(dtype, [&](auto tx) {
        using TX = typename decltype(tx)::type;
        hipLaunchKernelGGL((k_add_ln_regroup<TX, 3>), grid, dim3(256), 0, st, (const TX *)x, (const TX *)addend, (int)B,
                           (int)F, (int)P, (int)C, R, (int)cpr, ln, (TX *)x_out);
        return check_launch("k_add_ln_regroup");
    }, [&] { return not_16bit("tome_add_layernorm_regrouped", dtype); });
}

// The launch form of k_ln_rows_bwd for `rows` rows of C channels: R rows per wave as add_layernorm_impl picks them,
// and -- when the parameter gradients are wanted -- how many slabs every wave of a workgroup walks (spw) and how many
// workgroups (= partial rows of the workspace) that makes.  At most LN_BWD_MAX_PARTS workgroups: two per CU at
// the kernel's register count (206-209 VGPRs with the 48 column sums), so every workgroup is resident from the start
// and all of them end together.
#define LN_BWD_MAX_PARTS 512
struct LnBwdForm { int R; int64_t wgs; int64_t spw; int64_t parts; };
static LnBwdForm ln_bwd_form(int64_t rows, int64_t C) {
    const int R = ln_rows_per_wave(C / 8, 3);
    const int64_t waves = (rows + R - 1) / R;
    const int64_t wgs = (waves + 3) / 4;
    const int64_t spw = (wgs + LN_BWD_MAX_PARTS - 1) / LN_BWD_MAX_PARTS;
    return LnBwdForm{R, wgs, spw, (wgs + spw - 1) / spw};
}

// k_ln_param_grad over the `parts` fp32 partial rows [width] of a workspace: columns below `split` to lo, the others to hi
template <typename TX>
static int launch_param_grad(const void *ws, int64_t parts, int64_t width, int64_t split, void *lo, void *hi,
                             hipStream_t st) {
    hipLaunchKernelGGL((k_ln_param_grad<TX>), dim3((unsigned)((width + WAVE - 1) / WAVE)), dim3(LN_PG_RUNS * WAVE), 0, st,
                       (const float *)ws, (int)parts, (int)width, (int)split, (TX *)lo, (TX *)hi);
    return check_launch("k_ln_param_grad");
}

static bool ln_bwd_shape_ok(int64_t rows, int64_t C) {
    return rows > 0 && rows <= 0x7fffffffLL && C > 0 && C % 8 == 0 && C / 8 <= 2 * WAVE;
}

extern "C" size_t tome_layernorm_backward_workspace_bytes(int64_t rows, int64_t C) {
    if (!ln_bwd_shape_ok(rows, C)) return 0;
    return align_up((size_t)ln_bwd_form(rows, C).parts * 2 * (size_t)C * sizeof(float), 256);
}

// What the two backward entries share once their shapes are validated: `rows` token rows, `gy_rows` rows of gy, and the
// row map between them -- group_rows (skip_first, else 0) or REGROUP with F and P.
template <int REGROUP>
static int layernorm_backward_impl(Op<REGROUP>, const char *who, const void *gy, const void *xs, const void *gx_in,
                                   int dtype, int64_t rows, int64_t gy_rows, int64_t group_rows, int64_t F, int64_t P,
                                   int64_t C, const void *weight, float eps, void *gx, void *dweight, void *dbias,
                                   void *workspace, tome_stream_t stream) {
    if (!aligned16(gy) || !aligned16(xs) || !aligned16(gx_in) || !aligned16(weight) || !aligned16(gx) ||
        !aligned16(workspace))
        return fail(TOME_EINVAL, "%s: 16-byte aligned buffers required", who);
    const bool params = dweight || dbias;
    if (params && !workspace)
        return fail(TOME_EWORKSPACE, "%s: parameter gradients need a workspace of %s_workspace_bytes()", who, who);
    const int64_t cpr = C / 8;
    const LnBwdForm f = ln_bwd_form(rows, C);
    hipStream_t st = (hipStream_t)stream;
    return dispatch_x<false>(dtype, [&](auto tx) {
        using TX = typename decltype(tx)::type;
        if (params) {
            hipLaunchKernelGGL((k_ln_rows_bwd<TX, 3, true, REGROUP != 0>), dim3((unsigned)f.parts), dim3(256), 0, st,
                               (const TX *)gy, (const TX *)xs, (const TX *)gx_in, (const TX *)weight, (int)rows,
                               (int)gy_rows, (int)C, f.R, (int)cpr, eps, (int)group_rows, (int)f.spw, (TX *)gx,
                               (float *)workspace, (int)F, (int)P);
            if (int rc = check_launch("k_ln_rows_bwd")) return rc;
            return launch_param_grad<TX>(workspace, f.parts, 2 * C, C, dweight, dbias, st);
        }
        // frozen LayerNorm: one slab per wave, no column sums, no workspace
        hipLaunchKernelGGL((k_ln_rows_bwd<TX, 3, false, REGROUP != 0>), dim3((unsigned)f.wgs), dim3(256), 0, st,
                           (const TX *)gy, (const TX *)xs, (const TX *)gx_in, (const TX *)weight, (int)rows, (int)gy_rows,
                           (int)C, f.R, (int)cpr, eps, (int)group_rows, 1, (TX *)gx, (float *)nullptr, (int)F, (int)P);
        return check_launch("k_ln_rows_bwd");
    }, [&] { return not_16bit(who, dtype); });
}

extern "C" int tome_layernorm_backward(const void *gy, const void *xs, const void *gx_in, int dtype, int64_t groups,
                                       int64_t group_rows, int skip_first, int64_t C, const void *weight, float eps,
                                       void *gx, void *dweight, void *dbias, void *workspace, tome_stream_t stream) {
    if (!gy || !xs || !weight || !gx) return fail(TOME_EINVAL, "tome_layernorm_backward: null buffer");
    if (int rc = not_16bit("tome_layernorm_backward", dtype)) return rc;
    if (groups <= 0 || group_rows <= 0 || group_rows > 0x7fffffffLL || groups > 0x7fffffffLL ||
        !ln_bwd_shape_ok(groups * group_rows, C))
        return fail(TOME_EINVAL, "tome_layernorm_backward: C %% 8 == 0, C <= 1024 and 1 .. 2^31 - 1 rows required");
    if (skip_first && group_rows < 2)
        return fail(TOME_EINVAL, "tome_layernorm_backward: skip_first needs groups of at least two rows");
    const int64_t rows = groups * group_rows;
    return layernorm_backward_impl(Op<0>{}, "tome_layernorm_backward", gy, xs, gx_in, dtype, rows,
                                   skip_first ? groups * (group_rows - 1) : rows, skip_first ? group_rows : 0, 0, 0, C,
                                   weight, eps, gx, dweight, dbias, workspace, stream);
}

// tome_layernorm_backward_regrouped: the same kernel and launch form over the B (1 + P F) token rows, with the row map of
// tome_add_layernorm_regrouped in front of gy (k_ln_rows_bwd<.., REGROUP>).
static bool ln_bwd_regrouped_shape_ok(int64_t B, int64_t F, int64_t P, int64_t C) {
    if (B <= 0 || F <= 0 || P <= 0 || B > 0x7fffffffLL || F > 0x7fffffffLL || P > 0x7fffffffLL) return false;
    if (P * F >= 0x7fffffffLL) return false;
    const int64_t rows = B * (1 + P * F), gy_rows = B * F * (1 + P);
    return gy_rows <= 0x7fffffffLL && ln_bwd_shape_ok(rows, C);
}

extern "C" size_t tome_layernorm_backward_regrouped_workspace_bytes(int64_t B, int64_t F, int64_t P, int64_t C) {
    if (!ln_bwd_regrouped_shape_ok(B, F, P, C)) return 0;
    return tome_layernorm_backward_workspace_bytes(B * (1 + P * F), C);
}

extern "C" int tome_layernorm_backward_regrouped(const void *gy, const void *xs, const void *gx_in, int dtype, int64_t B,
                                                 int64_t F, int64_t P, int64_t C, const void *weight, float eps,
                                                 void *gx, void *dweight, void *dbias, void *workspace,
                                                 tome_stream_t stream) {
    if (!gy || !xs || !weight || !gx) return fail(TOME_EINVAL, "tome_layernorm_backward_regrouped: null buffer");
    if (int rc = not_16bit("tome_layernorm_backward_regrouped", dtype)) return rc;
    if (!ln_bwd_regrouped_shape_ok(B, F, P, C))
        return fail(TOME_EINVAL, "tome_layernorm_backward_regrouped: C %% 8 == 0, C <= 1024, B, F, P >= 1 and at most "
                                 "2^31 - 1 rows on either side required");
    return layernorm_backward_impl(Op<1>{}, "tome_layernorm_backward_regrouped", gy, xs, gx_in, dtype, B * (1 + P * F),
                                   B * F * (1 + P), 0, F, P, C, weight, eps, gx, dweight, dbias, workspace, stream);
}

// ------------------------------------------------------------------------------------------------
// The mixed-precision forms (a model under autocast with fp32 master weights): k_add_ln_rows with fp32 parameters and
// k_ln_rows_bwd_amp in the launch forms of the entries above (three slots per lane, ln_rows_per_wave, ln_bwd_form).
// ------------------------------------------------------------------------------------------------
// f(Dt<TS>{}, Dt<TA>{}, Dt<TY>{}) for the legal (stream, addend, y) dtypes: a 16-bit stream with everything of its
// dtype, or an fp32 stream with a 16-bit y and an addend of y's dtype or fp32.  has_addend = false: TA = TY.
template <typename F, typename Bad>
static int dispatch_amp(int x_dtype, int a_dtype, bool has_addend, int y_dtype, F &&f, Bad &&bad) {
    return dispatch_x<false>(y_dtype, [&](auto ty) {
        if (x_dtype == y_dtype) return (!has_addend || a_dtype == y_dtype) ? f(ty, ty, ty) : bad();
        if (x_dtype != TOME_F32) return bad();
        if (!has_addend || a_dtype == y_dtype) return f(Dt<float>{}, ty, ty);
        if (a_dtype == TOME_F32) return f(Dt<float>{}, Dt<float>{}, ty);
        return bad();
    }, bad);
}

extern "C" int tome_add_layernorm_amp(const void *x, int x_dtype, const void *addend, int addend_dtype, int64_t groups,
                                      int64_t group_rows, int skip_first, int64_t C, const void *weight_f32,
                                      const void *bias_f32, float eps, void *x_out, void *y_out, int y_dtype,
                                      tome_stream_t stream) {
    const char *who = "tome_add_layernorm_amp";
    if (!x || !weight_f32 || !bias_f32 || (addend && !x_out) || !y_out || groups <= 0 || group_rows <= 0 || C <= 0 ||
        groups > 0x7fffffffLL || group_rows > 0x7fffffffLL)
        return fail(TOME_EINVAL, "%s: bad shape/pointer", who);
    if (skip_first && group_rows < 2) return fail(TOME_EINVAL, "%s: skip_first needs groups of at least two rows", who);
    const int64_t cpr = C / 8, rows = groups * group_rows;
    if (C % 8 || cpr > 2 * WAVE || !aligned16(x) || !aligned16(addend) || (addend && !aligned16(x_out)) ||
        !aligned16(y_out) || !aligned16(weight_f32) || !aligned16(bias_f32))
        return fail(TOME_EINVAL, "%s: C %% 8 == 0, C <= 1024 and 16-byte aligned buffers required", who);
    return dispatch_amp(x_dtype, addend_dtype, addend != nullptr, y_dtype, [&](auto ts, auto ta, auto ty) {
        return launch_add_ln_rows<typename decltype(ts)::type, typename decltype(ta)::type, typename decltype(ty)::type,
                                  float>(who, x, addend, rows, C, weight_f32, bias_f32, eps,
                                         skip_first ? group_rows : 0, x_out, y_out, stream);
    }, [&] {
        return fail(TOME_EINVAL, "%s: unsupported dtypes x=%d addend=%d y=%d (a 16-bit y; x of y's dtype with an addend "
                                 "of the same, or fp32 x with an addend of y's dtype or fp32)", who, x_dtype,
                    addend_dtype, y_dtype);
    });
}

static bool ln_amp_dtypes_ok(int gy_dtype, int x_dtype) {
    return (gy_dtype == TOME_BF16 || gy_dtype == TOME_F16) && (x_dtype == gy_dtype || x_dtype == TOME_F32);
}

extern "C" size_t tome_layernorm_backward_amp_workspace_bytes(int64_t rows, int64_t C, int x_dtype) {
    if (x_dtype != TOME_F32 && x_dtype != TOME_BF16 && x_dtype != TOME_F16) return 0;
    return tome_layernorm_backward_workspace_bytes(rows, C);  // the same launch form for every stream dtype
}

extern "C" int tome_layernorm_backward_amp(const void *gy, int gy_dtype, const void *xs, const void *gx_in, int x_dtype,
                                           int64_t groups, int64_t group_rows, int skip_first, int64_t C,
                                           const void *weight_f32, float eps, void *gx, void *gx16, void *dweight_f32,
                                           void *dbias_f32, void *workspace, tome_stream_t stream) {
    const char *who = "tome_layernorm_backward_amp";
    if (!gy || !xs || !weight_f32 || !gx) return fail(TOME_EINVAL, "%s: null buffer", who);
    if (!ln_amp_dtypes_ok(gy_dtype, x_dtype))
        return fail(TOME_EINVAL, "%s: unsupported dtypes gy=%d x=%d (16-bit gy; x of gy's dtype or fp32)", who, gy_dtype,
                    x_dtype);
    if (gx16 && x_dtype != TOME_F32) return fail(TOME_EINVAL, "%s: gx16 belongs to an fp32 stream", who);
    if (groups <= 0 || group_rows <= 0 || group_rows > 0x7fffffffLL || groups > 0x7fffffffLL ||
        !ln_bwd_shape_ok(groups * group_rows, C))
        return fail(TOME_EINVAL, "%s: C %% 8 == 0, C <= 1024 and 1 .. 2^31 - 1 rows required", who);
    if (skip_first && group_rows < 2) return fail(TOME_EINVAL, "%s: skip_first needs groups of at least two rows", who);
    if (!aligned16(gy) || !aligned16(xs) || !aligned16(gx_in) || !aligned16(weight_f32) || !aligned16(gx) ||
        !aligned16(gx16) || !aligned16(workspace))
        return fail(TOME_EINVAL, "%s: 16-byte aligned buffers required", who);
    const bool params = dweight_f32 || dbias_f32;
    if (params && !workspace)
        return fail(TOME_EWORKSPACE, "%s: parameter gradients need a workspace of %s_workspace_bytes()", who, who);
    const int64_t rows = groups * group_rows, gy_rows = skip_first ? groups * (group_rows - 1) : rows;
    const int64_t cpr = C / 8;
    const LnBwdForm f = ln_bwd_form(rows, C);
    hipStream_t st = (hipStream_t)stream;
    return dispatch_x<false>(gy_dtype, [&](auto tg) {
        using TG = typename decltype(tg)::type;
        auto go = [&](auto ts) {
            using TS = typename decltype(ts)::type;
            if (params) {
                hipLaunchKernelGGL((k_ln_rows_bwd_amp<TS, TG, 3, true>), dim3((unsigned)f.parts), dim3(256), 0, st,
                                   (const TG *)gy, (const TS *)xs, (const TS *)gx_in, (const float *)weight_f32, (int)rows,
                                   (int)gy_rows, (int)C, f.R, (int)cpr, eps, skip_first ? (int)group_rows : 0, (int)f.spw,
                                   (TS *)gx, (TG *)gx16, (float *)workspace);
                if (int rc = check_launch("k_ln_rows_bwd_amp")) return rc;
                return launch_param_grad<float>(workspace, f.parts, 2 * C, C, dweight_f32, dbias_f32, st);
            }
            // frozen LayerNorm: one slab per wave, no column sums, no workspace
            hipLaunchKernelGGL((k_ln_rows_bwd_amp<TS, TG, 3, false>), dim3((unsigned)f.wgs), dim3(256), 0, st,
                               (const TG *)gy, (const TS *)xs, (const TS *)gx_in, (const float *)weight_f32, (int)rows,
                               (int)gy_rows, (int)C, f.R, (int)cpr, eps, skip_first ? (int)group_rows : 0, 1, (TS *)gx,
                               (TG *)gx16, (float *)nullptr);
            return check_launch("k_ln_rows_bwd_amp");
        };
        return x_dtype == TOME_F32 ? go(Dt<float>{}) : go(tg);
    }, [&] { return not_16bit(who, gy_dtype, "gy"); });
}

extern "C" int tome_merge(const void *x, int dtype, int64_t n, int64_t T, int64_t C, int64_t r,
                          const int64_t *src_idx, const int64_t *dst_idx, const int64_t *unm_idx, int distill_token,
                          int mode, const uint8_t *edge_keep, void *out, tome_stream_t stream) {
    if (int rc = check_merge_args("tome_merge", x, n, T, C, r, out)) return rc;
    if (!src_idx || !dst_idx || (!unm_idx && (T + 1) / 2 > r))
        return fail(TOME_EINVAL, "tome_merge: null index buffer");
    if (mode < TOME_SUM || mode > TOME_AMIN) return fail(TOME_EINVAL, "tome_merge: mode %d", mode);
    return dispatch_x<true>(dtype, [&](auto tx) {
        auto go = [&](auto op) {
            return launch_merge_rows<typename decltype(tx)::type, float, decltype(op)::value>(
                x, nullptr, n, T, C, r, src_idx, dst_idx, unm_idx, distill_token, edge_keep, out, nullptr,
                (hipStream_t)stream);
        };
        switch (mode) {
        case TOME_SUM: return go(Op<TOME_SUM>{});
        case TOME_MEAN: return go(Op<TOME_MEAN>{});
        case TOME_AMAX: return go(Op<TOME_AMAX>{});
        case TOME_PROD: return go(Op<TOME_PROD>{});
        default: return go(Op<TOME_AMIN>{});  // (mode range checked above)
        }
    }, [&] { return fail(TOME_EINVAL, "tome_merge: dtype %d", dtype); });
}

extern "C" int tome_drop(const void *x, int dtype, int64_t n, int64_t T, int64_t C, int64_t r,
                         const int64_t *und_idx, int distill_token, void *out, tome_stream_t stream) {
    if (int rc = check_merge_args("tome_drop", x, n, T, C, r, out)) return rc;
    if (!und_idx && (T + 1) / 2 > r) return fail(TOME_EINVAL, "tome_drop: null index buffer");
    return dispatch_x<true>(dtype, [&](auto tx) {
        return launch_merge_rows<typename decltype(tx)::type, float, OP_DROP>(
            x, nullptr, n, T, C, r, nullptr, nullptr, und_idx, distill_token, nullptr, out, nullptr, (hipStream_t)stream);
    }, [&] { return fail(TOME_EINVAL, "tome_drop: dtype %d", dtype); });
}

// tome_drop on the interleaved layout of TimeSformer / Motionformer (class token kept aside and copied through)
extern "C" int tome_drop_regrouped(const void *x, int dtype, int64_t B, int64_t F, int64_t P, int64_t C, int64_t r,
                                   int has_cls, const int64_t *und_idx, void *x_out, tome_stream_t stream) {
    if (B <= 0 || F <= 0) return fail(TOME_EINVAL, "tome_drop_regrouped: bad shape");
    const int64_t n = B * F;
    if (int rc = check_merge_args("tome_drop_regrouped", x, n, P, C, r, x_out)) return rc;
    if (!und_idx && (P + 1) / 2 > r) return fail(TOME_EINVAL, "tome_drop_regrouped: null index buffer");
    const int cls = has_cls ? 1 : 0;
    const TokLayout lin{cls * C, (cls + P * F) * C, C, F * C, (int)F};
    const TokLayout lout{cls * C, (cls + (P - r) * F) * C, C, F * C, (int)F};
    return dispatch_x<true>(dtype, [&](auto tx) {
        return launch_merge_rows<typename decltype(tx)::type, float, OP_DROP>(
            x, nullptr, n, P, C, r, nullptr, nullptr, und_idx, 0, nullptr, x_out, nullptr, (hipStream_t)stream, &lin,
            &lout, cls ? (int)B : 0);
    }, [&] { return fail(TOME_EINVAL, "tome_drop_regrouped: dtype %d", dtype); });
}

// What tome_drop_ln and tome_drop_regrouped_ln ask beyond check_merge_args, one text per fault, before any launch:
// 16-bit tokens of C % 8 == 0, C <= 1024 channels, every buffer the kernel moves in 16-byte chunks aligned.
static int check_drop_ln_args(const char *who, const void *x, int dtype, int64_t C, const void *ln_weight,
                              const void *ln_bias, const void *addend, const void *cls_addend, const void *x_out,
                              const void *y_out, const void *x_out_bias) {
    if (!y_out || !ln_weight || !ln_bias) return fail(TOME_EINVAL, "%s: null buffer", who);
    if (dtype != TOME_BF16 && dtype != TOME_F16) return fail(TOME_EINVAL, "%s: 16-bit tokens only (dtype=%d)", who, dtype);
    if (C % 8 != 0 || C > 1024)
        return fail(TOME_EINVAL, "%s: C=%lld must be a multiple of 8, at most 1024", who, (long long)C);
    if (!aligned16(x) || !aligned16(x_out)) return fail(TOME_EINVAL, "%s: x / x_out not 16-byte aligned", who);
    if (!aligned16(y_out)) return fail(TOME_EINVAL, "%s: y_out not 16-byte aligned", who);
    if (!aligned16(ln_weight) || !aligned16(ln_bias))
        return fail(TOME_EINVAL, "%s: ln_weight / ln_bias not 16-byte aligned", who);
    if ((addend && !aligned16(addend)) || (cls_addend && !aligned16(cls_addend)))
        return fail(TOME_EINVAL, "%s: addend not 16-byte aligned", who);
    if (x_out_bias && !aligned16(x_out_bias)) return fail(TOME_EINVAL, "%s: x_out_bias not 16-byte aligned", who);
    return TOME_OK;
}

// tome_drop with the residual add in front and the block's second LayerNorm behind it: the streaming waves of
// k_merge_rows_fast<.., OP_DROP, .., LN> (every kept row is one; there are no edge waves)
extern "C" int tome_drop_ln(const void *x, int dtype, int64_t n, int64_t T, int64_t C, int64_t r, const int64_t *und_idx,
                            int distill_token, const void *ln_weight, const void *ln_bias, float eps,
                            const void *addend, void *x_out, void *y_out, const void *x_out_bias,
                            tome_stream_t stream) {
    if (int rc = check_merge_args("tome_drop_ln", x, n, T, C, r, x_out)) return rc;
    if (!und_idx && (T + 1) / 2 > r) return fail(TOME_EINVAL, "tome_drop_ln: null index buffer");
    if (int rc = check_drop_ln_args("tome_drop_ln", x, dtype, C, ln_weight, ln_bias, addend, nullptr, x_out, y_out,
                                    x_out_bias))
        return rc;
    const LnArgs ln{ln_weight, ln_bias, y_out, eps, addend, 0, TokLayout{0, 0, 0, 0, 1}, nullptr, x_out_bias};
    return dispatch_x<false>(dtype, [&](auto tx) {
        return launch_merge_rows<typename decltype(tx)::type, float, OP_DROP>(
            x, nullptr, n, T, C, r, nullptr, nullptr, und_idx, distill_token, nullptr, x_out, nullptr,
            (hipStream_t)stream, nullptr, nullptr, 0, &ln);
    }, [&] { return fail(TOME_EINVAL, "tome_drop_ln: 16-bit tokens only (dtype=%d)", dtype); });
}

// tome_drop_ln on the interleaved layout: the class rows take the same add + LayerNorm (the gy >= n block)
extern "C" int tome_drop_regrouped_ln(const void *x, int dtype, int64_t B, int64_t F, int64_t P, int64_t C, int64_t r,
                                      int has_cls, const int64_t *und_idx, const void *ln_weight, const void *ln_bias,
                                      float eps, const void *addend, int addend_grouped, const void *cls_addend,
                                      void *x_out, void *y_out, const void *x_out_bias, tome_stream_t stream) {
    if (B <= 0 || F <= 0) return fail(TOME_EINVAL, "tome_drop_regrouped_ln: bad shape");
    const int64_t n = B * F;
    if (int rc = check_merge_args("tome_drop_regrouped_ln", x, n, P, C, r, x_out)) return rc;
    if (!und_idx && (P + 1) / 2 > r) return fail(TOME_EINVAL, "tome_drop_regrouped_ln: null index buffer");
    if (int rc = check_drop_ln_args("tome_drop_regrouped_ln", x, dtype, C, ln_weight, ln_bias, addend, cls_addend, x_out,
                                    y_out, x_out_bias))
        return rc;
    if (addend_grouped && !addend) return fail(TOME_EINVAL, "tome_drop_regrouped_ln: addend_grouped without addend");
    const int64_t cls = has_cls ? 1 : 0;
    LnArgs ln{ln_weight, ln_bias, y_out, eps, addend, 0, TokLayout{0, 0, 0, 0, 1}, nullptr, x_out_bias};
    if (addend_grouped) {  // addend [B*F, has_cls + P, C], as in tome_merge_wavg_regrouped_ln
        ln.a_own = 1;
        ln.la = TokLayout{cls * C, (cls + P) * C, 0, C, 1};
        ln.cls_addend = cls_addend;
    }
    const TokLayout lin{cls * C, (cls + P * F) * C, C, F * C, (int)F};
    const TokLayout lout{cls * C, (cls + (P - r) * F) * C, C, F * C, (int)F};
    return dispatch_x<false>(dtype, [&](auto tx) {
        return launch_merge_rows<typename decltype(tx)::type, float, OP_DROP>(
            x, nullptr, n, P, C, r, nullptr, nullptr, und_idx, 0, nullptr, x_out, nullptr, (hipStream_t)stream, &lin,
            &lout, cls ? (int)B : 0, &ln);
    }, [&] { return fail(TOME_EINVAL, "tome_drop_regrouped_ln: 16-bit tokens only (dtype=%d)", dtype); });
}

// ------------------------------------------------------------------------------------------------
// tome_merge_wavg_ln_amp / tome_drop_ln_amp: the add + reduction + LayerNorm launch under autocast (k_merge_rows_ln_amp,
// csrc/tome_merge_ln_amp.h) in the dtypes of tome_add_layernorm_amp (dispatch_amp) and its launch form (three slots per
// lane, ln_rows_per_wave); the grid is launch_merge_rows' (blocks of one group, group in y and z).  Every refusal is
// made here, before the launch, each with a text of its own.
// ------------------------------------------------------------------------------------------------
template <int OP>
static int merge_ln_amp_impl(const char *who, const void *x, int x_dtype, const void *addend, int addend_dtype,
                             const void *size, int size_dtype, int64_t n, int64_t T, int64_t C, int64_t r,
                             const int64_t *src_idx, const int64_t *dst_idx, const int64_t *unm_idx, int distill_token,
                             const uint8_t *edge_keep, const void *weight_f32, const void *bias_f32, float eps,
                             void *x_out, void *y_out, int y_dtype, void *size_out, void *log_size_out,
                             tome_stream_t stream) {
    if (int rc = check_merge_args(who, x, n, T, C, r, x_out)) return rc;
    if (!y_out || !weight_f32 || !bias_f32 || (!unm_idx && (T + 1) / 2 > r) ||
        (OP == OP_WAVG && (!src_idx || !dst_idx || !size_out)))
        return fail(TOME_EINVAL, "%s: null buffer", who);
    auto bad_dtypes = [&] {
        return fail(TOME_EINVAL, "%s: unsupported dtypes x=%d addend=%d y=%d (a 16-bit y; x of y's dtype with an addend of "
                                 "the same, or fp32 x with an addend of y's dtype or fp32)", who, x_dtype, addend_dtype,
                    y_dtype);
    };
    if (int rc = dispatch_amp(x_dtype, addend_dtype, addend != nullptr, y_dtype,
                              [](auto, auto, auto) -> int { return TOME_OK; }, bad_dtypes))
        return rc;
    if (OP == OP_WAVG && size_dtype != TOME_F32 && size_dtype != x_dtype)
        return fail(TOME_EINVAL, "%s: sizes must be of x's dtype or fp32 (x=%d size=%d)", who, x_dtype, size_dtype);
    if (C % 8 != 0 || C > 1024)
        return fail(TOME_EINVAL, "%s: C=%lld must be a multiple of 8, at most 1024", who, (long long)C);
    if (!aligned16(x) || !aligned16(x_out)) return fail(TOME_EINVAL, "%s: x / x_out not 16-byte aligned", who);
    if (!aligned16(addend)) return fail(TOME_EINVAL, "%s: addend not 16-byte aligned", who);
    if (!aligned16(y_out)) return fail(TOME_EINVAL, "%s: y_out not 16-byte aligned", who);
    if (!aligned16(weight_f32) || !aligned16(bias_f32))
        return fail(TOME_EINVAL, "%s: weight_f32 / bias_f32 not 16-byte aligned", who);
    const int64_t To = T - r, cpr = C / 8;
    const int R = ln_rows_per_wave(cpr, 3);
    const int64_t rg = (To + R - 1) / R;
    const int64_t bpg = (rg + (OP == OP_DROP ? 0 : r) + 3) / 4;
    const int64_t gy = n < 65535 ? n : 65535, gz = (n + gy - 1) / gy;
    if (gz > 65535) return fail(TOME_EINVAL, "%s: too many groups (%lld)", who, (long long)n);
    const dim3 grid((unsigned)bpg, (unsigned)gy, (unsigned)gz);
    hipStream_t st = (hipStream_t)stream;
    return dispatch_amp(x_dtype, addend_dtype, addend != nullptr, y_dtype, [&](auto tx, auto ta, auto ty) {
        using TX = typename decltype(tx)::type;
        using TA = typename decltype(ta)::type;
        using TY = typename decltype(ty)::type;
        auto launch = [&](auto ts) {
            using TS = typename decltype(ts)::type;
            hipLaunchKernelGGL((k_merge_rows_ln_amp<TX, TA, TY, TS, OP, 3>), grid, dim3(256), 0, st, (const TX *)x,
                               (const TA *)addend, (const TS *)size, (int)n, (int)T, (int)C, (int)r, R, (int)cpr, (int)rg,
                               src_idx, dst_idx, unm_idx, distill_token, edge_keep, (const float *)weight_f32,
                               (const float *)bias_f32, eps, (TX *)x_out, (TY *)y_out, (TS *)size_out,
                               (TS *)log_size_out);
            return check_launch("k_merge_rows_ln_amp");
        };
        if constexpr (OP == OP_DROP) {
            return launch(Dt<float>{});  // (no sizes: one instantiation per dtype triple)
        } else {
            if (size_dtype == TOME_F32) return launch(Dt<float>{});
            return launch(tx);
        }
    }, bad_dtypes);
}

extern "C" int tome_merge_wavg_ln_amp(const void *x, int x_dtype, const void *addend, int addend_dtype, const void *size,
                                      int size_dtype, int64_t n, int64_t T, int64_t C, int64_t r, const int64_t *src_idx,
                                      const int64_t *dst_idx, const int64_t *unm_idx, int distill_token,
                                      const uint8_t *edge_keep, const void *weight_f32, const void *bias_f32, float eps,
                                      void *x_out, void *y_out, int y_dtype, void *size_out, void *log_size_out,
                                      tome_stream_t stream) {
    return merge_ln_amp_impl<OP_WAVG>("tome_merge_wavg_ln_amp", x, x_dtype, addend, addend_dtype, size, size_dtype, n, T, C,
                                      r, src_idx, dst_idx, unm_idx, distill_token, edge_keep, weight_f32, bias_f32, eps,
                                      x_out, y_out, y_dtype, size_out, log_size_out, stream);
}

extern "C" int tome_drop_ln_amp(const void *x, int x_dtype, const void *addend, int addend_dtype, int64_t n, int64_t T,
                                int64_t C, int64_t r, const int64_t *und_idx, int distill_token, const void *weight_f32,
                                const void *bias_f32, float eps, void *x_out, void *y_out, int y_dtype,
                                tome_stream_t stream) {
    return merge_ln_amp_impl<OP_DROP>("tome_drop_ln_amp", x, x_dtype, addend, addend_dtype, nullptr, TOME_F32, n, T, C, r,
                                      nullptr, nullptr, und_idx, distill_token, nullptr, weight_f32, bias_f32, eps, x_out,
                                      y_out, y_dtype, nullptr, nullptr, stream);
}

// The dtype x bias dispatch of the attention kernels, forward and backward: f(Dt<TX>{}, Op<BIAS>{}) for a 16-bit
// dtype, BIAS = 1 with a per-key bias; otherwise bad()
template <typename F, typename Bad>
static int dispatch_attn(int dtype, bool bias, F &&f, Bad &&bad) {
    return dispatch_x<false>(dtype, [&](auto tx) { return bias ? f(tx, Op<1>{}) : f(tx, Op<0>{}); }, bad);
}

// The launch form of one forward attention call.  (tests/attn_oracle.expected_form mirrors this rule.)  The three
// TOME_ATTN_* variables are measurement switches, read per call and not cached: the tests force each form on small
// inputs.
enum AttnKernel { ATTN_RESIDENT, ATTN_STREAM, ATTN_PLAIN };
// waves: per workgroup of the plain kernel, 4 or 8; pair: the persistent kernel's 128-register form, -1 = by launch size
struct AttnForm { AttnKernel kernel; int waves; int pair; };
static AttnForm attn_form(const AttnArgs &a, int64_t B, int64_t H, int64_t N, int64_t Nk, int64_t nseg) {
    const char *re = getenv("TOME_ATTN_RESIDENT"), *we = getenv("TOME_ATTN_WAVES"), *se = getenv("TOME_ATTN_STREAM");
    // Short key sequences (TimeSformer's 1 + p <= 197 tokens per frame, Motionformer's <= 196 keys per frame segment):
    // the whole K / V of a (batch, head, segment) resident in LDS, one workgroup per item, no per-tile barrier
    // (tome_attn_resident.h).  TOME_ATTN_RESIDENT=0 keeps the streaming kernels.
    // (the kernel addresses the tokens of one (batch, head) slice with 32-bit element offsets)
    const bool off32 = N * a.q_sn < (1ll << 31) && Nk * a.k_sn < (1ll << 31) && Nk * a.v_sn < (1ll << 31) &&
                       N * a.o_sn < (1ll << 31);
    if (Nk <= RES_ROWS && off32 && !(re && re[0] == '0')) return AttnForm{ATTN_RESIDENT, 0, 0};
    // queries per workgroup: 256 (eight waves share every staged K/V tile: staging costs 18 % with four) unless the
    // sequence is short.  (Measured: 5, 6 or 7 waves per workgroup, chosen to leave no part-empty last block, are
    // 10-30 % slower per block than eight -- uneven staging passes and SIMD load -- and lose more than they save.)
    const int waves_set = we ? atoi(we) : 0;
    const int waves_env = (waves_set == 4 || waves_set == 8) ? waves_set : 0;
    // (the pipelined plain kernel keeps two waves per SIMD either way: two 4-wave workgroups share a CU.  They lose
    // 3-5 % on long launches -- every tile is staged twice per CU -- and win 7-13 % when the launch is short: fewer
    // than four rounds of 8-wave workgroups over the 256 CUs)
    const int waves = waves_env ? waves_env : ((N > 128 && B * H * nseg * ((N + 255) / 256) >= 1024) ? 8 : 4);
    // Eight-wave launches with at least two key tiles run as persistent workgroups, one per CU, that keep the K/V
    // pipeline going across query blocks (tome_attn_stream.h); TOME_ATTN_STREAM=0 keeps one workgroup per block
    const int64_t sn_max = 1 << 22;  // (the stream kernel keeps token offsets inside a tile / query block in 32 bits)
    const bool sn_ok = a.q_sn < sn_max && a.k_sn < sn_max && a.v_sn < sn_max && a.o_sn < sn_max;
    // (Round 3: also for launches the rule above gives four waves, as long as a block has work for more than four --
    // 8 x 12 x 1568: 597 -> 650 TFLOP/s, with the per-key bias 476 -> 537; 64 x 12 x 197: 242 -> 280 / 199 -> 240;
    // level at 16 x 12 x 197 and below, where the launch is the cost; the 4-wave persistent form was built and
    // measured too: 17-20 % slower than this one at 197 .. 1568 tokens, not kept)
    const bool stream_ok = Nk > ATT_BN && sn_ok && !(se && se[0] == '0');
    // TOME_ATTN_STREAM=2 / =1: the persistent kernel as two 128-register workgroups per CU
    // (k_prop_attention_stream<.., true>) / as one workgroup per CU, whatever the launch size
    const int pair = (se && se[0] == '2') ? 1 : (se && se[0] == '1') ? 0 : -1;
    if (stream_ok && (waves == 8 || (!waves_env && N > 128))) return AttnForm{ATTN_STREAM, waves, pair};
    return AttnForm{ATTN_PLAIN, waves, 0};
}

static int prop_attention_impl(const void *q, const void *k, const void *v, int dtype, int64_t B, int64_t H,
                               int64_t N, int64_t Nk, int64_t D, const int64_t *q_strides,
                               const int64_t *k_strides, const int64_t *v_strides, const float *log_size,
                               int64_t log_size_stride, int bias_skip, float scale, void *out,
                               const int64_t *out_strides, int64_t nseg, const int64_t *seg_strides,
                               tome_stream_t stream) {
    if (!q || !k || !v || !out || !q_strides || !k_strides || !v_strides || B <= 0 || H <= 0 || N <= 0 || Nk <= 0)
        return fail(TOME_EINVAL, "tome_prop_attention: bad shape/pointer");
    if (D != ATT_D) return fail(TOME_EINVAL, "tome_prop_attention: head dim %lld (only 64)", (long long)D);
    auto bad_dtype = [] { return fail(TOME_EINVAL, "tome_prop_attention: 16-bit q/k/v only"); };
    if (dtype != TOME_BF16 && dtype != TOME_F16) return bad_dtype();
    if (bias_skip != 0 && bias_skip != 1) return fail(TOME_EINVAL, "tome_prop_attention: bias_skip %d", bias_skip);
    if (bias_skip && N != Nk) return fail(TOME_EINVAL, "tome_prop_attention: bias_skip needs as many keys as queries");
    if (B * H * nseg > 0x7fffffffLL / 64 || N > 0x7fffffffLL / 4 || Nk > 0x7fffffffLL / 4)
        return fail(TOME_EINVAL, "tome_prop_attention: too large");
    const int64_t *ss[3] = {q_strides, k_strides, v_strides};
    const void *pp[3] = {q, k, v};
    for (int i = 0; i < 3; ++i) {
        if (!aligned16(pp[i]) || ss[i][0] % 8 || ss[i][1] % 8 || ss[i][2] % 8 || ss[i][2] < D)
            return fail(TOME_EINVAL, "tome_prop_attention: q/k/v rows must be 16-byte aligned (strides %% 8 == 0)");
    }
    AttnArgs a;
    a.q = q; a.k = k; a.v = v; a.out = out;
    a.q_sb = q_strides[0]; a.q_sh = q_strides[1]; a.q_sn = q_strides[2];
    a.k_sb = k_strides[0]; a.k_sh = k_strides[1]; a.k_sn = k_strides[2];
    a.v_sb = v_strides[0]; a.v_sh = v_strides[1]; a.v_sn = v_strides[2];
    if (out_strides) {  // {batch, head, token} element strides of out[b, q, h, 0..63]; rows 16-byte aligned
        if (out_strides[0] % 8 || out_strides[1] % 8 || out_strides[2] % 8 || ((uintptr_t)out & 15))
            return fail(TOME_EINVAL, "tome_prop_attention: out rows must be 16-byte aligned");
        a.o_sb = out_strides[0]; a.o_sh = out_strides[1]; a.o_sn = out_strides[2];
    } else {
        if ((uintptr_t)out & 15) return fail(TOME_EINVAL, "tome_prop_attention: out must be 16-byte aligned");
        a.o_sb = N * H * D; a.o_sh = D; a.o_sn = H * D;
    }
    a.log_size = log_size; a.ls_sb = log_size_stride;
    a.B = (int)B; a.H = (int)H; a.N = (int)N; a.Nk = (int)Nk; a.scale = scale; a.bias_skip = bias_skip;
    a.nseg = (int)nseg;
    a.k_seg = a.v_seg = a.o_seg = a.ls_seg = 0;
    if (seg_strides) {  // {k, v, out, log_size} element offsets from one segment to the next
        if (seg_strides[0] % 8 || seg_strides[1] % 8 || seg_strides[2] % 8)
            return fail(TOME_EINVAL, "tome_prop_attention_segments: segment offsets must keep rows 16/8-byte aligned");
        a.k_seg = seg_strides[0]; a.v_seg = seg_strides[1]; a.o_seg = seg_strides[2]; a.ls_seg = seg_strides[3];
    }
    hipStream_t st = (hipStream_t)stream;
    const AttnForm form = attn_form(a, B, H, N, Nk, nseg);
    if (form.kernel == ATTN_RESIDENT) {
        const int64_t items = (B * H + 7) / 8 * 8 * nseg;
        if (items > 0x7fffffffLL) return fail(TOME_EINVAL, "tome_prop_attention: grid too large");
        return dispatch_attn(dtype, log_size != nullptr, [&](auto tx, auto bias) {
            hipLaunchKernelGGL((k_resident_attention<typename decltype(tx)::type, decltype(bias)::value != 0>),
                               dim3((unsigned)items), dim3(512), 0, st, a);
            return check_launch("k_resident_attention");
        }, bad_dtype);
    }
    const int64_t bh8 = (B * H * nseg + 7) / 8 * 8;
    const int64_t qblocks = (N + 32 * form.waves - 1) / (32 * form.waves);
    if (bh8 * qblocks > 0x7fffffffLL) return fail(TOME_EINVAL, "tome_prop_attention: grid too large");
    if (form.kernel == ATTN_STREAM) {
        static const int cus = [] {
            int dev = 0, n = 0;
            if (hipGetDevice(&dev) != hipSuccess ||
                hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
                n = 256;
            return n / 8 * 8;
        }();
        const int nitems = (int)(bh8 * ((N + 255) / 256));
        // Two workgroups per CU (four waves per SIMD from two unrelated barriers, one workgroup's softmax under the
        // other's MFMAs: tome_attn_stream.h, PAIR) take the launches that have items for more than one workgroup per
        // CU.  Measured at 384 x 12 x 1568 / 1392 alone: 3.64 / 2.98 ms against 3.80 / 3.20 with the bias, where the
        // reference point rides for nothing on the k-step the bias takes anyway, and 3.47 / 2.87 against 3.39 / 2.81
        // without, where it costs two MFMAs per tile of its own; inside the VideoMAE forward (no bias, the matching
        // on the side stream) every one of the twelve layers' launches is 0.4-4 % shorter in the pair form and the
        // benchmark 0.9-1.3 % faster (profiles/attention_pair_ab.txt).
        const bool pair = form.pair < 0 ? nitems > cus : form.pair != 0;
        // TOME_ATTN_GRID: the persistent kernels' workgroup count (a measurement switch like the three above; rounded
        // down to the multiple of 8 the item numbering needs) -- one workgroup per CU for the pair form, or a handful
        // of workgroups that each walk many items of a small input
        int wgs = pair ? 2 * cus : cus;
        if (const char *ge = getenv("TOME_ATTN_GRID")) {
            const int g = atoi(ge) / 8 * 8;
            if (g >= 8) wgs = g;
        }
        const dim3 pgrid((unsigned)(nitems < wgs ? nitems : wgs));
        return dispatch_attn(dtype, log_size != nullptr, [&](auto tx, auto bias) {
            using TX = typename decltype(tx)::type;
            constexpr bool BIAS = decltype(bias)::value != 0;
            if (pair) {
                hipLaunchKernelGGL((k_prop_attention_stream<TX, BIAS, true>), pgrid, dim3(512), 0, st, a, nitems);
                return check_launch("k_prop_attention_stream<.., true>");
            }
            hipLaunchKernelGGL((k_prop_attention_stream<TX, BIAS, false>), pgrid, dim3(512), 0, st, a, nitems);
            return check_launch("k_prop_attention_stream");
        }, bad_dtype);
    }
    const dim3 grid((unsigned)(bh8 * qblocks));
    return dispatch_attn(dtype, log_size != nullptr, [&](auto tx, auto bias) {
        using TX = typename decltype(tx)::type;
        constexpr bool BIAS = decltype(bias)::value != 0;
        if (form.waves == 8) hipLaunchKernelGGL((k_prop_attention<TX, 8, BIAS>), grid, dim3(512), 0, st, a);
        else hipLaunchKernelGGL((k_prop_attention<TX, 4, BIAS>), grid, dim3(256), 0, st, a);
        return check_launch("k_prop_attention");
    }, bad_dtype);
}

extern "C" int tome_prop_attention(const void *q, const void *k, const void *v, int dtype, int64_t B, int64_t H,
                                   int64_t N, int64_t Nk, int64_t D, const int64_t *q_strides,
                                   const int64_t *k_strides, const int64_t *v_strides, const float *log_size,
                                   int64_t log_size_stride, int bias_skip, float scale, void *out,
                                   const int64_t *out_strides, tome_stream_t stream) {
    return prop_attention_impl(q, k, v, dtype, B, H, N, Nk, D, q_strides, k_strides, v_strides, log_size,
                               log_size_stride, bias_skip, scale, out, out_strides, 1, nullptr, stream);
}

extern "C" int tome_prop_attention_segments(const void *q, const void *k, const void *v, int dtype, int64_t B,
                                            int64_t H, int64_t N, int64_t Nk, int64_t D, const int64_t *q_strides,
                                            const int64_t *k_strides, const int64_t *v_strides, const float *log_size,
                                            int64_t log_size_stride, float scale, void *out,
                                            const int64_t *out_strides, int64_t nseg, const int64_t *seg_strides,
                                            tome_stream_t stream) {
    if (nseg < 1 || !seg_strides || !out_strides)
        return fail(TOME_EINVAL, "tome_prop_attention_segments: nseg >= 1, segment and out strides required");
    return prop_attention_impl(q, k, v, dtype, B, H, N, Nk, D, q_strides, k_strides, v_strides, log_size,
                               log_size_stride, 0, scale, out, out_strides, nseg, seg_strides, stream);
}

#ifdef ATT_DIAG
// diagnostic build: the phase stamps of the last k_prop_attention launch (tools/attn_diag.py)
extern "C" int tome_attn_diag_read(unsigned long long *host, int64_t count) {
    if (count > (int64_t)ATT_DIAG_WGS * 8 * ATT_DIAG_N) count = (int64_t)ATT_DIAG_WGS * 8 * ATT_DIAG_N;
    if (hipMemcpyFromSymbol(host, HIP_SYMBOL(g_att_stamps), count * sizeof(unsigned long long)) != hipSuccess)
        return fail(TOME_ELAUNCH, "tome_attn_diag_read: copy failed");
    return TOME_OK;
}
#endif

extern "C" int tome_trajectory_mix(const void *q2, const void *k2, const void *val, int dtype, int64_t B, int64_t S,
                                   int64_t F, int64_t H, int64_t D, int64_t k_row_stride, int64_t v_row_stride,
                                   float scale, void *out, int64_t out_batch_stride, float *tattn,
                                   tome_stream_t stream) {
    if (!q2 || !k2 || !val || !out || B <= 0 || S <= 0 || F <= 0 || H <= 0)
        return fail(TOME_EINVAL, "tome_trajectory_mix: bad shape/pointer");
    if (D != 64 || H > 16 || F > TRAJ_MAXF)
        return fail(TOME_EINVAL, "tome_trajectory_mix: head dim 64, at most 16 heads and %d frames", TRAJ_MAXF);
    if (int rc = not_16bit("tome_trajectory_mix", dtype, "tensors")) return rc;
    if (k_row_stride % 8 || v_row_stride % 8 || k_row_stride < H * D || v_row_stride < H * D || !aligned16(q2) ||
        !aligned16(k2) || !aligned16(val) || !aligned16(out))
        return fail(TOME_EINVAL, "tome_trajectory_mix: rows must be 16-byte aligned");
    if (out_batch_stride == 0) out_batch_stride = S * H * D;
    if (out_batch_stride < S * H * D || out_batch_stride % 8)
        return fail(TOME_EINVAL, "tome_trajectory_mix: out_batch_stride must be 0 or a multiple of 8 >= S*H*D");
    const int64_t rows = B * S;
    if (rows > 0x7fffffffLL) return fail(TOME_EINVAL, "tome_trajectory_mix: too many tokens");
    const dim3 grid((unsigned)((rows + 3) / 4));
    hipStream_t st = (hipStream_t)stream;
    return dispatch_x<false>(dtype, [&](auto tx) {
        using TX = typename decltype(tx)::type;
        hipLaunchKernelGGL(k_trajectory_mix<TX>, grid, dim3(256), 0, st, (const TX *)q2, (const TX *)k2, (const TX *)val,
                           rows, (int)S, (int)F, (int)H, k_row_stride, v_row_stride, scale, (TX *)out, out_batch_stride,
                           tattn);
        return check_launch("k_trajectory_mix");
    }, [&] { return not_16bit("tome_trajectory_mix", dtype, "tensors"); });
}

// ---- backward of tome_prop_attention (plain form) and of tome_prop_attention_segments (tome_attn_bwd.h)
static bool attn_bwd_shape_ok(int64_t B, int64_t H, int64_t N, int64_t Nk, int64_t nseg = 1) {
    return B > 0 && H > 0 && N > 0 && Nk > 0 && nseg > 0 && nseg <= 0x7fffffffLL / 64 &&
           B * H * nseg <= 0x7fffffffLL / 64 && N <= 0x7fffffffLL / 4 && Nk <= 0x7fffffffLL / 4 &&
           B * H * nseg * N <= (1ll << 40);
}

extern "C" size_t tome_prop_attention_backward_workspace_bytes(int64_t B, int64_t H, int64_t N, int64_t Nk) {
    if (!attn_bwd_shape_ok(B, H, N, Nk)) return 0;
    return align_up(2 * (size_t)(B * H * N) * sizeof(float), 256);  // L and delta, one fp32 each per query row
}

extern "C" size_t tome_prop_attention_segments_backward_workspace_bytes(int64_t B, int64_t H, int64_t N, int64_t Nk,
                                                                        int64_t nseg) {
    if (!attn_bwd_shape_ok(B, H, N, Nk, nseg)) return 0;
    return align_up(2 * (size_t)(nseg * B * H * N) * sizeof(float), 256);  // L and delta per (segment, query row)
}

// Both entries: nseg == 0 is the plain form (seg_strides / grad_seg_strides unused), nseg >= 1 the segmented one with
// seg_strides = {k, v, out, log_size} and grad_seg_strides = {dout, dk, dv} element offsets between segments.
static int attn_backward_impl(const char *fn, const void *q, const void *k, const void *v, const void *out,
                              const void *dout, int dtype, int64_t B, int64_t H, int64_t N, int64_t Nk, int64_t D,
                              const int64_t *q_strides, const int64_t *k_strides, const int64_t *v_strides,
                              const int64_t *out_strides, const int64_t *dout_strides, const float *log_size,
                              int64_t log_size_stride, int bias_skip, float scale, int64_t nseg,
                              const int64_t *seg_strides, const int64_t *grad_seg_strides, void *dq, void *dk, void *dv,
                              const int64_t *dq_strides, const int64_t *dk_strides, const int64_t *dv_strides,
                              void *workspace, size_t workspace_bytes, tome_stream_t stream) {
    const bool seg = nseg > 0;
    const int64_t ns = seg ? nseg : 1;
    if (!q || !k || !v || !out || !dout || !dq || !dk || !dv || !q_strides || !k_strides || !v_strides || !out_strides ||
        !dout_strides || !dq_strides || !dk_strides || !dv_strides || !attn_bwd_shape_ok(B, H, N, Nk, ns))
        return fail(TOME_EINVAL, "%s: bad shape/pointer", fn);
    if (D != ATT_D) return fail(TOME_EINVAL, "%s: head dim %lld (only 64)", fn, (long long)D);
    if (int rc = not_16bit(fn, dtype, "q/k/v")) return rc;
    if (bias_skip != 0 && bias_skip != 1) return fail(TOME_EINVAL, "%s: bias_skip %d", fn, bias_skip);
    if (bias_skip && N != Nk) return fail(TOME_EINVAL, "%s: bias_skip needs as many keys as queries", fn);
    const int64_t *ss[8] = {q_strides, k_strides, v_strides, out_strides, dout_strides, dq_strides, dk_strides, dv_strides};
    const void *pp[8] = {q, k, v, out, dout, dq, dk, dv};
    for (int i = 0; i < 8; ++i) {
        if (!aligned16(pp[i]) || ss[i][0] % 8 || ss[i][1] % 8 || ss[i][2] % 8 || ss[i][2] < D)
            return fail(TOME_EINVAL, "%s: rows must be 16-byte aligned (pointers, strides %% 8 == 0, token stride >= 64)", fn);
    }
    if (seg) {
        if (!seg_strides || !grad_seg_strides) return fail(TOME_EINVAL, "%s: segment offsets required", fn);
        if (seg_strides[0] % 8 || seg_strides[1] % 8 || seg_strides[2] % 8 || grad_seg_strides[0] % 8 ||
            grad_seg_strides[1] % 8 || grad_seg_strides[2] % 8)
            return fail(TOME_EINVAL, "%s: segment offsets must keep rows 16-byte aligned", fn);
    }
    const size_t need = seg ? tome_prop_attention_segments_backward_workspace_bytes(B, H, N, Nk, nseg)
                            : tome_prop_attention_backward_workspace_bytes(B, H, N, Nk);
    if (!workspace || workspace_bytes < need)
        return fail(TOME_EWORKSPACE, "%s: workspace %zu < %zu bytes", fn, workspace ? workspace_bytes : (size_t)0, need);
    if (!aligned16(workspace)) return fail(TOME_EINVAL, "%s: workspace not 16-byte aligned", fn);
    AttnBwdArgs a;
    a.q = q; a.k = k; a.v = v; a.o = out; a.dout = dout; a.dq = dq; a.dk = dk; a.dv = dv;
    a.q_sb = q_strides[0]; a.q_sh = q_strides[1]; a.q_sn = q_strides[2];
    a.k_sb = k_strides[0]; a.k_sh = k_strides[1]; a.k_sn = k_strides[2];
    a.v_sb = v_strides[0]; a.v_sh = v_strides[1]; a.v_sn = v_strides[2];
    a.o_sb = out_strides[0]; a.o_sh = out_strides[1]; a.o_sn = out_strides[2];
    a.do_sb = dout_strides[0]; a.do_sh = dout_strides[1]; a.do_sn = dout_strides[2];
    a.dq_sb = dq_strides[0]; a.dq_sh = dq_strides[1]; a.dq_sn = dq_strides[2];
    a.dk_sb = dk_strides[0]; a.dk_sh = dk_strides[1]; a.dk_sn = dk_strides[2];
    a.dv_sb = dv_strides[0]; a.dv_sh = dv_strides[1]; a.dv_sn = dv_strides[2];
    a.log_size = log_size; a.ls_sb = log_size_stride;
    a.lse = (float *)workspace; a.delta = (float *)workspace + ns * B * H * N;
    a.B = (int)B; a.H = (int)H; a.N = (int)N; a.Nk = (int)Nk; a.scale = scale; a.bias_skip = bias_skip;
    a.nseg = (int)ns;
    a.k_seg = a.v_seg = a.o_seg = a.do_seg = a.dk_seg = a.dv_seg = a.ls_seg = 0;
    if (seg) {
        a.k_seg = seg_strides[0]; a.v_seg = seg_strides[1]; a.o_seg = seg_strides[2]; a.ls_seg = seg_strides[3];
        a.do_seg = grad_seg_strides[0]; a.dk_seg = grad_seg_strides[1]; a.dv_seg = grad_seg_strides[2];
    }
    // dq: one workgroup per 128 queries of a (batch, head), every segment inside it; dk / dv: per (segment, batch, head)
    const int64_t bh8 = (B * H + 7) / 8 * 8, sbh8 = (ns * B * H + 7) / 8 * 8;
    const int64_t qblocks = (N + ATTB_BM - 1) / ATTB_BM, kblocks = (Nk + ATTB_BM - 1) / ATTB_BM;
    if (bh8 * qblocks > 0x7fffffffLL || sbh8 * kblocks > 0x7fffffffLL) return fail(TOME_EINVAL, "%s: grid too large", fn);
    hipStream_t st = (hipStream_t)stream;
    const dim3 qgrid((unsigned)(bh8 * qblocks)), kgrid((unsigned)(sbh8 * kblocks)), block(64 * ATTB_WAVES);
    auto go = [&](auto tx, auto bias, auto segf) {
        using TX = typename decltype(tx)::type;
        constexpr bool BIAS = decltype(bias)::value != 0;
        constexpr bool SEG = decltype(segf)::value != 0;
        hipLaunchKernelGGL((k_attn_bwd_dq<TX, BIAS, SEG>), qgrid, block, 0, st, a);
        if (int rc = check_launch("k_attn_bwd_dq")) return rc;
        hipLaunchKernelGGL((k_attn_bwd_dkv<TX, BIAS, SEG>), kgrid, block, 0, st, a);
        return check_launch("k_attn_bwd_dkv");
    };
    return dispatch_attn(dtype, log_size != nullptr, [&](auto tx, auto bias) {
        return seg ? go(tx, bias, Op<1>{}) : go(tx, bias, Op<0>{});
    }, [&] { return not_16bit(fn, dtype, "q/k/v"); });
}

extern "C" int tome_prop_attention_backward(const void *q, const void *k, const void *v, const void *out,
                                            const void *dout, int dtype, int64_t B, int64_t H, int64_t N, int64_t Nk,
                                            int64_t D, const int64_t *q_strides, const int64_t *k_strides,
                                            const int64_t *v_strides, const int64_t *out_strides,
                                            const int64_t *dout_strides, const float *log_size,
                                            int64_t log_size_stride, int bias_skip, float scale, void *dq, void *dk,
                                            void *dv, const int64_t *dq_strides, const int64_t *dk_strides,
                                            const int64_t *dv_strides, void *workspace, size_t workspace_bytes,
                                            tome_stream_t stream) {
    return attn_backward_impl("tome_prop_attention_backward", q, k, v, out, dout, dtype, B, H, N, Nk, D, q_strides,
                              k_strides, v_strides, out_strides, dout_strides, log_size, log_size_stride, bias_skip, scale,
                              0, nullptr, nullptr, dq, dk, dv, dq_strides, dk_strides, dv_strides, workspace,
                              workspace_bytes, stream);
}

extern "C" int tome_prop_attention_segments_backward(
    const void *q, const void *k, const void *v, const void *out, const void *dout, int dtype, int64_t B, int64_t H,
    int64_t N, int64_t Nk, int64_t D, const int64_t *q_strides, const int64_t *k_strides, const int64_t *v_strides,
    const int64_t *out_strides, const int64_t *dout_strides, const float *log_size, int64_t log_size_stride, float scale,
    int64_t nseg, const int64_t *seg_strides, const int64_t *grad_seg_strides, void *dq, void *dk, void *dv,
    const int64_t *dq_strides, const int64_t *dk_strides, const int64_t *dv_strides, void *workspace,
    size_t workspace_bytes, tome_stream_t stream) {
    const char *const fn = "tome_prop_attention_segments_backward";
    if (nseg < 1) return fail(TOME_EINVAL, "%s: nseg >= 1 required", fn);
    return attn_backward_impl(fn, q, k, v, out, dout, dtype, B, H, N, Nk, D, q_strides, k_strides, v_strides, out_strides,
                              dout_strides, log_size, log_size_stride, 0, scale, nseg, seg_strides, grad_seg_strides, dq,
                              dk, dv, dq_strides, dk_strides, dv_strides, workspace, workspace_bytes, stream);
}

// ---- backward of tome_trajectory_mix (tome_traj_bwd.h)
extern "C" int tome_trajectory_mix_backward(const void *q2, const void *k2, const void *val, const void *dout, int dtype,
                                            int64_t B, int64_t S, int64_t F, int64_t H, int64_t D, int64_t k_row_stride,
                                            int64_t v_row_stride, int64_t dout_batch_stride, float scale, void *dq2,
                                            void *dk2, void *dval, int64_t dk_row_stride, int64_t dv_row_stride,
                                            tome_stream_t stream) {
    const char *const fn = "tome_trajectory_mix_backward";
    if (!q2 || !k2 || !val || !dout || !dq2 || B <= 0 || S <= 0 || F <= 0 || H <= 0)
        return fail(TOME_EINVAL, "%s: bad shape/pointer", fn);
    if (D != 64 || H > 16 || F > TRAJ_MAXF)
        return fail(TOME_EINVAL, "%s: head dim 64, at most 16 heads and %d frames", fn, TRAJ_MAXF);
    if (int rc = not_16bit(fn, dtype, "tensors")) return rc;
    const int64_t C = H * D;
    if (k_row_stride % 8 || v_row_stride % 8 || k_row_stride < C || v_row_stride < C || !aligned16(q2) || !aligned16(k2) ||
        !aligned16(val) || !aligned16(dout) || !aligned16(dq2))
        return fail(TOME_EINVAL, "%s: rows must be 16-byte aligned", fn);
    if ((dk2 && (dk_row_stride % 8 || dk_row_stride < C || !aligned16(dk2))) ||
        (dval && (dv_row_stride % 8 || dv_row_stride < C || !aligned16(dval))))
        return fail(TOME_EINVAL, "%s: rows of dk2 / dval must be 16-byte aligned and at least H*64 elements apart", fn);
    if (dout_batch_stride == 0) dout_batch_stride = S * C;
    if (dout_batch_stride < S * C || dout_batch_stride % 8)
        return fail(TOME_EINVAL, "%s: dout_batch_stride must be 0 or a multiple of 8 >= S*H*D", fn);
    const int64_t rows = B * S;
    if (rows > 0x7fffffffLL) return fail(TOME_EINVAL, "%s: too many tokens", fn);
    TrajBwdArgs a;
    a.q2 = q2; a.k2 = k2; a.val = val; a.dout = dout; a.dq2 = dq2; a.dk2 = dk2; a.dval = dval;
    a.rows = rows; a.k_row = k_row_stride; a.v_row = v_row_stride; a.dk_row = dk_row_stride; a.dv_row = dv_row_stride;
    a.do_sb = dout_batch_stride; a.S = (int)S; a.F = (int)F; a.H = (int)H; a.scale = scale;
    const dim3 grid((unsigned)((rows + 3) / 4));
    hipStream_t st = (hipStream_t)stream;
    return dispatch_x<false>(dtype, [&](auto tx) {
        using TX = typename decltype(tx)::type;
        hipLaunchKernelGGL(k_trajectory_mix_bwd<TX>, grid, dim3(256), 0, st, a);
        return check_launch("k_trajectory_mix_bwd");
    }, [&] { return not_16bit(fn, dtype, "tensors"); });
}

// The rows tome_short_attention and its backward can walk: {batch, head, token} element strides with the heads of a
// token side by side (head stride 64), rows 16-byte aligned
static int check_short_rows(const char *who, const int64_t *const *strides, int nstrides, const void *const *ptrs,
                            int nptrs) {
    for (int i = 0; i < nstrides; ++i)
        if (strides[i][1] != 64 || strides[i][0] % 8 || strides[i][2] % 8)
            return fail(TOME_EINVAL, "%s: head stride must be 64, batch / token strides multiples of 8", who);
    for (int i = 0; i < nptrs; ++i)
        if (!aligned16(ptrs[i])) return fail(TOME_EINVAL, "%s: rows must be 16-byte aligned", who);
    return TOME_OK;
}

extern "C" int tome_short_attention(const void *q, const void *k, const void *v, int dtype, int64_t B, int64_t H,
                                    int64_t N, int64_t D, const int64_t *q_strides, const int64_t *k_strides,
                                    const int64_t *v_strides, float scale, void *out, tome_stream_t stream) {
    if (!q || !k || !v || !out || !q_strides || !k_strides || !v_strides || B <= 0 || H <= 0 || N <= 0)
        return fail(TOME_EINVAL, "tome_short_attention: bad shape/pointer");
    if (D != 64 || N > SHORT_MAXN)
        return fail(TOME_EINVAL, "tome_short_attention: head dim 64 and at most %d tokens per sequence", SHORT_MAXN);
    if (int rc = not_16bit("tome_short_attention", dtype, "tensors")) return rc;
    const int64_t *strides[3] = {q_strides, k_strides, v_strides};
    const void *ptrs[4] = {q, k, v, out};
    if (int rc = check_short_rows("tome_short_attention", strides, 3, ptrs, 4)) return rc;
    const int64_t units = B * H;  // (sequence, head) pairs, eight lanes each
    const int64_t blocks = (units + 31) / 32;
    if (blocks > 0x7fffffffLL) return fail(TOME_EINVAL, "tome_short_attention: too many sequences");
    hipStream_t st = (hipStream_t)stream;
    return dispatch_x<false>(dtype, [&](auto tx) {
        using TX = typename decltype(tx)::type;
        hipLaunchKernelGGL(k_short_attention<TX>, dim3((unsigned)blocks), dim3(256), 0, st, (const TX *)q, (const TX *)k,
                           (const TX *)v, q_strides[0], q_strides[2], k_strides[0], k_strides[2], v_strides[0],
                           v_strides[2], units, (int)H, (int)N, scale, (TX *)out);
        return check_launch("k_short_attention");
    }, [&] { return not_16bit("tome_short_attention", dtype, "tensors"); });
}

extern "C" int tome_short_attention_backward(const void *q, const void *k, const void *v, const void *dout, int dtype,
                                             int64_t B, int64_t H, int64_t N, int64_t D, const int64_t *q_strides,
                                             const int64_t *k_strides, const int64_t *v_strides, float scale, void *dq,
                                             void *dk, void *dv, const int64_t *dq_strides, const int64_t *dk_strides,
                                             const int64_t *dv_strides, tome_stream_t stream) {
    if (!q || !k || !v || !dout || !dq || !dk || !dv || !q_strides || !k_strides || !v_strides || !dq_strides ||
        !dk_strides || !dv_strides || B <= 0 || H <= 0 || N <= 0)
        return fail(TOME_EINVAL, "tome_short_attention_backward: bad shape/pointer");
    if (D != 64 || N > SHORT_MAXN)
        return fail(TOME_EINVAL, "tome_short_attention_backward: head dim 64 and at most %d tokens per sequence",
                    SHORT_MAXN);
    if (int rc = not_16bit("tome_short_attention_backward", dtype, "tensors")) return rc;
    const int64_t *strides[6] = {q_strides, k_strides, v_strides, dq_strides, dk_strides, dv_strides};
    const void *ptrs[7] = {q, k, v, dout, dq, dk, dv};
    if (int rc = check_short_rows("tome_short_attention_backward", strides, 6, ptrs, 7)) return rc;
    // a target's rows must not lie on top of each other: a token's H heads fill H * 64 elements
    for (int i = 3; i < 6; ++i)
        if ((B > 1 && strides[i][0] < H * 64) || (N > 1 && strides[i][2] < H * 64))
            return fail(TOME_EINVAL, "tome_short_attention_backward: rows of dq / dk / dv overlap");
    const int64_t units = B * H;  // (sequence, head) pairs, eight lanes each
    const int64_t blocks = (units + 31) / 32;
    if (blocks > 0x7fffffffLL) return fail(TOME_EINVAL, "tome_short_attention_backward: too many sequences");
    const ShortBwdStrides s{q_strides[0],  q_strides[2],  k_strides[0],  k_strides[2],  v_strides[0],  v_strides[2],
                            dq_strides[0], dq_strides[2], dk_strides[0], dk_strides[2], dv_strides[0], dv_strides[2]};
    hipStream_t st = (hipStream_t)stream;
    return dispatch_x<false>(dtype, [&](auto tx) {
        using TX = typename decltype(tx)::type;
        hipLaunchKernelGGL(k_short_attention_bwd<TX>, dim3((unsigned)blocks), dim3(256), 0, st, (const TX *)q,
                           (const TX *)k, (const TX *)v, (const TX *)dout, s, units, (int)H, (int)N, scale, (TX *)dq,
                           (TX *)dk, (TX *)dv);
        return check_launch("k_short_attention_bwd");
    }, [&] { return not_16bit("tome_short_attention_backward", dtype, "tensors"); });
}

// tome_gelu_erf / tome_gelu_tanh: one streaming launch of k_gelu_erf / k_gelu_tanh (FORM: GELU_ERF / GELU_TANH).
template <int FORM>
static int gelu_impl(const char *who, const void *x, int dtype, int64_t elements, void *y, tome_stream_t stream) {
    if (!x || !y || elements <= 0) return fail(TOME_EINVAL, "%s: bad shape/pointer", who);
    if (int rc = not_16bit(who, dtype, "tensors")) return rc;
    if (elements % 8 || !aligned16(x) || !aligned16(y))
        return fail(TOME_EINVAL, "%s: a multiple of 8 elements in 16-byte aligned buffers required", who);
    const int64_t chunks = elements / 8;
    const int64_t blocks = (chunks + 1023) / 1024;  // 256 threads x 4 chunks
    if (blocks > 0x7fffffffLL) return fail(TOME_EINVAL, "%s: too large", who);
    hipStream_t st = (hipStream_t)stream;
    return dispatch_x<false>(dtype, [&](auto tx) {
        using TX = typename decltype(tx)::type;
        if (FORM == GELU_TANH) {
            hipLaunchKernelGGL(k_gelu_tanh<TX>, dim3((unsigned)blocks), dim3(256), 0, st, (const TX *)x, (TX *)y, chunks);
            return check_launch("k_gelu_tanh");
        }
        hipLaunchKernelGGL(k_gelu_erf<TX>, dim3((unsigned)blocks), dim3(256), 0, st, (const TX *)x, (TX *)y, chunks);
        return check_launch("k_gelu_erf");
    }, [&] { return not_16bit(who, dtype, "tensors"); });
}

extern "C" int tome_gelu_erf(const void *x, int dtype, int64_t elements, void *y, tome_stream_t stream) {
    return gelu_impl<GELU_ERF>("tome_gelu_erf", x, dtype, elements, y, stream);
}

extern "C" int tome_gelu_tanh(const void *x, int dtype, int64_t elements, void *y, tome_stream_t stream) {
    return gelu_impl<GELU_TANH>("tome_gelu_tanh", x, dtype, elements, y, stream);
}

// tome_token_mean: one launch of k_token_mean, a workgroup per (group, 512-channel slab).
extern "C" int tome_token_mean(const void *x, int dtype, int64_t groups, int64_t tokens, int64_t width, int act,
                               float *out, tome_stream_t stream) {
    if (!x || !out) return fail(TOME_EINVAL, "tome_token_mean: null pointer");
    if (int rc = not_16bit("tome_token_mean", dtype, "tensors")) return rc;
    if (act != TOKEN_MEAN_NONE && act != TOKEN_MEAN_GELU_ERF)
        return fail(TOME_EINVAL, "tome_token_mean: act must be 0 (none) or 1 (exact-erf GELU), got %d", act);
    if (groups < 1 || tokens < 1 || width < 8 || width % 8)
        return fail(TOME_EINVAL, "tome_token_mean: groups >= 1, tokens >= 1 and width %% 8 == 0 required");
    if (!aligned16(x) || ((uintptr_t)out & 3))
        return fail(TOME_EINVAL, "tome_token_mean: x must be 16-byte aligned, out 4-byte aligned");
    const int64_t slabs = (width + TOKEN_MEAN_SLAB - 1) / TOKEN_MEAN_SLAB;
    if (width > 0x7fffffffLL - TOKEN_MEAN_SLAB || tokens > 0x7fffffffLL || groups > 0x7fffffffLL / slabs
        || groups > INT64_MAX / tokens / width)
        return fail(TOME_EINVAL, "tome_token_mean: too large");
    hipStream_t st = (hipStream_t)stream;
    return dispatch_x<false>(dtype, [&](auto tx) {
        using TX = typename decltype(tx)::type;
        auto launch = [&](auto a) {
            hipLaunchKernelGGL((k_token_mean<TX, decltype(a)::value>), dim3((unsigned)(groups * slabs)), dim3(256), 0, st,
                               (const TX *)x, tokens, (int)width, (int)slabs, out);
            return check_launch("k_token_mean");
        };
        return act == TOKEN_MEAN_GELU_ERF ? launch(Op<TOKEN_MEAN_GELU_ERF>{}) : launch(Op<TOKEN_MEAN_NONE>{});
    }, [&] { return not_16bit("tome_token_mean", dtype, "tensors"); });
}

// The launch form of k_gelu_bwd with the bias gradient for `rows` rows of `width`: S column slots per thread, U passes
// per step, RP rows per pass, and how many steps a workgroup walks (spw) so that at most GELU_BWD_MAX_PARTS workgroups
// (= partial rows of the workspace) run: two per CU, all resident from the start.
#define GELU_BWD_MAX_PARTS 512
#define GELU_BWD_MAX_WIDTH 8192
struct GeluBwdForm { int S; int U; int RP; int64_t spw; int64_t parts; };
static GeluBwdForm gelu_bwd_form(int64_t rows, int64_t width) {
    const int64_t cpr = width / 8;
    const int S = (int)((cpr + 255) / 256);
    const int U = S == 1 ? 4 : (S <= 3 ? 2 : 1);
    const int RP = S == 1 ? (int)(256 / cpr) : 1;
    const int64_t passes = (rows + RP - 1) / RP;
    const int64_t steps = (passes + U - 1) / U;
    const int64_t spw = (steps + GELU_BWD_MAX_PARTS - 1) / GELU_BWD_MAX_PARTS;
    return GeluBwdForm{S, U, RP, spw, (steps + spw - 1) / spw};
}

static bool gelu_bwd_shape_ok(int64_t rows, int64_t width) {
    return rows >= 1 && rows <= 0x7fffffffLL && width >= 8 && width % 8 == 0 && width <= GELU_BWD_MAX_WIDTH;
}

extern "C" size_t tome_gelu_erf_backward_workspace_bytes(int64_t rows, int64_t width) {
    if (!gelu_bwd_shape_ok(rows, width)) return 0;
    return align_up((size_t)gelu_bwd_form(rows, width).parts * (size_t)width * sizeof(float), 256);
}

// tome_gelu_erf_backward / tome_gelu_tanh_backward: the same checks, launch form and workspace; FORM picks the
// activation's formula inside k_gelu_bwd.
template <int FORM>
static int gelu_backward_impl(const char *who, const void *h, const void *ga, int dtype, int64_t rows, int64_t width,
                              void *gh, void *act, void *dbias, void *workspace, size_t workspace_bytes,
                              tome_stream_t stream) {
    if (!h || !ga || !gh) return fail(TOME_EINVAL, "%s: null buffer", who);
    if (int rc = not_16bit(who, dtype, "tensors")) return rc;
    if (!gelu_bwd_shape_ok(rows, width))
        return fail(TOME_EINVAL, "%s: width %% 8 == 0, width <= 8192 and 1 .. 2^31 - 1 rows required", who);
    if (!aligned16(h) || !aligned16(ga) || !aligned16(gh) || !aligned16(act) || !aligned16(dbias) ||
        !aligned16(workspace))
        return fail(TOME_EINVAL, "%s: 16-byte aligned buffers required", who);
    if (act && (act == h || act == ga || act == gh))
        return fail(TOME_EINVAL, "%s: the activation needs a buffer of its own", who);
    if (gh == h) return fail(TOME_EINVAL, "%s: gh may lie over ga, not over h", who);
    if (dbias && (!workspace || workspace_bytes < tome_gelu_erf_backward_workspace_bytes(rows, width)))
        return fail(TOME_EWORKSPACE, "%s: the bias gradient needs a workspace of "
                                     "tome_gelu_erf_backward_workspace_bytes()", who);
    const int64_t cpr = width / 8, chunks = rows * cpr;
    hipStream_t st = (hipStream_t)stream;
    return dispatch_x<false>(dtype, [&](auto tx) {
        using TX = typename decltype(tx)::type;
        // k_gelu_bwd<TX, column slots, with the bias gradient, with the activation, FORM>
        auto with_act = [&](auto launch) { return act ? launch(Op<1>{}) : launch(Op<0>{}); };
        if (!dbias) {  // flat: rows of 256 chunks, four per lane, as k_gelu_erf
            const int64_t blocks = (chunks + 1023) / 1024;
            return with_act([&](auto a) {
                hipLaunchKernelGGL((k_gelu_bwd<TX, 1, false, decltype(a)::value != 0, FORM>), dim3((unsigned)blocks),
                                   dim3(256), 0, st, (const TX *)h, (const TX *)ga, chunks, 256, 1, 1, (TX *)gh, (TX *)act,
                                   (float *)nullptr);
                return check_launch("k_gelu_bwd");
            });
        }
        const GeluBwdForm f = gelu_bwd_form(rows, width);
        auto launch = [&](auto slots) {
            return with_act([&](auto a) {
                hipLaunchKernelGGL((k_gelu_bwd<TX, decltype(slots)::value, true, decltype(a)::value != 0, FORM>),
                                   dim3((unsigned)f.parts), dim3(256), 0, st, (const TX *)h, (const TX *)ga, chunks, (int)cpr,
                                   f.RP, (int)f.spw, (TX *)gh, (TX *)act, (float *)workspace);
                return check_launch("k_gelu_bwd");
            });
        };
        int rc;
        switch (f.S) {
        case 1: rc = launch(Op<1>{}); break;
        case 2: rc = launch(Op<2>{}); break;
        case 3: rc = launch(Op<3>{}); break;
        default: rc = launch(Op<4>{}); break;
        }
        if (rc) return rc;
        return launch_param_grad<TX>(workspace, f.parts, width, width, dbias, nullptr, st);
    }, [&] { return not_16bit(who, dtype, "tensors"); });
}

extern "C" int tome_gelu_erf_backward(const void *h, const void *ga, int dtype, int64_t rows, int64_t width, void *gh,
                                      void *act, void *dbias, void *workspace, size_t workspace_bytes,
                                      tome_stream_t stream) {
    return gelu_backward_impl<GELU_ERF>("tome_gelu_erf_backward", h, ga, dtype, rows, width, gh, act, dbias, workspace,
                                        workspace_bytes, stream);
}

extern "C" int tome_gelu_tanh_backward(const void *h, const void *ga, int dtype, int64_t rows, int64_t width, void *gh,
                                       void *act, void *dbias, void *workspace, size_t workspace_bytes,
                                       tome_stream_t stream) {
    return gelu_backward_impl<GELU_TANH>("tome_gelu_tanh_backward", h, ga, dtype, rows, width, gh, act, dbias,
                                         workspace, workspace_bytes, stream);
}

extern "C" int tome_tubelet_rows(const void *x, int elem_bytes, int64_t B, int64_t C, int64_t T, int64_t H, int64_t W,
                                 const int64_t *x_strides, int64_t kt, int64_t kh, int64_t kw, void *rows,
                                 tome_stream_t stream) {
    if (!x || !rows || !x_strides || B <= 0 || C <= 0 || T <= 0 || H <= 0 || W <= 0 || kt <= 0 || kh <= 0 || kw <= 0)
        return fail(TOME_EINVAL, "tome_tubelet_rows: bad shape/pointer");
    if (elem_bytes != 2 && elem_bytes != 4) return fail(TOME_EINVAL, "tome_tubelet_rows: 2- or 4-byte elements only");
    if (T % kt || H % kh || W % kw) return fail(TOME_EINVAL, "tome_tubelet_rows: the clip must be whole tubelets");
    if ((kw * elem_bytes) % 16 || !aligned16(x) || !aligned16(rows))
        return fail(TOME_EINVAL, "tome_tubelet_rows: runs of kw elements must be whole 16-byte chunks in aligned buffers");
    for (int i = 0; i < 4; ++i)
        if (x_strides[i] < 0 || (x_strides[i] * elem_bytes) % 16)
            return fail(TOME_EINVAL, "tome_tubelet_rows: {b, c, t, h} strides must be non-negative multiples of 16 bytes");
    TubeArgs a;
    a.sb = x_strides[0]; a.sc = x_strides[1]; a.st = x_strides[2]; a.sh = x_strides[3];
    a.nt = (int)(T / kt); a.nh = (int)(H / kh); a.nw = (int)(W / kw);
    a.kt = (int)kt; a.kh = (int)kh;
    a.cpr = (int)(kw * elem_bytes / 16);
    const int64_t chunks = C * kt * kh * a.cpr;
    if (chunks > 0x7fffffffLL || T / kt > 0x7fffffffLL || H / kh > 0x7fffffffLL || W / kw > 0x7fffffffLL)
        return fail(TOME_EINVAL, "tome_tubelet_rows: too large");
    a.chunks = (int)chunks;
    a.items = B * a.nt * a.nh * chunks;
    const int64_t blocks = (a.items + 255) / 256;
    if (blocks > 0x7fffffffLL) return fail(TOME_EINVAL, "tome_tubelet_rows: too large");
    hipStream_t st = (hipStream_t)stream;
    if (elem_bytes == 2)
        hipLaunchKernelGGL(k_tubelet_rows<2>, dim3((unsigned)blocks), dim3(256), 0, st, (const uint8_t *)x, (uint8_t *)rows, a);
    else
        hipLaunchKernelGGL(k_tubelet_rows<4>, dim3((unsigned)blocks), dim3(256), 0, st, (const uint8_t *)x, (uint8_t *)rows, a);
    return check_launch("k_tubelet_rows");
}

extern "C" int tome_row_map(int64_t n, int64_t T, int64_t r, int distill_token, const int64_t *src_idx,
                            const int64_t *dst_idx, const int64_t *unm_idx, int32_t *row_map, tome_stream_t stream) {
    const int64_t T1 = (T + 1) / 2;
    if (n <= 0 || T <= 0 || r <= 0 || r > T1 || !row_map || !src_idx || !dst_idx || (!unm_idx && T1 > r))
        return fail(TOME_EINVAL, "tome_row_map: bad shape/pointer");
    if (n * T1 > 0x7fffffffLL) return fail(TOME_EINVAL, "tome_row_map: too large");
    hipLaunchKernelGGL(k_row_map, dim3((unsigned)((n * T1 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (int)n,
                       (int)T1, (int)r, distill_token, src_idx, dst_idx, unm_idx, row_map);
    return check_launch("k_row_map");
}

extern "C" int tome_source_init(int64_t n, int64_t T, int64_t r, int distill_token, int drop, const int32_t *row_map,
                                float *source_out, tome_stream_t stream) {
    const int64_t T1 = (T + 1) / 2;
    if (n <= 0 || T <= 0 || r <= 0 || r > T1 || !row_map || !source_out)
        return fail(TOME_EINVAL, "tome_source_init: bad shape/pointer");
    if (n * (T - r) > 0x7fffffffLL) return fail(TOME_EINVAL, "tome_source_init: too many rows");
    hipLaunchKernelGGL(k_source_init, dim3((unsigned)(n * (T - r))), dim3(256), 0, (hipStream_t)stream, (int)n, (int)T,
                       (int)r, distill_token, drop ? 1 : 0, row_map, source_out);
    return check_launch("k_source_init");
}

template <typename TX>
static int launch_unmerge(const void *x, int64_t n, int64_t T, int64_t C, int64_t r, const int64_t *src,
                          const int64_t *dst, const int64_t *unm, void *out, hipStream_t st) {
    const int64_t rows = n * (T - r);
    const unsigned nb = (unsigned)((rows + 3) / 4);
    return with_vec<TX>(C, x, out, [&](auto vec) {
        hipLaunchKernelGGL((k_unmerge_rows<TX, decltype(vec)::value>), dim3(nb), dim3(256), 0, st, (const TX *)x, (int)n,
                           (int)T, (int)C, (int)r, src, dst, unm, (TX *)out);
        return check_launch("k_unmerge_rows");
    });
}

extern "C" int tome_unmerge(const void *x, int dtype, int64_t n, int64_t T, int64_t C, int64_t r,
                            const int64_t *src_idx, const int64_t *dst_idx, const int64_t *unm_idx, void *out,
                            tome_stream_t stream) {
    if (int rc = check_merge_args("tome_unmerge", x, n, T, C, r, out)) return rc;
    if (!src_idx || !dst_idx || (!unm_idx && (T + 1) / 2 > r))
        return fail(TOME_EINVAL, "tome_unmerge: null index buffer");
    return dispatch_x<true>(dtype, [&](auto tx) {
        return launch_unmerge<typename decltype(tx)::type>(x, n, T, C, r, src_idx, dst_idx, unm_idx, out,
                                                           (hipStream_t)stream);
    }, [&] { return fail(TOME_EINVAL, "tome_unmerge: dtype %d", dtype); });
}

// ------------------------------------------------------------------------------------------------
// backward of merge / merge_wavg / drop with respect to the tokens (kernels in tome_merge_bwd.h)
// ------------------------------------------------------------------------------------------------
template <typename TX, typename TS>
static int launch_merge_bwd(const void *gy, const void *out_div, const void *in_mul, int64_t n, int64_t T, int64_t C,
                            int64_t r, const int32_t *row_map, int distill, int drop, void *gx, hipStream_t st,
                            const TokLayout *lgy_p = nullptr, const TokLayout *lgx_p = nullptr, int cls_rows = 0) {
    constexpr int VEC = 16 / sizeof(TX);
    const int64_t To = T - r;
    const bool vec_ok = (C % VEC == 0) && aligned16(gy) && aligned16(gx);
    const int64_t cpr = C / VEC;
    if (vec_ok && cpr <= FAST_NIT * WAVE) {
        const TokLayout lgy = lgy_p ? *lgy_p : contiguous_layout(To, C);
        const TokLayout lgx = lgx_p ? *lgx_p : contiguous_layout(T, C);
        int R = (int)((FAST_NIT * WAVE) / cpr);
        if (R > FAST_MAXR) R = FAST_MAXR;
        const int64_t wpg = (T + R - 1) / R, bpg = (wpg + 3) / 4;
        const int64_t ny = n + (cls_rows ? (cls_rows + 4 * bpg - 1) / (4 * bpg) : 0);
        const int64_t gy_ = ny < 65535 ? ny : 65535, gz = (ny + gy_ - 1) / gy_;
        if (gz > 65535) return fail(TOME_EINVAL, "merge backward: too many groups (%lld)", (long long)n);
        hipLaunchKernelGGL((k_merge_rows_bwd<TX, TS, FAST_NIT>), dim3((unsigned)bpg, (unsigned)gy_, (unsigned)gz),
                           dim3(256), 0, st, (const TX *)gy, (const TS *)out_div, (const TS *)in_mul, (int)n, (int)T,
                           (int)C, (int)r, R, (int)cpr, (int)wpg, row_map, distill, drop, (TX *)gx, lgy, lgx, cls_rows);
        return check_launch("k_merge_rows_bwd");
    }
    if (lgy_p || lgx_p || cls_rows)
        return fail(TOME_EINVAL, "regrouped merge backward needs rows of whole 16-byte chunks (C=%lld)", (long long)C);
    const unsigned nb = (unsigned)((n * T + 3) / 4);
    return with_vec<TX>(C, gy, gx, [&](auto vec) {
        hipLaunchKernelGGL((k_merge_rows_bwd_any<TX, TS, decltype(vec)::value>), dim3(nb), dim3(256), 0, st,
                           (const TX *)gy, (const TS *)out_div, (const TS *)in_mul, (int)n, (int)T, (int)C, (int)r, row_map,
                           distill, drop, (TX *)gx);
        return check_launch("k_merge_rows_bwd_any");
    });
}

extern "C" int tome_merge_backward(const void *grad_out, int x_dtype, const void *out_div, const void *in_mul,
                                   int size_dtype, int64_t n, int64_t T, int64_t C, int64_t r, const int32_t *row_map,
                                   int distill_token, int drop, void *grad_in, tome_stream_t stream) {
    if (int rc = check_merge_args("tome_merge_backward", grad_out, n, T, C, r, grad_in)) return rc;
    if (!row_map) return fail(TOME_EINVAL, "tome_merge_backward: null row_map");
    if (drop && (out_div || in_mul)) return fail(TOME_EINVAL, "tome_merge_backward: drop takes no scales");
    return dispatch_xs<true>(x_dtype, size_dtype, [&](auto tx, auto ts) {
        return launch_merge_bwd<typename decltype(tx)::type, typename decltype(ts)::type>(
            grad_out, out_div, in_mul, n, T, C, r, row_map, distill_token ? 1 : 0, drop ? 1 : 0, grad_in,
            (hipStream_t)stream);
    }, [&] { return fail(TOME_EINVAL, "tome_merge_backward: unsupported dtypes x=%d size=%d", x_dtype, size_dtype); });
}

extern "C" int tome_merge_backward_regrouped(const void *grad_out, int x_dtype, const void *out_div, const void *in_mul,
                                             int size_dtype, int64_t B, int64_t F, int64_t P, int64_t C, int64_t r,
                                             int has_cls, const int32_t *row_map, int drop, void *grad_in,
                                             tome_stream_t stream) {
    if (B <= 0 || F <= 0) return fail(TOME_EINVAL, "tome_merge_backward_regrouped: bad shape");
    const int64_t n = B * F;
    if (int rc = check_merge_args("tome_merge_backward_regrouped", grad_out, n, P, C, r, grad_in)) return rc;
    if (!row_map) return fail(TOME_EINVAL, "tome_merge_backward_regrouped: null row_map");
    if (drop && (out_div || in_mul)) return fail(TOME_EINVAL, "tome_merge_backward_regrouped: drop takes no scales");
    const int cls = has_cls ? 1 : 0;
    const TokLayout lgy{cls * C, (cls + (P - r) * F) * C, C, F * C, (int)F};
    const TokLayout lgx{cls * C, (cls + P * F) * C, C, F * C, (int)F};
    return dispatch_xs<true>(x_dtype, size_dtype, [&](auto tx, auto ts) {
        return launch_merge_bwd<typename decltype(tx)::type, typename decltype(ts)::type>(
            grad_out, out_div, in_mul, n, P, C, r, row_map, 0, drop ? 1 : 0, grad_in, (hipStream_t)stream, &lgy, &lgx,
            cls ? (int)B : 0);
    }, [&] {
        return fail(TOME_EINVAL, "tome_merge_backward_regrouped: unsupported dtypes x=%d size=%d", x_dtype, size_dtype);
    });
}

// ------------------------------------------------------------------------------------------------
// backward of tome_merge_wavg_ln / tome_drop_ln in the flat layout (kernel in tome_merge_ln_bwd.h)
// ------------------------------------------------------------------------------------------------
// The launch form of k_merge_ln_rows_bwd: R input-token rows per wave (three chunks per lane, as ln_bwd_form), wpg
// waves per group; with parameter gradients the n * wpg slabs are walked by at most LN_BWD_MAX_PARTS workgroups.
struct MergeLnBwdForm { int R; int64_t wpg; int64_t spw; int64_t parts; };
static MergeLnBwdForm merge_ln_bwd_form(int64_t n, int64_t T, int64_t C) {
    const int R = ln_rows_per_wave(C / 8, 3);
    const int64_t wpg = (T + R - 1) / R;
    const int64_t wgs = (n * wpg + 3) / 4;
    const int64_t spw = (wgs + LN_BWD_MAX_PARTS - 1) / LN_BWD_MAX_PARTS;
    return MergeLnBwdForm{R, wpg, spw, (wgs + spw - 1) / spw};
}

static bool merge_ln_bwd_shape_ok(int64_t n, int64_t T, int64_t C) {
    return n > 0 && T > 0 && n * T <= 0x7fffffffLL && C > 0 && C % 8 == 0 && C / 8 <= 2 * WAVE;
}

extern "C" size_t tome_merge_ln_backward_workspace_bytes(int64_t n, int64_t T, int64_t C) {
    if (!merge_ln_bwd_shape_ok(n, T, C)) return 0;
    return align_up((size_t)merge_ln_bwd_form(n, T, C).parts * 2 * (size_t)C * sizeof(float), 256);
}

extern "C" int tome_merge_ln_backward(const void *gy, const void *gx_out, const void *xs, int x_dtype,
                                      const void *out_div, const void *in_mul, int size_dtype, int64_t n, int64_t T,
                                      int64_t C, int64_t r, const int32_t *row_map, int distill_token, int drop,
                                      const void *weight, float eps, void *gx, void *dweight, void *dbias,
                                      void *workspace, tome_stream_t stream) {
    const char *who = "tome_merge_ln_backward";
    if (!xs || !weight) return fail(TOME_EINVAL, "%s: null buffer", who);
    if (int rc = check_merge_args(who, gy, n, T, C, r, gx)) return rc;
    if (int rc = not_16bit(who, x_dtype)) return rc;
    if (!row_map) return fail(TOME_EINVAL, "%s: null row_map", who);
    if (drop && (out_div || in_mul)) return fail(TOME_EINVAL, "%s: drop takes no scales", who);
    if (!merge_ln_bwd_shape_ok(n, T, C))
        return fail(TOME_EINVAL, "%s: C %% 8 == 0 and C <= 1024 required (C=%lld)", who, (long long)C);
    if (!aligned16(gy) || !aligned16(gx_out) || !aligned16(xs) || !aligned16(weight) || !aligned16(gx) ||
        !aligned16(workspace))
        return fail(TOME_EINVAL, "%s: 16-byte aligned buffers required", who);
    const bool params = dweight || dbias;
    if (params && !workspace)
        return fail(TOME_EWORKSPACE, "%s: parameter gradients need a workspace of %s_workspace_bytes()", who, who);
    const int64_t cpr = C / 8;
    const MergeLnBwdForm f = merge_ln_bwd_form(n, T, C);
    const int64_t bpg = (f.wpg + 3) / 4;
    const int64_t gy_ = n < 65535 ? n : 65535, gz = (n + gy_ - 1) / gy_;
    if (gz > 65535) return fail(TOME_EINVAL, "%s: too many groups (%lld)", who, (long long)n);
    hipStream_t st = (hipStream_t)stream;
    return dispatch_xs<false>(x_dtype, (out_div || in_mul) ? size_dtype : x_dtype, [&](auto tx, auto ts) {
        using TX = typename decltype(tx)::type;
        using TS = typename decltype(ts)::type;
        if (params) {
            hipLaunchKernelGGL((k_merge_ln_rows_bwd<TX, TS, 3, true>), dim3((unsigned)f.parts), dim3(256), 0, st,
                               (const TX *)gy, (const TX *)gx_out, (const TX *)xs, (const TS *)out_div,
                               (const TS *)in_mul, (const TX *)weight, (int)n, (int)T, (int)C, (int)r, f.R, (int)cpr,
                               (int)f.wpg, (int)f.spw, eps, row_map, distill_token ? 1 : 0, drop ? 1 : 0, (TX *)gx,
                               (float *)workspace);
            if (int rc = check_launch("k_merge_ln_rows_bwd")) return rc;
            return launch_param_grad<TX>(workspace, f.parts, 2 * C, C, dweight, dbias, st);
        }
        // frozen LayerNorm: one slab per wave, no column sums, no workspace
        hipLaunchKernelGGL((k_merge_ln_rows_bwd<TX, TS, 3, false>), dim3((unsigned)bpg, (unsigned)gy_, (unsigned)gz),
                           dim3(256), 0, st, (const TX *)gy, (const TX *)gx_out, (const TX *)xs, (const TS *)out_div,
                           (const TS *)in_mul, (const TX *)weight, (int)n, (int)T, (int)C, (int)r, f.R, (int)cpr,
                           (int)f.wpg, 1, eps, row_map, distill_token ? 1 : 0, drop ? 1 : 0, (TX *)gx, (float *)nullptr);
        return check_launch("k_merge_ln_rows_bwd");
    }, [&] { return fail(TOME_EINVAL, "%s: unsupported dtypes x=%d size=%d", who, x_dtype, size_dtype); });
}

// ------------------------------------------------------------------------------------------------
// backward of tome_merge_wavg_ln_amp / tome_drop_ln_amp in the flat layout (kernel in tome_merge_ln_bwd_amp.h): the
// launch form of tome_merge_ln_backward (merge_ln_bwd_form: slots of 8 channels, so the same for every stream dtype) in
// the dtypes of tome_layernorm_backward_amp.  Every refusal is made here, before the launch, each with a text of its own.
// ------------------------------------------------------------------------------------------------
extern "C" size_t tome_merge_ln_backward_amp_workspace_bytes(int64_t n, int64_t T, int64_t C, int x_dtype) {
    if (x_dtype != TOME_F32 && x_dtype != TOME_BF16 && x_dtype != TOME_F16) return 0;
    return tome_merge_ln_backward_workspace_bytes(n, T, C);
}

extern "C" int tome_merge_ln_backward_amp(const void *gy, int gy_dtype, const void *gx_out, const void *xs, int x_dtype,
                                          const void *out_div, const void *in_mul, int size_dtype, int64_t n, int64_t T,
                                          int64_t C, int64_t r, const int32_t *row_map, int distill_token, int drop,
                                          const void *weight_f32, float eps, void *gx, void *gx16, void *dweight_f32,
                                          void *dbias_f32, void *workspace, tome_stream_t stream) {
    const char *who = "tome_merge_ln_backward_amp";
    if (!xs || !weight_f32) return fail(TOME_EINVAL, "%s: null buffer", who);
    if (int rc = check_merge_args(who, gy, n, T, C, r, gx)) return rc;
    if (!ln_amp_dtypes_ok(gy_dtype, x_dtype))
        return fail(TOME_EINVAL, "%s: unsupported dtypes gy=%d x=%d (16-bit gy; x of gy's dtype or fp32)", who, gy_dtype,
                    x_dtype);
    if (gx16 && x_dtype != TOME_F32) return fail(TOME_EINVAL, "%s: gx16 belongs to an fp32 stream", who);
    if (!row_map) return fail(TOME_EINVAL, "%s: null row_map", who);
    if (drop && (out_div || in_mul)) return fail(TOME_EINVAL, "%s: drop takes no scales", who);
    const bool scales = out_div || in_mul;
    if (scales && size_dtype != TOME_F32 && size_dtype != x_dtype)
        return fail(TOME_EINVAL, "%s: sizes must be of x's dtype or fp32 (x=%d size=%d)", who, x_dtype, size_dtype);
    if (!merge_ln_bwd_shape_ok(n, T, C))
        return fail(TOME_EINVAL, "%s: C %% 8 == 0 and C <= 1024 required (C=%lld)", who, (long long)C);
    if (!aligned16(gy) || !aligned16(gx_out) || !aligned16(xs) || !aligned16(weight_f32) || !aligned16(gx) ||
        !aligned16(gx16) || !aligned16(workspace))
        return fail(TOME_EINVAL, "%s: 16-byte aligned buffers required", who);
    const bool params = dweight_f32 || dbias_f32;
    if (params && !workspace)  // (a null pointer, no size to fall short of: TOME_EINVAL like every refusal of this entry)
        return fail(TOME_EINVAL, "%s: parameter gradients need a workspace of %s_workspace_bytes()", who, who);
    const int64_t cpr = C / 8;
    const MergeLnBwdForm f = merge_ln_bwd_form(n, T, C);
    const int64_t bpg = (f.wpg + 3) / 4;
    const int64_t gy_ = n < 65535 ? n : 65535, gz = (n + gy_ - 1) / gy_;
    if (gz > 65535) return fail(TOME_EINVAL, "%s: too many groups (%lld)", who, (long long)n);
    hipStream_t st = (hipStream_t)stream;
    return dispatch_x<false>(gy_dtype, [&](auto tg) {
        using TG = typename decltype(tg)::type;
        auto go = [&](auto ts, auto tz) {
            using TS = typename decltype(ts)::type;
            using TZ = typename decltype(tz)::type;
            if (params) {
                hipLaunchKernelGGL((k_merge_ln_rows_bwd_amp<TS, TG, TZ, 3, true>), dim3((unsigned)f.parts), dim3(256), 0,
                                   st, (const TG *)gy, (const TS *)gx_out, (const TS *)xs, (const TZ *)out_div,
                                   (const TZ *)in_mul, (const float *)weight_f32, (int)n, (int)T, (int)C, (int)r, f.R,
                                   (int)cpr, (int)f.wpg, (int)f.spw, eps, row_map, distill_token ? 1 : 0, drop ? 1 : 0,
                                   (TS *)gx, (TG *)gx16, (float *)workspace);
                if (int rc = check_launch("k_merge_ln_rows_bwd_amp")) return rc;
                return launch_param_grad<float>(workspace, f.parts, 2 * C, C, dweight_f32, dbias_f32, st);
            }
            // frozen LayerNorm: one slab per wave, no column sums, no workspace
            hipLaunchKernelGGL((k_merge_ln_rows_bwd_amp<TS, TG, TZ, 3, false>),
                               dim3((unsigned)bpg, (unsigned)gy_, (unsigned)gz), dim3(256), 0, st, (const TG *)gy,
                               (const TS *)gx_out, (const TS *)xs, (const TZ *)out_div, (const TZ *)in_mul,
                               (const float *)weight_f32, (int)n, (int)T, (int)C, (int)r, f.R, (int)cpr, (int)f.wpg, 1, eps,
                               row_map, distill_token ? 1 : 0, drop ? 1 : 0, (TS *)gx, (TG *)gx16, (float *)nullptr);
            return check_launch("k_merge_ln_rows_bwd_amp");
        };
        // (no scales: the fp32 form of the scale loads, which are never made)
        if (x_dtype == TOME_F32) return go(Dt<float>{}, Dt<float>{});
        return (scales && size_dtype == x_dtype) ? go(tg, tg) : go(tg, Dt<float>{});
    }, [&] { return not_16bit(who, gy_dtype, "gy"); });
}

// ------------------------------------------------------------------------------------------------
// partition matching (kernels in tome_partition.h): kth_bipartite_soft_matching (merge.py:105-158),
// random_bipartite_soft_matching (merge.py:161-212)
// ------------------------------------------------------------------------------------------------
extern "C" size_t tome_partition_workspace_bytes(int64_t n, int64_t Na, int64_t Nb, int64_t D) {
    if (n <= 0 || Na <= 0 || Nb <= 0 || D <= 0) return 0;
    return carve_sets(nullptr, n, Na, Nb, D, false).bytes;
}

// the two sets of a partition call, checked: k > 1 (the kth rule, Na / Nb must be what it gives) or k == 0 with two
// position lists
static int check_part_sets(const char *who, int64_t n, int64_t T, int64_t k, const int64_t *a_idx, const int64_t *b_idx,
                           int64_t Na, int64_t Nb, PartSets *S) {
    if (n <= 0 || T <= 0) return fail(TOME_EINVAL, "%s: bad shape", who);
    if (Nb <= 0) return fail(TOME_EINVAL, "%s: empty destination set (Nb=%lld)", who, (long long)Nb);
    if (Na <= 0) return fail(TOME_EINVAL, "%s: empty source set (Na=%lld)", who, (long long)Na);
    if (k != 0) {
        if (k <= 1) return fail(TOME_EINVAL, "%s: k=%lld (k > 1 expected, or k = 0 with a_idx / b_idx)", who, (long long)k);
        if (k > T || Nb != T / k || Na != (T / k) * (k - 1))
            return fail(TOME_EINVAL, "%s: k=%lld on T=%lld gives Na=%lld, Nb=%lld, not Na=%lld, Nb=%lld", who, (long long)k,
                        (long long)T, (long long)((T / k) * (k - 1)), (long long)(T / k), (long long)Na, (long long)Nb);
    } else {
        if (!a_idx || !b_idx) return fail(TOME_EINVAL, "%s: null a_idx / b_idx (and k = 0)", who);
        if (((uintptr_t)a_idx & 7) || ((uintptr_t)b_idx & 7)) return fail(TOME_EINVAL, "%s: misaligned a_idx / b_idx", who);
        if (Na + Nb > T) return fail(TOME_EINVAL, "%s: Na + Nb = %lld > T = %lld", who, (long long)(Na + Nb), (long long)T);
    }
    if (n * T > 0x7fffffffLL || n * (Nb + 1) > 0x7fffffffLL) return fail(TOME_EINVAL, "%s: too many rows", who);
    *S = PartSets{(int)k, (int)Na, (int)Nb, k ? nullptr : a_idx, k ? nullptr : b_idx};
    return TOME_OK;
}

extern "C" int tome_match_partition(const void *metric, int dtype, int64_t n, int64_t T, int64_t D, int64_t stride_n,
                                    int64_t stride_t, int64_t k, const int64_t *a_idx, const int64_t *b_idx,
                                    int64_t Na, int64_t Nb, int64_t *dst_idx, int32_t *offsets, int32_t *sources,
                                    void *workspace, size_t workspace_bytes, tome_stream_t stream) {
    if (!metric || D <= 0) return fail(TOME_EINVAL, "tome_match_partition: bad shape/pointer");
    PartSets S;
    if (int rc = check_part_sets("tome_match_partition", n, T, k, a_idx, b_idx, Na, Nb, &S)) return rc;
    if ((int64_t)n * T * ((D + 63) / 64 * 64) > (int64_t)1 << 40)
        return fail(TOME_EINVAL, "tome_match_partition: problem too large");
    if (!dst_idx || !offsets || !sources) return fail(TOME_EINVAL, "tome_match_partition: null output buffer");
    if (((uintptr_t)dst_idx & 7) || ((uintptr_t)offsets & 3) || ((uintptr_t)sources & 3))
        return fail(TOME_EINVAL, "tome_match_partition: misaligned output buffer");
    if (int rc = check_workspace("tome_match_partition", workspace, workspace_bytes,
                                 tome_partition_workspace_bytes(n, Na, Nb, D)))
        return rc;
    hipStream_t st = (hipStream_t)stream;
    const SetsWs w = carve_sets(workspace, n, Na, Nb, D, false);
    // 1. unit vectors of both sets
    const int64_t items = n * (Na + Nb);
    if (int rc = launch_unit_rows("tome_match_partition", dtype, rows_16byte(metric, dtype, D, stride_n, stride_t), w.nchunk,
                                  [&](auto ty, auto nch) {
        using TY = typename decltype(ty)::type;
        hipLaunchKernelGGL((k_unit_rows_part<TY, decltype(nch)::value>), dim3((unsigned)((items + 31) / 32)), dim3(256), 0,
                           st, (const TY *)metric, stride_n, stride_t, (int)n, (int)T, (int)D, S, w.unitA, w.unitB,
                           w.groupA_f4, w.groupB_f4, w.badA, w.badB);
    }, [&](auto ty) {
        using TY = typename decltype(ty)::type;
        hipLaunchKernelGGL((k_unit_rows_part_generic<TY>), dim3((unsigned)((items + 255) / 256)), dim3(256), 0, st,
                           (const TY *)metric, stride_n, stride_t, (int)n, (int)T, (int)D, w.nchunk * 64, S, w.unitA,
                           w.unitB, w.groupA_f4, w.groupB_f4, w.badA, w.badB);
    }))
        return rc;
    if (int rc = check_launch("k_unit_rows_part")) return rc;

    // 2. similarity + row max / argmax of the Na sources against the Nb destinations
    int WJ = 1;
    if (int rc = launch_scores_rowmax("tome_match_partition", w, n, (int)Na, (int)Nb, 0, st, &WJ)) return rc;

    // 3. fold the column parts -> dst_idx
    if (n > 65535) return fail(TOME_EINVAL, "tome_match_partition: more than 65535 groups");
    hipLaunchKernelGGL(k_part_fold, dim3((unsigned)((Na + 255) / 256), (unsigned)n), dim3(256), 0, st, w.part_max,
                       w.part_idx, WJ, (int)Na, (int)Nb, w.badA, w.badB, dst_idx);
    if (int rc = check_launch("k_part_fold")) return rc;

    // 4. inverted list; groups whose indices and counts fit 48 KiB of LDS take the LDS form
    const size_t lds = sizeof(int) * (size_t)(((Na + 3) & ~(int64_t)3) + Nb + 1);
    if (lds <= 48 * 1024)
        hipLaunchKernelGGL(k_part_lists<true>, dim3((unsigned)n), dim3(1024), lds, st, dst_idx, (int)Na, (int)Nb, offsets,
                           sources);
    else
        hipLaunchKernelGGL(k_part_lists<false>, dim3((unsigned)n), dim3(1024), 0, st, dst_idx, (int)Na, (int)Nb, offsets,
                           sources);
    return check_launch("k_part_lists");
}

template <typename TX, typename TS, int OP>
static int launch_merge_part(const void *x, const void *size, int64_t n, int64_t T, int64_t C, const PartSets &S,
                             const int32_t *offsets, const int32_t *sources, void *xout, void *sout, void *lsout,
                             hipStream_t st) {
    const int64_t rows = n * S.Nb;
    const unsigned nb = (unsigned)((rows + 3) / 4);
    return with_vec<TX>(C, x, xout, [&](auto vec) {
        hipLaunchKernelGGL((k_merge_part<TX, TS, decltype(vec)::value, OP>), dim3(nb), dim3(256), 0, st, (const TX *)x,
                           (const TS *)size, (int)n, (int)T, (int)C, S, offsets, sources, (TX *)xout, (TS *)sout,
                           (TS *)lsout);
        return check_launch("k_merge_part");
    });
}

static int check_part_merge_args(const char *who, const void *x, int64_t C, const void *out, const int32_t *offsets,
                                 const int32_t *sources) {
    if (!x || !out || C <= 0) return fail(TOME_EINVAL, "%s: bad shape/pointer", who);
    if (!offsets || !sources) return fail(TOME_EINVAL, "%s: null list buffer", who);
    if (((uintptr_t)offsets & 3) || ((uintptr_t)sources & 3)) return fail(TOME_EINVAL, "%s: misaligned list buffer", who);
    return TOME_OK;
}

extern "C" int tome_merge_partition(const void *x, int dtype, int64_t n, int64_t T, int64_t C, int64_t k,
                                    const int64_t *a_idx, const int64_t *b_idx, int64_t Na, int64_t Nb,
                                    const int32_t *offsets, const int32_t *sources, int mode, void *out,
                                    tome_stream_t stream) {
    if (int rc = check_part_merge_args("tome_merge_partition", x, C, out, offsets, sources)) return rc;
    PartSets S;
    if (int rc = check_part_sets("tome_merge_partition", n, T, k, a_idx, b_idx, Na, Nb, &S)) return rc;
    if (mode < TOME_SUM || mode > TOME_AMIN) return fail(TOME_EINVAL, "tome_merge_partition: mode %d", mode);
    return dispatch_x<true>(dtype, [&](auto tx) {
        auto go = [&](auto op) {
            return launch_merge_part<typename decltype(tx)::type, float, decltype(op)::value>(
                x, nullptr, n, T, C, S, offsets, sources, out, nullptr, nullptr, (hipStream_t)stream);
        };
        switch (mode) {
        case TOME_SUM: return go(Op<TOME_SUM>{});
        case TOME_MEAN: return go(Op<TOME_MEAN>{});
        case TOME_AMAX: return go(Op<TOME_AMAX>{});
        case TOME_PROD: return go(Op<TOME_PROD>{});
        default: return go(Op<TOME_AMIN>{});  // (mode range checked above)
        }
    }, [&] { return fail(TOME_EINVAL, "tome_merge_partition: dtype %d", dtype); });
}

extern "C" int tome_merge_wavg_partition(const void *x, int x_dtype, const void *size, int size_dtype, int64_t n,
                                         int64_t T, int64_t C, int64_t k, const int64_t *a_idx, const int64_t *b_idx,
                                         int64_t Na, int64_t Nb, const int32_t *offsets, const int32_t *sources,
                                         void *x_out, void *size_out, void *log_size_out, tome_stream_t stream) {
    if (int rc = check_part_merge_args("tome_merge_wavg_partition", x, C, x_out, offsets, sources)) return rc;
    if (!size_out) return fail(TOME_EINVAL, "tome_merge_wavg_partition: null buffer");
    PartSets S;
    if (int rc = check_part_sets("tome_merge_wavg_partition", n, T, k, a_idx, b_idx, Na, Nb, &S)) return rc;
    return dispatch_xs<true>(x_dtype, size_dtype, [&](auto tx, auto ts) {
        return launch_merge_part<typename decltype(tx)::type, typename decltype(ts)::type, OP_WAVG>(
            x, size, n, T, C, S, offsets, sources, x_out, size_out, log_size_out, (hipStream_t)stream);
    }, [&] { return fail(TOME_EINVAL, "tome_merge_wavg_partition: unsupported dtypes x=%d size=%d", x_dtype, size_dtype); });
}

template <typename TX>
static int launch_unmerge_part(const void *x, int64_t n, int64_t T, int64_t Tout, int64_t C, const PartSets &S,
                               const int64_t *dst, void *out, hipStream_t st) {
    const int64_t items = n * ((int64_t)S.Na + S.Nb);
    const unsigned nb = (unsigned)((items + 3) / 4);
    return with_vec<TX>(C, x, out, [&](auto vec) {
        hipLaunchKernelGGL((k_unmerge_part<TX, decltype(vec)::value>), dim3(nb), dim3(256), 0, st, (const TX *)x, (int)n,
                           (int)T, (int)Tout, (int)C, S, dst, (TX *)out);
        return check_launch("k_unmerge_part");
    });
}

extern "C" int tome_unmerge_partition(const void *x, int dtype, int64_t n, int64_t T, int64_t C, int64_t k,
                                      const int64_t *a_idx, const int64_t *b_idx, int64_t Na, int64_t Nb,
                                      const int64_t *dst_idx, void *out, tome_stream_t stream) {
    if (!x || !out || C <= 0) return fail(TOME_EINVAL, "tome_unmerge_partition: bad shape/pointer");
    if (!dst_idx || ((uintptr_t)dst_idx & 7)) return fail(TOME_EINVAL, "tome_unmerge_partition: null or misaligned dst_idx");
    PartSets S;
    if (int rc = check_part_sets("tome_unmerge_partition", n, T, k, a_idx, b_idx, Na, Nb, &S)) return rc;
    const int64_t Tout = k ? (T / k) * k : T;
    return dispatch_x<true>(dtype, [&](auto tx) {
        return launch_unmerge_part<typename decltype(tx)::type>(x, n, T, Tout, C, S, dst_idx, out, (hipStream_t)stream);
    }, [&] { return fail(TOME_EINVAL, "tome_unmerge_partition: dtype %d", dtype); });
}

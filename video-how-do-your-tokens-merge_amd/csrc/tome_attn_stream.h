// tome_attn_stream.h -- k_prop_attention_stream: the attention of tome_attn.h as PERSISTENT workgroups that carry the
// K/V pipeline across query blocks.
//
// Why (tools/attn_diag.py, phase stamps of k_prop_attention at 128 x 12 x 1536, MI355X): a 256-query block spends
// 22.9 us in its 23 pipelined tile steps and 7 us around them -- 0.4 us index arithmetic + Q fetch, 2.5 us for the
// first K/V tile to reach LDS (two memory round trips in a row), 0.7 us first tile's softmax, 1.9 us last product,
// normalisation and stores, 1.5 us until the next workgroup starts on the CU (one 8-wave workgroup per CU: nothing
// overlaps these).  The tile loop itself runs at 1.17 PFLOP/s; the block as a whole at 0.85.
//
// Here one workgroup per CU walks items L = blockIdx.x, + gridDim.x, ... (item = (batch, head, segment, query block),
// same XCD-aware numbering as k_prop_attention) and never drains its pipeline between two of them:
//   * the staging stream (tile t+2 requested while tile t+1 is multiplied) runs on into the NEXT item's first two
//     tiles during the current item's last two steps;
//   * the next item's Q rows are requested when the last softmax of the current item has freed its registers;
//   * the step between two items ("switch") = last product, normalisation, stores (left in flight) + stage + ONE
//     barrier + the new item's first-tile softmax;
//   * the overflow guard of the first-pass softmax is settled inside the wave, tile by tile (see fast_step): no
//     workgroup-wide repeat of the block, hence no second code path through the whole item.
// The ring slot of a tile is (tiles streamed so far) & 1 -- a run-time value here (tiles per item may be odd).
// Everything else -- fragment layouts, the first-pass softmax against the first tile's reference point with the
// accumulators started at -m, the overflow guard with the general-path repeat, masked last tile, segments -- is
// k_prop_attention's, and both kernels call the same device functions for it (tome_attn_tile.h): item numbering, q~,
// the score and PV products, the fast step's weights, the general softmax, the output exchange.
//
// Needs at least two key tiles (Nk > 64) and eight waves; the host takes k_prop_attention otherwise.
#pragma once
#include "tome_attn.h"

#ifdef ATT_DIAG
// (diagnostic build: the third item of every workgroup stamps its phases)
#define ATS_STAMP(i)                                                                                       \
    do {                                                                                                   \
        if (diag_n == 2 && blockIdx.x < ATT_DIAG_WGS) {                                                    \
            const unsigned long long st_ = __builtin_amdgcn_s_memrealtime();                               \
            if (lane == 0) g_att_stamps[((size_t)blockIdx.x * 8 + wave) * ATT_DIAG_N + (i)] = st_;          \
        }                                                                                                  \
    } while (0)
#else
#define ATS_STAMP(i)
#endif

#define ATS_BIAS_GROUP 4  // tiles per bias load (power of two; 2 * GROUP * 64 words of LDS)
// Two forms.  PAIR = false: 208-221 registers, one workgroup per CU, a software pipeline inside the wave (tile t's
// scores and weights around tile t-1's PV product).  PAIR = true: held to 128 registers (__launch_bounds__(512, 4):
// four waves per SIMD) so that TWO workgroups share a CU -- four waves per SIMD from two unrelated barriers, one
// workgroup's softmax under the other's MFMAs.  What gives the registers back:
//   * no start values -m (16 registers): the scores start at the constant 0 and -m_ref rides on the matrix pipe, two
//     channels of the extra k-step that the bias already takes (ref_step; att_split16) -- the reference point IS what
//     those two channels carry, the first tile's and the general path's weights are taken against the same value;
//   * no V fragments held from one step to the next (16): a tile's PV product is taken in the step that staged it,
//     each fragment read right before its MFMA pair (a slot is only safe to read in the step that wrote it), so
//     nothing of tile t-1 is live while tile t's scores are formed either (packed P: 8).
template <typename TX, bool BIAS, bool PAIR>
__global__ __launch_bounds__(512, PAIR ? 4 : 2) void k_prop_attention_stream(AttnArgs a, int nitems) {
    constexpr int WAVES = 8;
    constexpr int ATT_BM = 32 * WAVES;
    __shared__ __attribute__((aligned(16))) short lds_k[ATT_SLOTS][ATT_BN * ATT_KS];
    __shared__ __attribute__((aligned(16))) short lds_v[ATT_SLOTS][ATT_BN * ATT_VS];
    __shared__ __attribute__((aligned(16))) unsigned lds_bias[2][ATS_BIAS_GROUP * ATT_BN];  // BIAS: (hi | lo << 16) per key, see bias_step()
    __shared__ __attribute__((aligned(16))) short lds_o[WAVES][32 * ATT_KS];  // a wave's output block on its way out

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);

    const int col = lane & 31, hf = lane >> 5;
    const int qblocks = (a.N + ATT_BM - 1) / ATT_BM;
    const int nbhs = a.B * a.H * a.nseg;
    const int G = gridDim.x;  // a multiple of 8: item L and item L + G belong to one XCD's group
    const int ntiles = (a.Nk + ATT_BN - 1) / ATT_BN;  // >= 2 (host)
    const int nfull = a.Nk / ATT_BN;
    const bool last_half = (ntiles - 1) * ATT_BN + 32 >= a.Nk;  // the last tile holds at most 32 keys
    const float LOG2E = 1.4426950408889634f;
    const float sl = a.scale * LOG2E;
    // The arguments that only the step between two items reads (strides, base pointers) are read again from the
    // kernel-argument segment there (scalar loads, cached) instead of living in ~50 scalar registers across the tile
    // loop: kept live they push the kernel past the 102-SGPR budget, and the spills go through vector registers.
    typedef const __attribute__((address_space(4))) AttnArgs *AttnArgsK;
    const AttnArgsK kargs = (AttnArgsK)__builtin_amdgcn_kernarg_segment_ptr();
    auto fresh = [&]() __attribute__((always_inline)) -> AttnArgsK {
        AttnArgsK p = kargs;
        asm volatile("" : "+s"(p));  // opaque: the loads behind it are not merged with earlier ones
        return p;
    };
    const int nseg = a.nseg, nheads = a.H, nq = a.N, nk = a.Nk, bias_skip = a.bias_skip;
    const int64_t k_tile = (int64_t)ATT_BN * a.k_sn * 2, v_tile = (int64_t)ATT_BN * a.v_sn * 2;  // bytes per tile

    // ---- item numbering (k_prop_attention's): the query blocks of one (batch, head, segment) -> ids congruent mod 8
    struct Item { int b, h, seg, qb; };
    auto item_ok = [&](int L) -> bool {
        int bhs, qb;
        return L < nitems && att_item(L, qblocks, nbhs, bhs, qb);
    };
    auto decode = [&](int L) -> Item {
        int bhs;
        Item it;
        att_item(L, qblocks, nbhs, bhs, it.qb);
        const int bh = bhs / nseg;
        it.seg = bhs - bh * nseg;
        it.b = bh / nheads;
        it.h = bh % nheads;
        return it;
    };

    // ---- staging: thread -> row r0, 16-byte column c0 of the 64 x 64 K and V tiles; byte offsets from the tile's
    // first row are per-thread constants (the rows of the partly filled last tile clamped to its last key: no bounds
    // branch, those keys' weights are masked)
    const int r0 = tid >> 3, c0 = tid & 7;
    const int rp = min(r0, max(nk - nfull * ATT_BN, 1) - 1);
    // (32-bit: 64 rows of at most 2^24 elements -- the host checks the strides)
    const unsigned koff = (unsigned)(((int64_t)r0 * a.k_sn + 8 * c0) * 2), koff_p = (unsigned)(((int64_t)rp * a.k_sn + 8 * c0) * 2);
    const unsigned voff = (unsigned)(((int64_t)r0 * a.v_sn + 8 * c0) * 2), voff_p = (unsigned)(((int64_t)rp * a.v_sn + 8 * c0) * 2);
#define ATS_TID_AGAIN(t)                        \
    int t = tid;                                \
    asm volatile("" : "+v"(t))
    // PAIR: a slot's offset kept a scalar (folded into the address arithmetic it becomes a multiply-add whose constant
    // needs a vector register of its own, one per stride, through the whole loop)
    auto slot_off = [&](int o) __attribute__((always_inline)) -> int {
        return __builtin_amdgcn_readfirstlane(o);
    };
    uint4 kreg, vreg;
    unsigned breg = 0u;
    int r_sub = 0, b_par = 0, b_off = 0;  // BIAS: the staged tile's place in its group, the group buffer in use
    // The stream: the next tile to request is tile s_t of item s_item and starts at s_kt / s_vt (bias row: s_ls).
    // n_q / n_o / n_qb: where that item's query block and output block start -- once the stream has moved on to the
    // item after the one being computed (two steps before the switch) these describe the computing side's NEXT item.
    const char *s_kt = nullptr, *s_vt = nullptr;
    const float *s_ls = nullptr;
    int s_t = 0, s_item = 0;
    const short *n_q = nullptr;
    short *n_o = nullptr;
    int n_qb = 0;
    auto stream_set = [&](int L) __attribute__((always_inline)) {
        const Item it = decode(L);
        const AttnArgsK A = fresh();
        s_kt = reinterpret_cast<const char *>(reinterpret_cast<const short *>(A->k) + it.b * A->k_sb + it.h * A->k_sh + it.seg * A->k_seg);
        s_vt = reinterpret_cast<const char *>(reinterpret_cast<const short *>(A->v) + it.b * A->v_sb + it.h * A->v_sh + it.seg * A->v_seg);
        if (BIAS) s_ls = A->log_size + it.b * A->ls_sb + it.seg * A->ls_seg;
        n_q = reinterpret_cast<const short *>(A->q) + it.b * A->q_sb + it.h * A->q_sh + (int64_t)it.qb * ATT_BM * A->q_sn;
        n_o = reinterpret_cast<short *>(A->out) + it.b * A->o_sb + it.h * A->o_sh + it.seg * A->o_seg + (int64_t)it.qb * ATT_BM * A->o_sn;
        n_qb = it.qb;
        s_item = L;
        s_t = 0;
    };
    // request the stream's next tile and move on (past the last item the stream repeats its last tile: valid memory,
    // never used)
    auto stream_load = [&]() __attribute__((always_inline)) {
        const bool part = s_t >= nfull;  // wave-uniform
        if constexpr (PAIR) {
            // (the four offsets above and the two LDS addresses below, formed again from the thread number in every
            // step: ~10 vector instructions against six registers held through the tile loop)
            ATS_TID_AGAIN(t);
            const unsigned r = min(t >> 3, (part ? max(nk - nfull * ATT_BN, 1) : ATT_BN) - 1), c16 = 16 * (t & 7);
            kreg = *reinterpret_cast<const uint4 *>(s_kt + (r * (unsigned)(k_tile >> 6) + c16));
            vreg = *reinterpret_cast<const uint4 *>(s_vt + (r * (unsigned)(v_tile >> 6) + c16));
        } else {
            kreg = *reinterpret_cast<const uint4 *>(s_kt + (part ? koff_p : koff));
            vreg = *reinterpret_cast<const uint4 *>(s_vt + (part ? voff_p : voff));
        }
        // BIAS: the per-key term of ATS_BIAS_GROUP tiles at a time, one key per thread -- staging it tile by tile
        // put ~25 instructions per step on wave 0 alone, and every wave waits for the slowest at the barrier
        // (measured: 10 % of the kernel)
        r_sub = s_t & (ATS_BIAS_GROUP - 1);
        if (BIAS && r_sub == 0 && tid < ATS_BIAS_GROUP * ATT_BN) {
            const int key = min(s_t * ATT_BN + tid, nk - 1);
            // log2-domain bias as two 16-bit terms hi + lo (what is left is below 2^-15 of the bias for bf16)
            const float bv = key >= bias_skip ? s_ls[key - bias_skip] * LOG2E : 0.0f;
            const short bh = att_bits<TX>(bv);
            TX th;
            __builtin_memcpy(&th, &bh, 2);
            const short bl = att_bits<TX>(bv - to_f32(th));
            breg = (unsigned)(unsigned short)bh | ((unsigned)(unsigned short)bl << 16);
        }
        if (++s_t == ntiles) {
            if (item_ok(s_item + G)) stream_set(s_item + G);
            else s_t = ntiles - 1;
        } else {
            s_kt += k_tile;
            s_vt += v_tile;
        }
    };
    short *const wk = &lds_k[0][0] + r0 * ATT_KS + 8 * c0, *const wv = &lds_v[0][0] + r0 * ATT_VS + 8 * c0;
    auto stage_write = [&](int S) __attribute__((always_inline)) {
        if constexpr (PAIR) {
            ATS_TID_AGAIN(t);
            *reinterpret_cast<uint4 *>(&lds_k[0][0] + slot_off(S * ATT_BN * ATT_KS) + (t >> 3) * ATT_KS + 8 * (t & 7)) = kreg;
            *reinterpret_cast<uint4 *>(&lds_v[0][0] + slot_off(S * ATT_BN * ATT_VS) + (t >> 3) * ATT_VS + 8 * (t & 7)) = vreg;
        } else {
            *reinterpret_cast<uint4 *>(wk + S * ATT_BN * ATT_KS) = kreg;
            *reinterpret_cast<uint4 *>(wv + S * ATT_BN * ATT_VS) = vreg;
        }
        if (BIAS) {  // (wave-uniform) a tile that opens a group brings the group's bias words along
            if (r_sub == 0) {
                b_par ^= 1;
                if (tid < ATS_BIAS_GROUP * ATT_BN) lds_bias[b_par][tid] = breg;
            }
            b_off = b_par * (ATS_BIAS_GROUP * ATT_BN) + r_sub * ATT_BN;  // where the tile now in slot S finds its words
        }
    };

    // ---- per-item state of the computing side
    const int lrow0 = wave * 32 + col;  // this lane's query row inside a block
    const int q_sn = (int)a.q_sn, o_sn = (int)a.o_sn;  // (< 2^24: host)
    // PAIR: what only the step between two items computes from the lane number (Q and output addresses, row numbers)
    // starts from an opaque copy of it there: hoisted out of the item loop, those ~20 values per lane would have to
    // live through the tile loop, where there is no register for them
#define ATS_LANE_AGAIN(l)                       \
    int l = lane;                               \
    if constexpr (PAIR) asm volatile("" : "+v"(l))
    int c_qb = 0;             // the item's query block
    short *c_o = nullptr;     // where its output block starts
    int qrow = 0;
    bool active = false;
    float bfac = 1.0f;
    att_s16x8 qf[4];
    uint4 qraw[4];
    // request the Q rows of the stream's item (the computing side's NEXT item) and note where its output goes --
    // before the stream moves on; item_take then makes it the current item
    int t_qb = 0;
    short *t_o = nullptr;
    auto q_request = [&]() __attribute__((always_inline)) {
        t_qb = n_qb;
        t_o = n_o;
        ATS_LANE_AGAIN(ln);
        const int lrow = max(min(PAIR ? wave * 32 + (ln & 31) : lrow0, nq - 1 - t_qb * ATT_BM), 0);
        const short *qp = n_q + lrow * q_sn + 8 * (PAIR ? ln >> 5 : hf);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) qraw[ks] = *reinterpret_cast<const uint4 *>(qp + 16 * ks);
    };
    auto item_take = [&]() __attribute__((always_inline)) {
        c_qb = t_qb;
        c_o = t_o;
        ATS_LANE_AGAIN(ln);
        qrow = c_qb * ATT_BM + (PAIR ? wave * 32 + (ln & 31) : lrow0);
        active = c_qb * ATT_BM + wave * 32 < nq;  // wave-uniform
        bfac = (bias_skip && qrow == 0) ? 0.0f : 1.0f;
    };
    auto q_convert = [&]() __attribute__((always_inline)) {  // q * scale * log2(e), rounded once to the 16-bit format
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            att_s16x8 raw;
            __builtin_memcpy(&raw, &qraw[ks], 16);
            qf[ks] = att_scaled<TX>(raw, PAIR ? fresh()->scale * LOG2E : sl);
        }
    };

    att_f32x16 o0, o1, negm, s0, s1;
    float m_run = -INFINITY, l_run = 0.0f;
#ifdef ATT_DIAG
    int diag_n = 0;
    unsigned long long diag_wait_stage = 0, diag_wait_barrier = 0;
#endif
    auto item_reset = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int v = 0; v < 16; ++v) o0[v] = o1[v] = negm[v] = 0.0f;
        m_run = -INFINITY;
        l_run = 0.0f;
    };

    // ---- fragments and products (tome_attn.h's layouts; the slot is a run-time value)
    const short *const vbase = att_tr_base(&lds_v[0][0], lane, 0);
    att_s16x4 vfr[2][2][4];
    auto v_fragments = [&](int S) __attribute__((always_inline)) { att_tr_read_tile(vbase + S * ATT_BN * ATT_VS, vfr); };
    // BIAS: the per-key term rides on the matrix pipe as a fifth k-step of the score product -- K gets two more
    // "channels" (hi, lo of the bias), Q gets bfac in both -- instead of 32 fma + 8 wide LDS reads per tile on the
    // vector pipe; the lanes of the upper half (channels 8..15 of that k-step) hold zeros
    auto bias_step = [&](int S) __attribute__((always_inline)) {
        const unsigned w0 = lds_bias[0][b_off + col], w1 = lds_bias[0][b_off + 32 + col];
        const unsigned one = (unsigned)(unsigned short)att_bits<TX>(bfac);
        const unsigned qw = hf ? 0u : (one | (one << 16));
        const uint4 q5 = make_uint4(qw, 0u, 0u, 0u), k0 = make_uint4(hf ? 0u : w0, 0u, 0u, 0u), k1 = make_uint4(hf ? 0u : w1, 0u, 0u, 0u);
        att_s16x8 fq, f0, f1;
        __builtin_memcpy(&fq, &q5, 16);
        __builtin_memcpy(&f0, &k0, 16);
        __builtin_memcpy(&f1, &k1, 16);
        s0 = AttMfma<TX>::run(f0, fq, s0);
        s1 = AttMfma<TX>::run(f1, fq, s1);
    };
    // PAIR: that k-step also brings the reference point -- channels 0, 1 as above (BIAS), the next two channels K side
    // 1, Q side qref = -m_ref as hi | lo << 16 (0 while a softmax looks for its maximum).  Without a bias the step
    // exists for the reference point alone: 2 MFMAs per tile on the pipe that is not binding.
    unsigned qref = 0u;
    auto ref_set = [&](float m) __attribute__((always_inline)) -> float {  // -> the reference point the step carries
        float carried;
        const unsigned w = att_split16<TX>(-m, carried);
        qref = w;
        return -carried;
    };
    auto ref_step = [&](unsigned ref, bool first_half_only, int col, int hf) __attribute__((always_inline)) {
        ref = hf ? 0u : ref;
        const unsigned one = (unsigned)(unsigned short)att_bits<TX>(1.0f), ones = hf ? 0u : (one | (one << 16));
        uint4 q5, k0, k1;
        if (BIAS) {
            const unsigned w0 = lds_bias[0][b_off + col], w1 = lds_bias[0][b_off + 32 + col];
            const unsigned bf = (unsigned)(unsigned short)att_bits<TX>(bfac);
            q5 = make_uint4(hf ? 0u : (bf | (bf << 16)), ref, 0u, 0u);
            k0 = make_uint4(hf ? 0u : w0, ones, 0u, 0u);
            k1 = make_uint4(hf ? 0u : w1, ones, 0u, 0u);
        } else {
            q5 = make_uint4(ref, 0u, 0u, 0u);
            k0 = k1 = make_uint4(ones, 0u, 0u, 0u);
        }
        att_s16x8 fq, f0, f1;
        __builtin_memcpy(&fq, &q5, 16);
        __builtin_memcpy(&f0, &k0, 16);
        __builtin_memcpy(&f1, &k1, 16);
        s0 = AttMfma<TX>::run(f0, fq, s0);
        if (!first_half_only) s1 = AttMfma<TX>::run(f1, fq, s1);
    };
    auto scores = [&](int S, const att_f32x16 &cinit, bool first_half_only) __attribute__((always_inline)) {
        const short *kt = &lds_k[0][0] + S * ATT_BN * ATT_KS;
        s0 = cinit;
        s1 = cinit;
        if (BIAS) bias_step(S);
        att_rows_block<TX>(kt, col, hf, 0, qf, s0);
        if (!first_half_only) att_rows_block<TX>(kt, col, hf, 1, qf, s1);
    };
    // PAIR: the scores of the tile in slot S minus the reference point in `ref` (qref, or 0), from the constant 0
    auto scores_ref = [&](int S, unsigned ref, bool first_half_only) __attribute__((always_inline)) {
        ATS_LANE_AGAIN(ln);  // (the lane's place in the fragments formed again: see q_request)
        const int col = ln & 31, hf = ln >> 5;
        const short *kt = &lds_k[0][0] + slot_off(S * ATT_BN * ATT_KS);
#pragma unroll
        for (int v = 0; v < 16; ++v) s0[v] = s1[v] = 0.0f;
        ref_step(ref, first_half_only, col, hf);
        att_rows_block<TX>(kt, col, hf, 0, qf, s0);
        if (!first_half_only) att_rows_block<TX>(kt, col, hf, 1, qf, s1);
    };
    att_s16x8 pf[2][2];
    // general softmax of tile t from scores that start at zero: range mask, maximum, rescale of O and l
    auto general_softmax = [&](int t, int S) __attribute__((always_inline)) {
        if constexpr (PAIR) {
            scores_ref(S, 0u, false);
            ATS_LANE_AGAIN(ln);
            att_general_softmax_at<TX>(s0, s1, t * ATT_BN + 4 * (ln >> 5), nk, m_run, l_run, o0, o1, pf, ref_set);
        } else {
            att_f32x16 zero;
#pragma unroll
            for (int v = 0; v < 16; ++v) zero[v] = 0.0f;
            scores(S, zero, false);
            att_general_softmax<TX>(s0, s1, t * ATT_BN + 4 * hf, nk, m_run, l_run, o0, o1, negm, pf);
        }
    };
    // the first tile of an item (full: an item has at least two tiles): nothing to rescale, nothing to mask --
    // m = the tile's row maximum, P = exp2(s - m), l = the row sum
    auto first_softmax = [&](int S) __attribute__((always_inline)) {
        if constexpr (PAIR) {
            scores_ref(S, 0u, false);
        } else {
            att_f32x16 zero;
#pragma unroll
            for (int v = 0; v < 16; ++v) zero[v] = 0.0f;
            scores(S, zero, false);
        }
        float mt = fmaxf(s0[0], s1[0]);
#pragma unroll
        for (int v = 1; v < 16; ++v) mt = fmaxf(mt, fmaxf(s0[v], s1[v]));
        mt = att_half_max(mt);
        if constexpr (PAIR) mt = ref_set(mt);  // (the value the later tiles' scores will have had subtracted)
        float lsum = 0.0f;
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            s0[v] = __builtin_amdgcn_exp2f(s0[v] - mt);
            s1[v] = __builtin_amdgcn_exp2f(s1[v] - mt);
            lsum += s0[v] + s1[v];
        }
        l_run = lsum;
        m_run = mt;
#pragma unroll
        for (int v = 0; v < 16; ++v) negm[v] = -mt;
        att_pack_tile<TX>(s0, s1, pf);
    };
    auto pv = [&](bool first_half_only) __attribute__((always_inline)) {
        att_tr_mfma_tile<TX>(vfr, pf, first_half_only, o0, o1);
    };
    // PAIR: O += V P of the tile in slot S, in the step that staged it
    auto pv_slot = [&](int S, bool first_half_only) __attribute__((always_inline)) {
        ATS_LANE_AGAIN(ln);
        att_tr_tile_product<TX>(att_tr_base(&lds_v[0][0], ln, 0) + slot_off(S * ATT_BN * ATT_VS), pf, first_half_only, o0, o1);
    };
    // PAIR: one step inside an item, nothing carried from the step before but O, l and the reference point: tile tn ->
    // slot S, the stream's next tile requested, ONE barrier, S(tn) - m_ref, P(tn), the guard, O += V(tn) P(tn)
    auto pair_step = [&](int S, int tn, bool masked) __attribute__((always_inline)) {
        stage_write(S);
        stream_load();
        __syncthreads();
        // (priority on the score product, not on the weights as in fast_step: with four waves on the SIMD the wave
        // that has just passed its barrier gets its reads and MFMAs in first and the others' softmax fills in behind
        // -- measured at 384 x 12 x 1568 with the bias: 3.64 ms against 3.73 with the priority on the weights, 3.70
        // with none)
        __builtin_amdgcn_s_setprio(1);
        scores_ref(S, qref, masked && last_half);
        __builtin_amdgcn_s_setprio(0);
        ATS_LANE_AGAIN(ln);
        const float lsum = att_fast_weights<TX>(s0, s1, masked, tn * ATT_BN + 4 * (ln >> 5), nk, pf);
        const float l_before = l_run;
        l_run += lsum;
#ifndef ATS_NOGUARD
        if (__builtin_amdgcn_ballot_w64(!(lsum <= AttLimit<TX>::value)) != 0) {  // (fast_step's guard)
            l_run = l_before;
            general_softmax(tn, S);
        }
#endif
        pv_slot(S, masked && last_half);
    };
    // one pipelined step inside an item: tile tn (in the staging registers) -> slot S, the stream's next tile
    // requested, ONE barrier, S(tn) and O += V(tn-1) P(tn-1), then P(tn) against the item's reference point
    auto fast_step = [&](int S, int tn, bool masked) __attribute__((always_inline)) {
#ifdef ATT_DIAG
        // (diagnostic build: how long does a step wait for the tile it requested one step ago, and at the barrier?)
        unsigned long long d0_ = 0, d1_ = 0, d2_ = 0;
        if (diag_n == 2) d0_ = __builtin_amdgcn_s_memrealtime();
#endif
        stage_write(S);
#ifdef ATT_DIAG
        if (diag_n == 2) {
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
            d1_ = __builtin_amdgcn_s_memrealtime();
        }
#endif
        stream_load();
        __syncthreads();
#ifdef ATT_DIAG
        if (diag_n == 2) {
            d2_ = __builtin_amdgcn_s_memrealtime();
            diag_wait_stage += d1_ - d0_;
            diag_wait_barrier += d2_ - d1_;
        }
#endif
        scores(S, negm, masked && last_half);
        pv(false);
        v_fragments(S);
        __builtin_amdgcn_s_setprio(1);
        const float lsum = att_fast_weights<TX>(s0, s1, masked, tn * ATT_BN + 4 * hf, nk, pf);
        __builtin_amdgcn_s_setprio(0);
        const float l_before = l_run;
        l_run += lsum;
        // Overflow guard, at the very end of the step (a branch in the middle of it keeps the compiler from
        // interleaving the conversions with what follows: +10 % per step, measured): a row sum beyond the 16-bit
        // format's range (or inf / NaN) says the reference point lags the scores by more than the format allows.
        // The WAVE then takes this tile again on the general path -- its K tile is still in slot S, O and l hold the
        // tiles before it -- which moves the reference point to the new maximum; the following tiles continue on
        // the fast path against it.  (Wave-uniform branch, adversarial inputs only; k_prop_attention repeats the
        // whole block instead.)
#ifndef ATS_NOGUARD
        if (__builtin_amdgcn_ballot_w64(!(lsum <= AttLimit<TX>::value)) != 0) {
            l_run = l_before;
            general_softmax(tn, S);
        }
#endif
    };
    auto helper_step = [&](int S) __attribute__((always_inline)) {  // a wave without queries stages and meets the barrier
        stage_write(S);
        stream_load();
        __syncthreads();
    };
    // out[b, q, h*64 + d] = O^T[d][q] / l.  A lane holds 4 x 8 channels of ONE query row; stored from there, one store
    // instruction touches 32 rows x 2 x 16 bytes and the eight waves' stores queue up behind each other (measured:
    // waves 4-7 spend 2.2 us here, waves 0-3 0.7).  So the wave's 32 x 64 block goes through a region of LDS of its
    // own (row stride 144 B, the K tile's conflict-free stride) and leaves as whole 128-byte rows: 8 rows per store
    // instruction.  LDS operations of one wave execute in order: no barrier.
    auto store_item = [&]() __attribute__((always_inline)) {
        const float l_tot = PAIR ? att_half_sum(l_run) : l_run + __shfl_xor(l_run, 32);
        const float inv = __builtin_amdgcn_rcpf(l_tot);  // (1 ulp; the result is rounded to 8 or 11 bits)
        ATS_LANE_AGAIN(ln);  // (PAIR: see q_request; the other form keeps the values it holds)
#define ATS_SI_LANE (PAIR ? ln : lane)
        short *ow = &lds_o[0][0] + wave * (32 * ATT_KS);
        // (att_store_row's exchange: the lower lanes end up with channels 8g .. 8g+7, the upper with 32+8g .. 32+8g+7)
        att_store_row<TX>(ow + (PAIR ? ln & 31 : col) * ATT_KS + 32 * (PAIR ? ln >> 5 : hf), true, o0, o1, inv);
        const int rows = nq - c_qb * ATT_BM - wave * 32;  // rows of this wave inside the sequence (>= 1: active)
        short *op = c_o + (wave * 32 + (ATS_SI_LANE >> 3)) * o_sn + 8 * (ATS_SI_LANE & 7);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint4 row16 = *reinterpret_cast<const uint4 *>(ow + ((ATS_SI_LANE >> 3) + 8 * i) * ATT_KS + 8 * (ATS_SI_LANE & 7));
            if ((ATS_SI_LANE >> 3) + 8 * i < rows) *reinterpret_cast<uint4 *>(op + 8 * i * o_sn) = row16;
        }
#undef ATS_SI_LANE
    };
    // first item of a workgroup: nothing is in flight yet
    auto cold_start = [&](int L) __attribute__((always_inline)) {
        stream_set(L);
        q_request();    // Q rows requested first,
        item_take();
        item_reset();
        stream_load();  // tile 0 behind them, before anything waits
        q_convert();
        stage_write(0);
        stream_load();  // tile 1
        __syncthreads();
        if (active) {
            first_softmax(0);
            if constexpr (PAIR) pv_slot(0, false);
            else v_fragments(0);
        }
    };

    int item = blockIdx.x;
    if (!item_ok(item)) return;  // (then so is every later item of this workgroup)
    cold_start(item);
    int par = 0;  // ring slot of the current item's tile 0
    for (;;) {
        ATS_STAMP(0);  // tile loop starts
        // ---- steps inside the item: tiles 1 .. ntiles-1 (tile tn -> slot (par + tn) & 1)
        if (active) {
            int tn = 1;
            if constexpr (PAIR) {
                for (; tn < nfull; ++tn) pair_step((par + tn) & 1, tn, false);
                if (tn < ntiles) pair_step((par + tn) & 1, tn, true);
            } else {
                for (; tn < nfull; ++tn) fast_step((par + tn) & 1, tn, false);
                if (tn < ntiles) fast_step((par + tn) & 1, tn, true);  // the partly filled last tile
            }
        } else {
            for (int tn = 1; tn < ntiles; ++tn) helper_step((par + tn) & 1);
        }
        ATS_STAMP(1);  // tile loop done
#ifdef ATT_DIAG
        if (diag_n == 2 && blockIdx.x < ATT_DIAG_WGS && lane == 0) {
            g_att_stamps[((size_t)blockIdx.x * 8 + wave) * ATT_DIAG_N + 6] = diag_wait_stage;
            g_att_stamps[((size_t)blockIdx.x * 8 + wave) * ATT_DIAG_N + 7] = diag_wait_barrier;
        }
#endif
        // ---- switch: the staging registers hold the next item's tile 0 (if there is a next item).  Order: everything
        // that READS memory for the next item is issued first (its tile 0 to LDS, its Q rows, its tile 1), then the
        // current item's last product, normalisation and stores -- a wait for any of those loads then never waits
        // for the stores behind them (the vector-memory counter runs in order).  The two arms of `active` each hold
        // the barrier, so that the wait counts in front of it stay exact on both.
        const int next = item + G;
        const bool has_next = item_ok(next);  // workgroup-uniform
        const int Sn = (par + ntiles) & 1;
        if constexpr (PAIR) {
            // (the last item leaves here: behind this point the compiler knows that the Q rows requested below are
            // the only ones alive -- left to the two `has_next` tests further down it carries the previous item's 16
            // raw Q registers through the whole tile loop)
            if (!has_next) {
                if (active) store_item();
                return;
            }
        }
        if (has_next) {
            stage_write(Sn);
            q_request();    // (the stream is at the next item since two steps)
            stream_load();  // the next item's tile 1
        }
        const bool was_active = active;
        if (was_active) {
            if constexpr (!PAIR) pv(last_half);
            store_item();
            ATS_STAMP(2);  // stores issued
            if (!has_next) return;
            __syncthreads();
            ATS_STAMP(3);  // behind the barrier
        } else {
            if (!has_next) return;
            __syncthreads();
        }
        item = next;
        par = Sn;
        item_take();
        item_reset();
        q_convert();
        ATS_STAMP(4);  // Q fragment ready
        if (active) {
            first_softmax(Sn);
            if constexpr (PAIR) pv_slot(Sn, false);
            else v_fragments(Sn);
        }
        ATS_STAMP(5);  // first tile's weights
#ifdef ATT_DIAG
        ++diag_n;
#endif
    }
}
#undef ATS_LANE_AGAIN
#undef ATS_TID_AGAIN

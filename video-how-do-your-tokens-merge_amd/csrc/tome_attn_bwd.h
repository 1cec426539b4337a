// tome_attn_bwd.h -- backward of proportional attention (the plain form of tome_prop_attention, bias_skip included).
//
//   out = softmax(q k^T * scale + log(size)[keys]) v          (tome_attn.h; ToMeAttention.forward:
//   tome/patch/videomae.py:55-66, vivit.py:95-113, timesformer.py:66-78)
//   given dout:   dV = P^T dO,   dP = dO V^T,   delta = rowsum(dO . O),   dS = P o (dP - delta),
//                 dQ = scale dS K,   dK = scale dS^T Q.          size gets no gradient.
//
// The forward saves nothing: P is recomputed from q, k and the bias with the forward's definition of the logits --
// q~ = round16(q * scale * log2 e), bias in log2 units, exp2 -- so it is the P of the stored 16-bit O that delta is
// taken against.  No atomics, every output row written once, same bits on every run: two launches.
//
//   k_attn_bwd_dq   one workgroup = 4 waves = 128 queries of one (batch, head); wave w owns queries 32w .. 32w+31, one
//                   per lane pair (l, l^32).  Sweep 1 walks the key tiles with a plain online softmax (true maximum
//                   and sum: no reference-point trick, no retry -- the maximum is known before any weight is used) and
//                   leaves L = m + log2(l) per row; delta from the stored O.  Sweep 2 walks them again:
//                       S^T  = K Q~^T  + (bias - L)       accumulator register <-> key, lane <-> query
//                       dP^T = V dO^T  - delta
//                       dS^T = exp2(S^T) o dP^T           rounded to the 16-bit format, B operand as it sits
//                       dQ^T += K^T dS^T                  K^T fragments by ds_read_b64_tr_b16
//                   writes dq = scale * dQ (one rounding) and L, delta (fp32) to the workspace.
//   k_attn_bwd_dkv  one workgroup = 4 waves = 128 keys of one (batch, head); wave w owns keys 32w .. 32w+31 with their
//                   K and V rows as B fragments in registers, and walks the query tiles:
//                       S    = Q~ K^T  + (bias - L)       accumulator register <-> query, lane <-> key
//                       dP   = dO V^T  - delta
//                       dV^T += dO^T P                    P rounded to the 16-bit format, B operand as it sits
//                       dK^T += Q^T dS                    dS likewise; Q (not Q~) by transposed reads, scale at the end
//                   out-of-range queries weigh exactly zero in both sums.
// Both stream 64-row tiles through ONE LDS slot, register-staged (the loads of tile t+1 are issued before tile t is
// multiplied), two barriers per tile; a tile that one product reads by rows and another by columns is kept as two
// images (row stride 144 B for the ds_read_b128 rows, 192 B for the transposed reads: the forward's conflict-free
// strides).  32 matrix instructions (32x32x16) per wave and tile in each kernel: eight tile products where the forward
// does two.  The products, q~, the masked maximum, the output rows and the item numbering are the forward's functions
// (tome_attn_tile.h).
//
// The segmented form (SEG = true: the backward of tome_prop_attention_segments, Motionformer's per-frame stage,
// tome/patch/motionformer.py:98-121) shares every line of the two kernels.  Segment s has keys, values, bias, O, dO, dK
// and dV of its own and the queries in common, so dQ = scale * sum_s dS_s K_s:
//   k_attn_bwd_dq   walks its two sweeps once per segment with the dQ accumulators kept in registers across the segments
//                   (one fp32 sum, one rounding when dq is stored); dO and delta are per segment, L and delta go to the
//                   workspace per (segment, batch*head, row).
//   k_attn_bwd_dkv  takes the segment as one more grid factor: (segment, batch*head) in the place of batch*head.
// The plain instantiations (SEG = false) never read the segment fields and keep their code.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tome_attn.h"

#define ATTB_WAVES 4
#define ATTB_BM (32 * ATTB_WAVES)  // queries (dq) / keys (dkv) per workgroup

struct AttnBwdArgs {
    const void *q, *k, *v, *o, *dout;
    void *dq, *dk, *dv;
    int64_t q_sb, q_sh, q_sn, k_sb, k_sh, k_sn, v_sb, v_sh, v_sn;  // element strides: batch, head, token
    int64_t o_sb, o_sh, o_sn, do_sb, do_sh, do_sn;
    int64_t dq_sb, dq_sh, dq_sn, dk_sb, dk_sh, dk_sn, dv_sb, dv_sh, dv_sn;
    const float *log_size;  // NULL or [B, Nk - bias_skip] fp32
    int64_t ls_sb;
    float *lse;    // workspace [B*H*N]: m + log2(l) of every row, log2 units (bias included)
    float *delta;  // workspace [B*H*N]: sum_c dO * O
    int B, H, N, Nk;
    float scale;
    int bias_skip;
    // the segmented form only (SEG = true): element offsets from one segment to the next; lse / delta [nseg, B*H, N]
    int nseg;
    int64_t k_seg, v_seg, o_seg, do_seg, dk_seg, dv_seg, ls_seg;
};

template <typename TX, bool BIAS, bool SEG = false>
__global__ __launch_bounds__(64 * ATTB_WAVES, 2) void k_attn_bwd_dq(AttnBwdArgs a) {
    __shared__ __attribute__((aligned(16))) short lds_kr[ATT_BN * ATT_KS];  // K, rows      (S^T)
    __shared__ __attribute__((aligned(16))) short lds_kt[ATT_BN * ATT_VS];  // K, transposed reads (dQ^T)
    __shared__ __attribute__((aligned(16))) short lds_vr[ATT_BN * ATT_KS];  // V, rows      (dP^T)
    __shared__ __attribute__((aligned(16))) float lds_bias[ATT_BN];        // log(size) * log2(e) per key

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col = lane & 31, hf = lane >> 5;
    int bh, qb;
    if (!att_item(blockIdx.x, (a.N + ATTB_BM - 1) / ATTB_BM, a.B * a.H, bh, qb)) return;
    const int b = bh / a.H, h = bh % a.H;
    const short *qp = reinterpret_cast<const short *>(a.q) + b * a.q_sb + h * a.q_sh;
    // (SEG: the five below move on by a segment offset at the end of every pass of the segment loop)
    const short *kp = reinterpret_cast<const short *>(a.k) + b * a.k_sb + h * a.k_sh;
    const short *vp = reinterpret_cast<const short *>(a.v) + b * a.v_sb + h * a.v_sh;
    const short *op = reinterpret_cast<const short *>(a.o) + b * a.o_sb + h * a.o_sh;
    const short *gp = reinterpret_cast<const short *>(a.dout) + b * a.do_sb + h * a.do_sh;
    const float *lsp = BIAS ? a.log_size + b * a.ls_sb : nullptr;

    const int qrow = qb * ATTB_BM + wave * 32 + col;
    const bool qon = qrow < a.N;
    const int qload = qon ? qrow : a.N - 1;  // (a lane past the end repeats the last query and stores nothing)
    const float LOG2E = 1.4426950408889634f;
    const int skip = SEG ? 0 : a.bias_skip;                  // (the segmented form has no skip form)
    const float bfac = (skip && qrow == 0) ? 0.0f : 1.0f;  // the class query carries no bias
    const float sl = a.scale * LOG2E;
    att_s16x8 qf[4], gf[4];  // q~ and dO of this lane's query: channels 16ks + 8hf .. +7
    float delta = 0.0f;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
        const att_s16x8 raw = *reinterpret_cast<const att_s16x8 *>(qp + (int64_t)qload * a.q_sn + 16 * ks + 8 * hf);
        qf[ks] = att_scaled<TX>(raw, sl);
        gf[ks] = *reinterpret_cast<const att_s16x8 *>(gp + (int64_t)qload * a.do_sn + 16 * ks + 8 * hf);
        const att_s16x8 of = *reinterpret_cast<const att_s16x8 *>(op + (int64_t)qload * a.o_sn + 16 * ks + 8 * hf);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            TX x, y;
            const short sx = gf[ks][e], sy = of[e];
            __builtin_memcpy(&x, &sx, 2);
            __builtin_memcpy(&y, &sy, 2);
            delta = __builtin_fmaf(to_f32(x), to_f32(y), delta);
        }
    }
    delta += __shfl_xor(delta, 32);  // the partner lane holds the other 32 channels
    // SEG: dO and delta of the next segment (the loop above without q~; gp and op have moved on)
    auto next_rows = [&]() __attribute__((always_inline)) {
        delta = 0.0f;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            gf[ks] = *reinterpret_cast<const att_s16x8 *>(gp + (int64_t)qload * a.do_sn + 16 * ks + 8 * hf);
            const att_s16x8 of = *reinterpret_cast<const att_s16x8 *>(op + (int64_t)qload * a.o_sn + 16 * ks + 8 * hf);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                TX x, y;
                const short sx = gf[ks][e], sy = of[e];
                __builtin_memcpy(&x, &sx, 2);
                __builtin_memcpy(&y, &sy, 2);
                delta = __builtin_fmaf(to_f32(x), to_f32(y), delta);
            }
        }
        delta += __shfl_xor(delta, 32);
    };

    const int ntiles = (a.Nk + ATT_BN - 1) / ATT_BN;
    // staging through registers: thread -> rows r0 and r0 + 32, 16-byte column c0 of the 64 x 64 K and V tiles
    const int r0 = tid >> 3, c0 = tid & 7;
    uint4 kreg[2], vreg[2];
    float breg = 0.0f;
    auto stage_load = [&](int t, bool with_v) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int key = t * ATT_BN + r0 + 32 * i;
            const int kl = key < a.Nk ? key : a.Nk - 1;
            kreg[i] = *reinterpret_cast<const uint4 *>(kp + (int64_t)kl * a.k_sn + 8 * c0);
            if (with_v) vreg[i] = *reinterpret_cast<const uint4 *>(vp + (int64_t)kl * a.v_sn + 8 * c0);
            if (key >= a.Nk) {  // zeros: weight 0 times a finite value
                kreg[i] = uint4{0, 0, 0, 0};
                vreg[i] = uint4{0, 0, 0, 0};
            }
        }
        if (BIAS && tid < ATT_BN) {
            const int key = t * ATT_BN + tid;
            const int kl = key < a.Nk ? key : a.Nk - 1;
            breg = kl >= skip ? lsp[kl - skip] * LOG2E : 0.0f;
        }
    };
    auto stage_write = [&](bool with_v) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            *reinterpret_cast<uint4 *>(lds_kr + (r0 + 32 * i) * ATT_KS + 8 * c0) = kreg[i];
            if (with_v) {
                *reinterpret_cast<uint4 *>(lds_kt + (r0 + 32 * i) * ATT_VS + 8 * c0) = kreg[i];
                *reinterpret_cast<uint4 *>(lds_vr + (r0 + 32 * i) * ATT_KS + 8 * c0) = vreg[i];
            }
        }
        if (BIAS && tid < ATT_BN) lds_bias[tid] = breg;
    };
    // start values of the score accumulators: c (+ this key's bias); register v <-> key (v&3) + 8*(v>>2) + 4*hf (+32)
    auto start = [&](float c, att_f32x16 &s0, att_f32x16 &s1) __attribute__((always_inline)) {
#pragma unroll
        for (int v = 0; v < 16; ++v) s0[v] = s1[v] = c;
        if (BIAS) {
            const float *brow = lds_bias + 4 * hf;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const float4 b0 = *reinterpret_cast<const float4 *>(brow + 8 * g);
                const float4 b1 = *reinterpret_cast<const float4 *>(brow + 32 + 8 * g);
                s0[4 * g + 0] = __builtin_fmaf(bfac, b0.x, c); s0[4 * g + 1] = __builtin_fmaf(bfac, b0.y, c);
                s0[4 * g + 2] = __builtin_fmaf(bfac, b0.z, c); s0[4 * g + 3] = __builtin_fmaf(bfac, b0.w, c);
                s1[4 * g + 0] = __builtin_fmaf(bfac, b1.x, c); s1[4 * g + 1] = __builtin_fmaf(bfac, b1.y, c);
                s1[4 * g + 2] = __builtin_fmaf(bfac, b1.z, c); s1[4 * g + 3] = __builtin_fmaf(bfac, b1.w, c);
            }
        }
    };

    att_f32x16 dq0, dq1;  // dQ^T of this lane's query, summed over the key tiles (SEG: of every segment)
    const int nseg = SEG ? a.nseg : 1;
#pragma unroll 1
    for (int seg = 0; seg < nseg; ++seg) {
        if (SEG && seg > 0) next_rows();
        // ---- sweep 1: row maximum and sum (log2 units), plain online softmax over this lane's half of every tile's keys
        float m_run = -INFINITY, l_run = 0.0f;
        stage_load(0, false);
        for (int t = 0; t < ntiles; ++t) {
            __syncthreads();  // every wave has left tile t-1
            stage_write(false);
            if (t + 1 < ntiles) stage_load(t + 1, false);
            __syncthreads();
            att_f32x16 s0, s1;
            start(0.0f, s0, s1);
            att_rows_product<TX>(lds_kr, col, hf, qf, s0, s1);
            const float mt = att_masked_max(s0, s1, t * ATT_BN + 4 * hf, a.Nk);
            const float m_new = fmaxf(m_run, mt);  // finite: every tile holds at least one key in range
            float lsum = 0.0f;
#pragma unroll
            for (int v = 0; v < 16; ++v)
                lsum += __builtin_amdgcn_exp2f(s0[v] - m_new) + __builtin_amdgcn_exp2f(s1[v] - m_new);
            l_run = l_run * __builtin_amdgcn_exp2f(m_run - m_new) + lsum;
            m_run = m_new;
        }
        const float l_tot = l_run + __shfl_xor(l_run, 32);
        const float lse = m_run + __builtin_log2f(l_tot);
        if (qon && hf == 0) {  // (SEG: the workspace rows of segment `seg` lie seg * B*H*N further on)
            const int64_t wrow = ((int64_t)(SEG ? seg * (a.B * a.H) : 0) + bh) * a.N + qrow;
            a.lse[wrow] = lse;
            a.delta[wrow] = delta;
        }

        // ---- sweep 2: dQ^T += K^T (P o (dP - delta))^T
        if (!SEG || seg == 0) {
#pragma unroll
            for (int v = 0; v < 16; ++v) dq0[v] = dq1[v] = 0.0f;
        }
        stage_load(0, true);
        for (int t = 0; t < ntiles; ++t) {
            __syncthreads();
            stage_write(true);
            if (t + 1 < ntiles) stage_load(t + 1, true);
            __syncthreads();
            att_f32x16 s0, s1, p0, p1;
            start(-lse, s0, s1);
            att_rows_product<TX>(lds_kr, col, hf, qf, s0, s1);
#pragma unroll
            for (int v = 0; v < 16; ++v) p0[v] = p1[v] = -delta;
            att_rows_product<TX>(lds_vr, col, hf, gf, p0, p1);
            const int key0 = t * ATT_BN + 4 * hf;
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int key = key0 + (v & 3) + 8 * (v >> 2);
                const float w0 = key < a.Nk ? __builtin_amdgcn_exp2f(s0[v]) : 0.0f;  // out-of-range keys weigh exactly zero
                const float w1 = key + 32 < a.Nk ? __builtin_amdgcn_exp2f(s1[v]) : 0.0f;
                s0[v] = w0 * p0[v];
                s1[v] = w1 * p1[v];
            }
            att_tr_product<TX>(lds_kt, lane, s0, s1, dq0, dq1);
        }
        if (SEG) {  // the next segment's keys, values, bias, O and dO
            kp += a.k_seg; vp += a.v_seg; op += a.o_seg; gp += a.do_seg;
            if (BIAS) lsp += a.ls_seg;
        }
    }  // segments
    short *dqp = reinterpret_cast<short *>(a.dq) + b * a.dq_sb + h * a.dq_sh + (int64_t)(qon ? qrow : 0) * a.dq_sn;
    att_store_row<TX>(dqp + 32 * hf, qon, dq0, dq1, a.scale);
}

template <typename TX, bool BIAS, bool SEG = false>
__global__ __launch_bounds__(64 * ATTB_WAVES, 2) void k_attn_bwd_dkv(AttnBwdArgs a) {
    __shared__ __attribute__((aligned(16))) short lds_qr[ATT_BN * ATT_KS];  // Q~, rows     (S)
    __shared__ __attribute__((aligned(16))) short lds_qt[ATT_BN * ATT_VS];  // Q, transposed reads (dK^T)
    __shared__ __attribute__((aligned(16))) short lds_gr[ATT_BN * ATT_KS];  // dO, rows     (dP)
    __shared__ __attribute__((aligned(16))) short lds_gt[ATT_BN * ATT_VS];  // dO, transposed reads (dV^T)
    __shared__ __attribute__((aligned(16))) float lds_row[2 * ATT_BN];      // -L and -delta per query of the tile

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col = lane & 31, hf = lane >> 5;
    int bh, kb;
    const int BH = a.B * a.H;
    if (!att_item(blockIdx.x, (a.Nk + ATTB_BM - 1) / ATTB_BM, SEG ? BH * a.nseg : BH, bh, kb)) return;
    const int seg = SEG ? bh / BH : 0;  // (SEG: the items are (segment, batch*head) pairs)
    if (SEG) bh -= seg * BH;
    const int b = bh / a.H, h = bh % a.H;
    const short *qp = reinterpret_cast<const short *>(a.q) + b * a.q_sb + h * a.q_sh;
    const short *kp = reinterpret_cast<const short *>(a.k) + b * a.k_sb + h * a.k_sh + (SEG ? seg * a.k_seg : 0);
    const short *vp = reinterpret_cast<const short *>(a.v) + b * a.v_sb + h * a.v_sh + (SEG ? seg * a.v_seg : 0);
    const short *gp = reinterpret_cast<const short *>(a.dout) + b * a.do_sb + h * a.do_sh + (SEG ? seg * a.do_seg : 0);
    const int64_t wrow = ((int64_t)(SEG ? seg * BH : 0) + bh) * a.N;
    const float *lsep = a.lse + wrow, *dlp = a.delta + wrow;

    const int krow = kb * ATTB_BM + wave * 32 + col;
    const bool kon = krow < a.Nk;
    const int kload = kon ? krow : a.Nk - 1;  // (a lane past the end repeats the last key and stores nothing)
    const float LOG2E = 1.4426950408889634f;
    const float sl = a.scale * LOG2E;
    float beta = 0.0f;  // this lane's key: log(size) * log2(e); key 0 of the skip form carries none
    if (BIAS)
        beta = kload >= a.bias_skip ? a.log_size[b * a.ls_sb + (SEG ? seg * a.ls_seg : 0) + kload - a.bias_skip] * LOG2E
                                    : 0.0f;
    att_s16x8 kf[4], vf[4];  // K and V rows of this lane's key: channels 16ks + 8hf .. +7
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
        kf[ks] = *reinterpret_cast<const att_s16x8 *>(kp + (int64_t)kload * a.k_sn + 16 * ks + 8 * hf);
        vf[ks] = *reinterpret_cast<const att_s16x8 *>(vp + (int64_t)kload * a.v_sn + 16 * ks + 8 * hf);
    }

    const int ntiles = (a.N + ATT_BN - 1) / ATT_BN;
    const int r0 = tid >> 3, c0 = tid & 7;
    uint4 qreg[2], greg[2];
    float rreg = 0.0f;
    auto stage_load = [&](int t) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int qr = t * ATT_BN + r0 + 32 * i;
            const int ql = qr < a.N ? qr : a.N - 1;
            qreg[i] = *reinterpret_cast<const uint4 *>(qp + (int64_t)ql * a.q_sn + 8 * c0);
            greg[i] = *reinterpret_cast<const uint4 *>(gp + (int64_t)ql * a.do_sn + 8 * c0);
            if (qr >= a.N) {  // rows past the end: zeros (their weights are forced to zero below)
                qreg[i] = uint4{0, 0, 0, 0};
                greg[i] = uint4{0, 0, 0, 0};
            }
        }
        if (tid < 2 * ATT_BN) {
            const int qr = t * ATT_BN + (tid & (ATT_BN - 1));
            const int ql = qr < a.N ? qr : a.N - 1;
            rreg = -(tid < ATT_BN ? lsep[ql] : dlp[ql]);
        }
    };
    auto stage_write = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            att_s16x8 raw;
            __builtin_memcpy(&raw, &qreg[i], 16);
            *reinterpret_cast<att_s16x8 *>(lds_qr + (r0 + 32 * i) * ATT_KS + 8 * c0) = att_scaled<TX>(raw, sl);
            *reinterpret_cast<uint4 *>(lds_qt + (r0 + 32 * i) * ATT_VS + 8 * c0) = qreg[i];
            *reinterpret_cast<uint4 *>(lds_gr + (r0 + 32 * i) * ATT_KS + 8 * c0) = greg[i];
            *reinterpret_cast<uint4 *>(lds_gt + (r0 + 32 * i) * ATT_VS + 8 * c0) = greg[i];
        }
        if (tid < 2 * ATT_BN) lds_row[tid] = rreg;
    };
    // start values of one 32-query block: register v <-> query (v&3) + 8*(v>>2) + 4*hf of the block
    auto start = [&](const float *rowc, float add, att_f32x16 &s) __attribute__((always_inline)) {
        const float *r = rowc + 4 * hf;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float4 x = *reinterpret_cast<const float4 *>(r + 8 * g);
            s[4 * g + 0] = x.x + add; s[4 * g + 1] = x.y + add; s[4 * g + 2] = x.z + add; s[4 * g + 3] = x.w + add;
        }
    };

    att_f32x16 dk0, dk1, dv0, dv1;
#pragma unroll
    for (int v = 0; v < 16; ++v) dk0[v] = dk1[v] = dv0[v] = dv1[v] = 0.0f;
    stage_load(0);
    for (int t = 0; t < ntiles; ++t) {
        __syncthreads();  // every wave has left tile t-1
        stage_write();
        if (t + 1 < ntiles) stage_load(t + 1);
        __syncthreads();
        // one 32-query block at a time: a block's scores and dP are dead before the next block's are made
#pragma unroll 1
        for (int qb = 0; qb < 2; ++qb) {
            att_f32x16 s, p;
            start(lds_row + 32 * qb, beta, s);
            // the skip form's class query (query 0: register 0 of the lower lanes, block 0 of tile 0) carries no bias
            if (BIAS && qb == 0 && a.bias_skip && t == 0 && hf == 0) s[0] = lds_row[0];
            att_rows_block<TX>(lds_qr, col, hf, qb, kf, s);
            start(lds_row + ATT_BN + 32 * qb, 0.0f, p);
            att_rows_block<TX>(lds_gr, col, hf, qb, vf, p);
            const int q0 = t * ATT_BN + 32 * qb + 4 * hf;
#pragma unroll
            for (int v = 0; v < 16; ++v)  // out-of-range queries contribute nothing
                s[v] = q0 + (v & 3) + 8 * (v >> 2) < a.N ? __builtin_amdgcn_exp2f(s[v]) : 0.0f;
            att_tr_block<TX>(lds_gt, lane, qb, s, dv0, dv1);
#pragma unroll
            for (int v = 0; v < 16; ++v) s[v] *= p[v];
            att_tr_block<TX>(lds_qt, lane, qb, s, dk0, dk1);
        }
    }
    const int64_t kst = kon ? krow : 0;
    short *dkp = reinterpret_cast<short *>(a.dk) + b * a.dk_sb + h * a.dk_sh + kst * a.dk_sn + (SEG ? seg * a.dk_seg : 0);
    short *dvp = reinterpret_cast<short *>(a.dv) + b * a.dv_sb + h * a.dv_sh + kst * a.dv_sn + (SEG ? seg * a.dv_seg : 0);
    att_store_row<TX>(dkp + 32 * hf, kon, dk0, dk1, a.scale);
    att_store_row<TX>(dvp + 32 * hf, kon, dv0, dv1, 1.0f);
}

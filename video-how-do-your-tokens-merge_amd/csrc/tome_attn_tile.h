// tome_attn_tile.h -- the tile arithmetic of the MFMA attention kernels, each piece once: k_prop_attention
// (tome_attn.h), k_prop_attention_stream (tome_attn_stream.h), k_resident_attention (tome_attn_resident.h),
// k_attn_bwd_dq and k_attn_bwd_dkv (tome_attn_bwd.h) all call the functions below and differ in what surrounds them
// (staging, the LDS ring, the bias treatment, the guard policy, where s_setprio sits).
//
// One layout throughout (v_mfma_f32_32x32x16, wave of 64 lanes, col = lane & 31, hf = lane >> 5):
//   * A operand of a row product: 8 consecutive channels 16 ks + 8 hf .. +7 of row `col` of a 32-row block, read from an
//     LDS row image of stride ATT_KS; B operand: the same channels of this lane's own row (query / key) in registers;
//   * accumulator register v of lane l <-> row (v & 3) + 8 (v >> 2) + 4 hf of the block (a KEY of the forward's scores),
//     column col (a QUERY): a column's 32 values sit in the lane pair (l, l ^ 32);
//   * that accumulator, rounded to the 16-bit format in register order (v = 8 p .. 8 p + 7 -> B fragment p), is the B
//     operand of the second product as it sits; its A operand comes from an image of stride ATT_VS by
//     ds_read_b64_tr_b16 (4 consecutive rows of one channel per lane), channels 0..31 -> acc0, 32..63 -> acc1.
// Every fp32 operation below keeps the operands and the order the kernels have always had; the outputs are the bits
// of the copies these functions replace.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tome_common.h"

#define ATT_D 64        // head dim
#define ATT_BN 64       // keys per tile
#define ATT_KS 72       // K tile row stride in elements (144 B: conflict-free ds_read_b128 over 16 rows)
#define ATT_VS 96       // V tile row stride in elements (192 B: conflict-free ds_read_b64_tr_b16 over 4 rows)

typedef float att_f32x16 __attribute__((ext_vector_type(16)));
typedef short att_s16x4 __attribute__((ext_vector_type(4)));
typedef short att_s16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 att_bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 att_f16x8 __attribute__((ext_vector_type(8)));

template <typename TX> struct AttMfma;
template <> struct AttMfma<bf16_t> {
    static __device__ __forceinline__ att_f32x16 run(att_s16x8 a, att_s16x8 b, att_f32x16 c) {
        att_bf16x8 x, y;
        __builtin_memcpy(&x, &a, 16);
        __builtin_memcpy(&y, &b, 16);
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(x, y, c, 0, 0, 0);
    }
};
template <> struct AttMfma<f16_t> {
    static __device__ __forceinline__ att_f32x16 run(att_s16x8 a, att_s16x8 b, att_f32x16 c) {
        att_f16x8 x, y;
        __builtin_memcpy(&x, &a, 16);
        __builtin_memcpy(&y, &b, 16);
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(x, y, c, 0, 0, 0);
    }
};

// Largest lane sum of un-normalised weights the plain path accepts before it moves the reference point: the weights
// go to the second product in the 16-bit format (fp16 tops out at 65504; bf16 has fp32's range) and O / l
// accumulate N of them in fp32.
template <typename TX> struct AttLimit;
template <> struct AttLimit<bf16_t> { static constexpr float value = 1.152921504606847e18f; };  // 2^60
template <> struct AttLimit<f16_t> { static constexpr float value = 32768.0f; };                // 2^15

__device__ __forceinline__ float att_add(float x, float y) {
    // one v_add_f32 that the vectoriser cannot pair into v_pk_add_f32: the sum passes through an empty asm statement
    // (the add itself stays a compiler instruction, so its hazards -- a transcendental result read by the next
    // VALU instruction -- are padded by hipcc, which it would not do inside an asm string)
    float r = x + y;
    asm("" : "+v"(r));
    return r;
}

template <typename TX> __device__ __forceinline__ short att_bits(float f) {
    const TX t = from_f32<TX>(f);
    short s;
    __builtin_memcpy(&s, &t, 2);
    return s;
}

// x as two terms hi + lo of the 16-bit format, packed hi | lo << 16: what a value costs to ride on the matrix pipe (two
// channels of a k-step against a constant 1).  `carried` = hi + lo, exact in fp32 (16 significant bits at most; what
// is left of x is below 2^-16 |x| for bf16, 2^-22 |x| for fp16 above its subnormals).
template <typename TX> __device__ __forceinline__ unsigned att_split16(float x, float &carried) {
    const short bh = att_bits<TX>(x);
    TX th, tl;
    __builtin_memcpy(&th, &bh, 2);
    const float hi = to_f32(th);
    const short bl = att_bits<TX>(x - hi);
    __builtin_memcpy(&tl, &bl, 2);
    carried = hi + to_f32(tl);
    return (unsigned)(unsigned short)bh | ((unsigned)(unsigned short)bl << 16);
}

// workgroup L -> (item, block): the `blocks` blocks of one item get ids congruent mod 8, i.e. one XCD, whose L2 then
// serves the K/V (forward, dq), Q/dO (dkv) or Q rows (resident: the blocks are the segments) they all stream.
// False: L lies past the last of `count` items.
__device__ __forceinline__ bool att_item(int L, int blocks, int count, int &item, int &blk) {
    const int xcd = L & 7, sq = L >> 3;
    item = (sq / blocks) * 8 + xcd;
    blk = sq % blocks;
    return item < count;
}

// A 16-byte chunk of 16-bit values times a fp32 factor, rounded once to the format: q -> q~ = q * scale * log2(e).
// Element e of the chunk stays element e (channel 16 ks + 8 hf + e of the lane's row).
template <typename TX> __device__ __forceinline__ att_s16x8 att_scaled(const att_s16x8 raw, float f) {
    att_s16x8 r;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        TX t;
        const short s = raw[e];
        __builtin_memcpy(&t, &s, 2);
        r[e] = att_bits<TX>(to_f32(t) * f);
    }
    return r;
}

// Accumulator registers 8 p .. 8 p + 7 (rows 16 p + 4 hf + {0..3, 8..11} of the block) -> B fragment p of the second
// product, one rounding each; att_pack_tile: the four fragments of a 64-row tile, pf[block][p].
template <typename TX> __device__ __forceinline__ att_s16x8 att_pack(const att_f32x16 &w, int p) {
    att_s16x8 r;
#pragma unroll
    for (int e = 0; e < 8; ++e) r[e] = att_bits<TX>(w[8 * p + e]);
    return r;
}
template <typename TX>
__device__ __forceinline__ void att_pack_tile(const att_f32x16 &w0, const att_f32x16 &w1, att_s16x8 (&pf)[2][2]) {
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        pf[0][p] = att_pack<TX>(w0, p);
        pf[1][p] = att_pack<TX>(w1, p);
    }
}

// c += X_blk Y^T for rows 32 blk .. 32 blk + 31 of X (LDS row image, stride ATT_KS: lane reads row 32 blk + col, channels
// 16 ks + 8 hf .. +7) and this lane's Y fragment yf[ks] (the same channels of its own row): four MFMAs, ks ascending.
template <typename TX>
__device__ __forceinline__ void att_rows_block(const short *img, int col, int hf, int blk, const att_s16x8 (&yf)[4],
                                               att_f32x16 &c) {
    const short *base = img + (32 * blk + col) * ATT_KS + 8 * hf;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) c = AttMfma<TX>::run(*reinterpret_cast<const att_s16x8 *>(base + 16 * ks), yf[ks], c);
}
template <typename TX>
__device__ __forceinline__ void att_rows_product(const short *img, int col, int hf, const att_s16x8 (&yf)[4],
                                                 att_f32x16 &c0, att_f32x16 &c1) {
    att_rows_block<TX>(img, col, hf, 0, yf, c0);
    att_rows_block<TX>(img, col, hf, 1, yf, c1);
}

// Transposed reads of an image of stride ATT_VS.  att_tr_base: the lane's address in rows row .. row + 15 -- row + 4 hf
// + ((lane & 15) >> 2) (+8), channel 16 ((lane >> 4) & 1) + 4 (lane & 3) (+32).  att_tr_read: the four reads of the 16-row
// group at va = base + 16 group * ATT_VS -- f[0], f[1]: rows +0, +8 of channels 0..31; f[2], f[3]: of channels 32..63.
// att_tr_mfma: (acc0, acc1) += X_group^T W from those reads and the group's B fragment wf (att_pack).
__device__ __forceinline__ const short *att_tr_base(const short *img, int lane, int row) {
    const int hf = lane >> 5;
    return img + (row + 4 * hf + ((lane & 15) >> 2)) * ATT_VS + 16 * ((lane >> 4) & 1) + 4 * (lane & 3);
}
__device__ __forceinline__ void att_tr_read(const short *va, att_s16x4 &f0, att_s16x4 &f1, att_s16x4 &f2, att_s16x4 &f3) {
    typedef __attribute__((address_space(3))) att_s16x4 *lds_s16x4_p;
    f0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_p)(va));
    f1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_p)(va + 8 * ATT_VS));
    f2 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_p)(va + 32));
    f3 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_p)(va + 8 * ATT_VS + 32));
}
template <typename TX>
__device__ __forceinline__ void att_tr_mfma(const att_s16x4 f0, const att_s16x4 f1, const att_s16x4 f2, const att_s16x4 f3,
                                            const att_s16x8 wf, att_f32x16 &acc0, att_f32x16 &acc1) {
    att_s16x8 x0, x1;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        x0[e] = f0[e];
        x0[4 + e] = f1[e];
        x1[e] = f2[e];
        x1[4 + e] = f3[e];
    }
    acc0 = AttMfma<TX>::run(x0, wf, acc0);
    acc1 = AttMfma<TX>::run(x1, wf, acc1);
}
// (acc0, acc1) += X_blk^T W for rows 32 blk .. 32 blk + 31 of X and W = the accumulator block w rounded to the 16-bit
// format, fragments read where they are used (the backward; the resident kernel packs its weights beforehand)
template <typename TX>
__device__ __forceinline__ void att_tr_block(const short *img, int lane, int blk, const att_f32x16 &w, att_f32x16 &acc0,
                                             att_f32x16 &acc1) {
    const short *base = att_tr_base(img, lane, 32 * blk);
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const att_s16x8 wf = att_pack<TX>(w, p);
        att_s16x4 f0, f1, f2, f3;
        att_tr_read(base + 16 * p * ATT_VS, f0, f1, f2, f3);
        // (att_tr_mfma written out: through the call the compiler orders the dq kernels' second sweep differently --
        // 198 vector registers for 200 and two backward shapes 0.2 % slower than the parent's slowest round)
        att_s16x8 x0, x1;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            x0[e] = f0[e];
            x0[4 + e] = f1[e];
            x1[e] = f2[e];
            x1[4 + e] = f3[e];
        }
        acc0 = AttMfma<TX>::run(x0, wf, acc0);
        acc1 = AttMfma<TX>::run(x1, wf, acc1);
    }
}
template <typename TX>
__device__ __forceinline__ void att_tr_product(const short *img, int lane, const att_f32x16 &w0, const att_f32x16 &w1,
                                               att_f32x16 &acc0, att_f32x16 &acc1) {
    att_tr_block<TX>(img, lane, 0, w0, acc0, acc1);
    att_tr_block<TX>(img, lane, 1, w1, acc0, acc1);
}
// The streaming forward kernels read a whole 64-key tile's fragments one step before they multiply them (software
// pipeline): vfr[block][p] of the tile whose lane address is vs = att_tr_base(slot image, lane, 0); first_half_only: the
// weights of keys 32..63 are zero, their four MFMAs are left out (wave-uniform).
__device__ __forceinline__ void att_tr_read_tile(const short *vs, att_s16x4 (&vfr)[2][2][4]) {
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int p = 0; p < 2; ++p)
            att_tr_read(vs + (32 * kb + 16 * p) * ATT_VS, vfr[kb][p][0], vfr[kb][p][1], vfr[kb][p][2], vfr[kb][p][3]);
}
template <typename TX>
__device__ __forceinline__ void att_tr_mfma_tile(const att_s16x4 (&vfr)[2][2][4], const att_s16x8 (&pf)[2][2],
                                                 bool first_half_only, att_f32x16 &o0, att_f32x16 &o1) {
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
        if (kb == 1 && first_half_only) break;
#pragma unroll
        for (int p = 0; p < 2; ++p)
            att_tr_mfma<TX>(vfr[kb][p][0], vfr[kb][p][1], vfr[kb][p][2], vfr[kb][p][3], pf[kb][p], o0, o1);
    }
}

// The same products with every fragment read right before its MFMA pair (4 registers of fragments live instead of a
// tile's 16): for a kernel that multiplies the tile in the step that staged it and has other waves to cover the reads.
template <typename TX>
__device__ __forceinline__ void att_tr_tile_product(const short *vs, const att_s16x8 (&pf)[2][2], bool first_half_only,
                                                    att_f32x16 &o0, att_f32x16 &o1) {
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
        if (kb == 1 && first_half_only) break;
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            att_s16x4 f0, f1, f2, f3;
            att_tr_read(vs + (32 * kb + 16 * p) * ATT_VS, f0, f1, f2, f3);
            att_tr_mfma<TX>(f0, f1, f2, f3, pf[kb][p], o0, o1);
        }
    }
}

// Rows of a block past the end: register v holds row row0 + (v & 3) + 8 (v >> 2), row0 = the block's first row + 4 hf;
// rows >= n get `fill` (-inf in front of a maximum, 0 for a weight).
__device__ __forceinline__ void att_fill_tail(att_f32x16 &s, int row0, int n, float fill) {
#pragma unroll
    for (int v = 0; v < 16; ++v) s[v] = row0 + (v & 3) + 8 * (v >> 2) < n ? s[v] : fill;
}
// a column's maximum from its two half columns in lanes l and l ^ 32 (one v_permlane32_swap)
__device__ __forceinline__ float att_half_max(float mt) {
    const unsigned mb = __float_as_uint(mt);
    const auto sw = __builtin_amdgcn_permlane32_swap(mb, mb, false, false);
    return fmaxf(__uint_as_float(sw[0]), __uint_as_float(sw[1]));
}
// own + partner of the same lane pair (the same bits as own + __shfl_xor(own, 32): the addition commutes), without the
// lane number a shuffle needs
__device__ __forceinline__ float att_half_sum(float x) {
    const unsigned xb = __float_as_uint(x);
    const auto sw = __builtin_amdgcn_permlane32_swap(xb, xb, false, false);
    return __uint_as_float(sw[0]) + __uint_as_float(sw[1]);
}
// Keys past nk masked to -inf, then the column maximum of the 64-key tile (s0: keys key0 + ..., s1: 32 further on;
// key0 = the tile's first key + 4 hf) or of one 32-key block.
__device__ __forceinline__ float att_masked_max(att_f32x16 &s0, att_f32x16 &s1, int key0, int nk) {
    float mt = -INFINITY;
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        const int key = key0 + (v & 3) + 8 * (v >> 2);
        s0[v] = key < nk ? s0[v] : -INFINITY;
        s1[v] = key + 32 < nk ? s1[v] : -INFINITY;
        mt = fmaxf(mt, fmaxf(s0[v], s1[v]));
    }
    return att_half_max(mt);
}
__device__ __forceinline__ float att_masked_max(att_f32x16 &s, int key0, int nk) {
    float mt = -INFINITY;
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        s[v] = key0 + (v & 3) + 8 * (v >> 2) < nk ? s[v] : -INFINITY;
        mt = fmaxf(mt, s[v]);
    }
    return att_half_max(mt);
}

// Row sum of this lane's half column as four att_add chains c[j] over registers j, j + 4, ...: att_sum_block starts
// them from a block's 16 weights, att_sum_more adds a further block's, att_sum_end joins them (c0 + c1) + (c2 + c3).
__device__ __forceinline__ void att_sum_block(const att_f32x16 &s, float (&c)[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) c[j] = att_add(s[j], s[4 + j]);
#pragma unroll
    for (int v = 8; v < 16; v += 4) {
#pragma unroll
        for (int j = 0; j < 4; ++j) c[j] = att_add(c[j], s[v + j]);
    }
}
__device__ __forceinline__ void att_sum_more(const att_f32x16 &s, float (&c)[4]) {
#pragma unroll
    for (int v = 0; v < 16; v += 4) {
#pragma unroll
        for (int j = 0; j < 4; ++j) c[j] = att_add(c[j], s[v + j]);
    }
}
__device__ __forceinline__ float att_sum_end(const float (&c)[4]) { return att_add(att_add(c[0], c[1]), att_add(c[2], c[3])); }

// Weights of a 64-key tile on the fast path: the scores arrive as s - m_ref (+ bias), a weight is one v_exp_f32;
// masked: the partly filled last tile, keys past nk weigh nothing (key0 = the tile's first key + 4 hf).  Leaves the
// weights in s0 / s1, their 16-bit fragments in pf and returns the lane's row sum (taken before the rounding).
// (The additions are compiler instructions: an asm add reading a v_exp_f32 result gets no hazard padding.)
template <typename TX>
__device__ __forceinline__ float att_fast_weights(att_f32x16 &s0, att_f32x16 &s1, bool masked, int key0, int nk,
                                                  att_s16x8 (&pf)[2][2]) {
#pragma unroll
    for (int v = 0; v < 16; ++v) s0[v] = __builtin_amdgcn_exp2f(s0[v]);
#pragma unroll
    for (int v = 0; v < 16; ++v) s1[v] = __builtin_amdgcn_exp2f(s1[v]);
    if (masked) {
        att_fill_tail(s0, key0, nk, 0.0f);
        att_fill_tail(s1, key0 + 32, nk, 0.0f);
    }
    float c[4];
    att_sum_block(s0, c);
    att_sum_more(s1, c);
    const float lsum = att_sum_end(c);
    att_pack_tile<TX>(s0, s1, pf);
    return lsum;
}

// General softmax of a 64-key tile whose scores (s0, s1) started at zero: range mask, maximum, rescale of O and l,
// weights and their fragments.  The new reference point is ref(maximum so far): the value the caller can subtract from
// the scores to come (the maximum itself, or the nearest value it can carry on the matrix pipe); it ends up in m_run.
template <typename TX, typename Ref>
__device__ __forceinline__ void att_general_softmax_at(att_f32x16 &s0, att_f32x16 &s1, int key0, int nk, float &m_run,
                                                       float &l_run, att_f32x16 &o0, att_f32x16 &o1,
                                                       att_s16x8 (&pf)[2][2], Ref &&ref) {
    const float mt = att_masked_max(s0, s1, key0, nk);
    const float m_new = ref(fmaxf(m_run, mt));  // finite: every tile holds at least one key in range
    const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
    float lsum = 0.0f;
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        s0[v] = __builtin_amdgcn_exp2f(s0[v] - m_new);
        s1[v] = __builtin_amdgcn_exp2f(s1[v] - m_new);
        lsum += s0[v] + s1[v];
    }
    l_run = l_run * alpha + lsum;
    m_run = m_new;
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        o0[v] *= alpha;
        o1[v] *= alpha;
    }
    att_pack_tile<TX>(s0, s1, pf);
}
// The same with the reference point at the maximum, handed on as the start values -m of the scores to come (negm).
template <typename TX>
__device__ __forceinline__ void att_general_softmax(att_f32x16 &s0, att_f32x16 &s1, int key0, int nk, float &m_run,
                                                    float &l_run, att_f32x16 &o0, att_f32x16 &o1, att_f32x16 &negm,
                                                    att_s16x8 (&pf)[2][2]) {
    const float mt = att_masked_max(s0, s1, key0, nk);
    const float m_new = fmaxf(m_run, mt);  // finite: every tile holds at least one key in range
    const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
    float lsum = 0.0f;
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        s0[v] = __builtin_amdgcn_exp2f(s0[v] - m_new);
        s1[v] = __builtin_amdgcn_exp2f(s1[v] - m_new);
        lsum += s0[v] + s1[v];
    }
    l_run = l_run * alpha + lsum;
    m_run = m_new;
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        o0[v] *= alpha;
        o1[v] *= alpha;
        negm[v] = -m_new;
    }
    att_pack_tile<TX>(s0, s1, pf);
}

// row[0..63] = f * (acc0, acc1)^T of this lane's column, one rounding; `half` = row + 32 hf, the 32 channels this lane
// stores (the caller forms it: with 32-bit offsets where it has them).  Register v <-> channel (v&3) + 8*(v>>2) + 4*hf
// (+32 in acc1).  A lane holds channels 8g + 4*hf .. +3 (w0) and 32 + 8g + 4*hf .. +3 (w1) of its row; its partner lane
// l^32 holds the other halves.  One v_permlane32_swap per dword hands the lower lane the partner's w0 and the upper
// lane the partner's w1, so every lane stores 16 contiguous bytes (channels 8g .. 8g+7, +32 for the upper lanes): four
// 16-byte stores per lane instead of eight 8-byte ones.  All 64 lanes take part in the swaps; `on` predicates the stores.
template <typename TX>
__device__ __forceinline__ void att_store_row(short *half, bool on, const att_f32x16 &acc0, const att_f32x16 &acc1, float f) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        att_s16x4 w0, w1;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            w0[e] = att_bits<TX>(acc0[4 * g + e] * f);
            w1[e] = att_bits<TX>(acc1[4 * g + e] * f);
        }
        unsigned a2[2], b2[2];
        __builtin_memcpy(a2, &w0, 8);
        __builtin_memcpy(b2, &w1, 8);
        const auto s0w = __builtin_amdgcn_permlane32_swap(a2[0], b2[0], false, false);
        const auto s1w = __builtin_amdgcn_permlane32_swap(a2[1], b2[1], false, false);
        const uint4 row16 = uint4{s0w[0], s1w[0], s0w[1], s1w[1]};
        if (on) *reinterpret_cast<uint4 *>(half + 8 * g) = row16;
    }
}

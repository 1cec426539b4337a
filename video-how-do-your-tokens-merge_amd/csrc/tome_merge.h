// tome_merge.h -- part of the single translation unit csrc/tome_kernels.hip (merge / unmerge row kernels).
#pragma once
// ------------------------------------------------------------------------------------------------
// k_merge_rows: merge.py:75-85 (+ :365-368 when OP_WAVG).  One wave per OUTPUT row; the wave finds
// the sources of a destination row by ballot-scanning dst_idx (r entries, rank order), so the sum is
// atomic-free and in the contract's order.  Every input row is read once, every output row written once.
// ------------------------------------------------------------------------------------------------
enum { OP_WAVG = 100, OP_DROP = 101 };

template <int OP> __device__ __forceinline__ float reduce_step(float acc, float v) {
    if (OP == TOME_SUM || OP == TOME_MEAN || OP == OP_WAVG) return __fadd_rn(acc, v);
    if (OP == TOME_PROD) return __fmul_rn(acc, v);
    if (OP == TOME_AMAX) return (acc != acc) ? acc : (!(v <= acc) ? v : acc);
    if (OP == TOME_AMIN) return (acc != acc) ? acc : (!(v >= acc) ? v : acc);
    return acc;
}

// round(v + xbias[c..]) for a 16-byte pack of stored tokens
template <typename TX, int VEC>
__device__ __forceinline__ uint4 add_xbias(const uint4 &v, const TX *__restrict__ xb) {
    Pack<TX, VEC> pk;
    __builtin_memcpy(&pk, &v, 16);
    float b8[VEC];
    load_pack<TX, VEC>(xb, b8);
#pragma unroll
    for (int e = 0; e < VEC; ++e) pk.e[e] = from_f32<TX>(__fadd_rn(to_f32(pk.e[e]), b8[e]));
    uint4 o;
    __builtin_memcpy(&o, &pk, 16);
    return o;
}

// round(x + a) in the token dtype, element-wise on two 16-byte packs (what torch's `x + a` stores)
template <typename TX, int VEC>
__device__ __forceinline__ Pack<TX, VEC> add_packs(const Pack<TX, VEC> &x, const Pack<TX, VEC> &a) {
    Pack<TX, VEC> o;
#pragma unroll
    for (int e = 0; e < VEC; ++e) o.e[e] = from_f32<TX>(__fadd_rn(to_f32(x.e[e]), to_f32(a.e[e])));
    return o;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// The tail of one destination row held by a whole wave as two 16-byte column chunks per lane (acc0 at column c0, acc1
// at c1; a0 / a1 say which exist): division by the summed size (or the count, for "mean"), the stores of x' (with the
// folded bias), size' (and its log), and the fused LayerNorm of the row as stored.  Shared by merge_dst_row and
// merge_dst_row_r64, so both build bit-identical rows.
// (pre: the lane's chunks of xbias / LayerNorm weight / bias when the caller has requested them ahead of its own
// waits -- merge_dst_row_r64; nullptr: fetched here)
template <typename TX, int VEC> struct RowConsts { Pack<TX, VEC> xb0, xb1, w0, w1, b0, b1; };

template <typename TX, int VEC>
__device__ __forceinline__ void unpack_f32(const Pack<TX, VEC> &p, float (&out)[VEC]) {
#pragma unroll
    for (int e = 0; e < VEC; ++e) out[e] = to_f32(p.e[e]);
}

template <typename TX, typename TS, int VEC, int OP, bool LN, bool PRE = false>
__device__ __forceinline__ void dst_row_finish(float (&acc0)[VEC], float (&acc1)[VEC], bool a0, bool a1, int c0, int c1,
                                               float ssum, int cnt, int C, TX *__restrict__ orow, TS *__restrict__ srow,
                                               TS *__restrict__ lrow, const LnArgs *ln, TX *__restrict__ yrow, int lane,
                                               const RowConsts<TX, VEC> pre = RowConsts<TX, VEC>()) {
    if (OP == OP_WAVG) {
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            if (a0) acc0[e] = __fdiv_rn(acc0[e], ssum);
            if (a1) acc1[e] = __fdiv_rn(acc1[e], ssum);
        }
    } else if (OP == TOME_MEAN && cnt > 1) {
        const float fc = (float)cnt;
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            if (a0) acc0[e] = __fdiv_rn(acc0[e], fc);
            if (a1) acc1[e] = __fdiv_rn(acc1[e], fc);
        }
    }
    if (LN && ln->xbias) {
        const TX *xb = reinterpret_cast<const TX *>(ln->xbias);
        float b8[VEC], o8[VEC];
        if (a0) {
            if (PRE) unpack_f32<TX, VEC>(pre.xb0, b8); else load_pack<TX, VEC>(xb + c0, b8);
#pragma unroll
            for (int e = 0; e < VEC; ++e) o8[e] = __fadd_rn(to_f32(from_f32<TX>(acc0[e])), b8[e]);
            store_pack<TX, VEC>(orow + c0, o8);
        }
        if (a1) {
            if (PRE) unpack_f32<TX, VEC>(pre.xb1, b8); else load_pack<TX, VEC>(xb + c1, b8);
#pragma unroll
            for (int e = 0; e < VEC; ++e) o8[e] = __fadd_rn(to_f32(from_f32<TX>(acc1[e])), b8[e]);
            store_pack<TX, VEC>(orow + c1, o8);
        }
    } else {
        if (a0) store_pack<TX, VEC>(orow + c0, acc0);
        if (a1) store_pack<TX, VEC>(orow + c1, acc1);
    }
    if (OP == OP_WAVG && lane == 0) store_size<TS>(srow, lrow, ssum);
    if (LN) {
        // LayerNorm of the row as stored (rounded to the token dtype), the whole row is in this wave
        float part = 0.0f;
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            acc0[e] = a0 ? to_f32(from_f32<TX>(acc0[e])) : 0.0f;
            acc1[e] = a1 ? to_f32(from_f32<TX>(acc1[e])) : 0.0f;
            part += acc0[e] + acc1[e];
        }
        const float mean = wave_sum(part) / (float)C;
        part = 0.0f;
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            const float d0 = a0 ? acc0[e] - mean : 0.0f, d1 = a1 ? acc1[e] - mean : 0.0f;
            part += d0 * d0 + d1 * d1;
        }
        const float rstd = 1.0f / __builtin_sqrtf(wave_sum(part) / (float)C + ln->eps);
        const TX *lw = reinterpret_cast<const TX *>(ln->weight), *lb = reinterpret_cast<const TX *>(ln->bias);
        if (a0) {
            float w8[VEC], b8[VEC];
            if (PRE) { unpack_f32<TX, VEC>(pre.w0, w8); unpack_f32<TX, VEC>(pre.b0, b8); }
            else { load_pack<TX, VEC>(lw + c0, w8); load_pack<TX, VEC>(lb + c0, b8); }
#pragma unroll
            for (int e = 0; e < VEC; ++e) acc0[e] = (acc0[e] - mean) * rstd * w8[e] + b8[e];
            store_pack<TX, VEC>(yrow + c0, acc0);
        }
        if (a1) {
            float w8[VEC], b8[VEC];
            if (PRE) { unpack_f32<TX, VEC>(pre.w1, w8); unpack_f32<TX, VEC>(pre.b1, b8); }
            else { load_pack<TX, VEC>(lw + c1, w8); load_pack<TX, VEC>(lb + c1, b8); }
#pragma unroll
            for (int e = 0; e < VEC; ++e) acc1[e] = (acc1[e] - mean) * rstd * w8[e] + b8[e];
            store_pack<TX, VEC>(yrow + c1, acc1);
        }
    }
}

// merge_dst_row for the launches whose whole index list fits one lane each (r <= 64) and whose rows are at most two
// 16-byte chunks per lane: the form the edge waves of TimeSformer / Motionformer's frame groups run (196 tokens, r up to
// 32: a third to all of the destinations receive sources, so this path IS the kernel there).  merge_dst_row walks five
// dependent memory round trips (dst_idx[k] -> own row | dst_idx scan -> src_idx -> source sizes -> source rows); here
// lane L holds dst_idx[L], src_idx[L] and the keep flag of rank L from ONE batch of loads, every decision (is k the first
// edge into its destination, which ranks merge into it, in which order) is a ballot over registers, and the second
// batch holds everything else at once: the own row, the first NB source rows (with their residual rows), all sizes, the
// bias / LayerNorm constants.  Two round trips.  Arithmetic and order are merge_dst_row's (own term, then the sources
// in rank = lane order; shared tail dst_row_finish), so the rows are bit-identical.
// Returns without doing anything when rank k is not the first edge into its destination.
template <typename TX, typename TS, int VEC, int OP, bool LN>
__device__ __forceinline__ void merge_dst_row_r64(const TX *__restrict__ xg, const TS *__restrict__ sg, int C,
                                                  int64_t tstride, int r, int g, int k,
                                                  const int64_t *__restrict__ srcg, const int64_t *__restrict__ dstg,
                                                  const uint8_t *__restrict__ keep, TX *__restrict__ og,
                                                  int64_t ostride, TS *__restrict__ sog, TS *__restrict__ log, int U,
                                                  int distill, int lane, const LnArgs *ln, TX *__restrict__ yg,
                                                  const TX *__restrict__ ag, int64_t astride) {
    typedef Pack<TX, VEC> __attribute__((aligned(sizeof(TX) * VEC))) PK;
    constexpr int NB = 1;  // source rows requested together with the own row
    // ---- batch 1: the group's index lists, one rank per lane
    const int li = lane < r ? lane : 0;
    const int d_l = lane < r ? (int)dstg[li] : -1;
    const int s_l = (int)srcg[li];
    const int keep_l = keep ? (int)keep[(int64_t)g * r + li] : 1;
    const int j = __builtin_amdgcn_readlane(d_l, k);
    const unsigned long long mk = __ballot(d_l == j);  // the ranks that merge into j, rank order = bit order
    if ((int)__ffsll((long long)mk) - 1 != k) return;  // an earlier rank builds this destination
    const bool kill = keep && OP != OP_DROP && (__ballot((d_l == j) && keep_l == 0) != 0ull);
    // ---- batch 2: everything the row needs
    const int t = 2 * j + 1;
    const bool has_s = (OP == OP_WAVG) && sg;
    const TS sz_raw = (has_s ? sg : reinterpret_cast<const TS *>(xg))[has_s ? 2 * s_l : 0];  // size of rank `lane`'s source
    const TS own_raw = (has_s ? sg : reinterpret_cast<const TS *>(xg))[has_s ? t : 0];
    const int c0 = lane * VEC, c1 = (WAVE + lane) * VEC;
    const bool a0 = c0 < C, a1 = c1 < C;
    const int c0s = a0 ? c0 : 0, c1s = a1 ? c1 : 0;  // (loads are unconditional: a lane without a chunk re-reads column 0)
    const bool add = LN && ag;
    const TX *xr = xg + (int64_t)t * tstride;
    const TX *ar = add ? ag + (int64_t)t * astride : xr;
    const PK x0 = *reinterpret_cast<const PK *>(xr + c0s), x1 = *reinterpret_cast<const PK *>(xr + c1s);
    PK y0 = x0, y1 = x1;
    if (add) { y0 = *reinterpret_cast<const PK *>(ar + c0s); y1 = *reinterpret_cast<const PK *>(ar + c1s); }
    unsigned long long rest = mk;
    int bsel[NB];
    bool have[NB];
    PK p0[NB], p1[NB], q0[NB], q1[NB];
#pragma unroll
    for (int u = 0; u < NB; ++u) {
        have[u] = rest != 0ull;
        bsel[u] = have[u] ? (int)__ffsll((long long)rest) - 1 : k;
        rest = have[u] ? (rest & (rest - 1ull)) : rest;
        const int tsu = 2 * __builtin_amdgcn_readlane(s_l, bsel[u]);
        const TX *sr = xg + (int64_t)tsu * tstride;
        p0[u] = *reinterpret_cast<const PK *>(sr + c0s);
        p1[u] = *reinterpret_cast<const PK *>(sr + c1s);
        if (add) {
            const TX *sa = ag + (int64_t)tsu * astride;
            q0[u] = *reinterpret_cast<const PK *>(sa + c0s);
            q1[u] = *reinterpret_cast<const PK *>(sa + c1s);
        }
    }
    RowConsts<TX, VEC> rc;
    if (LN) {
        // (every field is loaded, the bias chunks from the weight when there is no folded bias: no conditional
        // initialisation, so the struct lives in registers)
        const TX *lw = reinterpret_cast<const TX *>(ln->weight), *lb = reinterpret_cast<const TX *>(ln->bias);
        const TX *xb = ln->xbias ? reinterpret_cast<const TX *>(ln->xbias) : lw;
        rc.w0 = *reinterpret_cast<const PK *>(lw + c0s);
        rc.w1 = *reinterpret_cast<const PK *>(lw + c1s);
        rc.b0 = *reinterpret_cast<const PK *>(lb + c0s);
        rc.b1 = *reinterpret_cast<const PK *>(lb + c1s);
        rc.xb0 = *reinterpret_cast<const PK *>(xb + c0s);
        rc.xb1 = *reinterpret_cast<const PK *>(xb + c1s);
    }
    // ---- arithmetic, merge_dst_row's order
    const float sz_l = has_s ? to_f32(sz_raw) : 1.0f;
    const float s_own = has_s ? to_f32(own_raw) : 1.0f;
    float acc0[VEC], acc1[VEC];
    {
        const Pack<TX, VEC> s0 = add ? add_packs<TX, VEC>(x0, y0) : (Pack<TX, VEC>)x0;
        const Pack<TX, VEC> s1 = add ? add_packs<TX, VEC>(x1, y1) : (Pack<TX, VEC>)x1;
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            acc0[e] = to_f32(s0.e[e]);
            acc1[e] = to_f32(s1.e[e]);
        }
    }
    float ssum = s_own;
    int cnt = 1;
    if (OP == OP_WAVG) {
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            acc0[e] = __fmul_rn(acc0[e], s_own);
            acc1[e] = __fmul_rn(acc1[e], s_own);
        }
    }
    if (kill) {
        if (OP == OP_WAVG) ssum = __fmul_rn(ssum, 0.0f);
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            acc0[e] = __fmul_rn(acc0[e], 0.0f);
            acc1[e] = __fmul_rn(acc1[e], 0.0f);
        }
    }
    for (;;) {
#pragma unroll
        for (int u = 0; u < NB; ++u) {
            if (!have[u]) continue;  // (wave-uniform)
            const float sq = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(sz_l), bsel[u]));
            const Pack<TX, VEC> v0 = add ? add_packs<TX, VEC>(p0[u], q0[u]) : (Pack<TX, VEC>)p0[u];
            const Pack<TX, VEC> v1 = add ? add_packs<TX, VEC>(p1[u], q1[u]) : (Pack<TX, VEC>)p1[u];
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                const float f0 = to_f32(v0.e[e]), f1 = to_f32(v1.e[e]);
                acc0[e] = reduce_step<OP>(acc0[e], (OP == OP_WAVG) ? __fmul_rn(f0, sq) : f0);
                acc1[e] = reduce_step<OP>(acc1[e], (OP == OP_WAVG) ? __fmul_rn(f1, sq) : f1);
            }
            if (OP == OP_WAVG) ssum = __fadd_rn(ssum, sq);
            ++cnt;
        }
        if (rest == 0ull) break;
        // a destination with more than NB sources (rare): the next NB, one more round trip
        // (the block above a second time, on purpose: as one lambda k_merge_rows_fast<wavg, LN> compiles to other code)
#pragma unroll
        for (int u = 0; u < NB; ++u) {
            have[u] = rest != 0ull;
            bsel[u] = have[u] ? (int)__ffsll((long long)rest) - 1 : k;
            rest = have[u] ? (rest & (rest - 1ull)) : rest;
            const int tsu = 2 * __builtin_amdgcn_readlane(s_l, bsel[u]);
            const TX *sr = xg + (int64_t)tsu * tstride;
            p0[u] = *reinterpret_cast<const PK *>(sr + c0s);
            p1[u] = *reinterpret_cast<const PK *>(sr + c1s);
            if (add) {
                const TX *sa = ag + (int64_t)tsu * astride;
                q0[u] = *reinterpret_cast<const PK *>(sa + c0s);
                q1[u] = *reinterpret_cast<const PK *>(sa + c1s);
            }
        }
    }
    const int o = out_row_dst(j, U, distill);
    dst_row_finish<TX, TS, VEC, OP, LN, LN>(acc0, acc1, a0, a1, c0, c1, ssum, cnt, C, og + (int64_t)o * ostride,
                                            sog ? sog + o : nullptr, log ? log + o : nullptr, ln,
                                            LN ? yg + (int64_t)o * ostride : nullptr, lane, rc);
}

// One destination row (odd token 2j+1 plus every source merged into it), whole wave, contract order:
// own term first, then the sources in src_idx (rank) order found by ballot-scanning dst_idx.
// Two shapes of the same arithmetic:
//   * rows of at most 2*64 lane-chunks (C <= 1024 bf16 / 512 fp32 with 16-byte lanes): the sources of one
//     64-rank block are compacted onto lanes 0..nsrc-1 (ds_permute), their tokens and sizes fetched as ONE
//     vector load each, and their row chunks fetched four sources at a time before the sequential adds --
//     a destination with k sources costs ~2 + k/4 dependent memory round trips instead of ~2k;
//   * anything wider: the plain sequential loop.
template <typename TX, typename TS, int VEC, int OP, bool LN = false>
__device__ __forceinline__ void merge_dst_row(const TX *__restrict__ xg, const TS *__restrict__ sg, int C,
                                              int64_t tstride, int r, int g, int j,
                                              const int64_t *__restrict__ srcg,
                                              const int64_t *__restrict__ dstg, const uint8_t *__restrict__ keep,
                                              TX *__restrict__ orow, TS *__restrict__ srow, int lane,
                                              const LnArgs *ln = nullptr, TX *__restrict__ yrow = nullptr,
                                              const TX *__restrict__ ag = nullptr, TS *__restrict__ lrow = nullptr,
                                              int64_t astride = 0) {
    const int t = 2 * j + 1;
    const TX *xr = xg + (int64_t)t * tstride;
    float s_own = 1.0f;
    if (OP == OP_WAVG) s_own = sg ? to_f32(sg[t]) : 1.0f;
    const bool narrow_row = C <= 2 * WAVE * VEC;
    constexpr int NB = VEC >= 8 ? 2 : 4;  // source rows fetched together (register budget)

    if (narrow_row) {
        const int c0 = lane * VEC, c1 = (WAVE + lane) * VEC;
        const bool a0 = c0 < C, a1 = c1 < C;
        typedef Pack<TX, VEC> __attribute__((aligned(sizeof(TX) * VEC))) PKA;
        float acc0[VEC], acc1[VEC];
        if (LN && ag) {
            const TX *ar = ag + (int64_t)t * astride;
            PKA x0, x1, y0, y1;
            if (a0) { x0 = *reinterpret_cast<const PKA *>(xr + c0); y0 = *reinterpret_cast<const PKA *>(ar + c0); }
            if (a1) { x1 = *reinterpret_cast<const PKA *>(xr + c1); y1 = *reinterpret_cast<const PKA *>(ar + c1); }
            if (a0) { const Pack<TX, VEC> s0 = add_packs<TX, VEC>(x0, y0);
#pragma unroll
                for (int e = 0; e < VEC; ++e) acc0[e] = to_f32(s0.e[e]); }
            if (a1) { const Pack<TX, VEC> s1 = add_packs<TX, VEC>(x1, y1);
#pragma unroll
                for (int e = 0; e < VEC; ++e) acc1[e] = to_f32(s1.e[e]); }
        } else {
            if (a0) load_pack<TX, VEC>(xr + c0, acc0);
            if (a1) load_pack<TX, VEC>(xr + c1, acc1);
        }
        // hybrid: does any incoming edge fall below the threshold (merge.py:326)?
        bool kill = false;
        if (keep && OP != OP_DROP) {
            for (int base = 0; base < r; base += WAVE) {
                const int k = base + lane;
                const bool m = (k < r) && ((int)dstg[k] == j);
                kill = kill || (__ballot(m && keep[(int64_t)g * r + k] == 0) != 0ull);
            }
        }
        float ssum = s_own;
        int cnt = 1;
        if (OP == OP_WAVG) {
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                if (a0) acc0[e] = __fmul_rn(acc0[e], s_own);
                if (a1) acc1[e] = __fmul_rn(acc1[e], s_own);
            }
        }
        if (kill) {
            if (OP == OP_WAVG) ssum = __fmul_rn(ssum, 0.0f);
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                if (a0) acc0[e] = __fmul_rn(acc0[e], 0.0f);
                if (a1) acc1[e] = __fmul_rn(acc1[e], 0.0f);
            }
        }
        if (OP != OP_DROP) {
            for (int base = 0; base < r; base += WAVE) {
                const int k = base + lane;
                const bool m = (k < r) && ((int)dstg[k] == j);
                const unsigned long long mk = __ballot(m);
                if (mk == 0ull) continue;
                const int nsrc = __popcll(mk);
                // lane L < nsrc learns the lane (= rank offset) of the L-th source of this block
                const int myrank = __popcll(mk & ((1ull << lane) - 1ull));
                const int kL = __builtin_amdgcn_ds_permute(m ? myrank * 4 : 63 * 4 + 256, m ? lane : 0);
                int tsL = 0;
                float sL = 1.0f;
                if (lane < nsrc) {
                    tsL = 2 * (int)srcg[base + kL];
                    if (OP == OP_WAVG && sg) sL = to_f32(sg[tsL]);
                }
                for (int e0 = 0; e0 < nsrc; e0 += NB) {
                    typedef Pack<TX, VEC> __attribute__((aligned(sizeof(TX) * VEC))) PK;
                    PK p0[NB], p1[NB];  // raw chunks of up to NB source rows, all in flight together
                    PK q0[NB], q1[NB];  // ... and of the addend rows when the residual is fused
                    float sq[NB];
#pragma unroll
                    for (int u = 0; u < NB; ++u) {
                        const int e = (e0 + u < nsrc) ? e0 + u : nsrc - 1;
                        const int tsu = __builtin_amdgcn_readlane(tsL, e);
                        sq[u] = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(sL), e));
                        const TX *sr = xg + (int64_t)tsu * tstride;
                        if (a0) p0[u] = *reinterpret_cast<const PK *>(sr + c0);
                        if (a1) p1[u] = *reinterpret_cast<const PK *>(sr + c1);
                        if (LN && ag) {
                            const TX *sa = ag + (int64_t)tsu * astride;
                            if (a0) q0[u] = *reinterpret_cast<const PK *>(sa + c0);
                            if (a1) q1[u] = *reinterpret_cast<const PK *>(sa + c1);
                        }
                    }
                    if (LN && ag) {
#pragma unroll
                        for (int u = 0; u < NB; ++u) {
                            if (a0) p0[u] = add_packs<TX, VEC>(p0[u], q0[u]);
                            if (a1) p1[u] = add_packs<TX, VEC>(p1[u], q1[u]);
                        }
                    }
#pragma unroll
                    for (int u = 0; u < NB; ++u) {
                        if (e0 + u < nsrc) {
#pragma unroll
                            for (int e = 0; e < VEC; ++e) {
                                if (a0) {
                                    const float v = to_f32(p0[u].e[e]);
                                    acc0[e] = reduce_step<OP>(acc0[e], (OP == OP_WAVG) ? __fmul_rn(v, sq[u]) : v);
                                }
                                if (a1) {
                                    const float v = to_f32(p1[u].e[e]);
                                    acc1[e] = reduce_step<OP>(acc1[e], (OP == OP_WAVG) ? __fmul_rn(v, sq[u]) : v);
                                }
                            }
                            if (OP == OP_WAVG) ssum = __fadd_rn(ssum, sq[u]);
                            ++cnt;
                        }
                    }
                }
            }
        }
        dst_row_finish<TX, TS, VEC, OP, LN>(acc0, acc1, a0, a1, c0, c1, ssum, cnt, C, orow, srow, lrow, ln, yrow, lane);
        return;
    }

    // wide rows: sequential form
    unsigned long long mask0 = 0ull;
    bool kill = false;
    if (OP != OP_DROP) {
        for (int base = 0; base < r; base += WAVE) {
            const int k = base + lane;
            const bool m = (k < r) && ((int)dstg[k] == j);
            const unsigned long long mk = __ballot(m);
            if (base == 0) mask0 = mk;
            if (keep) kill = kill || (__ballot(m && keep[(int64_t)g * r + k] == 0) != 0ull);
        }
    }
    float ssum = s_own;
    int cnt = 1;
    if (OP == OP_WAVG) {
        if (kill) ssum = __fmul_rn(ssum, 0.0f);
    }
    bool first_chunk = true;
    for (int c0 = 0; c0 < C; c0 += WAVE * VEC) {
        const int c = c0 + lane * VEC;
        const bool act = c < C;
        float acc[VEC];
        if (act) {
            load_pack<TX, VEC>(xr + c, acc);
            if (OP == OP_WAVG) {
#pragma unroll
                for (int e = 0; e < VEC; ++e) acc[e] = __fmul_rn(acc[e], s_own);
            }
            if (kill) {
#pragma unroll
                for (int e = 0; e < VEC; ++e) acc[e] = __fmul_rn(acc[e], 0.0f);
            }
        }
        if (OP != OP_DROP) {
            for (int base = 0; base < r; base += WAVE) {
                unsigned long long mk;
                if (base == 0) mk = mask0;
                else {
                    const int k = base + lane;
                    mk = __ballot((k < r) && ((int)dstg[k] == j));
                }
                while (mk) {
                    const int b = __ffsll((long long)mk) - 1;
                    mk &= mk - 1ull;
                    const int ts = 2 * (int)srcg[base + b];
                    float s2 = 1.0f;
                    if (OP == OP_WAVG) s2 = sg ? to_f32(sg[ts]) : 1.0f;
                    if (act) {
                        float v[VEC];
                        load_pack<TX, VEC>(xg + (int64_t)ts * tstride + c, v);
#pragma unroll
                        for (int e = 0; e < VEC; ++e) {
                            float p = (OP == OP_WAVG) ? __fmul_rn(v[e], s2) : v[e];
                            acc[e] = reduce_step<OP>(acc[e], p);
                        }
                    }
                    if (first_chunk) {
                        if (OP == OP_WAVG) ssum = __fadd_rn(ssum, s2);
                        ++cnt;
                    }
                }
            }
        }
        first_chunk = false;
        if (act) {
            if (OP == OP_WAVG) {
#pragma unroll
                for (int e = 0; e < VEC; ++e) acc[e] = __fdiv_rn(acc[e], ssum);
            } else if (OP == TOME_MEAN) {
                if (cnt > 1) {
                    const float fc = (float)cnt;
#pragma unroll
                    for (int e = 0; e < VEC; ++e) acc[e] = __fdiv_rn(acc[e], fc);
                }
            }
            store_pack<TX, VEC>(orow + c, acc);
        }
    }
    if (OP == OP_WAVG && lane == 0) store_size<TS>(srow, lrow, ssum);
}

// Generic form: one wave per output row, any C / alignment / r.  (The hot shapes go through
// k_merge_rows_fast below; this one serves odd channel counts such as the size column or source matrices.)
template <typename TX, typename TS, int VEC, int OP>
__global__ __launch_bounds__(256) void k_merge_rows(const TX *__restrict__ x, const TS *__restrict__ size,
                                                    int n, int T_, int C, int r,
                                                    const int64_t *__restrict__ src_idx,
                                                    const int64_t *__restrict__ dst_idx,
                                                    const int64_t *__restrict__ unm_idx, int distill,
                                                    const uint8_t *__restrict__ keep, TX *__restrict__ xout,
                                                    TS *__restrict__ sout, TokLayout lin, TokLayout lout,
                                                    TS *__restrict__ lsout) {
    const int lane = threadIdx.x & 63;
    const int To = T_ - r;
    const int64_t row = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (row >= (int64_t)n * To) return;
    const int g = (int)(row / To);
    const int o = (int)(row - (int64_t)g * To);
    const int T1 = (T_ + 1) >> 1, U = T1 - r;
    bool is_dst;
    int idx;
    decode_out_row(o, U, distill, is_dst, idx);

    const TX *xg = group_ptr(x, lin, g);
    const TS *sg = size ? size + (int64_t)g * T_ : nullptr;
    TX *orow = group_ptr(xout, lout, g) + (int64_t)o * lout.tok_stride;
    if (!is_dst) {
        const int t = 2 * (int)unm_idx[(int64_t)g * U + idx];
        const TX *xr = xg + (int64_t)t * lin.tok_stride;
        float s = 1.0f;
        if (OP == OP_WAVG) s = sg ? to_f32(sg[t]) : 1.0f;
        for (int c = lane * VEC; c < C; c += WAVE * VEC) {
            float v[VEC];
            load_pack<TX, VEC>(xr + c, v);
            if (OP == OP_WAVG) {
#pragma unroll
                for (int e = 0; e < VEC; ++e) v[e] = __fdiv_rn(__fmul_rn(v[e], s), s);
            }
            store_pack<TX, VEC>(orow + c, v);
        }
        if (OP == OP_WAVG && lane == 0) store_size<TS>(sout + row, lsout ? lsout + row : nullptr, s);
        return;
    }
    merge_dst_row<TX, TS, VEC, OP>(xg, sg, C, lin.tok_stride, r, g, idx, src_idx ? src_idx + (int64_t)g * r : nullptr,
                                   dst_idx ? dst_idx + (int64_t)g * r : nullptr, keep, orow,
                                   sout ? sout + row : nullptr, lane, nullptr, nullptr, nullptr,
                                   lsout ? lsout + row : nullptr);
}

// ------------------------------------------------------------------------------------------------
// k_merge_rows_fast: the HBM-bound form for rows made of whole 16-byte chunks (C*sizeof(TX) % 16 == 0,
// at most 384 chunks per R rows).  A wave owns R consecutive OUTPUT rows of one group, flattens their
// R*cpr 16-byte chunks over its lanes (6 chunks per lane, every lane busy, stores contiguous across the
// R rows) and issues all of its loads before touching any of them, so ~6 KiB per wave are in flight.
// The slab walk -- per-row facts, slot map, edge rows, the rows that move as raw bits -- and what keeps its loads
// together is tome_merge_slab.h; the few rows that receive sources are finished by merge_dst_row.  Launch geometry:
// grid.x = the blocks of one group (streaming waves, then r edge waves), grid.(y, z) = the group, class-token rows
// behind the groups -- no wave starts with an integer division.
// ------------------------------------------------------------------------------------------------
#define FAST_NIT 6
#define FAST_MAXR 4

// How the hardware workgroups of a k_merge_rows_fast launch map onto (group, block of the group).  on = 0: grid
// (blocks of one group, group.y, group.z) as launched.  on = 1: a 1-D grid of 8 * per_xcd workgroups renumbered so that
// each of the 8 XCDs (workgroup L -> XCD L % 8) walks whole groups in order.
struct MergeSched {
    unsigned bpg, total, per_xcd;  // blocks per group, bpg * (groups + class-row block rows), ceil(total / 8)
    int on;
    unsigned long long magic;      // ceil(2^40 / bpg)
};

// EAGER (round 3): when r is a large share of the destinations (TimeSformer / Motionformer late layers, r = 32 sweeps:
// r >= T2 / 4) the streaming waves first wait for dst_idx and do NOT read the rows that receive sources -- those are
// read (own row + sources) by the edge waves anyway; without it they were read twice (measured, tools/regroup_layers.py:
// 5.4 TB/s at 196 -> 164 tokens per group falling to 3.2 at 68 -> 36).  Costs the streaming waves of such launches one
// dependent round trip (index -> rows), which the default path avoids for the r << T2 case of the benchmark.
// OP_DROP with LN (tome_drop_ln, tome_drop_regrouped_ln): every kept row is a streamed row -- the launch has no edge
// waves and never the EAGER form; the addend, the folded bias and ln_rows below are reached as they are for the merge.
template <typename TX, typename TS, int OP, int NIT, bool LN = false, bool EAGER = false>
__global__ __launch_bounds__(256) void k_merge_rows_fast(const TX *__restrict__ x, const TS *__restrict__ size,
                                                         int n, int T_, int C, int r, int R, int cpr,
                                                         int rg_per_group, const int64_t *__restrict__ src_idx,
                                                         const int64_t *__restrict__ dst_idx,
                                                         const int64_t *__restrict__ unm_idx, int distill,
                                                         const uint8_t *__restrict__ keep, TX *__restrict__ xout,
                                                         TS *__restrict__ sout, TokLayout lin, TokLayout lout,
                                                         int cls_rows, LnArgs ln, TS *__restrict__ lsout,
                                                         MergeSched sch) {
    constexpr int VEC = 16 / sizeof(TX);
    const int lane = threadIdx.x & 63;
    const int To = T_ - r;
    // Grid: x = the blocks of ONE merge group (four waves each), (y, z) = the group -- so that no wave starts with
    // integer divisions of a flat index (they were ~250 dependent scalar instructions before the first load).  Waves
    // 0 .. rg-1 of a group stream R output rows each, the next r waves are the edge waves, the rest leave; the class
    // tokens kept aside by the regrouped callers are handled by the blocks of the (y, z) rows behind the n groups.
    // (rg_per_group = ceil((T - r) / R), from the host)
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int gy, bx;
    if (sch.on) {
        // XCD-aware numbering (MergeSched): hardware workgroup L runs on XCD L % 8; virtual block V walks the groups in
        // order WITHIN one XCD, so an XCD works on whole groups (their index lists stay in its L2) and every XCD sees the
        // same mix of streaming and edge blocks at any time, whatever gridDim.x is
        const unsigned L = blockIdx.x;
        const unsigned V = (L & 7u) * sch.per_xcd + (L >> 3);
        if (V >= sch.total) return;
        const unsigned q = (unsigned)(((unsigned long long)V * sch.magic) >> 40);  // V / bpg (exact: V * bpg < 2^40)
        gy = (int)q;
        bx = (int)(V - q * sch.bpg);
    } else {
        gy = (int)(blockIdx.z * gridDim.y + blockIdx.y);
        bx = (int)blockIdx.x;
    }
    const int lw = bx * (int)(blockDim.x >> 6) + wv;
    if (gy >= n) {
        // the class tokens kept aside by the regrouped callers (timesformer.py:89,107): plain row copies
        const int64_t b = ((int64_t)(gy - n) * sch.bpg + bx) * (blockDim.x >> 6) + wv;
        if (b < cls_rows) {
            const uint4 *src = reinterpret_cast<const uint4 *>(x + b * lin.outer_stride);
            uint4 *dst = reinterpret_cast<uint4 *>(xout + b * lout.outer_stride);
            if (!LN) {
                for (int c = lane; c < cpr; c += WAVE) dst[c] = src[c];
            } else {
                // class-token row: same fused residual and LayerNorm as the merged rows (cpr <= 128 here)
                const int c0 = lane, c1 = WAVE + lane;
                const bool a0 = c0 < cpr, a1 = c1 < cpr;
                Pack<TX, VEC> p0, p1;
                uint4 r0 = a0 ? src[c0] : uint4{0, 0, 0, 0}, r1 = a1 ? src[c1] : uint4{0, 0, 0, 0};
                __builtin_memcpy(&p0, &r0, 16);
                __builtin_memcpy(&p1, &r1, 16);
                if (ln.a_own ? ln.cls_addend != nullptr : ln.addend != nullptr) {
                    const uint4 *asrc = ln.a_own
                        ? reinterpret_cast<const uint4 *>(reinterpret_cast<const TX *>(ln.cls_addend) + b * (int64_t)C)
                        : reinterpret_cast<const uint4 *>(reinterpret_cast<const TX *>(ln.addend) + b * lin.outer_stride);
                    Pack<TX, VEC> q0, q1;
                    uint4 s0 = a0 ? asrc[c0] : uint4{0, 0, 0, 0}, s1 = a1 ? asrc[c1] : uint4{0, 0, 0, 0};
                    __builtin_memcpy(&q0, &s0, 16);
                    __builtin_memcpy(&q1, &s1, 16);
                    p0 = add_packs<TX, VEC>(p0, q0);
                    p1 = add_packs<TX, VEC>(p1, q1);
                    __builtin_memcpy(&r0, &p0, 16);
                    __builtin_memcpy(&r1, &p1, 16);
                }
                if (ln.xbias) {
                    const TX *xb = reinterpret_cast<const TX *>(ln.xbias);
                    if (a0) dst[c0] = add_xbias<TX, VEC>(r0, xb + c0 * VEC);
                    if (a1) dst[c1] = add_xbias<TX, VEC>(r1, xb + c1 * VEC);
                } else {
                    if (a0) dst[c0] = r0;
                    if (a1) dst[c1] = r1;
                }
                float t = 0.0f, u = 0.0f;
#pragma unroll
                for (int e = 0; e < VEC; ++e) t += (a0 ? to_f32(p0.e[e]) : 0.0f) + (a1 ? to_f32(p1.e[e]) : 0.0f);
                const float fc = (float)C;
                const float m = wave_sum(t) / fc;
#pragma unroll
                for (int e = 0; e < VEC; ++e) {  // centred second pass over the registers, like every other row
                    const float d0 = a0 ? to_f32(p0.e[e]) - m : 0.0f, d1 = a1 ? to_f32(p1.e[e]) - m : 0.0f;
                    u = __fmaf_rn(d0, d0, u);
                    u = __fmaf_rn(d1, d1, u);
                }
                const float rs = 1.0f / __builtin_sqrtf(wave_sum(u) / fc + ln.eps);
                const TX *lw = reinterpret_cast<const TX *>(ln.weight), *lb = reinterpret_cast<const TX *>(ln.bias);
                uint4 *ydst = reinterpret_cast<uint4 *>(reinterpret_cast<TX *>(ln.y) + b * lout.outer_stride);
                if (a0) {
                    float w8[VEC], b8[VEC];
                    load_pack<TX, VEC>(lw + c0 * VEC, w8);
                    load_pack<TX, VEC>(lb + c0 * VEC, b8);
#pragma unroll
                    for (int e = 0; e < VEC; ++e) p0.e[e] = from_f32<TX>((to_f32(p0.e[e]) - m) * rs * w8[e] + b8[e]);
                    __builtin_memcpy(&r0, &p0, 16);
                    ydst[c0] = r0;
                }
                if (a1) {
                    float w8[VEC], b8[VEC];
                    load_pack<TX, VEC>(lw + c1 * VEC, w8);
                    load_pack<TX, VEC>(lb + c1 * VEC, b8);
#pragma unroll
                    for (int e = 0; e < VEC; ++e) p1.e[e] = from_f32<TX>((to_f32(p1.e[e]) - m) * rs * w8[e] + b8[e]);
                    __builtin_memcpy(&r1, &p1, 16);
                    ydst[c1] = r1;
                }
            }
        }
        return;
    }
    const int g = gy;
    if (lw >= rg_per_group) {
        // edge waves: one per (group, rank k).  The wave of the FIRST edge into a destination builds that
        // row (all its sources, rank order); the others leave.  Destinations with sources therefore never
        // hold up the streaming waves above, and run concurrently with them.
        const int k = lw - rg_per_group;
        if (OP == OP_DROP || k >= r) return;
        const int64_t *dstg = dst_idx + (int64_t)g * r;
        int64_t astride;
        const TX *agp = ln_addend_rows<TX>(ln, lin, g, astride);  // (no LayerNorm: no addend, x's stride)
        if (r <= WAVE && cpr <= 2 * WAVE) {
            // the whole index list in one lane each: two memory round trips instead of five (merge_dst_row_r64)
            const int T1e = (T_ + 1) >> 1;
            merge_dst_row_r64<TX, TS, VEC, OP, LN>(
                group_ptr(x, lin, g), size ? size + (int64_t)g * T_ : nullptr, C, lin.tok_stride, r, g, k,
                src_idx + (int64_t)g * r, dstg, keep, group_ptr(xout, lout, g), lout.tok_stride,
                sout ? sout + (int64_t)g * To : nullptr, lsout ? lsout + (int64_t)g * To : nullptr, T1e - r, distill, lane,
                &ln, LN ? group_ptr(reinterpret_cast<TX *>(ln.y), lout, g) : nullptr, agp, astride);
            return;
        }
        const int j = (int)dstg[k];
        bool earlier = false;
        for (int base = 0; base < k; base += WAVE) {
            const int kk = base + lane;
            earlier = earlier || (__ballot((kk < k) && ((int)dstg[kk] == j)) != 0ull);
        }
        if (earlier) return;
        const int T1e = (T_ + 1) >> 1, Ue = T1e - r;
        const int o = out_row_dst(j, Ue, distill);
        merge_dst_row<TX, TS, VEC, OP, LN>(
            group_ptr(x, lin, g), size ? size + (int64_t)g * T_ : nullptr, C, lin.tok_stride, r, g, j,
            src_idx + (int64_t)g * r, dstg, keep, group_ptr(xout, lout, g) + (int64_t)o * lout.tok_stride,
            sout ? sout + (int64_t)g * To + o : nullptr, lane, &ln,
            LN ? group_ptr(reinterpret_cast<TX *>(ln.y), lout, g) + (int64_t)o * lout.tok_stride : nullptr,
            agp, lsout ? lsout + (int64_t)g * To + o : nullptr, astride);
        return;
    }
    const int o0 = lw * R;
    const int T1 = (T_ + 1) >> 1, U = T1 - r;
    const TX *xg = group_ptr(x, lin, g);
    TX *og = group_ptr(xout, lout, g);
    const TS *sg = size ? size + (int64_t)g * T_ : nullptr;
    const int64_t *dstg = dst_idx ? dst_idx + (int64_t)g * r : nullptr;

    // per-row facts (fwd_slab, tome_merge_slab.h): the first block of dst_idx goes out together with its unm_idx reads.
    // (Several R-row slabs per wave behind ONE index round trip were measured in round 2: no gain for this kernel, a
    // loss for the plain merge -- the kernel is bound by its vector instructions, not by latency.)
    const int d_first = (OP != OP_DROP && lane < r) ? (int)dstg[lane] : -2;
    const bool load_size = (OP == OP_WAVG) && sg;  // wave-uniform
    const FwdSlab<TS> f = fwd_slab<TS>(load_size ? sg : reinterpret_cast<const TS *>(xg), unm_idx, g, o0, R, To, U,
                                       distill, lane);
    const int tok0 = f.tok0, tok1 = f.tok1, tok2 = f.tok2, tok3 = f.tok3;
    bool va0 = f.vmask & 1ull, va1 = f.vmask & 2ull, va2 = f.vmask & 4ull, va3 = f.vmask & 8ull;  // rows that exist
    if (EAGER && OP != OP_DROP) {  // (r <= 64: the host's condition -- every dst_idx entry of the group is in d_first)
        va0 = va0 && (__ballot(d_first == f.j0) == 0ull);
        va1 = va1 && (__ballot(d_first == f.j1) == 0ull);
        va2 = va2 && (__ballot(d_first == f.j2) == 0ull);
        va3 = va3 && (__ballot(d_first == f.j3) == 0ull);
    }

    // flattened chunk loop (slab_row / slab_col): every chunk of the slab requested
    const int total = R * cpr;
    uint4 raw[NIT];
    int rowof[NIT];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int q = it * WAVE + lane;
        const int rr = slab_row(cpr, it, lane), cc = slab_col(q, rr, cpr), t = SEL4(rr, tok0, tok1, tok2, tok3);
        const bool ok = SEL4(rr, va0, va1, va2, va3) && (q < total);
        rowof[it] = ok ? rr : -1;
        // unconditional: a lane without a chunk re-reads the start of the wave's first row (always a real token)
        raw[it] = ld16(reinterpret_cast<const char *>(xg + (int64_t)(ok ? t : tok0) * lin.tok_stride) + (ok ? cc : 0) * 16);
    }
    uint4 rawa[NIT];
    if (LN && ln.addend) {  // fused residual: the rows that are merged are round(x + addend)
        int64_t astride;
        const TX *agp = ln_addend_rows<TX>(ln, lin, g, astride);
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int rr = rowof[it];
            const int cc = rr < 0 ? 0 : it * WAVE + lane - rr * cpr;
            const int t = SEL4(rr < 0 ? 0 : rr, tok0, tok1, tok2, tok3);
            rawa[it] = ld16(reinterpret_cast<const char *>(agp + (int64_t)t * astride) + cc * 16);
        }
    }
    SlabEdges e{false, false, false, false};  // rows that receive sources
    if (OP != OP_DROP) e = slab_edge_rows(d_first, f.j0, f.j1, f.j2, f.j3, dstg, r, lane);
    const bool e0 = e.e0, e1 = e.e1, e2 = e.e2, e3 = e.e3;
    const bool ok0 = va0 && !e0, ok1 = va1 && !e1, ok2 = va2 && !e2, ok3 = va3 && !e3;
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int rr = rowof[it];
        const bool ok = rr >= 0 && SEL4(rr, ok0, ok1, ok2, ok3);
        rowof[it] = ok ? rr : -1;
    }
    if (LN && ln.addend) {
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            if (rowof[it] < 0) continue;
            Pack<TX, VEC> px, pa;
            __builtin_memcpy(&px, &raw[it], 16);
            __builtin_memcpy(&pa, &rawa[it], 16);
            const Pack<TX, VEC> ps = add_packs<TX, VEC>(px, pa);
            __builtin_memcpy(&raw[it], &ps, 16);
        }
    }
    // the bias folded into x' (xbias): its chunks are requested here, ahead of the stores that need them
    uint4 xbraw[NIT];
    if (LN && ln.xbias) {
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int rr = rowof[it];
            xbraw[it] = *(reinterpret_cast<const uint4 *>(ln.xbias) + (rr < 0 ? 0 : it * WAVE + lane - rr * cpr));
        }
    }
    const float my_s = (load_size && f.my_valid) ? to_f32(f.my_s_raw) : 1.0f;
    float sz0, sz1, sz2, sz3;
    lanes4(my_s, sz0, sz1, sz2, sz3);
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int rr = rowof[it];
        if (rr < 0) continue;
        const int q = it * WAVE + lane;
        const float s = SEL4(rr, sz0, sz1, sz2, sz3);
        uint4 outv = raw[it];
        if (OP == OP_WAVG && !wavg_moves_raw<TX>(s)) outv = wavg_rescaled<TX>(raw[it], s);
        const int cc = q - rr * cpr;
        char *xdst = reinterpret_cast<char *>(og + (int64_t)(o0 + rr) * lout.tok_stride) + cc * 16;
        if (LN && ln.xbias)
            st16(xdst, add_xbias<TX, VEC>(outv, reinterpret_cast<const TX *>(&xbraw[it])));
        else
            st16(xdst, outv);
        if (LN) raw[it] = outv;  // keep the merged bits: LayerNorm runs on x' itself (what is written without xbias)
    }
    if constexpr (LN) {
        // LayerNorm of the (up to) four rows of this wave as they were stored (ln_rows, tome_ln_rows.h)
        TX *yg = group_ptr(reinterpret_cast<TX *>(ln.y), lout, g);
        const int64_t ystride = lout.tok_stride;
        const LnParams<TX, NIT> prm = ln_params<TX, NIT>(reinterpret_cast<const TX *>(ln.weight),
                                                         reinterpret_cast<const TX *>(ln.bias), rowof, cpr, lane);
        Slot<TX> stored[NIT];
#pragma unroll
        for (int it = 0; it < NIT; ++it) stored[it].q[0] = raw[it];
        ln_rows<TX, TX, TX, NIT>(stored, rowof, R, cpr, C, ln.eps, prm, lane,
                                 [&](int rr, int cc, const Slot<TX> &yv) __attribute__((always_inline)) {
                                     st_slot<TX>(yg + (int64_t)(o0 + rr) * ystride, cc, yv);
                                 });
    }
    if (OP == OP_WAVG && lane < R && f.my_valid)
        slab_store_size<TS>(SEL4(lane, e0, e1, e2, e3), sout, lsout, (int64_t)g * To + o0 + lane, my_s);
}

// k_unmerge_rows: merge.py:87-100 as a scatter from the merged sequence: one wave per INPUT row; a
// destination row also lands on every even slot that was merged into it.  src and unm partition the
// even slots, so every output row is written exactly once and no zero fill is needed.
template <typename TX, int VEC>
__global__ __launch_bounds__(256) void k_unmerge_rows(const TX *__restrict__ x, int n, int T_, int C, int r,
                                                      const int64_t *__restrict__ src_idx,
                                                      const int64_t *__restrict__ dst_idx,
                                                      const int64_t *__restrict__ unm_idx,
                                                      TX *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int To = T_ - r;
    const int64_t row = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (row >= (int64_t)n * To) return;
    const int g = (int)(row / To);
    const int o = (int)(row - (int64_t)g * To);
    const int T1 = (T_ + 1) >> 1, U = T1 - r;
    const TX *xr = x + row * C;
    TX *og = out + (int64_t)g * T_ * C;
    if (o < U) {
        TX *dst = og + (int64_t)(2 * (int)unm_idx[(int64_t)g * U + o]) * C;
        for (int c = lane * VEC; c < C; c += WAVE * VEC) {
            float v[VEC];
            load_pack<TX, VEC>(xr + c, v);
            store_pack<TX, VEC>(dst + c, v);
        }
        return;
    }
    const int j = o - U;
    const int64_t *srcg = src_idx + (int64_t)g * r, *dstg = dst_idx + (int64_t)g * r;
    for (int c = lane * VEC; c < C; c += WAVE * VEC) {
        float v[VEC];
        load_pack<TX, VEC>(xr + c, v);
        store_pack<TX, VEC>(og + (int64_t)(2 * j + 1) * C + c, v);
    }
    for (int base = 0; base < r; base += WAVE) {
        const int k = base + lane;
        unsigned long long mk = __ballot((k < r) && ((int)dstg[k] == j));
        while (mk) {
            const int b = __ffsll((long long)mk) - 1;
            mk &= mk - 1ull;
            TX *dst = og + (int64_t)(2 * (int)srcg[base + b]) * C;
            for (int c = lane * VEC; c < C; c += WAVE * VEC) {
                float v[VEC];
                load_pack<TX, VEC>(xr + c, v);
                store_pack<TX, VEC>(dst + c, v);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Source tracking, first layer (merge.py:372-384 with source=None): the reference merges an identity matrix
// with mode "max" -- output row o, column t is 1 exactly when token t ends up in merged row o.  That is the
// row map of the matching, so the [n,T,T] identity and the amax over its zeros are never made:
//   k_row_map      src/dst/unm_idx -> row_map[n,T1] (for plans that were matched without one)
//   k_source_init  out[g,o,t] = (row of token t == o), one coalesced pass over the [n,T-r,T] result;
//                  drop mode (merge.py:215-271 applied to the identity): merged-away tokens have no row
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_row_map(int n, int T1, int r, int distill,
                                                 const int64_t *__restrict__ src_idx,
                                                 const int64_t *__restrict__ dst_idx,
                                                 const int64_t *__restrict__ unm_idx, int *__restrict__ row_map) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)n * T1) return;
    const int g = (int)(i / T1), k = (int)(i - (int64_t)g * T1), U = T1 - r;
    if (k < r) row_map[(int64_t)g * T1 + (int)src_idx[(int64_t)g * r + k]] = out_row_dst((int)dst_idx[(int64_t)g * r + k], U, distill);
    else row_map[(int64_t)g * T1 + (int)unm_idx[(int64_t)g * U + (k - r)]] = out_row_unm(k - r, distill);
}

__global__ __launch_bounds__(256) void k_source_init(int n, int T_, int r, int distill, int drop,
                                                     const int *__restrict__ row_map, float *__restrict__ out) {
    const int To = T_ - r, T1 = (T_ + 1) >> 1, U = T1 - r;
    const int64_t row = blockIdx.x;  // (g, o)
    const int g = (int)(row / To), o = (int)(row - (int64_t)g * To);
    const int *rm = row_map + (int64_t)g * T1;
    float *orow = out + row * T_;
    for (int t = threadIdx.x; t < T_; t += blockDim.x) {
        int rt;
        bool live = true;
        if (t & 1) rt = out_row_dst(t >> 1, U, distill);
        else {
            rt = rm[t >> 1];
            if (drop) {
                bool is_dst;
                int idx;
                decode_out_row(rt, U, distill, is_dst, idx);
                live = !is_dst;  // an even token that maps onto a destination row was merged away: dropped
            }
        }
        orow[t] = (live && rt == o) ? 1.0f : 0.0f;
    }
}

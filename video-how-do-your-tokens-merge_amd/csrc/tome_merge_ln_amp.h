// tome_merge_ln_amp.h -- part of the single translation unit csrc/tome_kernels.hip (the residual add + merge + LayerNorm
// launch for a model under autocast: tome_merge_wavg_ln_amp, tome_drop_ln_amp).
#pragma once
// ------------------------------------------------------------------------------------------------
// k_merge_rows_ln_amp: k_merge_rows_fast<.., LN = true> (csrc/tome_merge.h) for the tensors a block has under
// torch.autocast with fp32 master weights (tools/train_net.py:123, tome/utils.py:54):
//     x = x + attn; x, size = merge_wavg(merge, x, size); self.norm2(x)       tome/patch/videomae.py:20-27
//     the same in the ViViT layer                                              tome/patch/vivit.py:35-41
// TX: the residual stream (x, x_out), 16-bit or fp32; TA: the addend; TY: y, the 16-bit autocast dtype; TS: the sizes;
// LayerNorm weight and bias fp32.
//   16-bit stream: x' = round16(x + a), the bits k_merge_rows_fast merges
//   fp32 stream:   x' = x + (float)a, the fp32 sum, one rounding -- `x + a.float()` bit for bit
// The merge is tome_merge_wavg's contract (fp32 products, the destination's own term first, then its sources in src_idx
// order, one division, one rounding to TX -- none for fp32); the LayerNorm is ln_rows (tome_ln_rows.h: statistics from the
// STORED row, two passes, centred variance, fp32 parameters, y rounded once to TY).
// Work layout: the lane SLOTS of k_add_ln_rows (8 channels: one 16-byte move of a 16-bit row, two of an fp32 one), so
// rows per wave and slots per lane are those of the 16-bit launch.  The slab walk is k_merge_rows_fast's, from the same
// functions (tome_merge_slab.h); rows that receive sources are left to edge waves (one per rank, the first edge into a
// destination builds it); grid.x = the blocks of one group, grid.(y, z) = the group; OP_DROP has no edge waves.  Flat
// layout only, no folded bias.
// ------------------------------------------------------------------------------------------------
// One destination row (odd token 2j+1 plus every source merged into it) by a whole wave, two slots per lane (C <= 1024):
// merge_dst_row's arithmetic and order, then the LayerNorm of the row as stored.  k: the rank whose edge wave this is;
// returns without a store when an earlier rank merges into the same destination.
template <typename TX, typename TA, typename TY, typename TS, int OP>
__device__ __forceinline__ void merge_dst_row_amp(const TX *__restrict__ xg, const TA *__restrict__ ag,
                                                  const TS *__restrict__ sg, int C, int cpr, int r, int g, int k,
                                                  const int64_t *__restrict__ srcg, const int64_t *__restrict__ dstg,
                                                  const uint8_t *__restrict__ keep, TX *__restrict__ og,
                                                  TY *__restrict__ yg, TS *__restrict__ sog, TS *__restrict__ log,
                                                  int U, int distill, int lane, const float *__restrict__ lw,
                                                  const float *__restrict__ lb, float eps) {
    constexpr int VEC = 8;
    const int j = (int)dstg[k];
    // which rank is the first edge into j, and (hybrid, merge.py:326) does any edge into j fall below the threshold
    int first = -1;
    bool kill = false;
    for (int base = 0; base < r; base += WAVE) {
        const int kk = base + lane;
        const bool m = (kk < r) && ((int)dstg[kk] == j);
        const unsigned long long mk = __ballot(m);
        if (first < 0 && mk != 0ull) first = base + (int)__ffsll((long long)mk) - 1;
        if (keep) kill = kill || (__ballot(m && keep[(int64_t)g * r + kk] == 0) != 0ull);
    }
    if (first != k) return;  // (wave-uniform)
    const int t = 2 * j + 1;
    const int c0 = lane, c1 = WAVE + lane;
    const bool a0 = c0 < cpr, a1 = c1 < cpr;
    const int c0s = a0 ? c0 : 0, c1s = a1 ? c1 : 0;  // (unconditional loads: a lane without a slot re-reads slot 0)
    const bool add = ag != nullptr, has_s = sg != nullptr;
    const TX *xr = xg + (int64_t)t * C;
    Slot<TX> x0 = ld_slot<TX>(xr, c0s), x1 = ld_slot<TX>(xr, c1s);
    if (add) {
        const TA *ar = ag + (int64_t)t * C;
        const Slot<TA> y0 = ld_slot<TA>(ar, c0s), y1 = ld_slot<TA>(ar, c1s);
        x0 = slot_add<TX, TA>(x0, y0);
        x1 = slot_add<TX, TA>(x1, y1);
    }
    const float s_own = has_s ? to_f32(sg[t]) : 1.0f;
    float acc0[VEC], acc1[VEC];
    slot_f32<TX>(x0, acc0);
    slot_f32<TX>(x1, acc1);
    float ssum = s_own;
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
        acc0[e] = __fmul_rn(acc0[e], s_own);
        acc1[e] = __fmul_rn(acc1[e], s_own);
    }
    if (kill) {
        ssum = __fmul_rn(ssum, 0.0f);
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            acc0[e] = __fmul_rn(acc0[e], 0.0f);
            acc1[e] = __fmul_rn(acc1[e], 0.0f);
        }
    }
    for (int base = 0; base < r; base += WAVE) {
        const int kk = base + lane;
        const int ks = kk < r ? kk : 0;
        const int d_l = kk < r ? (int)dstg[ks] : -1;
        unsigned long long mk = __ballot(d_l == j);
        if (mk == 0ull) continue;
        // the block's source tokens and sizes, one rank per lane: one vector load each
        const int ts_l = 2 * (int)srcg[ks];
        const float sz_l = has_s ? to_f32(sg[ts_l]) : 1.0f;
        while (mk) {
            const int b = (int)__ffsll((long long)mk) - 1;
            mk &= mk - 1ull;
            const int ts = __builtin_amdgcn_readlane(ts_l, b);
            const float sq = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(sz_l), b));
            const TX *sr = xg + (int64_t)ts * C;
            Slot<TX> p0 = ld_slot<TX>(sr, c0s), p1 = ld_slot<TX>(sr, c1s);
            if (add) {
                const TA *sa = ag + (int64_t)ts * C;
                const Slot<TA> q0 = ld_slot<TA>(sa, c0s), q1 = ld_slot<TA>(sa, c1s);
                p0 = slot_add<TX, TA>(p0, q0);
                p1 = slot_add<TX, TA>(p1, q1);
            }
            float v0[VEC], v1[VEC];
            slot_f32<TX>(p0, v0);
            slot_f32<TX>(p1, v1);
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                acc0[e] = __fadd_rn(acc0[e], __fmul_rn(v0[e], sq));
                acc1[e] = __fadd_rn(acc1[e], __fmul_rn(v1[e], sq));
            }
            ssum = __fadd_rn(ssum, sq);
        }
    }
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
        acc0[e] = __fdiv_rn(acc0[e], ssum);
        acc1[e] = __fdiv_rn(acc1[e], ssum);
    }
    const int o = out_row_dst(j, U, distill);
    const Slot<TX> o0 = f32_slot<TX>(acc0), o1 = f32_slot<TX>(acc1);
    TX *orow = og + (int64_t)o * C;
    if (a0) st_slot<TX>(orow, c0, o0);
    if (a1) st_slot<TX>(orow, c1, o1);
    if (lane == 0) store_size<TS>(sog + o, log ? log + o : nullptr, ssum);
    // LayerNorm of the row as stored: ln_rows' body behind the mean (NIT = 2, R = 1).  The mean is taken here: the
    // lane's two sums are added to each other, not onto ln_row_means' 0.0f, and 0.0f + t is not t for a negative zero.
    const Slot<TX> stored[2] = {o0, o1};
    const int rowof[2] = {a0 ? 0 : -1, a1 ? 0 : -1};
    const LnParams<float, 2> prm = ln_params<float, 2>(lw, lb, rowof, cpr, lane);
    const float inv_c = __builtin_amdgcn_rcpf((float)C);
    const float m = wave_total((a0 ? slot_sum<TX>(o0) : 0.0f) + (a1 ? slot_sum<TX>(o1) : 0.0f)) * inv_c;
    TY *yrow = yg + (int64_t)o * C;
    ln_rows_finish<TX, float, TY, 2>(stored, rowof, 1, cpr, inv_c, eps, Row4{m, 0.0f, 0.0f, 0.0f}, prm, lane,
                                     [&](int, int cc, const Slot<TY> &yv) __attribute__((always_inline)) {
                                         st_slot<TY>(yrow, cc, yv);
                                     });
}

template <typename TX, typename TA, typename TY, typename TS, int OP, int NIT>
__global__ __launch_bounds__(256) void k_merge_rows_ln_amp(const TX *__restrict__ x, const TA *__restrict__ a,
                                                           const TS *__restrict__ size, int n, int T_, int C, int r,
                                                           int R, int cpr, int rg_per_group,
                                                           const int64_t *__restrict__ src_idx,
                                                           const int64_t *__restrict__ dst_idx,
                                                           const int64_t *__restrict__ unm_idx, int distill,
                                                           const uint8_t *__restrict__ keep,
                                                           const float *__restrict__ lw, const float *__restrict__ lb,
                                                           float eps, TX *__restrict__ xout, TY *__restrict__ y,
                                                           TS *__restrict__ sout, TS *__restrict__ lsout) {
    const int lane = threadIdx.x & 63;
    const int To = T_ - r;
    // grid: x = the blocks of ONE group (streaming waves, then the r edge waves), (y, z) = the group
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int g = (int)(blockIdx.z * gridDim.y + blockIdx.y);
    if (g >= n) return;
    const int wg = (int)blockIdx.x * (int)(blockDim.x >> 6) + wv;
    const bool add = a != nullptr;
    const TX *xg = x + (int64_t)g * T_ * C;
    const TA *ag = add ? a + (int64_t)g * T_ * C : nullptr;
    TX *og = xout + (int64_t)g * To * C;
    TY *yg = y + (int64_t)g * To * C;
    const TS *sg = (OP == OP_WAVG && size) ? size + (int64_t)g * T_ : nullptr;
    const int T1 = (T_ + 1) >> 1, U = T1 - r;
    if (wg >= rg_per_group) {
        const int k = wg - rg_per_group;
        if (OP == OP_DROP || k >= r) return;
        merge_dst_row_amp<TX, TA, TY, TS, OP>(xg, ag, sg, C, cpr, r, g, k, src_idx + (int64_t)g * r,
                                              dst_idx + (int64_t)g * r, keep, og, yg, sout + (int64_t)g * To,
                                              lsout ? lsout + (int64_t)g * To : nullptr, U, distill, lane, lw, lb, eps);
        return;
    }
    const int o0 = wg * R;
    const int64_t *dstg = OP != OP_DROP ? dst_idx + (int64_t)g * r : nullptr;
    // per-row facts, the slot walk and the edge rows: tome_merge_slab.h.  The first block of dst_idx goes out with
    // fwd_slab's unm_idx reads; which rows receive sources is decided after the row loads have been issued.
    const int d_first = (OP != OP_DROP && lane < r) ? (int)dstg[lane] : -2;
    const bool load_size = sg != nullptr;  // wave-uniform
    const FwdSlab<TS> f = fwd_slab<TS>(load_size ? sg : reinterpret_cast<const TS *>(xg), unm_idx, g, o0, R, To, U,
                                       distill, lane);
    const int tok0 = f.tok0, tok1 = f.tok1, tok2 = f.tok2, tok3 = f.tok3;
    const bool va0 = f.vmask & 1ull, va1 = f.vmask & 2ull, va2 = f.vmask & 4ull, va3 = f.vmask & 8ull;

    const int total = R * cpr;
    Slot<TX> raw[NIT];
    Slot<TA> rawa[NIT] = {};
    int rowof[NIT];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int q = it * WAVE + lane;
        const int rr = slab_row(cpr, it, lane), t = SEL4(rr, tok0, tok1, tok2, tok3);
        const bool ok = SEL4(rr, va0, va1, va2, va3) && (q < total);
        rowof[it] = ok ? rr : -1;
        const int64_t toff = (int64_t)(ok ? t : tok0) * C;
        const int cc = ok ? slab_col(q, rr, cpr) : 0;
        raw[it] = ld_slot<TX>(xg + toff, cc);
        if (add) rawa[it] = ld_slot<TA>(ag + toff, cc);  // (wave-uniform)
    }
    SlabEdges e{false, false, false, false};  // rows that receive sources: the edge waves build them
    if (OP != OP_DROP) e = slab_edge_rows(d_first, f.j0, f.j1, f.j2, f.j3, dstg, r, lane);
    const bool e0 = e.e0, e1 = e.e1, e2 = e.e2, e3 = e.e3;
    const bool ok0 = va0 && !e0, ok1 = va1 && !e1, ok2 = va2 && !e2, ok3 = va3 && !e3;
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int rr = rowof[it];
        const bool ok = rr >= 0 && SEL4(rr, ok0, ok1, ok2, ok3);
        rowof[it] = ok ? rr : -1;
    }
    // the parameter slots of every slot column this lane holds: requested now, used after the two reductions
    const LnParams<float, NIT> prm = ln_params<float, NIT>(lw, lb, rowof, cpr, lane);
    const float my_s = (load_size && f.my_valid) ? to_f32(f.my_s_raw) : 1.0f;
    float sz0, sz1, sz2, sz3;
    lanes4(my_s, sz0, sz1, sz2, sz3);
    // x' = x + a, the merge of a row without sources ((x' s) / s: raw bits when that is x' itself) and the store
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int rr = rowof[it];
        if (rr < 0) continue;
        if (add) raw[it] = slot_add<TX, TA>(raw[it], rawa[it]);
        if (OP == OP_WAVG) {
            const float s = SEL4(rr, sz0, sz1, sz2, sz3);
            if (!wavg_moves_raw<TX>(s)) raw[it] = wavg_rescaled<TX>(raw[it], s);
        }
        st_slot<TX>(og + (int64_t)(o0 + rr) * C, it * WAVE + lane - rr * cpr, raw[it]);
    }
    if (OP == OP_WAVG && f.my_valid) {
        // (this store stays here: through slab_store_size the all-bf16 form takes 98 vector registers for 96)
        const bool mine_has_edges = SEL4(lane, e0, e1, e2, e3);
        if (!mine_has_edges)
            store_size<TS>(sout + (int64_t)g * To + o0 + lane, lsout ? lsout + (int64_t)g * To + o0 + lane : nullptr, my_s);
    }
    // LayerNorm of the rows as stored
    ln_rows<TX, float, TY, NIT>(raw, rowof, R, cpr, C, eps, prm, lane,
                                [&](int rr, int cc, const Slot<TY> &yv) __attribute__((always_inline)) {
                                    st_slot<TY>(yg + (int64_t)(o0 + rr) * C, cc, yv);
                                });
}

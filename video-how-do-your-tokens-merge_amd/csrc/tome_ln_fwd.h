// tome_ln_fwd.h -- part of the single translation unit csrc/tome_kernels.hip (residual add + LayerNorm, forward).
#pragma once
// k_add_ln_rows: the other residual of the patched block, fused with the LayerNorm that reads its result:
//     x = x + mlp(norm2(x))            (tome/patch/videomae.py:29, end of ToMeBlock.forward)
//     ... next block: self.norm1(x)    (tome/patch/videomae.py:19)
// x' = x + a and y = LayerNorm(x') in one pass (ln_rows, tome_ln_rows.h).  A wave owns R consecutive rows, NIT slots per
// lane, everything loaded before use.  TS: the residual stream (x, x'); TA: the addend; TY: y; TP: weight and bias.
//   tome_add_layernorm[_skip_first]: everything of one 16-bit dtype; x' = round16(x + a)
//   tome_add_layernorm_amp (a model under autocast, fp32 master weights): TP fp32, TY the 16-bit autocast dtype,
//     16-bit stream: x' = round16(x + a), the same bits;  fp32 stream: x' = x + (float)a -- `x + a.float()` bit for bit
// The statistics are taken from the STORED row; y is rounded once to TY.
// a == nullptr: LayerNorm only (x is the finished sum -- the caller's GEMM accumulated onto it), nothing is written to
// xout.
// y_group > 0: rows come in groups of y_group whose FIRST row (a class token) has no place in y -- y holds the other
// y_group - 1 rows of every group, compacted (TimeSformer's temporal_norm1 feeds only the patch tokens,
// tome/patch/timesformer.py:24-26, so `xn[:, 1:]` regrouped '(b p) t m' is a view instead of a copy)
template <typename TS, typename TA, typename TY, typename TP, int NIT>
__global__ __launch_bounds__(256) void k_add_ln_rows(const TS *__restrict__ x, const TA *__restrict__ a, int64_t rows,
                                                     int C, int R, int cpr, const TP *__restrict__ lw,
                                                     const TP *__restrict__ lb, float eps, int y_group,
                                                     TS *__restrict__ xout, TY *__restrict__ y) {
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * (blockDim.x >> 6) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t row0 = w * R;
    if (row0 >= rows) return;
    const int nrow = (int)((rows - row0) < R ? (rows - row0) : R);
    const int total = nrow * cpr;
    const bool add = a != nullptr;
    const TS *xs = x + row0 * C;
    const TA *as = a + row0 * C;
    Slot<TS> raw[NIT] = {};
    Slot<TA> rawa[NIT] = {};
    int rowof[NIT];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int q = it * WAVE + lane;
        rowof[it] = q < total ? slab_row(cpr, it, lane) : -1;
        if (q < total) {
            raw[it] = ld_slot<TS>(xs, q);
            if (add) rawa[it] = ld_slot<TA>(as, q);
        }
    }
    const LnParams<TP, NIT> prm = ln_params<TP, NIT>(lw, lb, rowof, cpr, lane);
    if (add) {
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            if (rowof[it] < 0) continue;
            raw[it] = slot_add<TS, TA>(raw[it], rawa[it]);
            st_slot<TS>(xout + row0 * C, it * WAVE + lane, raw[it]);
        }
    }
    ln_rows<TS, TP, TY, NIT>(raw, rowof, nrow, cpr, C, eps, prm, lane,
                             [&](int rr, int cc, const Slot<TY> &yv) __attribute__((always_inline)) {
                                 int64_t yrow = row0 + rr;
                                 if (y_group > 0) {
                                     const int64_t gb = yrow / y_group;
                                     if (yrow - gb * y_group == 0) return;
                                     yrow -= gb + 1;
                                 }
                                 st_slot<TY>(y + yrow * C, cc, yv);
                             });
}

// k_add_ln_regroup: the middle of TimeSformer's divided space-time block (tome/patch/timesformer.py:24-38):
//     xt = x[:, 1:] + temporal_fc(res_temporal)                       residual of the temporal attention
//     xs = cat(cls replicated per frame, 'b (p t) m -> (b t) p m' of xt) spatial regrouping
//     ... self.norm1(xs)
// One pass: x1 = cat(cls, xt) in the token layout [B, 1 + P*F, C], and y = norm1 of every row written straight to
// its place in the regrouped [B*F, 1 + P, C] tensor (a LayerNorm is per row, so normalising before the permutation
// is the same thing); the class row is normalised once and stored F times.  Replaces an add, a strided copy and a
// LayerNorm (7 passes over the tokens) by 2 reads + 2 writes.  Same arithmetic as k_add_ln_rows.
template <typename TX, int NIT>
__global__ __launch_bounds__(256) void k_add_ln_regroup(const TX *__restrict__ x, const TX *__restrict__ a, int B, int F,
                                                        int P, int C, int R, int cpr, LnArgs ln,
                                                        TX *__restrict__ xout) {
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * (blockDim.x >> 6) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int N = 1 + P * F;
    const int64_t rows = (int64_t)B * N;
    const int64_t row0 = w * R;
    if (row0 >= rows) return;
    const int nrow = (int)((rows - row0) < R ? (rows - row0) : R);
    const int total = nrow * cpr;
    // per-row facts (wave-uniform): addend row (-1: class token, nothing is added) and the row of y
    int64_t arow[FAST_MAXR], yrow[FAST_MAXR];
#pragma unroll
    for (int rr = 0; rr < FAST_MAXR; ++rr) {
        const int64_t gr = row0 + (rr < nrow ? rr : 0);
        const int64_t b = gr / N;
        const int k = (int)(gr - b * N);
        if (k == 0) {
            arow[rr] = -1;
            yrow[rr] = b * F * (1 + P);  // frame 0; frames 1..F-1 follow at (1+P) rows each
        } else {
            const int p = (k - 1) / F, t = (k - 1) - p * F;
            arow[rr] = b * (int64_t)(P * F) + (k - 1);
            yrow[rr] = (b * F + t) * (int64_t)(1 + P) + 1 + p;
        }
    }
    const TX *xs = x + row0 * C;
    Slot<TX> raw[NIT], rawa[NIT];
    int rowof[NIT];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int q = it * WAVE + lane;
        const int rr = slab_row(cpr, it, lane);
        rowof[it] = q < total ? rr : -1;
        if (q >= total) continue;
        raw[it] = ld_slot<TX>(xs, q);
        const int64_t ar = SEL4(rr, arow[0], arow[1], arow[2], arow[3]);
        if (ar >= 0) rawa[it] = ld_slot<TX>(a + ar * C, slab_col(q, rr, cpr));
    }
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int rr = rowof[it];
        if (rr < 0) continue;
        const int64_t ar = SEL4(rr, arow[0], arow[1], arow[2], arow[3]);
        if (ar >= 0) raw[it] = slot_add<TX, TX>(raw[it], rawa[it]);
        st_slot<TX>(xout + row0 * C, it * WAVE + lane, raw[it]);
    }
    TX *yb = reinterpret_cast<TX *>(ln.y);
    const LnParams<TX, NIT> prm = ln_params<TX, NIT>(reinterpret_cast<const TX *>(ln.weight),
                                                     reinterpret_cast<const TX *>(ln.bias), rowof, cpr, lane);
    ln_rows<TX, TX, TX, NIT>(raw, rowof, nrow, cpr, C, ln.eps, prm, lane,
                             [&](int rr, int cc, const Slot<TX> &yv) __attribute__((always_inline)) {
                                 const int64_t ar = SEL4(rr, arow[0], arow[1], arow[2], arow[3]);
                                 const int64_t yr = SEL4(rr, yrow[0], yrow[1], yrow[2], yrow[3]);
                                 TX *yp = yb + yr * C;
                                 st_slot<TX>(yp, cc, yv);
                                 if (ar < 0)  // class token: the same normalised row in front of every frame's tokens
                                     for (int t = 1; t < F; ++t) st_slot<TX>(yp + (int64_t)t * (1 + P) * C, cc, yv);
                             });
}

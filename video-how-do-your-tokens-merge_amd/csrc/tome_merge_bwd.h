// tome_merge_bwd.h -- part of the single translation unit csrc/tome_kernels.hip (backward of the merge kernels).
#pragma once
// ------------------------------------------------------------------------------------------------
// k_merge_rows_bwd: the gradient of merge(x, "sum" | "mean"), merge_wavg(merge, x, size) and drop(x) with respect
// to the tokens (merge.py:75-85, :253-262, :355-369; the reference leaves it to autograd, only the matching is under
// no_grad, merge.py:49).  With o(t) the merged row token t lands in (odd token 2j+1: destination row j; even token:
// row_map, as k_row_map / tome_match write it) all of them are ONE gather with two optional per-row scales
//     gx[t, :] = (gy[o(t), :] / out_div[o(t)]) * in_mul[t]
//   sum:   no scale                         mean: out_div = 1 + number of sources of the row
//   wavg:  out_div = size', in_mul = size   (division first, then the product: the order in which autograd walks the
//          reference's chain x*size -> sum -> /size' back, so fp32 gradients are bit-comparable with it)
//   drop:  an even token that was merged away has no row: its gradient is 0
// No atomics: a wave owns R consecutive INPUT-token rows of one group (the rows of gx), every row of gx is written
// once and a row of gy is read once per token that landed in it (1 + its sources; r of them come from L2).
// Streaming form of k_merge_rows_fast (the slab of tome_merge_slab.h, per-row facts from bwd_slab), non-temporal both
// ways, fp32 arithmetic, one rounding; a chunk whose two scales are absent or 1 moves as raw bits (v / 1 * 1 == v bit
// for bit).  One dependent round trip more than a plain copy: row_map -> rows of gy.
// Grid as k_merge_rows_fast: x = the blocks of one group, (y, z) = the group, class-token rows of the regrouped
// callers behind the groups.
// ------------------------------------------------------------------------------------------------
template <typename TX, int VEC>
__device__ __forceinline__ uint4 bwd_scale(const uint4 &raw, float d, float m) {
    Pack<TX, VEC> pk;
    __builtin_memcpy(&pk, &raw, 16);
#pragma unroll
    for (int e = 0; e < VEC; ++e) pk.e[e] = from_f32<TX>(__fmul_rn(__fdiv_rn(to_f32(pk.e[e]), d), m));
    uint4 o;
    __builtin_memcpy(&o, &pk, 16);
    return o;
}

template <typename TX, typename TS, int NIT>
__global__ __launch_bounds__(256) void k_merge_rows_bwd(const TX *__restrict__ gy, const TS *__restrict__ out_div,
                                                        const TS *__restrict__ in_mul, int n, int T_, int C, int r,
                                                        int R, int cpr, int wpg, const int *__restrict__ row_map,
                                                        int distill, int drop, TX *__restrict__ gx, TokLayout lgy,
                                                        TokLayout lgx, int cls_rows) {
    constexpr int VEC = 16 / sizeof(TX);
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int g = (int)(blockIdx.z * gridDim.y + blockIdx.y);
    const int lw = (int)blockIdx.x * (int)(blockDim.x >> 6) + wv;
    if (g >= n) {
        // the class tokens the regrouped callers keep aside (timesformer.py:89,107): their gradient passes through
        const int64_t b = ((int64_t)(g - n) * gridDim.x + blockIdx.x) * (blockDim.x >> 6) + wv;
        if (b < cls_rows) {
            const uint4 *src = reinterpret_cast<const uint4 *>(gy + b * lgy.outer_stride);
            uint4 *dst = reinterpret_cast<uint4 *>(gx + b * lgx.outer_stride);
            for (int c = lane; c < cpr; c += WAVE) dst[c] = src[c];
        }
        return;
    }
    if (lw >= wpg) return;
    const int To = T_ - r, T1 = (T_ + 1) >> 1, U = T1 - r;
    const int t0 = lw * R;
    const TX *gyg = group_ptr(gy, lgy, g);
    TX *gxg = group_ptr(gx, lgx, g);

    // per-row facts (bwd_slab, tome_merge_slab.h): merged row and the two scales
    const BwdSlab f = bwd_slab<false, TS>(out_div, in_mul, row_map, g, t0, R, T_, T1, U, To, distill, drop, lane);
    const int o0 = f.o0, o1 = f.o1, o2 = f.o2, o3 = f.o3, os0 = f.os0;

    const int total = R * cpr;
    uint4 raw[NIT];
    int rowof[NIT];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int q = it * WAVE + lane;
        const int rr = slab_row(cpr, it, lane), cc = slab_col(q, rr, cpr);
        const int o = SEL4(rr, o0, o1, o2, o3);
        const bool live = (q < total) && o >= -1;
        rowof[it] = live ? rr : -1;
        const bool ok = live && o >= 0;
        // unconditional: a lane without a chunk re-reads the start of the wave's first row of gy and ignores it
        raw[it] = ld16(reinterpret_cast<const char *>(gyg + (int64_t)(ok ? o : os0) * lgy.tok_stride) + (ok ? cc : 0) * 16);
    }
    float d0, d1, d2, d3, m0, m1, m2, m3;
    lanes4(f.my_d, d0, d1, d2, d3);
    lanes4(f.my_m, m0, m1, m2, m3);
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int rr = rowof[it];
        if (rr < 0) continue;
        const int cc = it * WAVE + lane - rr * cpr;
        const int o = SEL4(rr, o0, o1, o2, o3);
        const float d = SEL4(rr, d0, d1, d2, d3), m = SEL4(rr, m0, m1, m2, m3);
        uint4 v = raw[it];
        if (o < 0) v = uint4{0u, 0u, 0u, 0u};
        else if (d != 1.0f || m != 1.0f) v = bwd_scale<TX, VEC>(v, d, m);
        st16(reinterpret_cast<char *>(gxg + (int64_t)(t0 + rr) * lgx.tok_stride) + cc * 16, v);
    }
}

// Generic form: one wave per row of gx, any C / alignment (VEC = 1: element by element).
template <typename TX, typename TS, int VEC>
__global__ __launch_bounds__(256) void k_merge_rows_bwd_any(const TX *__restrict__ gy, const TS *__restrict__ out_div,
                                                            const TS *__restrict__ in_mul, int n, int T_, int C, int r,
                                                            const int *__restrict__ row_map, int distill, int drop,
                                                            TX *__restrict__ gx) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (row >= (int64_t)n * T_) return;
    const int g = (int)(row / T_), t = (int)(row - (int64_t)g * T_);
    const int To = T_ - r, T1 = (T_ + 1) >> 1, U = T1 - r;
    const int o = bwd_row_of(t, g, T1, U, To, distill, drop, row_map);
    TX *xr = gx + row * C;
    if (o < 0) {
        float z[VEC];
#pragma unroll
        for (int e = 0; e < VEC; ++e) z[e] = 0.0f;
        for (int c = lane * VEC; c < C; c += WAVE * VEC) store_pack<TX, VEC>(xr + c, z);
        return;
    }
    const float d = out_div ? to_f32(out_div[(int64_t)g * To + o]) : 1.0f;
    const float m = in_mul ? to_f32(in_mul[row]) : 1.0f;
    const TX *yr = gy + ((int64_t)g * To + o) * C;
    for (int c = lane * VEC; c < C; c += WAVE * VEC) {
        float v[VEC];
        load_pack<TX, VEC>(yr + c, v);
#pragma unroll
        for (int e = 0; e < VEC; ++e) v[e] = __fmul_rn(__fdiv_rn(v[e], d), m);
        store_pack<TX, VEC>(xr + c, v);
    }
}

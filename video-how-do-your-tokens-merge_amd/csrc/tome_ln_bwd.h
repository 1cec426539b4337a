// tome_ln_bwd.h -- part of the single translation unit csrc/tome_kernels.hip (backward of the add + LayerNorm kernels).
#pragma once
// ------------------------------------------------------------------------------------------------
// k_ln_rows_bwd: the gradient of y = LayerNorm(x') with respect to x', where x' is the STORED 16-bit row the forward
// kernels normalised (k_add_ln_rows: x' = round(x + addend); the reference leaves this to autograd, models are patched
// for training: tools/train_net.py:727-741, tome/patch/videomae.py:19,26-29).  With gw = gy * weight, d = x' - mean,
// xhat = d * rstd:
//     gx = gx_in + rstd * (gw - mean(gw) - xhat * mean(gw * xhat))
// gx_in (optional) is the gradient that reaches x' directly through the residual stream; the sum is rounded once.
// mean and rstd are RECOMPUTED from x' with the arithmetic of ln_rows (tome_ln_rows.h: two passes, centred variance,
// wave_total, v_rsq_f32, 1/C as a multiplication): the forward normalised the row as stored, so nothing is saved by
// the forward.  Two reduction rounds per row: sum x, then sum d^2, sum gw and sum gw*d together.
// The two rounds are this kernel's OWN COPY, not ln_row_means / ln_rows_bwd_stats of tome_ln_rows.h, which
// k_ln_rows_bwd_amp calls: through the shared rounds the frozen bf16 form needs 141 registers instead of 127 (3 waves
// per SIMD instead of 4) and every form measured 0.3-2.1 % slower (one row array with a class-row bit and one set of
// row comparisons here, against two row arrays and two sets there).  What keeps the copy honest is a test of bits:
// tests/test_layernorm_forms_agree_gpu.py holds gx of this kernel to gx of k_ln_rows_bwd_amp on a 16-bit stream.
// Packing of k_add_ln_rows: a wave owns R consecutive rows, NIT 16-byte chunks per lane flattened over the rows, all
// loads of a slab issued before any use, non-temporal both ways, fp32 arithmetic.
// group_rows > 0 (backward of tome_add_layernorm_skip_first): rows come in groups of group_rows whose first row (a
// class token) had no place in y -- gy holds the other group_rows - 1 rows of every group, compacted.  The class rows
// get gx = gx_in bit for bit (or 0) and add nothing to the parameter gradients.
// PARAMS: dweight[c] = sum_rows gy * xhat, dbias[c] = sum_rows gy, without atomics.  A workgroup walks `spw` slabs
// per wave in ascending order (spw and the grid depend on the shape only); chunk slot (it, lane) of a wave holds the
// same channels in every slab, so the column sums live in registers.  At the end the four waves' slots are combined
// through LDS in the order wave 0..3, row-in-wave 0..R-1, and the workgroup writes ONE partial row [2, C] of fp32 to
// ws[blockIdx.x].  k_ln_param_grad sums the partial rows.  Same bits on every run.
// REGROUP (backward of tome_add_layernorm_regrouped, the middle of TimeSformer's divided space-time block,
// tome/patch/timesformer.py:24-38): xs / gx_in / gx are token rows [B, 1 + P*F, C], gy is the gradient of the regrouped
// tensor [B*F, 1 + P, C].  Only the row map differs: token row 1 + p*F + t of clip b reads row (b*F + t)(1 + P) + 1 + p
// of gy; a clip's class row, which the forward stored F times, takes the fp32 sum of rows (b*F + t)(1 + P) in frame
// order t = 0 .. F-1 (what autograd's `expand` backward computes, without its F - 1 roundings) and enters the formula
// and the parameter gradients once.  The gradient is carried as fp32 (gyf) from the loads on; everything else is the
// arithmetic above.  The other instantiations do not see any of it.
// ------------------------------------------------------------------------------------------------
template <typename TX, int NIT, bool PARAMS, bool REGROUP = false>
__global__ __launch_bounds__(256) void k_ln_rows_bwd(const TX *__restrict__ gy, const TX *__restrict__ xs,
                                                     const TX *__restrict__ gx_in, const TX *__restrict__ weight,
                                                     int rows, int gy_rows, int C, int R, int cpr, float eps,
                                                     int group_rows, int spw, TX *__restrict__ gx,
                                                     float *__restrict__ ws, int F = 0, int P = 0) {
    constexpr int VEC = 8;
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const float inv_c = __builtin_amdgcn_rcpf((float)C);
    const bool has_in = gx_in != nullptr;

    // the place of this lane's chunk slots in a slab: the same in every slab
    int rr_of[NIT], cc_of[NIT];
    uint4 wraw[NIT];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int q = it * WAVE + lane;
        const int rr = slab_row(cpr, it, lane);
        const bool slot = q < R * cpr;
        rr_of[it] = slot ? rr : -1;
        cc_of[it] = slot ? slab_col(q, rr, cpr) : 0;
        wraw[it] = *(reinterpret_cast<const uint4 *>(weight) + cc_of[it]);
    }
    float aw[NIT][VEC], ab[NIT][VEC];
    if (PARAMS) {
#pragma unroll
        for (int it = 0; it < NIT; ++it)
#pragma unroll
            for (int e = 0; e < VEC; ++e) aw[it][e] = ab[it][e] = 0.0f;
    }

    const int64_t slab0 = (int64_t)blockIdx.x * spw * 4;
    for (int s = 0; s < spw; ++s) {
        const int64_t row0_64 = (slab0 + (int64_t)s * 4 + wv) * R;
        if (row0_64 >= rows) break;  // (wave-uniform)
        const int row0 = (int)row0_64;
        const int nrow = (rows - row0) < R ? (rows - row0) : R;
        const int total = nrow * cpr;

        // row of gy for each of the wave's rows, -1 for a class row: lanes 0..3, then wave-uniform scalars
        int my_g = row0 + (lane & 3);
        int my_c = 0;  // REGROUP: 1 for a class row, whose gy is the sum of F rows (1 + P) apart, my_g the first
        if (REGROUP) {
            const unsigned ntok = 1u + (unsigned)P * (unsigned)F;
            const unsigned cb = (unsigned)my_g / ntok, ck = (unsigned)my_g - cb * ntok;
            if (ck == 0u) {
                my_c = 1;
                my_g = (int)(cb * (unsigned)F * (1u + (unsigned)P));
            } else {
                const unsigned cp = (ck - 1u) / (unsigned)F, ct = (ck - 1u) - cp * (unsigned)F;
                my_g = (int)((cb * (unsigned)F + ct) * (1u + (unsigned)P) + 1u + cp);
            }
        } else if (group_rows > 0) {
            const unsigned gb = (unsigned)my_g / (unsigned)group_rows;
            my_g = ((unsigned)my_g - gb * (unsigned)group_rows == 0u) ? -1 : my_g - (int)gb - 1;
        }
        int g0, g1, g2, g3;
        lanes4(my_g, g0, g1, g2, g3);
        int c0 = 0, c1 = 0, c2 = 0, c3 = 0;
        if (REGROUP) {  // (written out: through lanes4 the REGROUP form takes 134 vector registers for 132)
            c0 = __builtin_amdgcn_readlane(my_c, 0), c1 = __builtin_amdgcn_readlane(my_c, 1);
            c2 = __builtin_amdgcn_readlane(my_c, 2), c3 = __builtin_amdgcn_readlane(my_c, 3);
        }

        const uint4 *xsl = reinterpret_cast<const uint4 *>(xs) + (int64_t)row0 * cpr;
        const uint4 *gil = reinterpret_cast<const uint4 *>(has_in ? gx_in : xs) + (int64_t)row0 * cpr;
        uint4 xraw[NIT], graw[NIT], iraw[NIT];
        int rowof[NIT];  // row-in-wave of a live chunk, -1: no chunk; bit 2 set: chunk of a class row
        float gyf[REGROUP ? NIT : 1][VEC];  // REGROUP: the chunk's gradient in fp32 (a class row's is a sum)
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int q = it * WAVE + lane;
            const bool live = q < total;
            const int rr = rr_of[it];
            const int g = SEL4(rr, g0, g1, g2, g3);
            // unconditional loads: a lane without a chunk re-reads the slab's first chunk, a class row the start of
            // some row of gy, and ignores it
            int gr = (live && g >= 0) ? g : 0;
            gr = gr < gy_rows ? gr : gy_rows - 1;
            xraw[it] = ld16(xsl + (live ? q : 0));
            graw[it] = ld16(reinterpret_cast<const uint4 *>(gy) + (int64_t)gr * cpr + cc_of[it]);
            if (has_in) iraw[it] = ld16(gil + (live ? q : 0));
            rowof[it] = live ? (g < 0 ? (rr | 4) : rr) : -1;
            if (REGROUP) {
                Pack<TX, VEC> pg;
                __builtin_memcpy(&pg, &graw[it], 16);
#pragma unroll
                for (int e = 0; e < VEC; ++e) gyf[it][e] = to_f32(pg.e[e]);
                const int c = SEL4(rr, c0, c1, c2, c3);
                if (live && c) {  // class row: frames 1 .. F-1 added in frame order, fp32, nothing rounded
                    const uint4 *gsrc = reinterpret_cast<const uint4 *>(gy) + (int64_t)gr * cpr + cc_of[it];
                    for (int t = 1; t < F; ++t) {
                        const uint4 more = ld16(gsrc + (int64_t)t * (1 + P) * cpr);
                        __builtin_memcpy(&pg, &more, 16);
#pragma unroll
                        for (int e = 0; e < VEC; ++e) gyf[it][e] += to_f32(pg.e[e]);
                    }
                }
            }
        }

        // round 1: mean of every row (as ln_rows)
        float p0 = 0.0f, p1 = 0.0f, p2 = 0.0f, p3 = 0.0f;
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int rr = rowof[it] < 0 ? -1 : (rowof[it] & 3);
            const float t = rr >= 0 ? chunk_sum<TX>(xraw[it]) : 0.0f;
            p0 += rr == 0 ? t : 0.0f;
            if (R > 1) p1 += rr == 1 ? t : 0.0f;
            if (R > 2) {
                p2 += rr == 2 ? t : 0.0f;
                p3 += rr == 3 ? t : 0.0f;
            }
        }
        float m0 = wave_total(p0) * inv_c, m1 = 0.0f, m2 = 0.0f, m3 = 0.0f;
        if (R > 1) m1 = wave_total(p1) * inv_c;
        if (R > 2) {
            m2 = wave_total(p2) * inv_c;
            m3 = wave_total(p3) * inv_c;
        }

        // round 2: sum d^2, sum gw, sum gw * d
        float d[NIT][VEC];
        float v0 = 0.0f, v1 = 0.0f, v2 = 0.0f, v3 = 0.0f;  // sum d^2
        float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;  // sum gw
        float b0 = 0.0f, b1 = 0.0f, b2 = 0.0f, b3 = 0.0f;  // sum gw * d
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int ro = rowof[it];
            const int rr = ro < 0 ? -1 : (ro & 3);
            const bool grad = ro >= 0 && ro < 4;  // a live chunk of a row that has a gradient
            const float m = pick4(rr, m0, m1, m2, m3, R);
            Pack<TX, VEC> px, pg, pw;
            __builtin_memcpy(&px, &xraw[it], 16);
            __builtin_memcpy(&pg, &graw[it], 16);
            __builtin_memcpy(&pw, &wraw[it], 16);
            float u = 0.0f, sa = 0.0f, sb = 0.0f;
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                d[it][e] = to_f32(px.e[e]) - m;
                const float gwe = (REGROUP ? gyf[it][e] : to_f32(pg.e[e])) * to_f32(pw.e[e]);
                u = __fmaf_rn(d[it][e], d[it][e], u);
                sa += gwe;
                sb = __fmaf_rn(gwe, d[it][e], sb);
            }
            u = rr >= 0 ? u : 0.0f;
            sa = grad ? sa : 0.0f;
            sb = grad ? sb : 0.0f;
            v0 += rr == 0 ? u : 0.0f;
            a0 += rr == 0 ? sa : 0.0f;
            b0 += rr == 0 ? sb : 0.0f;
            if (R > 1) {
                v1 += rr == 1 ? u : 0.0f;
                a1 += rr == 1 ? sa : 0.0f;
                b1 += rr == 1 ? sb : 0.0f;
            }
            if (R > 2) {
                v2 += rr == 2 ? u : 0.0f;
                a2 += rr == 2 ? sa : 0.0f;
                b2 += rr == 2 ? sb : 0.0f;
                v3 += rr == 3 ? u : 0.0f;
                a3 += rr == 3 ? sa : 0.0f;
                b3 += rr == 3 ? sb : 0.0f;
            }
        }
        // per row: rstd, mean(gw), k = rstd * mean(gw * xhat) = rstd^2 * sum(gw * d) / C   (xhat * mean(.) = d * k)
        float r0 = __builtin_amdgcn_rsqf(wave_total(v0) * inv_c + eps), r1 = 0.0f, r2 = 0.0f, r3 = 0.0f;
        float g_0 = wave_total(a0) * inv_c, g_1 = 0.0f, g_2 = 0.0f, g_3 = 0.0f;
        float k0 = r0 * (r0 * (wave_total(b0) * inv_c)), k1 = 0.0f, k2 = 0.0f, k3 = 0.0f;
        if (R > 1) {
            r1 = __builtin_amdgcn_rsqf(wave_total(v1) * inv_c + eps);
            g_1 = wave_total(a1) * inv_c;
            k1 = r1 * (r1 * (wave_total(b1) * inv_c));
        }
        if (R > 2) {
            r2 = __builtin_amdgcn_rsqf(wave_total(v2) * inv_c + eps);
            g_2 = wave_total(a2) * inv_c;
            k2 = r2 * (r2 * (wave_total(b2) * inv_c));
            r3 = __builtin_amdgcn_rsqf(wave_total(v3) * inv_c + eps);
            g_3 = wave_total(a3) * inv_c;
            k3 = r3 * (r3 * (wave_total(b3) * inv_c));
        }

        uint4 *gxl = reinterpret_cast<uint4 *>(gx) + (int64_t)row0 * cpr;
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int ro = rowof[it];
            if (ro < 0) continue;
            const int q = it * WAVE + lane;
            if (ro >= 4) {  // class row: its gradient is what the residual stream brings, moved as raw bits
                st16(gxl + q, has_in ? iraw[it] : uint4{0u, 0u, 0u, 0u});
                continue;
            }
            const float rs = pick4(ro, r0, r1, r2, r3, R), mg = pick4(ro, g_0, g_1, g_2, g_3, R),
                        kk = pick4(ro, k0, k1, k2, k3, R);
            Pack<TX, VEC> pi, pg, pw, po;
            if (has_in) __builtin_memcpy(&pi, &iraw[it], 16);
            __builtin_memcpy(&pg, &graw[it], 16);
            __builtin_memcpy(&pw, &wraw[it], 16);
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                const float gyv = REGROUP ? gyf[it][e] : to_f32(pg.e[e]);
                const float t = __fmaf_rn(-d[it][e], kk, gyv * to_f32(pw.e[e]) - mg);
                po.e[e] = from_f32<TX>(has_in ? __fmaf_rn(rs, t, to_f32(pi.e[e])) : rs * t);
                if (PARAMS) {
                    aw[it][e] = __fmaf_rn(gyv, d[it][e] * rs, aw[it][e]);
                    ab[it][e] += gyv;
                }
            }
            uint4 o;
            __builtin_memcpy(&o, &po, 16);
            st16(gxl + q, o);
        }
    }

    if (PARAMS) {
        // the workgroup's partial row: slots of the four waves through LDS, summed wave 0..3, row-in-wave 0..R-1
        __shared__ float red[4][NIT * WAVE][VEC];
#pragma unroll
        for (int which = 0; which < 2; ++which) {
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                if (rr_of[it] < 0) continue;
#pragma unroll
                for (int e = 0; e < VEC; ++e) red[wv][it * WAVE + lane][e] = which == 0 ? aw[it][e] : ab[it][e];
            }
            __syncthreads();
            float *dst = ws + ((int64_t)blockIdx.x * 2 + which) * C;
            for (int cc = threadIdx.x; cc < cpr; cc += 256) {
                float sum[VEC];
#pragma unroll
                for (int e = 0; e < VEC; ++e) sum[e] = 0.0f;
                for (int w = 0; w < 4; ++w)
                    for (int rr = 0; rr < R; ++rr)
#pragma unroll
                        for (int e = 0; e < VEC; ++e) sum[e] += red[w][rr * cpr + cc][e];
                *reinterpret_cast<float4 *>(dst + cc * VEC) = float4{sum[0], sum[1], sum[2], sum[3]};
                *reinterpret_cast<float4 *>(dst + cc * VEC + 4) = float4{sum[4], sum[5], sum[6], sum[7]};
            }
            __syncthreads();
        }
    }
}

// k_ln_param_grad: parameter gradients from fp32 partial rows ws [parts, width]: of k_ln_rows_bwd (width = 2 C, the
// columns [dweight | dbias], split = C) and of k_gelu_bwd (width = split = Hd, fc1's bias gradient, no second output).
// A thread owns one of the `width` columns; the parts are summed in index order in LN_PG_RUNS contiguous runs (one per
// wave of the workgroup), the runs combined in run order; one rounding to the parameter dtype.  The order depends on
// `parts` only: same bits on every run.  Columns below `split` go to out_lo, the others to out_hi; either may be NULL
// (that parameter is frozen).
#define LN_PG_RUNS 16
template <typename TP>
__global__ __launch_bounds__(LN_PG_RUNS * WAVE) void k_ln_param_grad(const float *__restrict__ ws, int parts, int width,
                                                                    int split, TP *__restrict__ out_lo,
                                                                    TP *__restrict__ out_hi) {
    __shared__ float runs[LN_PG_RUNS][WAVE];
    const int lane = threadIdx.x & 63, run = threadIdx.x >> 6;
    const int col = (int)blockIdx.x * WAVE + lane;
    const int per = (parts + LN_PG_RUNS - 1) / LN_PG_RUNS;
    const int lo = run * per, hi = (lo + per) < parts ? (lo + per) : parts;
    float acc = 0.0f;
    if (col < width) {
        const float *src = ws + col;
#pragma unroll 8
        for (int p = lo; p < hi; ++p) acc += src[(int64_t)p * width];
    }
    runs[run][lane] = acc;
    __syncthreads();
    if (run != 0 || col >= width) return;
    float total = runs[0][lane];
#pragma unroll
    for (int k = 1; k < LN_PG_RUNS; ++k) total += runs[k][lane];
    if (col < split) {
        if (out_lo) out_lo[col] = from_f32<TP>(total);
    } else if (out_hi) {
        out_hi[col - split] = from_f32<TP>(total);
    }
}

// ------------------------------------------------------------------------------------------------
// k_ln_rows_bwd_amp: k_ln_rows_bwd for a model that runs under autocast with fp32 master weights
// (tome_layernorm_backward_amp; tools/train_net.py:123, tome/utils.py:54): the backward of k_add_ln_rows with fp32 parameters.
// TG: gy, the 16-bit autocast dtype; TS: the residual stream (xs, gx_in, gx), 16-bit or fp32; weight fp32; the partial
// rows of dweight / dbias fp32 as before, summed by k_ln_param_grad<float> into fp32 parameters.  Formula, reduction
// rounds, packing (slots of 8 channels, tome_ln_rows.h), slab walk and the order of every sum are those of k_ln_rows_bwd;
// mean and rstd are recomputed from the stored row as in k_ln_rows_bwd.  gx is rounded once to TS (not
// at all for an fp32 stream).  gx16 (fp32 stream, optional): round16(gx) from the same registers, the gradient of a
// 16-bit addend without a cast pass; a class row's is round16(gx_in).
// ------------------------------------------------------------------------------------------------
template <typename TS, typename TG, int NIT, bool PARAMS>
__global__ __launch_bounds__(256, 2) void k_ln_rows_bwd_amp(const TG *__restrict__ gy, const TS *__restrict__ xs,
                                                         const TS *__restrict__ gx_in, const float *__restrict__ weight,
                                                         int rows, int gy_rows, int C, int R, int cpr, float eps,
                                                         int group_rows, int spw, TS *__restrict__ gx,
                                                         TG *__restrict__ gx16, float *__restrict__ ws) {
    constexpr int VEC = 8;
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const float inv_c = __builtin_amdgcn_rcpf((float)C);
    const bool has_in = gx_in != nullptr;

    // the place of this lane's slots in a slab: the same in every slab
    int rr_of[NIT], cc_of[NIT];
    float wgt[NIT][VEC];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int q = it * WAVE + lane;
        const int rr = slab_row(cpr, it, lane);
        const bool slot = q < R * cpr;
        rr_of[it] = slot ? rr : -1;
        cc_of[it] = slot ? slab_col(q, rr, cpr) : 0;
        slot_f32<float>(ld_param_slot<float>(weight, cc_of[it]), wgt[it]);
    }
    float aw[NIT][VEC], ab[NIT][VEC];
    if (PARAMS) {
#pragma unroll
        for (int it = 0; it < NIT; ++it)
#pragma unroll
            for (int e = 0; e < VEC; ++e) aw[it][e] = ab[it][e] = 0.0f;
    }

    const int64_t slab0 = (int64_t)blockIdx.x * spw * 4;
    for (int s = 0; s < spw; ++s) {
        const int64_t row0_64 = (slab0 + (int64_t)s * 4 + wv) * R;
        if (row0_64 >= rows) break;  // (wave-uniform)
        const int row0 = (int)row0_64;
        const int nrow = (rows - row0) < R ? (rows - row0) : R;
        const int total = nrow * cpr;

        // row of gy for each of the wave's rows, -1 for a class row: lanes 0..3, then wave-uniform scalars
        int my_g = row0 + (lane & 3);
        if (group_rows > 0) {
            const unsigned gb = (unsigned)my_g / (unsigned)group_rows;
            my_g = ((unsigned)my_g - gb * (unsigned)group_rows == 0u) ? -1 : my_g - (int)gb - 1;
        }
        int g0, g1, g2, g3;
        lanes4(my_g, g0, g1, g2, g3);

        const TS *xsl = xs + (int64_t)row0 * C;
        const TS *gil = (has_in ? gx_in : xs) + (int64_t)row0 * C;
        Slot<TS> xraw[NIT], iraw[NIT];
        Slot<TG> graw[NIT];
        int srow[NIT], grow[NIT];  // as in k_ln_rows_bwd
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int q = it * WAVE + lane;
            const bool live = q < total;
            const int rr = rr_of[it];
            const int g = SEL4(rr, g0, g1, g2, g3);
            // unconditional loads: a lane without a slot re-reads the slab's first slot, a class row the start of
            // some row of gy, and ignores it
            int gr = (live && g >= 0) ? g : 0;
            gr = gr < gy_rows ? gr : gy_rows - 1;
            xraw[it] = ld_slot<TS>(xsl, live ? q : 0);
            graw[it] = ld_slot<TG>(gy + (int64_t)gr * C, cc_of[it]);
            if (has_in) iraw[it] = ld_slot<TS>(gil, live ? q : 0);
            srow[it] = live ? rr : -1;
            grow[it] = (live && g >= 0) ? rr : -1;
        }

        // mean and rstd of every row with the forward's own functions, then mean(gw) and k (tome_ln_rows.h)
        float d[NIT][VEC];
        const LnBwdRows st = ln_rows_bwd_stats<TS, NIT>(
            xraw, srow, grow, ln_row_means<TS, NIT>(xraw, srow, R, inv_c), R, inv_c, eps,
            [&](int it, int e) __attribute__((always_inline)) { return slot_at<TG>(graw[it], e) * wgt[it][e]; }, d);

        TS *gxl = gx + (int64_t)row0 * C;
        TG *g16l = gx16 ? gx16 + (int64_t)row0 * C : nullptr;
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            if (srow[it] < 0) continue;
            const int q = it * WAVE + lane;
            const int ro = grow[it];
            float o[VEC];
            if (ro < 0) {  // class row: its gradient is what the residual stream brings, moved as raw bits
                Slot<TS> z = {};
                if (has_in) z = iraw[it];
                st_slot<TS>(gxl, q, z);
                if (g16l) {
                    slot_f32<TS>(z, o);
                    st_slot<TG>(g16l, q, f32_slot<TG>(o));
                }
                continue;
            }
            const float rs = st.rstd.at(ro, R), mg = st.mgw.at(ro, R), kk = st.k.at(ro, R);
            float gi[VEC];
            if (has_in) slot_f32<TS>(iraw[it], gi);
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                const float gyv = slot_at<TG>(graw[it], e);
                const float t = __fmaf_rn(-d[it][e], kk, gyv * wgt[it][e] - mg);
                // one rounding to the stream's dtype (none for fp32); gx16 rounds the stored fp32 value
                o[e] = to_f32(from_f32<TS>(has_in ? __fmaf_rn(rs, t, gi[e]) : rs * t));
                if (PARAMS) {
                    aw[it][e] = __fmaf_rn(gyv, d[it][e] * rs, aw[it][e]);
                    ab[it][e] += gyv;
                }
            }
            st_slot<TS>(gxl, q, f32_slot<TS>(o));
            if (g16l) st_slot<TG>(g16l, q, f32_slot<TG>(o));
        }
    }

    if (PARAMS) {
        // the workgroup's partial row: slots of the four waves through LDS, summed wave 0..3, row-in-wave 0..R-1
        __shared__ float red[4][NIT * WAVE][VEC];
#pragma unroll
        for (int which = 0; which < 2; ++which) {
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                if (rr_of[it] < 0) continue;
#pragma unroll
                for (int e = 0; e < VEC; ++e) red[wv][it * WAVE + lane][e] = which == 0 ? aw[it][e] : ab[it][e];
            }
            __syncthreads();
            float *dst = ws + ((int64_t)blockIdx.x * 2 + which) * C;
            for (int cc = threadIdx.x; cc < cpr; cc += 256) {
                float sum[VEC];
#pragma unroll
                for (int e = 0; e < VEC; ++e) sum[e] = 0.0f;
                for (int w = 0; w < 4; ++w)
                    for (int rr = 0; rr < R; ++rr)
#pragma unroll
                        for (int e = 0; e < VEC; ++e) sum[e] += red[w][rr * cpr + cc][e];
                *reinterpret_cast<float4 *>(dst + cc * VEC) = float4{sum[0], sum[1], sum[2], sum[3]};
                *reinterpret_cast<float4 *>(dst + cc * VEC + 4) = float4{sum[4], sum[5], sum[6], sum[7]};
            }
            __syncthreads();
        }
    }
}

// tome_merge_ln_bwd.h -- part of the single translation unit csrc/tome_kernels.hip (backward of the fused residual add +
// merge + LayerNorm launches, tome_merge_wavg_ln and tome_drop_ln, in the flat layout).
#pragma once
// ------------------------------------------------------------------------------------------------
// k_merge_ln_rows_bwd: k_ln_rows_bwd and k_merge_rows_bwd as one pass (tome/patch/videomae.py:20-29, vivit.py:35-41
// patched for training, tools/train_net.py:727-741; the reference leaves all of it to autograd).  The forward stored
// x' = merge_wavg(x + addend) [n, To, C] and y = LayerNorm(x'); with o(t) the merged row of token t (bwd_row_of),
// gw = gy * weight, d = x' - mean, xhat = d * rstd:
//     gm[o]  = gx_out[o] + rstd * (gw - mean(gw) - xhat * mean(gw * xhat))        fp32, NOT rounded
//     gx[t]  = round((gm[o(t)] / out_div[o(t)]) * in_mul[t])                      division first, then the product
// -- one rounding where tome_layernorm_backward followed by tome_merge_backward round twice.  gx is the gradient of x
// and of the addend alike.  drop: no scales, a merged-away token (no row) gets 0.
// mean and rstd are recomputed from x' with ln_rows' arithmetic, exactly as k_ln_rows_bwd does it: the two rounds
// are a copy of that kernel's, kept for the same reason (through the shared rounds of tome_ln_rows.h this kernel went
// from 44 to 78 scalar registers and measured 1.3 % slower).
// A wave owns R consecutive INPUT-token rows of one group (the rows of gx): the slab of tome_merge_slab.h, per-row facts
// (merged row, the two scales, "owns its row") from bwd_slab; the loads of a slab are x', gy, gx_out at row o(t).  A
// destination with k sources has its LayerNorm term computed 1 + k times (r extra rows of T); the rows come from L2.
// PARAMS: dweight[c] = sum gy * xhat, dbias[c] = sum gy over the MERGED rows, each counted once -- by the token that
// owns it: an odd token its destination row, an even token its own row unless it was merged away.  The scheme is
// k_ln_rows_bwd's: a workgroup walks `spw` slabs per wave in ascending order over the flat list of all groups' slabs
// (slab s: group s / wpg, wave s % wpg of it), column sums in registers, ONE partial row [2, C] per workgroup through
// LDS in the order wave 0..3, row-in-wave 0..R-1, k_ln_param_grad sums them.  No atomics, same bits on every run.
// Without PARAMS (frozen LayerNorm): one slab per wave, grid x = the blocks of one group, (y, z) = the group as in
// k_merge_rows_bwd; no workspace.
// ------------------------------------------------------------------------------------------------
template <typename TX, typename TS, int NIT, bool PARAMS>
__global__ __launch_bounds__(256) void k_merge_ln_rows_bwd(const TX *__restrict__ gy, const TX *__restrict__ gx_out,
                                                           const TX *__restrict__ xs, const TS *__restrict__ out_div,
                                                           const TS *__restrict__ in_mul,
                                                           const TX *__restrict__ weight, int n, int T_, int C, int r,
                                                           int R, int cpr, int wpg, int spw, float eps,
                                                           const int *__restrict__ row_map, int distill, int drop,
                                                           TX *__restrict__ gx, float *__restrict__ ws) {
    constexpr int VEC = 8;
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const float inv_c = __builtin_amdgcn_rcpf((float)C);
    const bool has_in = gx_out != nullptr;
    const int To = T_ - r, T1 = (T_ + 1) >> 1, U = T1 - r;

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

    const int64_t slabs = (int64_t)n * wpg;
    for (int s = 0; s < (PARAMS ? spw : 1); ++s) {
        int g, lw;
        if (PARAMS) {
            const int64_t flat = ((int64_t)blockIdx.x * spw + s) * 4 + wv;
            if (flat >= slabs) break;  // (wave-uniform)
            g = (int)(flat / wpg);
            lw = (int)(flat - (int64_t)g * wpg);
        } else {
            g = (int)(blockIdx.z * gridDim.y + blockIdx.y);
            lw = (int)blockIdx.x * 4 + wv;
            if (g >= n || lw >= wpg) break;  // (wave-uniform)
        }
        const int t0 = lw * R;

        // per-row facts (bwd_slab, tome_merge_slab.h): merged row, the two scales, "owns its row"
        const BwdSlab f = bwd_slab<true, TS>(out_div, in_mul, row_map, g, t0, R, T_, T1, U, To, distill, drop, lane);
        const int o0 = f.o0, o1 = f.o1, o2 = f.o2, o3 = f.o3, os0 = f.os0;

        const uint4 *xsg = reinterpret_cast<const uint4 *>(xs) + (int64_t)g * To * cpr;
        const uint4 *gyg = reinterpret_cast<const uint4 *>(gy) + (int64_t)g * To * cpr;
        const uint4 *gig = reinterpret_cast<const uint4 *>(has_in ? gx_out : xs) + (int64_t)g * To * cpr;
        uint4 xraw[NIT], graw[NIT], iraw[NIT];
        int rowof[NIT];  // row-in-wave of a live chunk, -1: no chunk; bit 2 set: chunk of a token without a row
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int rr = rr_of[it];
            const int o = SEL4(rr, o0, o1, o2, o3);
            const bool live = rr >= 0 && o >= -1;
            const bool ok = live && o >= 0;
            // unconditional loads: a lane without a chunk re-reads the start of the wave's first row and ignores it
            const int64_t at = (int64_t)(ok ? o : os0) * cpr + (ok ? cc_of[it] : 0);
            xraw[it] = ld16(xsg + at);
            graw[it] = ld16(gyg + at);
            if (has_in) iraw[it] = ld16(gig + at);
            rowof[it] = live ? (ok ? rr : (rr | 4)) : -1;
        }
        int w0, w1, w2, w3;
        float d0, d1, d2, d3, s0, s1, s2, s3;
        lanes4(f.my_owns ? 1 : 0, w0, w1, w2, w3);
        lanes4(f.my_d, d0, d1, d2, d3);
        lanes4(f.my_m, s0, s1, s2, s3);

        // round 1: mean of every row (as ln_rows)
        float p0 = 0.0f, p1 = 0.0f, p2 = 0.0f, p3 = 0.0f;
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int rr = (rowof[it] < 0 || rowof[it] >= 4) ? -1 : rowof[it];
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
            const int rr = (rowof[it] < 0 || rowof[it] >= 4) ? -1 : rowof[it];
            const float m = pick4(rr, m0, m1, m2, m3, R);
            Pack<TX, VEC> px, pg, pw;
            __builtin_memcpy(&px, &xraw[it], 16);
            __builtin_memcpy(&pg, &graw[it], 16);
            __builtin_memcpy(&pw, &wraw[it], 16);
            float u = 0.0f, sa = 0.0f, sb = 0.0f;
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                d[it][e] = to_f32(px.e[e]) - m;
                const float gwe = to_f32(pg.e[e]) * to_f32(pw.e[e]);
                u = __fmaf_rn(d[it][e], d[it][e], u);
                sa += gwe;
                sb = __fmaf_rn(gwe, d[it][e], sb);
            }
            u = rr >= 0 ? u : 0.0f;
            sa = rr >= 0 ? sa : 0.0f;
            sb = rr >= 0 ? sb : 0.0f;
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

        uint4 *gxl = reinterpret_cast<uint4 *>(gx) + ((int64_t)g * T_ + t0) * cpr;
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int ro = rowof[it];
            if (ro < 0) continue;
            const int q = it * WAVE + lane;  // chunk (ro & 3) * cpr + cc of the wave's rows of gx, which are contiguous
            if (ro >= 4) {  // a token without a row (drop)
                st16(gxl + q, uint4{0u, 0u, 0u, 0u});
                continue;
            }
            const float rs = pick4(ro, r0, r1, r2, r3, R), mg = pick4(ro, g_0, g_1, g_2, g_3, R),
                        kk = pick4(ro, k0, k1, k2, k3, R);
            const float dv = pick4(ro, d0, d1, d2, d3, R), mu = pick4(ro, s0, s1, s2, s3, R);
            const bool scaled = dv != 1.0f || mu != 1.0f;
            const int own = SEL4(ro, w0, w1, w2, w3);
            Pack<TX, VEC> pi, pg, pw, po;
            if (has_in) __builtin_memcpy(&pi, &iraw[it], 16);
            __builtin_memcpy(&pg, &graw[it], 16);
            __builtin_memcpy(&pw, &wraw[it], 16);
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                const float gyv = to_f32(pg.e[e]);
                const float t = __fmaf_rn(-d[it][e], kk, gyv * to_f32(pw.e[e]) - mg);
                float gm = has_in ? __fmaf_rn(rs, t, to_f32(pi.e[e])) : rs * t;
                if (scaled) gm = __fmul_rn(__fdiv_rn(gm, dv), mu);
                po.e[e] = from_f32<TX>(gm);
                if (PARAMS) {
                    const float gyo = own ? gyv : 0.0f;
                    aw[it][e] = __fmaf_rn(gyo, d[it][e] * rs, aw[it][e]);
                    ab[it][e] += gyo;
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

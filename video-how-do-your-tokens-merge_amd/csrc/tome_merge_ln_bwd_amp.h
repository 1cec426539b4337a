// tome_merge_ln_bwd_amp.h -- part of the single translation unit csrc/tome_kernels.hip (backward of the fused residual
// add + merge + LayerNorm launches under autocast, tome_merge_wavg_ln_amp and tome_drop_ln_amp, in the flat layout).
#pragma once
// ------------------------------------------------------------------------------------------------
// k_merge_ln_rows_bwd_amp: k_merge_ln_rows_bwd for a model that runs under autocast with fp32 master weights
// (tome_merge_ln_backward_amp; tools/train_net.py:123, tome/utils.py:54): k_ln_rows_bwd_amp and k_merge_rows_bwd as one
// pass.  TG: gy, the 16-bit autocast dtype; TS: the residual stream (xs = the forward's stored x', gx_out, gx), TG or
// fp32; TZ: the two scales, TS or fp32; weight fp32.  With o(t) the merged row of token t (bwd_row_owner), gw = gy * weight,
// d = x' - mean, xhat = d * rstd:
//     gm[o]  = gx_out[o] + rstd * (gw - mean(gw) - xhat * mean(gw * xhat))        fp32, NOT rounded
//     gx[t]  = round_TS((gm[o(t)] / out_div[o(t)]) * in_mul[t])                   division first, then the product
// -- one rounding on a 16-bit stream (tome_layernorm_backward_amp followed by tome_merge_backward round twice), none on
// an fp32 one.  drop: no scales, a merged-away token (no row) gets 0.  gx16 (fp32 stream, optional): round16(gx) from
// the same registers, the gradient of a 16-bit addend without a cast pass.
// mean and rstd are recomputed from x' by the forward's own functions, ln_row_means and ln_rows_bwd_stats of
// tome_ln_rows.h, which k_ln_rows_bwd_amp calls too, and the expression behind them is that kernel's term for term: a
// token's row has the bits that kernel gives its merged row whenever the row sits in the same place of the slab.
// A wave owns R consecutive INPUT-token rows of one group (the rows of gx): the slab of tome_merge_slab.h with slots of
// 8 channels (tome_ln_rows.h: one 16-byte move for 16-bit data, two for fp32), per-row facts from bwd_slab<true>; the
// loads of a slab are x', gy, gx_out at row o(t).
// PARAMS: dweight[c] = sum gy * xhat, dbias[c] = sum gy over the MERGED rows, each counted once -- by the token that
// owns it, whatever its scales make of its gx row.  The scheme is k_merge_ln_rows_bwd's:
// a workgroup walks `spw` slabs per wave in ascending order over the flat list of all groups' slabs, column sums in
// registers, ONE partial row [2, C] per workgroup through LDS in the order wave 0..3, row-in-wave 0..R-1;
// k_ln_param_grad<float> sums them.  No atomics, same bits on every run.  Without PARAMS (frozen LayerNorm): one slab
// per wave, grid x = the blocks of one group, (y, z) = the group; no workspace.
// ------------------------------------------------------------------------------------------------
template <typename TS, typename TG, typename TZ, int NIT, bool PARAMS>
__global__ __launch_bounds__(256, 2) void k_merge_ln_rows_bwd_amp(
    const TG *__restrict__ gy, const TS *__restrict__ gx_out, const TS *__restrict__ xs, const TZ *__restrict__ out_div,
    const TZ *__restrict__ in_mul, const float *__restrict__ weight, int n, int T_, int C, int r, int R, int cpr, int wpg,
    int spw, float eps, const int *__restrict__ row_map, int distill, int drop, TS *__restrict__ gx,
    TG *__restrict__ gx16, float *__restrict__ ws) {
    constexpr int VEC = 8;
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const float inv_c = __builtin_amdgcn_rcpf((float)C);
    const bool has_in = gx_out != nullptr;
    const int To = T_ - r, T1 = (T_ + 1) >> 1, U = T1 - r;

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
        const BwdSlab f = bwd_slab<true, TZ>(out_div, in_mul, row_map, g, t0, R, T_, T1, U, To, distill, drop, lane);
        const int o0 = f.o0, o1 = f.o1, o2 = f.o2, o3 = f.o3, os0 = f.os0;

        const TS *xsg = xs + (int64_t)g * To * C;
        const TG *gyg = gy + (int64_t)g * To * C;
        const TS *gig = (has_in ? gx_out : xs) + (int64_t)g * To * C;
        Slot<TS> xraw[NIT], iraw[NIT];
        Slot<TG> graw[NIT];
        int srow[NIT];   // row-in-wave of a slot whose token has a merged row, -1: none
        int rowof[NIT];  // row-in-wave of a live slot, -1: no slot; bit 2 set: slot of a token without a row
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int rr = rr_of[it];
            const int o = SEL4(rr, o0, o1, o2, o3);
            const bool live = rr >= 0 && o >= -1;
            const bool ok = live && o >= 0;
            // unconditional loads: a lane without a slot re-reads the start of the wave's first row and ignores it
            const int64_t at = (int64_t)(ok ? o : os0) * cpr + (ok ? cc_of[it] : 0);
            xraw[it] = ld_slot<TS>(xsg, at);
            graw[it] = ld_slot<TG>(gyg, at);
            if (has_in) iraw[it] = ld_slot<TS>(gig, at);
            srow[it] = ok ? rr : -1;
            rowof[it] = live ? (ok ? rr : (rr | 4)) : -1;
        }
        int w0, w1, w2, w3;
        float d0, d1, d2, d3, s0, s1, s2, s3;
        lanes4(f.my_owns ? 1 : 0, w0, w1, w2, w3);
        lanes4(f.my_d, d0, d1, d2, d3);
        lanes4(f.my_m, s0, s1, s2, s3);

        // mean and rstd of every row with the forward's own functions, then mean(gw) and k (tome_ln_rows.h)
        float d[NIT][VEC];
        const LnBwdRows st = ln_rows_bwd_stats<TS, NIT>(
            xraw, srow, srow, ln_row_means<TS, NIT>(xraw, srow, R, inv_c), R, inv_c, eps,
            [&](int it, int e) __attribute__((always_inline)) { return slot_at<TG>(graw[it], e) * wgt[it][e]; }, d);

        TS *gxl = gx + ((int64_t)g * T_ + t0) * C;
        TG *g16l = gx16 ? gx16 + ((int64_t)g * T_ + t0) * C : nullptr;
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int ro = rowof[it];
            if (ro < 0) continue;
            const int q = it * WAVE + lane;  // slot (ro & 3) * cpr + cc of the wave's rows of gx, which are contiguous
            if (ro >= 4) {  // a token without a row (drop)
                const Slot<TS> z = {};
                st_slot<TS>(gxl, q, z);
                if (g16l) {
                    const Slot<TG> z16 = {};
                    st_slot<TG>(g16l, q, z16);
                }
                continue;
            }
            const float rs = st.rstd.at(ro, R), mg = st.mgw.at(ro, R), kk = st.k.at(ro, R);
            const float dv = pick4(ro, d0, d1, d2, d3, R), mu = pick4(ro, s0, s1, s2, s3, R);
            const bool scaled = dv != 1.0f || mu != 1.0f;
            const int own = SEL4(ro, w0, w1, w2, w3);
            float gi[VEC], o[VEC];
            if (has_in) slot_f32<TS>(iraw[it], gi);
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                const float gyv = slot_at<TG>(graw[it], e);
                const float t = __fmaf_rn(-d[it][e], kk, gyv * wgt[it][e] - mg);
                float gm = has_in ? __fmaf_rn(rs, t, gi[e]) : rs * t;
                if (scaled) gm = __fmul_rn(__fdiv_rn(gm, dv), mu);
                // one rounding to the stream's dtype (none for fp32); gx16 rounds the stored fp32 value
                o[e] = to_f32(from_f32<TS>(gm));
                if (PARAMS) {
                    const float gyo = own ? gyv : 0.0f;
                    aw[it][e] = __fmaf_rn(gyo, d[it][e] * rs, aw[it][e]);
                    ab[it][e] += gyo;
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

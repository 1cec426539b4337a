// tome_traj_bwd.h -- backward of tome_trajectory_mix (k_trajectory_mix, tome_attn.h): the temporal stage of
// Motionformer's trajectory attention (ToMeTrajectoryAttention.forward, tome/patch/motionformer.py:122-139)
//     p   = softmax_f( (q2 * scale) . k2[f] )            one logit per frame of the token's trajectory
//     out = sum_f p_f * val[f]
// per (batch, token, head).  Given dout, with p recomputed exactly as the forward computes it (fp32 dot products over
// this lane's 8 channels with fmaf, xor-shuffle sum over the 8 lanes of a head, __expf(l - m) divided by the sum):
//     dval[f] = p_f * dout
//     dp_f    = dout . val[f]          (reduced like the logits)
//     delta   = sum_f p_f dp_f
//     ds_f    = p_f (dp_f - delta)
//     dq2     = scale * sum_f ds_f k2[f]
//     dk2[f]  = scale * ds_f * q2
// fp32 throughout, one rounding per output element.  The forward's `tattn` output (the map itself) gets NO gradient:
// the patched block never consumes it (it asks for _want_attn=False), and a caller that wants the map under grad keeps
// the framework's ops (tome/patch/motionformer.py).
//
// One streaming pass, the forward's layout: one wave per token, lane l owns the 16-byte chunks l and l + 64 of the
// H*64 channels (H <= 16), F <= 8.  k2, val, q2 and dout are read once and dk2, dval, dq2 written once; no LDS, no
// workspace, no atomics, same bits on every run.  As in the forward, every load of a chunk group is unconditional (a
// lane without a chunk reads chunk 0, a frame past F reads frame F-1, both ignored) and is issued before any arithmetic,
// with a sched_barrier between the loads and their first use: inside `if (on && f < F)` hipcc waits for each load in
// turn, one round trip per frame.  A chunk group no lane of the wave owns (H <= 8: the second one) is skipped as a whole.
// dk2 / dval may be NULL (wave-uniform): that gradient is not wanted and nothing is computed or written for it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tome_attn.h"

struct TrajBwdArgs {
    const void *q2, *k2, *val, *dout;
    void *dq2, *dk2, *dval;  // dk2, dval: NULL = not wanted
    int64_t rows;            // B * S
    int64_t k_row, v_row, dk_row, dv_row;  // element strides between (b, s, f) rows
    int64_t do_sb;                         // dout: batch b starts do_sb elements after batch b-1, rows S*C contiguous
    int S, F, H;
    float scale;
};

template <typename TX> __global__ __launch_bounds__(256) void k_trajectory_mix_bwd(TrajBwdArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * (blockDim.x >> 6) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (row >= a.rows) return;  // wave-uniform
    const int F = a.F, C = a.H * 64, chunks = C >> 3;
    const TX *qr = reinterpret_cast<const TX *>(a.q2) + row * C;
    const TX *kr = reinterpret_cast<const TX *>(a.k2) + row * F * a.k_row;
    const TX *vr = reinterpret_cast<const TX *>(a.val) + row * F * a.v_row;
    const int64_t ob = row / a.S;
    const TX *gr = reinterpret_cast<const TX *>(a.dout) + ob * a.do_sb + (row - ob * a.S) * C;
    TX *const dqr = reinterpret_cast<TX *>(a.dq2) + row * C;
    TX *const dkr = a.dk2 ? reinterpret_cast<TX *>(a.dk2) + row * F * a.dk_row : nullptr;
    TX *const dvr = a.dval ? reinterpret_cast<TX *>(a.dval) + row * F * a.dv_row : nullptr;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        if (64 * i >= chunks) break;  // (wave-uniform: no lane owns a chunk of this group)
        const int c = lane + 64 * i;
        const bool on = c < chunks;
        const int cl = on ? c : 0;
        uint4 kraw[TRAJ_MAXF], vraw[TRAJ_MAXF];
#pragma unroll
        for (int f = 0; f < TRAJ_MAXF; ++f) kraw[f] = traj_ld16(kr + (int64_t)(f < F ? f : F - 1) * a.k_row + 8 * cl);
        const uint4 qraw = *reinterpret_cast<const uint4 *>(qr + 8 * cl);
        const uint4 graw = *reinterpret_cast<const uint4 *>(gr + 8 * cl);
#pragma unroll
        for (int f = 0; f < TRAJ_MAXF; ++f) vraw[f] = traj_ld16(vr + (int64_t)(f < F ? f : F - 1) * a.v_row + 8 * cl);
        __builtin_amdgcn_sched_barrier(0);  // (the scheduler would otherwise sink the val loads below the dot products)
        float qv[8], gv[8];
        {
            Pack<TX, 8> pq, pg;
            __builtin_memcpy(&pq, &qraw, 16);
            __builtin_memcpy(&pg, &graw, 16);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                qv[e] = to_f32(pq.e[e]);
                gv[e] = to_f32(pg.e[e]);
            }
        }
        // the forward's logits and weights, operation for operation (k_trajectory_mix), and dp_f = dout . val[f]
        float lg[TRAJ_MAXF], dp[TRAJ_MAXF];
#pragma unroll
        for (int f = 0; f < TRAJ_MAXF; ++f) {
            float d = 0.0f, t = 0.0f;
            Pack<TX, 8> pk, pv;
            __builtin_memcpy(&pk, &kraw[f], 16);
            __builtin_memcpy(&pv, &vraw[f], 16);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                d = __builtin_fmaf(qv[e], to_f32(pk.e[e]), d);
                t = __builtin_fmaf(gv[e], to_f32(pv.e[e]), t);
            }
            // the 8 lanes of a head (consecutive chunks) hold its 64 channels
            d += __shfl_xor(d, 1);
            t += __shfl_xor(t, 1);
            d += __shfl_xor(d, 2);
            t += __shfl_xor(t, 2);
            d += __shfl_xor(d, 4);
            t += __shfl_xor(t, 4);
            lg[f] = (f < F) ? d * a.scale : -INFINITY;
            dp[f] = t;
        }
        float m = lg[0];
#pragma unroll
        for (int f = 1; f < TRAJ_MAXF; ++f) m = fmaxf(m, lg[f]);
        float w[TRAJ_MAXF], sum = 0.0f;
#pragma unroll
        for (int f = 0; f < TRAJ_MAXF; ++f) {
            w[f] = (f < F) ? __expf(lg[f] - m) : 0.0f;
            sum += w[f];
        }
        const float inv = 1.0f / sum;
        float delta = 0.0f;
#pragma unroll
        for (int f = 0; f < TRAJ_MAXF; ++f) {
            w[f] *= inv;  // (0 for a frame past F: it adds nothing below)
            delta = __builtin_fmaf(w[f], dp[f], delta);
        }
        float dq[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) dq[e] = 0.0f;
#pragma unroll
        for (int f = 0; f < TRAJ_MAXF; ++f) {
            if (f < F) {  // (wave-uniform)
                const float ds = w[f] * (dp[f] - delta) * a.scale;  // scale * ds_f
                Pack<TX, 8> pk;
                __builtin_memcpy(&pk, &kraw[f], 16);
                float dk[8], dv[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    dq[e] = __builtin_fmaf(ds, to_f32(pk.e[e]), dq[e]);
                    dk[e] = ds * qv[e];
                    dv[e] = w[f] * gv[e];
                }
                if (dkr && on) store_pack<TX, 8>(dkr + (int64_t)f * a.dk_row + 8 * c, dk);
                if (dvr && on) store_pack<TX, 8>(dvr + (int64_t)f * a.dv_row + 8 * c, dv);
            }
        }
        if (on) store_pack<TX, 8>(dqr + 8 * c, dq);
    }
}

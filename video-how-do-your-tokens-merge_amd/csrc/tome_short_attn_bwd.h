// tome_short_attn_bwd.h -- part of the single translation unit csrc/tome_kernels.hip (backward of k_short_attention).
#pragma once
// ------------------------------------------------------------------------------------------------
// k_short_attention_bwd: the gradient of out = softmax(q k^T * scale) v over sequences of at most 8 tokens --
// TimeSformer's temporal attention (ToMeBlock.forward, tome/patch/timesformer.py:25-27) when the model is patched for
// training (tools/train_net.py:727-741).  The forward saves nothing: P is recomputed with the forward's definition of
// the logits (v_dot2 products reduced over the eight lanes, scale * log2 e, exp2, row maximum subtracted), then
//     dP = dO V^T        delta_i = sum_j P_ij dP_ij        dS = P o (dP - delta)
//     dQ = scale dS K    dK = scale dS^T Q                 dV = P^T dO
// in fp32 with one rounding per output.  delta comes from the recomputed P, so the stored output is not read: seven
// streams (q, k, v, dout in; dq, dk, dv out), HBM bound, no matrix pipe, no LDS, no workspace, no atomics; the order of
// every sum is fixed, so the bits are the same on every run.
// Eight lanes own one (sequence, head) as in the forward: lane c holds channels 8c .. 8c+7.  k and v are held whole
// (2 x 8 16-byte registers), dk and dv are accumulated in registers over the query rows (2 x 8 x 8 fp32); q and dout
// are streamed one row at a time, the next row's two loads issued before the current row's arithmetic.  The loop over
// the query rows is a runtime loop (every register array is indexed by key and channel only).  Registers: the 192 of
// k, v, dk and dv plus k's fp32 form, which the compiler keeps outside the loop, make 340 of the 512 a wave of a
// 256-thread workgroup may hold (the part above 256 lives in accumulation registers, not in scratch): one wave per
// SIMD, 0 bytes of scratch.  Capped at 256 registers the allocator spills, so the cap is not set.  A key past the end
// repeats the last one and gets P = 0; a lane past the last unit repeats the last unit's loads and stores nothing.
// Every one of the 64 channels of every row of dq, dk and dv is written exactly once.
// ------------------------------------------------------------------------------------------------
struct ShortBwdStrides {  // {batch, token} element strides; the head stride is 64 everywhere
    int64_t q_sb, q_sn, k_sb, k_sn, v_sb, v_sn, dq_sb, dq_sn, dk_sb, dk_sn, dv_sb, dv_sn;
};

template <typename TX>
__global__ __launch_bounds__(256) void k_short_attention_bwd(const TX *__restrict__ q, const TX *__restrict__ k,
                                                             const TX *__restrict__ v, const TX *__restrict__ dout,
                                                             ShortBwdStrides s, int64_t units, int H, int N, float scale,
                                                             TX *__restrict__ dq, TX *__restrict__ dk,
                                                             TX *__restrict__ dv) {
    const int lane = threadIdx.x & 63;
    const int64_t unit = ((int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * 8 + (lane >> 3);
    const bool on = unit < units;
    const int64_t u = on ? unit : units - 1;  // (a lane past the end repeats the last unit's loads, stores nothing)
    const int64_t b = u / H;
    const int h = (int)(u - b * H);
    const int ch = h * 64 + 8 * (lane & 7);
    const int64_t g_sn = (int64_t)H * 64;
    const TX *qr = q + b * s.q_sb + ch, *kr = k + b * s.k_sb + ch, *vr = v + b * s.v_sb + ch;
    const TX *gr = dout + (b * N) * g_sn + ch;
    uint4 kraw[SHORT_MAXN], vraw[SHORT_MAXN];
#pragma unroll
    for (int t = 0; t < SHORT_MAXN; ++t) {
        const int tt = t < N ? t : N - 1;  // (wave-uniform; a token past the end repeats the last one, masked below)
        kraw[t] = traj_ld16(kr + tt * s.k_sn);
        vraw[t] = traj_ld16(vr + tt * s.v_sn);
    }
    uint4 qnext = traj_ld16(qr), gnext = traj_ld16(gr);
    float dka[SHORT_MAXN][8], dva[SHORT_MAXN][8];
#pragma unroll
    for (int j = 0; j < SHORT_MAXN; ++j)
#pragma unroll
        for (int e = 0; e < 8; ++e) dka[j][e] = dva[j][e] = 0.0f;
    const float LOG2E = 1.4426950408889634f;
    const float sl = scale * LOG2E;
    TX *dqr = dq + b * s.dq_sb + ch;
    // (not unrolled: every register array below is indexed by key and channel only)
#pragma unroll 1
    for (int i = 0; i < N; ++i) {
        const uint4 qraw = qnext, graw = gnext;
        {
            const int ii = i + 1 < N ? i + 1 : N - 1;  // (the last row is read twice: no branch around the loads)
            qnext = traj_ld16(qr + ii * s.q_sn);
            gnext = traj_ld16(gr + ii * g_sn);
        }
        float p[SHORT_MAXN], dp[SHORT_MAXN];
#pragma unroll
        for (int j = 0; j < SHORT_MAXN; ++j) {
            float t = short_dot8<TX>(qraw, kraw[j]);
            float w = short_dot8<TX>(graw, vraw[j]);
            t += __shfl_xor(t, 1);
            w += __shfl_xor(w, 1);
            t += __shfl_xor(t, 2);
            w += __shfl_xor(w, 2);
            t += __shfl_xor(t, 4);
            w += __shfl_xor(w, 4);
            p[j] = j < N ? t * sl : -INFINITY;
            dp[j] = w;
        }
        float m = p[0];
#pragma unroll
        for (int j = 1; j < SHORT_MAXN; ++j) m = fmaxf(m, p[j]);
        float sum = 0.0f;
#pragma unroll
        for (int j = 0; j < SHORT_MAXN; ++j) {
            p[j] = __builtin_amdgcn_exp2f(p[j] - m);
            sum += p[j];
        }
        const float inv = 1.0f / sum;
        float delta = 0.0f;
#pragma unroll
        for (int j = 0; j < SHORT_MAXN; ++j) {
            p[j] *= inv;  // (0 for a masked key)
            delta = __builtin_fmaf(p[j], dp[j], delta);
        }
        Pack<TX, 8> pq, pg;
        __builtin_memcpy(&pq, &qraw, 16);
        __builtin_memcpy(&pg, &graw, 16);
        float acc[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = 0.0f;
#pragma unroll
        for (int j = 0; j < SHORT_MAXN; ++j) {
            const float ds = p[j] * (dp[j] - delta);
            Pack<TX, 8> pk;
            __builtin_memcpy(&pk, &kraw[j], 16);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                acc[e] = __builtin_fmaf(ds, to_f32(pk.e[e]), acc[e]);
                dka[j][e] = __builtin_fmaf(ds, to_f32(pq.e[e]), dka[j][e]);
                dva[j][e] = __builtin_fmaf(p[j], to_f32(pg.e[e]), dva[j][e]);
            }
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] *= scale;
        if (on) store_pack<TX, 8>(dqr + (int64_t)i * s.dq_sn, acc);
    }
    TX *dkr = dk + b * s.dk_sb + ch, *dvr = dv + b * s.dv_sb + ch;
#pragma unroll
    for (int j = 0; j < SHORT_MAXN; ++j) {
        if (j >= N) break;  // (wave-uniform)
#pragma unroll
        for (int e = 0; e < 8; ++e) dka[j][e] *= scale;
        if (on) {
            store_pack<TX, 8>(dkr + (int64_t)j * s.dk_sn, dka[j]);
            store_pack<TX, 8>(dvr + (int64_t)j * s.dv_sn, dva[j]);
        }
    }
}

// tome_gelu_bwd.h -- part of the single translation unit csrc/tome_kernels.hip (backward of the MLP's GELU, exact-erf and tanh form).
#pragma once
// ------------------------------------------------------------------------------------------------
// k_gelu_bwd: the one pass over the hidden tensors [rows, Hd] in the backward of `fc2(gelu(fc1(y)))` (the reference
// leaves the MLP to autograd: `self.mlp(self.norm2(x))`, tome/patch/videomae.py:29; models are patched for training,
// tools/train_net.py:727-741).  From the saved pre-activation h and the gradient ga of the activation, v = h in fp32:
//     gh = round(ga * (Phi(v) + v phi(v))),   Phi(v) = 0.5 (1 + erf(v / sqrt 2)),   phi(v) = exp(-v^2 / 2) / sqrt(2 pi)
//     a  = gelu(h)            (optional)  gelu_erf_value, the forward's expression: the bits k_gelu_erf stored
//     db[c] = sum_rows gh     (BIAS)      of the ROUNDED gh, the values fc1's weight-gradient GEMM reads
// fp32 arithmetic, one rounding per output.  1 + erf(v / sqrt 2) is evaluated once per element and feeds both a and gh.
// FORM == GELU_TANH (ViViT's `layer.intermediate`, HF's gelu_fast; the contract is in include/tome_hip.h at
// tome_gelu_tanh): with u = beta (v + kappa v^3), s = sigma(2u) and c = 1 - s from gelu_tanh_sigmoid (no cancellation),
//     gh = round(ga * (s + v (s c) * 2 beta (1 + 3 kappa v^2))),   a = v s    gelu_tanh_value: the bits k_gelu_tanh stored
// Everything else -- packing, loads, the fence in front of both roundings, the bias sums -- is the same code.
// gh may be ga (every thread reads the 16 bytes it overwrites before it writes them); a never lies over h.
// A pure streaming pass: 16-byte chunks, non-temporal both ways.  The 2 S U loads of a step (8, 8, 12, 8 for S = 1 .. 4)
// are issued back to back, h and ga of a chunk side by side, before the first value is used: a lane without a chunk in
// a slot loads the tensor's last chunk instead of branching, and a compiler barrier keeps the loads from being sunk into
// the branches of the compute phase (h is not `restrict` for the same reason: a load from a restrict pointer may cross
// that barrier).  ACT is a template parameter: without the activation nothing of it is computed.
// Packing.  cpr = Hd / 8 chunks per row.  S = ceil(cpr / 256) column slots per thread: slot s of thread t holds chunk
// t + 256 s of a row, one row per pass.  S == 1: RP = 256 / cpr rows per pass, thread t holds chunk t mod cpr of row
// t / cpr of the pass (a narrow row leaves at most cpr - 1 threads idle).  A step is U passes (S * U = 4, 4, 6, 4 chunks
// per lane and tensor), their loads issued together.
// BIAS: a workgroup walks `spw` consecutive steps in ascending row order (spw and the grid depend on the shape only),
// the column sums of the slots it owns in registers.  At the end the RP rows-in-pass are combined through LDS in the
// order 0 .. RP - 1, and the workgroup writes ONE fp32 partial row [Hd] to ws[blockIdx.x]; k_ln_param_grad sums the
// partial rows in index order.  No atomics: same bits on every run.
// !BIAS (flat): the host passes cpr = 256, RP = 1, spw = 1 and the tensor is walked as rows of 256 chunks, as
// k_gelu_erf walks it; `chunks` ends the last one.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float fp32_value(float x) {
    asm("" : "+v"(x));  // no instruction: the compiler has to hold x as an fp32 value here
    return x;
}

template <int S> struct GeluBwdUnroll { static constexpr int U = S == 1 ? 4 : (S <= 3 ? 2 : 1); };

template <typename TX, int S, bool BIAS, bool ACT, int FORM>
__global__ __launch_bounds__(256) void k_gelu_bwd(const TX *h, const TX *ga, int64_t chunks, int cpr,
                                                  int RP, int spw, TX *gh, TX *__restrict__ act,
                                                  float *__restrict__ ws) {
    constexpr int VEC = 8;
    constexpr int U = GeluBwdUnroll<S>::U;
    const int t = threadIdx.x;
    // the place of this thread's slots in a pass: the same in every pass
    const int rr = S == 1 ? t / cpr : 0;
    int cc_of[S];
    bool slot[S];
#pragma unroll
    for (int s = 0; s < S; ++s) {
        cc_of[s] = S == 1 ? t - rr * cpr : t + s * 256;
        slot[s] = S == 1 ? rr < RP : cc_of[s] < cpr;
    }
    float acc[S][VEC];
    if (BIAS) {
#pragma unroll
        for (int s = 0; s < S; ++s)
#pragma unroll
            for (int e = 0; e < VEC; ++e) acc[s][e] = 0.0f;
    }

    const int64_t step0 = (int64_t)blockIdx.x * spw;
    for (int st = 0; st < spw; ++st) {
        const int64_t row0 = (step0 + st) * U * RP;  // first row of the step
        if (row0 * cpr >= chunks) break;             // (workgroup-uniform)
        // a lane without a chunk in a slot reads the tensor's last chunk (in bounds, never used): no load behind a branch
        uint4 hraw[U][S], graw[U][S];
        int64_t at[U][S];  // chunk index, -1: no chunk
        const uint4 *hp[U][S], *gp[U][S];
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int s = 0; s < S; ++s) {
                const int64_t q = (row0 + (int64_t)u * RP + rr) * cpr + cc_of[s];
                at[u][s] = (slot[s] && q < chunks) ? q : -1;
                const int64_t qc = q < chunks ? q : chunks - 1;
                hp[u][s] = reinterpret_cast<const uint4 *>(h) + qc;
                gp[u][s] = reinterpret_cast<const uint4 *>(ga) + qc;
            }
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int s = 0; s < S; ++s) {
                hraw[u][s] = ld16(hp[u][s]);
                graw[u][s] = ld16(gp[u][s]);
            }
        asm volatile("" ::: "memory");  // no instruction: the loads stay above, in front of the first branch
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int s = 0; s < S; ++s) {
                const int64_t q = at[u][s];
                if (q < 0) continue;
                Pack<TX, VEC> ph, pg, pa;
                __builtin_memcpy(&ph, &hraw[u][s], 16);
                __builtin_memcpy(&pg, &graw[u][s], 16);
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    const float v = to_f32(ph.e[e]);
                    // a1: what the activation is built from (sigma(2u) / 1 + erf); w: the derivative's second term
                    // (tanh form) or phi(v) (erf form)
                    float a1, w;
                    if (FORM == GELU_TANH) {
                        float c, v2;
                        a1 = gelu_tanh_sigmoid(v, c, v2);
                        w = v * (a1 * c) * (2.0f * GELU_TANH_BETA * (1.0f + 3.0f * GELU_TANH_KAPPA * v2));
                    } else {
                        a1 = gelu_erf_one_plus(v);
                        w = expf(-0.5f * (v * v)) * 0.39894228040143267794f;
                    }
                    // both results exist as fp32 values before they are rounded to the format: without the fence the
                    // fp16 forms that also sum the bias take v_fma_mixlo_f16 for product and rounding in one step, and
                    // gh would depend on what else the launch was asked for
                    const TX r = from_f32<TX>(fp32_value(to_f32(pg.e[e]) *
                                                         (FORM == GELU_TANH ? a1 + w : 0.5f * a1 + v * w)));
                    pg.e[e] = r;
                    if (ACT)
                        pa.e[e] = from_f32<TX>(fp32_value(FORM == GELU_TANH ? gelu_tanh_value(v, a1)
                                                                            : gelu_erf_value(v, a1)));
                    if (BIAS) acc[s][e] += to_f32(r);
                }
                uint4 o;
                __builtin_memcpy(&o, &pg, 16);
                st16(reinterpret_cast<uint4 *>(gh) + q, o);
                if (ACT) {
                    __builtin_memcpy(&o, &pa, 16);
                    st16(reinterpret_cast<uint4 *>(act) + q, o);
                }
            }
    }

    if (BIAS) {
        float *dst = ws + (int64_t)blockIdx.x * cpr * VEC;
        if (S == 1) {
            // the workgroup's partial row: the rows-in-pass through LDS, summed in the order 0 .. RP - 1
            __shared__ float red[256][VEC];
#pragma unroll
            for (int e = 0; e < VEC; ++e) red[t][e] = acc[0][e];
            __syncthreads();
            if (t < cpr) {
                float sum[VEC];
#pragma unroll
                for (int e = 0; e < VEC; ++e) sum[e] = red[t][e];
                for (int r = 1; r < RP; ++r)
#pragma unroll
                    for (int e = 0; e < VEC; ++e) sum[e] += red[r * cpr + t][e];
                *reinterpret_cast<float4 *>(dst + t * VEC) = float4{sum[0], sum[1], sum[2], sum[3]};
                *reinterpret_cast<float4 *>(dst + t * VEC + 4) = float4{sum[4], sum[5], sum[6], sum[7]};
            }
        } else {
#pragma unroll
            for (int s = 0; s < S; ++s) {
                if (!slot[s]) continue;
                float *d = dst + cc_of[s] * VEC;
                *reinterpret_cast<float4 *>(d) = float4{acc[s][0], acc[s][1], acc[s][2], acc[s][3]};
                *reinterpret_cast<float4 *>(d + 4) = float4{acc[s][4], acc[s][5], acc[s][6], acc[s][7]};
            }
        }
    }
}

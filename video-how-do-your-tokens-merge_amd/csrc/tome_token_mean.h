// tome_token_mean.h -- part of the single translation unit csrc/tome_kernels.hip (the column mean over a clip's tokens).
#pragma once

// k_token_mean: out[g, c] = (1 / tokens) * sum_t v[g, t, c] for contiguous 16-bit x [groups, tokens, width], fp32 out
// [groups, width] -- what is left of the last block of a mean-pooling ViT (`x.mean(1)` in front of `fc_norm`,
// slowfast/models/videomae_video_model_builder.py forward_features) once the linear steps behind the MLP's activation
// are moved behind the mean (`Mlp.forward`: fc2 of the mean instead of the mean of fc2).
//   ACT == TOKEN_MEAN_NONE: v = x.
//   ACT == TOKEN_MEAN_GELU_ERF: v = the 16-bit value k_gelu_erf would have stored (gelu_erf_value of tome_common.h, rounded
//                               to TX, widened again): the mean of exactly the activation bits fc2 used to read; the
//                               activation itself is never written.
// One workgroup per (group, slab of 512 channels): a wave reads a 1 KB row segment, 16 bytes per lane, non-temporal (the
// tensor is read once); wave w of the four walks rows w, w + 4, w + 8, ... in ascending order, eight of them in flight,
// with eight fp32 sums per lane in registers.  The four waves' sums meet in LDS and are added in wave order by wave 0: no
// atomics, one summation order, the same bits on every run.  Lanes whose channels lie beyond `width` (the last slab)
// load and store nothing.
enum { TOKEN_MEAN_NONE = 0, TOKEN_MEAN_GELU_ERF = 1 };
#define TOKEN_MEAN_SLAB 512  // channels per workgroup: 64 lanes x 8

template <typename TX, int ACT>
__global__ __launch_bounds__(256) void k_token_mean(const TX *__restrict__ x, int64_t tokens, int width, int slabs,
                                                    float *__restrict__ out) {
    constexpr int VEC = 8;    // 16 bytes of a 16-bit type
    constexpr int WAVES = 4;
    constexpr int U = 8;      // rows in flight per wave
    static_assert(sizeof(TX) == 2, "16-bit tokens");
    __shared__ float part[WAVES - 1][VEC * WAVE];
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x >> 6;
    const int64_t g = blockIdx.x / slabs;
    const int slab = (int)(blockIdx.x - g * slabs);
    const int c0 = slab * TOKEN_MEAN_SLAB + lane * VEC;
    const bool live = c0 < width;
    float sum[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) sum[e] = 0.0f;
    if (live) {
        const TX *base = x + g * tokens * width + c0;
        for (int64_t t0 = wave; t0 < tokens; t0 += WAVES * U) {
            uint4 raw[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t t = t0 + u * WAVES;
                if (t < tokens) raw[u] = ld16(base + t * width);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (t0 + u * WAVES >= tokens) continue;
                Pack<TX, VEC> pk;
                __builtin_memcpy(&pk, &raw[u], 16);
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    float v = to_f32(pk.e[e]);
                    // (fp32_value, tome_gelu_bwd.h: the activation exists as an fp32 value before it is rounded, as in
                    // k_gelu_erf -- without the fence the fp16 form rounds the last product once, in v_fma_mixlo_f16)
                    if (ACT == TOKEN_MEAN_GELU_ERF)
                        v = to_f32(from_f32<TX>(fp32_value(gelu_erf_value(v, gelu_erf_one_plus(v)))));
                    sum[e] += v;
                }
            }
        }
    }
    if (wave > 0) {
#pragma unroll
        for (int e = 0; e < VEC; ++e) part[wave - 1][e * WAVE + lane] = sum[e];
    }
    __syncthreads();
    if (wave == 0 && live) {
        const float n = (float)tokens;
        float *o = out + g * width + c0;
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
#pragma unroll
            for (int w = 0; w < WAVES - 1; ++w) sum[e] += part[w][e * WAVE + lane];
            o[e] = sum[e] / n;
        }
    }
}

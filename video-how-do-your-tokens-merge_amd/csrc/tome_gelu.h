// tome_gelu.h -- part of the single translation unit csrc/tome_kernels.hip (GELU forward; the backward is tome_gelu_bwd.h).
#pragma once
// k_gelu_erf: the activation between the two GEMMs of the MLP the patched block calls (`self.mlp(self.norm2(x))`,
// tome/patch/videomae.py:29; nn.GELU() = exact erf form in VideoMAE / TimeSformer / Motionformer):
//     y = x * 0.5 * (1 + erf(x / sqrt(2)))      fp32 arithmetic on 16-bit values, one rounding -- the expression and
// operation order of the framework's kernel, so the result is bit-identical to it.  A pure streaming pass: four
// 16-byte chunks per lane in flight, non-temporal both ways (the [tokens, 4C] activation is 1.2 GB at batch 128).
// k_gelu_tanh: ViViT's activation (`layer.intermediate`, tome/patch/vivit.py layer forward; HF's "gelu_fast"), the same
// pass with the tanh form of tome_common.h: y = x * sigma(2 beta (x + kappa x^3)).
template <typename TX, int FORM>
__device__ __forceinline__ void gelu_stream(const TX *__restrict__ x, TX *__restrict__ y, int64_t chunks) {
    constexpr int VEC = 16 / sizeof(TX);
    constexpr int NIT = 4;
    const int64_t base = ((int64_t)blockIdx.x * blockDim.x) * NIT + threadIdx.x;
    uint4 raw[NIT];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int64_t q = base + (int64_t)it * blockDim.x;
        if (q < chunks) raw[it] = ld16(reinterpret_cast<const uint4 *>(x) + q);
    }
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int64_t q = base + (int64_t)it * blockDim.x;
        if (q >= chunks) continue;
        Pack<TX, VEC> pk;
        __builtin_memcpy(&pk, &raw[it], 16);
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            const float v = to_f32(pk.e[e]);
            if (FORM == GELU_TANH) {
                float c, v2;
                pk.e[e] = from_f32<TX>(gelu_tanh_value(v, gelu_tanh_sigmoid(v, c, v2)));
            } else {
                pk.e[e] = from_f32<TX>(gelu_erf_value(v, gelu_erf_one_plus(v)));
            }
        }
        uint4 o;
        __builtin_memcpy(&o, &pk, 16);
        st16(reinterpret_cast<uint4 *>(y) + q, o);
    }
}

template <typename TX>
__global__ __launch_bounds__(256) void k_gelu_erf(const TX *__restrict__ x, TX *__restrict__ y, int64_t chunks) {
    gelu_stream<TX, GELU_ERF>(x, y, chunks);
}

template <typename TX>
__global__ __launch_bounds__(256) void k_gelu_tanh(const TX *__restrict__ x, TX *__restrict__ y, int64_t chunks) {
    gelu_stream<TX, GELU_TANH>(x, y, chunks);
}

// tome_common.h -- part of the single translation unit csrc/tome_kernels.hip (element types, 16-byte packs, output-row layout).
#pragma once
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

#define WAVE 64

// ------------------------------------------------------------------------------------------------
// element types
// ------------------------------------------------------------------------------------------------
struct bf16_t { uint16_t v; };
struct f16_t { _Float16 v; };

__device__ __forceinline__ float to_f32(float x) { return x; }
__device__ __forceinline__ float to_f32(bf16_t x) { return __uint_as_float(((uint32_t)x.v) << 16); }
__device__ __forceinline__ float to_f32(f16_t x) { return (float)x.v; }

template <typename T> __device__ __forceinline__ T from_f32(float f);
template <> __device__ __forceinline__ float from_f32<float>(float f) { return f; }
template <> __device__ __forceinline__ bf16_t from_f32<bf16_t>(float f) {
    // round-to-nearest-even, NaN stays NaN (v_cvt_pk_bf16_f32 on gfx950)
    __bf16 b = (__bf16)f;
    bf16_t r;
    __builtin_memcpy(&r.v, &b, 2);
    return r;
}
template <> __device__ __forceinline__ f16_t from_f32<f16_t>(float f) {
    f16_t r;
    r.v = (_Float16)f;
    return r;
}

// nn.GELU() in its exact erf form, x * 0.5 * (1 + erf(x / sqrt(2))), in the framework kernel's expression and operation
// order (k_gelu_erf stores these bits; k_gelu_bwd rebuilds them from the saved pre-activation, and its Phi(x) is half
// of the same 1 + erf).
__device__ __forceinline__ float gelu_erf_one_plus(float x) { return 1.0f + erff(x * 0.70710678118654752440f); }
__device__ __forceinline__ float gelu_erf_value(float x, float one_plus_erf) { return x * 0.5f * one_plus_erf; }

// The activation's form, a template parameter of the GELU kernels (k_gelu_erf / k_gelu_tanh, k_gelu_bwd).
enum { GELU_ERF = 0, GELU_TANH = 1 };

// The tanh GELU (HF's "gelu_fast" in ViViT's MLP, F.gelu(approximate="tanh")) in its sigmoid form (include/tome_hip.h,
// tome_gelu_tanh): u = beta (x + kappa x^3), s = sigma(2u) = 0.5 (1 + tanh u), the activation x s.  s and 1 - s both
// come from e = exp(-2|u|) in (0, 1] as r = 1 / (1 + e) and e r, picked by the sign of u: neither cancels, where the
// framework's 1 + tanh(u) has lost every bit below x = -4.  e is one v_exp_f32 of -2 log2(e) |u| and r one v_rcp_f32
// (1 ulp each; 1 + e lies in [1, 2]): with the library's expf and two IEEE divisions the backward pass was bound by
// the vector ALU at 0.4 of the memory rate.  Returns s, leaves 1 - s in `one_minus` and x^2 in `x2` (k_gelu_tanh stores
// x s; k_gelu_bwd rebuilds those bits from the saved pre-activation and needs all three).
#define GELU_TANH_BETA 0.7978845608028654f
#define GELU_TANH_KAPPA 0.044715f
__device__ __forceinline__ float gelu_tanh_sigmoid(float x, float &one_minus, float &x2) {
    x2 = x * x;
    const float u = GELU_TANH_BETA * (x + GELU_TANH_KAPPA * x2 * x);
    const float e = __builtin_amdgcn_exp2f(-2.8853900817779268f * fabsf(u));  // 2 log2(e)
    const float big = __builtin_amdgcn_rcpf(1.0f + e), small = e * big;
    one_minus = u >= 0.0f ? small : big;
    return u >= 0.0f ? big : small;
}
__device__ __forceinline__ float gelu_tanh_value(float x, float s) { return x * s; }

// A lane's slice of a row: VEC consecutive elements moved with one 16-byte (or narrower) access.
template <typename T, int VEC> struct Pack { T e[VEC]; };

template <typename T, int VEC>
__device__ __forceinline__ void load_pack(const T *p, float (&out)[VEC]) {
    typedef Pack<T, VEC> __attribute__((aligned(sizeof(T) * VEC))) P;
    P v = *reinterpret_cast<const P *>(p);
#pragma unroll
    for (int i = 0; i < VEC; ++i) out[i] = to_f32(v.e[i]);
}

template <typename T, int VEC>
__device__ __forceinline__ void store_pack(T *p, const float (&in)[VEC]) {
    typedef Pack<T, VEC> __attribute__((aligned(sizeof(T) * VEC))) P;
    P v;
#pragma unroll
    for (int i = 0; i < VEC; ++i) v.e[i] = from_f32<T>(in[i]);
    *reinterpret_cast<P *>(p) = v;
}

// Output layout of a merged sequence (merge.py:82-85): row of the k-th unmerged A token / of B token j.
__device__ __forceinline__ int out_row_unm(int k, int distill) { return (distill && k >= 1) ? k + 1 : k; }
__device__ __forceinline__ int out_row_dst(int j, int U, int distill) {
    if (!distill) return U + j;
    return j == 0 ? 1 : U + j;
}


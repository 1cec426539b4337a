// tome_ln_rows.h -- part of the single translation unit csrc/tome_kernels.hip: the row statistics of every kernel that
// normalises "up to four rows per wave, NIT slots per lane" -- the LayerNorm tails of k_merge_rows_fast<LN>,
// k_add_ln_rows (16-bit and autocast forms), k_add_ln_regroup, k_merge_rows_ln_amp (tome_merge.h, tome_ln_fwd.h, tome_merge_ln_amp.h) and
// the statistics k_ln_rows_bwd_amp and k_merge_ln_rows_bwd_amp recompute (tome_ln_bwd.h, tome_merge_ln_bwd_amp.h).  No
// forward kernel saves mean or rstd: those backward kernels reproduce the forward's bits because they call the forward's
// own functions (ln_row_means, slot_centre, ln_rstd), not a copy of them.  The 16-bit backward kernels (k_ln_rows_bwd, k_merge_ln_rows_bwd) keep a copy of the
// two rounds, for their speed (tome_ln_bwd.h says what the shared rounds cost them); a test of bits ties k_ln_rows_bwd
// to k_ln_rows_bwd_amp.
#pragma once

// 16-byte moves of the streaming kernels (k_merge_rows_fast, k_add_ln_rows, k_add_ln_regroup): tokens are read once
// and written once, 0.3-1.2 GB per launch against 256 MB of Infinity Cache, so both directions are issued
// non-temporal.  Measured at batch 128, same box, alternating builds: merge+LN 226 -> 214 us (5.12 -> 5.40 TB/s),
// add+LN 215 -> 189 us (5.37 -> 6.12 TB/s); inside the model (rocprofv3) 228 -> 221 and 204 -> 188 us with the GEMMs
// that read the results unchanged (581 vs 578 us).
typedef unsigned int nt_u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint4 ld16(const void *p) {
    const nt_u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const nt_u32x4 *>(p));
    return uint4{v.x, v.y, v.z, v.w};
}
__device__ __forceinline__ void st16(void *p, const uint4 &v) {
    nt_u32x4 w;
    w.x = v.x; w.y = v.y; w.z = v.z; w.w = v.w;
    __builtin_nontemporal_store(w, reinterpret_cast<nt_u32x4 *>(p));
}

// ------------------------------------------------------------------------------------------------
// The streaming kernels sit at the vector-issue limit of the SIMDs, not only at the HBM limit (measured in round 2:
// adding ~75 vector instructions per lane cost the merge kernel 6 %; occupancy and index prefetch changed nothing), so
// the LayerNorm is written for few instructions:
//   * the sum of a 16-byte chunk by dot products with a vector of ones (v_dot2c_f32_bf16 / _f16: two elements per
//     instruction, no unpacking);
//   * wave totals by a DPP scan (row_shr 1/2/4/8, row_bcast 15/31) read back from lane 63 as a wave-uniform scalar,
//     instead of six ds_bpermute round trips per total -- and only for the rows the wave really holds (R of 4);
//   * the centred values d = x - mean kept in registers between the variance pass and the output pass;
//   * y = d * (rstd * w) + b as one multiply and one fma per element; 1/C as a multiplication, rstd by v_rsq_f32.
// Two passes (mean, then centred variance): a row far from zero keeps its variance.
// ------------------------------------------------------------------------------------------------
template <int CTRL, int ROW_MASK> __device__ __forceinline__ float dpp_add(float v) {
    const int t = __builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, ROW_MASK, 0xf, false);
    return v + __int_as_float(t);
}
__device__ __forceinline__ float wave_total(float v) {  // sum over the 64 lanes, wave-uniform
    v = dpp_add<0x111, 0xf>(v);  // row_shr:1
    v = dpp_add<0x112, 0xf>(v);  // row_shr:2
    v = dpp_add<0x114, 0xf>(v);  // row_shr:4
    v = dpp_add<0x118, 0xf>(v);  // row_shr:8  -> lane 15 of every row of 16 holds the row's total
    v = dpp_add<0x142, 0xa>(v);  // row_bcast:15 into rows 1 and 3
    v = dpp_add<0x143, 0xc>(v);  // row_bcast:31 into rows 2 and 3 -> lane 63 holds the total
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}

typedef __bf16 dot_bf16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 dot_f16x2 __attribute__((ext_vector_type(2)));
template <typename TX> __device__ __forceinline__ float chunk_sum(const uint4 &v);
template <> __device__ __forceinline__ float chunk_sum<bf16_t>(const uint4 &v) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w}, ones = 0x3f803f80u;
    dot_bf16x2 o, p;
    __builtin_memcpy(&o, &ones, 4);
    float t = 0.0f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        __builtin_memcpy(&p, &w[i], 4);
        t = __builtin_amdgcn_fdot2_f32_bf16(p, o, t, false);
    }
    return t;
}
template <> __device__ __forceinline__ float chunk_sum<f16_t>(const uint4 &v) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w}, ones = 0x3c003c00u;
    dot_f16x2 o, p;
    __builtin_memcpy(&o, &ones, 4);
    float t = 0.0f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        __builtin_memcpy(&p, &w[i], 4);
        t = __builtin_amdgcn_fdot2(p, o, t, false);
    }
    return t;
}

__device__ __forceinline__ float pick4(int rr, float a0, float a1, float a2, float a3, int R) {
    float v = a0;
    if (R > 1) v = rr == 1 ? a1 : v;
    if (R > 2) {
        v = rr == 2 ? a2 : v;
        v = rr == 3 ? a3 : v;
    }
    return v;
}

// ------------------------------------------------------------------------------------------------
// A lane SLOT is the 8 channels a 16-byte chunk of 16-bit tokens holds, whatever the byte width of the tensor it is
// taken from: 16 bytes of a 16-bit tensor, 32 bytes (two 16-byte moves) of an fp32 one (a model under torch.autocast
// with fp32 master weights: tools/train_net.py:123, tome/utils.py:54).  Slot q of a wave's rows sits in lane q % 64,
// iteration q / 64, so the packing (rows per wave, slots per lane) is the same for every dtype.
// ------------------------------------------------------------------------------------------------
template <typename T> struct Slot { uint4 q[sizeof(T) / 2]; };

template <typename T> __device__ __forceinline__ Slot<T> ld_slot(const T *base, int64_t slot) {
    Slot<T> s;
    const uint4 *p = reinterpret_cast<const uint4 *>(base) + slot * (int64_t)(sizeof(T) / 2);
#pragma unroll
    for (int k = 0; k < (int)(sizeof(T) / 2); ++k) s.q[k] = ld16(p + k);
    return s;
}
template <typename T> __device__ __forceinline__ void st_slot(T *base, int64_t slot, const Slot<T> &s) {
    uint4 *p = reinterpret_cast<uint4 *>(base) + slot * (int64_t)(sizeof(T) / 2);
#pragma unroll
    for (int k = 0; k < (int)(sizeof(T) / 2); ++k) st16(p + k, s.q[k]);
}
// a slot of a parameter vector (weight, bias: 16-bit, or fp32 under autocast): plain cached loads
template <typename T> __device__ __forceinline__ Slot<T> ld_param_slot(const T *__restrict__ base, int slot) {
    Slot<T> s;
    const uint4 *p = reinterpret_cast<const uint4 *>(base) + slot * (int)(sizeof(T) / 2);
#pragma unroll
    for (int k = 0; k < (int)(sizeof(T) / 2); ++k) s.q[k] = p[k];
    return s;
}
template <typename T> __device__ __forceinline__ void slot_f32(const Slot<T> &s, float (&v)[8]) {
    Pack<T, 8> p;
    __builtin_memcpy(&p, &s, sizeof(p));
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = to_f32(p.e[e]);
}
template <typename T> __device__ __forceinline__ float slot_at(const Slot<T> &s, int e) {  // value e of the 8
    Pack<T, 8> p;
    __builtin_memcpy(&p, &s, sizeof(p));
    return to_f32(p.e[e]);
}
template <typename T> __device__ __forceinline__ Slot<T> f32_slot(const float (&v)[8]) {  // one rounding (none: fp32)
    Pack<T, 8> p;
#pragma unroll
    for (int e = 0; e < 8; ++e) p.e[e] = from_f32<T>(v[e]);
    Slot<T> s;
    __builtin_memcpy(&s, &p, sizeof(p));
    return s;
}
// the sum of a slot's 8 stored values: chunk_sum's dot products for 16-bit rows, a chain of seven fp32 additions in
// channel order for fp32 rows
template <typename T> __device__ __forceinline__ float slot_sum(const Slot<T> &s) {
    if constexpr (std::is_same<T, float>::value) {
        float v[8];
        slot_f32<T>(s, v);
        float t = v[0];
#pragma unroll
        for (int e = 1; e < 8; ++e) t += v[e];
        return t;
    } else {
        return chunk_sum<T>(s.q[0]);
    }
}
// x + a in fp32, rounded once to the stream's dtype (not at all for an fp32 stream: `x + a.float()` bit for bit)
template <typename TX, typename TA> __device__ __forceinline__ Slot<TX> slot_add(const Slot<TX> &x, const Slot<TA> &a) {
    float xv[8], av[8];
    slot_f32<TX>(x, xv);
    slot_f32<TA>(a, av);
#pragma unroll
    for (int e = 0; e < 8; ++e) xv[e] = __fadd_rn(xv[e], av[e]);
    return f32_slot<TX>(xv);
}

// ------------------------------------------------------------------------------------------------
// Per-row sums of the (up to) four rows of a wave.  Every lane adds what its slots hold to the row each slot belongs
// to (rr: 0..R-1, anything else: to none); mean() is the wave total of each row the wave holds times a scale.
// ------------------------------------------------------------------------------------------------
struct Row4 {
    float r0, r1, r2, r3;
    __device__ __forceinline__ float at(int rr, int R) const { return pick4(rr, r0, r1, r2, r3, R); }
};
struct RowAcc {
    float p0 = 0.0f, p1 = 0.0f, p2 = 0.0f, p3 = 0.0f;
    __device__ __forceinline__ void add(int rr, float v, int R) {
        p0 += rr == 0 ? v : 0.0f;
        if (R > 1) p1 += rr == 1 ? v : 0.0f;
        if (R > 2) {
            p2 += rr == 2 ? v : 0.0f;
            p3 += rr == 3 ? v : 0.0f;
        }
    }
    __device__ __forceinline__ Row4 mean(float inv_c, int R) const {
        Row4 m{wave_total(p0) * inv_c, 0.0f, 0.0f, 0.0f};
        if (R > 1) m.r1 = wave_total(p1) * inv_c;
        if (R > 2) {
            m.r2 = wave_total(p2) * inv_c;
            m.r3 = wave_total(p3) * inv_c;
        }
        return m;
    }
};

// Round 1 of the forward AND of k_ln_rows_bwd_amp: the mean of each row, from the stored slots.
template <typename TS, int NIT>
__device__ __forceinline__ Row4 ln_row_means(const Slot<TS> (&raw)[NIT], const int (&rowof)[NIT], int R, float inv_c) {
    RowAcc p;  // (rowof < 0, a lane without a slot: what it loaded is zeroed before it meets any addition)
#pragma unroll
    for (int it = 0; it < NIT; ++it) p.add(rowof[it], rowof[it] >= 0 ? slot_sum<TS>(raw[it]) : 0.0f, R);
    return p.mean(inv_c, R);
}
// d = x - m for the 8 stored values of a slot (converted here, not before round 1: the slots stay packed across the
// first reduction); returns the slot's sum of d^2
template <typename TS> __device__ __forceinline__ float slot_centre(const Slot<TS> &raw, float m, float (&d)[8]) {
    slot_f32<TS>(raw, d);
    float u = 0.0f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        d[e] = d[e] - m;
        u = __fmaf_rn(d[e], d[e], u);
    }
    return u;
}
__device__ __forceinline__ Row4 ln_rstd(const Row4 &var, float eps, int R) {
    Row4 r{__builtin_amdgcn_rsqf(var.r0 + eps), 0.0f, 0.0f, 0.0f};
    if (R > 1) r.r1 = __builtin_amdgcn_rsqf(var.r1 + eps);
    if (R > 2) {
        r.r2 = __builtin_amdgcn_rsqf(var.r2 + eps);
        r.r3 = __builtin_amdgcn_rsqf(var.r3 + eps);
    }
    return r;
}

// The weight and bias slots of every slot column this lane holds.  Request (ln_params) and use (ln_rows) are two calls:
// a kernel issues the loads where they cost it least and uses them after the two reductions.
template <typename TP, int NIT> struct LnParams { Slot<TP> w[NIT], b[NIT]; };

template <typename TP, int NIT>
__device__ __forceinline__ LnParams<TP, NIT> ln_params(const TP *__restrict__ lw, const TP *__restrict__ lb,
                                                       const int (&rowof)[NIT], int cpr, int lane) {
    LnParams<TP, NIT> p;
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int rr = rowof[it];
        const int cc = rr < 0 ? 0 : it * WAVE + lane - rr * cpr;  // (unconditional: a lane without a slot reads column 0)
        p.w[it] = ld_param_slot<TP>(lw, cc);
        p.b[it] = ld_param_slot<TP>(lb, cc);
    }
    return p;
}

// The LayerNorm of the rows of a wave as they were stored.  raw[it]: the stored bits of slot `it` of this lane, rowof[it]
// its row 0..R-1 or -1; TS the rows' dtype, TP the parameters', TY y's.  store_y(rr, cc, slot) writes one normalised slot
// (cc = slot column in its row), rounded once to TY -- every value straight into its place in the pack: through an fp32
// array and f32_slot the compiler pairs the bf16 conversions across elements and shuffles the halves back (three more
// instructions per four values, and up to 12 more VGPRs in k_merge_rows_fast<LN>).
// ln_rows_finish is the body behind round 1, for the one caller that takes the mean itself (merge_dst_row_amp).
template <typename TS, typename TP, typename TY, int NIT, typename StoreY>
__device__ __forceinline__ void ln_rows_finish(const Slot<TS> (&raw)[NIT], const int (&rowof)[NIT], int R, int cpr,
                                               float inv_c, float eps, const Row4 &mean, const LnParams<TP, NIT> &prm,
                                               int lane, StoreY store_y) {
    float d[NIT][8];
    RowAcc v;
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const float u = slot_centre<TS>(raw[it], mean.at(rowof[it], R), d[it]);
        v.add(rowof[it], rowof[it] >= 0 ? u : 0.0f, R);
    }
    const Row4 rstd = ln_rstd(v.mean(inv_c, R), eps, R);
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int rr = rowof[it];
        if (rr < 0) continue;
        const float rs = rstd.at(rr, R);
        Pack<TY, 8> py;
#pragma unroll
        for (int e = 0; e < 8; ++e)
            py.e[e] = from_f32<TY>(__fmaf_rn(d[it][e], slot_at<TP>(prm.w[it], e) * rs, slot_at<TP>(prm.b[it], e)));
        Slot<TY> ys;
        __builtin_memcpy(&ys, &py, sizeof(py));
        store_y(rr, it * WAVE + lane - rr * cpr, ys);
    }
}

template <typename TS, typename TP, typename TY, int NIT, typename StoreY>
__device__ __forceinline__ void ln_rows(const Slot<TS> (&raw)[NIT], const int (&rowof)[NIT], int R, int cpr, int C,
                                        float eps, const LnParams<TP, NIT> &prm, int lane, StoreY store_y) {
    const float inv_c = __builtin_amdgcn_rcpf((float)C);
    ln_rows_finish<TS, TP, TY, NIT>(raw, rowof, R, cpr, inv_c, eps, ln_row_means<TS, NIT>(raw, rowof, R, inv_c), prm, lane,
                                    store_y);
}

// Round 2 of k_ln_rows_bwd_amp, behind ln_row_means: with gw = gy * weight (gw_of(it, e): value e of slot `it`) and
// d = x' - mean (returned), per row
//     rstd,   mgw = mean(gw),   k = rstd * mean(gw * xhat) = rstd^2 * sum(gw * d) / C        (xhat * mean(.) = d * k)
// srow[it]: the row whose statistics slot `it` enters, grow[it]: the row whose gradient sums it enters (-1: none; a
// class row of skip_first has statistics and no gradient).
struct LnBwdRows { Row4 rstd, mgw, k; };

template <typename TS, int NIT, typename GwOf>
__device__ __forceinline__ LnBwdRows ln_rows_bwd_stats(const Slot<TS> (&xraw)[NIT], const int (&srow)[NIT],
                                                       const int (&grow)[NIT], const Row4 &mean, int R, float inv_c,
                                                       float eps, GwOf gw_of, float (&d)[NIT][8]) {
    RowAcc v, a, b;  // sum d^2, sum gw, sum gw * d
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        v.add(srow[it], slot_centre<TS>(xraw[it], mean.at(srow[it], R), d[it]), R);
        float sa = 0.0f, sb = 0.0f;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float gw = gw_of(it, e);
            sa += gw;
            sb = __fmaf_rn(gw, d[it][e], sb);
        }
        a.add(grow[it], sa, R);
        b.add(grow[it], sb, R);
    }
    LnBwdRows o;
    o.rstd = ln_rstd(v.mean(inv_c, R), eps, R);
    o.mgw = a.mean(inv_c, R);
    const Row4 s = b.mean(inv_c, R);
    o.k = Row4{o.rstd.r0 * (o.rstd.r0 * s.r0), 0.0f, 0.0f, 0.0f};
    if (R > 1) o.k.r1 = o.rstd.r1 * (o.rstd.r1 * s.r1);
    if (R > 2) {
        o.k.r2 = o.rstd.r2 * (o.rstd.r2 * s.r2);
        o.k.r3 = o.rstd.r3 * (o.rstd.r3 * s.r3);
    }
    return o;
}

// tome_merge_slab.h -- part of the single translation unit csrc/tome_kernels.hip: the row slab the streaming kernels of
// the merge family walk, each fact about it written once.  A wave owns R <= 4 consecutive rows of one group; their
// R * cpr 16-byte slots are flattened over the lanes (slot q = it * 64 + lane, it < NIT), and every load of the slab is
// issued before any use.  Lanes 0..R-1 work out the facts of row 0..R-1 in parallel and hand them to the whole wave as
// scalars.  What keeps the loads together is kept HERE: they are unconditional (hipcc sinks the first use of a
// conditionally loaded value into the `if`, an s_waitcnt vmcnt(0) behind every load), so a lane without a row is
// clamped onto a harmless entry and a size or scale that is absent is read from a pointer the caller knows to be valid.
// Callers: k_merge_rows_fast, k_merge_rows_ln_amp, k_merge_rows_bwd, k_merge_ln_rows_bwd[_amp]; the slot map, broadcast and
// select also serve tome_ln_fwd.h and tome_ln_bwd.h.  DESIGN.md, "Where the merge slab lives": who calls what, copies kept.
#pragma once

// Where the token rows of group g live.  Contiguous [n,T,C] is {0, T*C, 0, C, 1}; the regrouped views of
// TimeSformer / Motionformer ('b (p t) m -> (b t) p m', timesformer.py:89-90; 'b (s f) d -> (b f) s d',
// motionformer.py:150-151) are {cls*C, (cls+P*F)*C, C, F*C, F}: no permuted copy of x is ever made.
struct TokLayout {
    int64_t base, outer_stride, inner_stride, tok_stride;  // elements
    int inner;                                             // groups per outer index
};

template <typename TX> __device__ __forceinline__ TX *group_ptr(TX *p, const TokLayout &L, int g) {
    if (L.inner == 1) return p + L.base + (int64_t)g * L.outer_stride;  // (no integer division on the plain layout)
    return p + L.base + (int64_t)(g / L.inner) * L.outer_stride + (int64_t)(g % L.inner) * L.inner_stride;
}

// Optional LayerNorm fused behind the merge (the block's norm2 -- tome/patch/videomae.py:27 `self.norm2(x)`,
// vivit.py:41 `layernorm_after`): y = (x' - mean) * rstd * weight + bias over the channels of every merged
// row, fp32 statistics (two passes over the registers: mean, then centred variance), written next to x'.
struct LnArgs {
    const void *weight, *bias;  // [C] of the token dtype
    void *y;                    // [n, T-r, C] of the token dtype, same row layout as x_out
    float eps;
    const void *addend;         // optional [n, T, C]: the tokens that are merged are round(x + addend), i.e. the
                                // block's residual `x = x + attn(...)` (videomae.py:20,25) is taken on the fly
    // The addend may live in a layout of its own (a_own): TimeSformer's second residual is the spatial attention's
    // output [(b t), 1 + p, m] (timesformer.py:40-52), read where it lies instead of being permuted to 'b (p t) m'
    // first; the class rows' addend (the class token averaged over the frames, timesformer.py:42-44) is then a
    // separate [B, C] tensor.
    int a_own;
    TokLayout la;
    const void *cls_addend;
    // optional [C]: the rows of x_out are stored as round(x' + xbias) while y stays LayerNorm(x').  The caller's next
    // GEMM accumulates onto x_out in place (`x = x + fc2(...)`, tome/patch/videomae.py:29, as beta = 1 on the residual
    // buffer), so its bias has to be in the buffer beforehand and the separate residual add disappears.
    const void *xbias;
};

// the addend rows of group g (nullptr without an addend: no pointer is formed from a null one) and their token stride:
// in the addend's own layout (a_own) or in x's
template <typename TX>
__device__ __forceinline__ const TX *ln_addend_rows(const LnArgs &ln, const TokLayout &lin, int g, int64_t &astride) {
    astride = ln.a_own ? ln.la.tok_stride : lin.tok_stride;
    if (!ln.addend) return nullptr;
    return ln.a_own ? group_ptr(reinterpret_cast<const TX *>(ln.addend), ln.la, g)
                    : group_ptr(reinterpret_cast<const TX *>(ln.addend), lin, g);
}

// size' of one output row, and -- for the proportional-attention bias of the next block
// (`size.log()`, tome/patch/videomae.py:62-63, timesformer.py:73-74, motionformer.py:107-111, vivit.py:103-104)
// -- log of the STORED size, fp32 logf rounded to the size dtype: what torch's `size.log()` gives on this device.
template <typename TS>
__device__ __forceinline__ void store_size(TS *__restrict__ srow, TS *__restrict__ lrow, float s) {
    const TS st = from_f32<TS>(s);
    *srow = st;
    if (lrow) *lrow = from_f32<TS>(logf(to_f32(st)));
}

// inverse of the output layout (merge.py:82-85): output row o -> (is it a B/dst row?, index in its set)
__device__ __forceinline__ void decode_out_row(int o, int U, int distill, bool &is_dst, int &idx) {
    if (!distill) {
        is_dst = o >= U;
        idx = is_dst ? o - U : o;
    } else if (o == 0) { is_dst = false; idx = 0; }
    else if (o == 1) { is_dst = true; idx = 0; }
    else if (o <= U) { is_dst = false; idx = o - 1; }
    else { is_dst = true; idx = o - U; }
}

// ---- slot map: slot q = it * 64 + lane of a slab of rows `cpr` slots wide -> row-in-wave rr (0..3), and its slot column
// in that row.  (q is formed in here: handed in as an argument, the compares come out with their operands swapped.)
__device__ __forceinline__ int slab_row(int cpr, int it, int lane) {
    const int q = it * WAVE + lane;
    return (q >= cpr) + (q >= 2 * cpr) + (q >= 3 * cpr);
}
__device__ __forceinline__ int slab_col(int q, int rr, int cpr) { return q - rr * cpr; }

// ---- select: the value of row rr (0..3; anything else takes a3) among four wave-uniform ones, any type.  pick4
// (tome_ln_rows.h) is the float form that knows R.  A macro, and fed with plain locals: as a function (by value, by
// reference, as a member of a struct of four) the selects reach the kernel already folded, where the written-out form
// is folded together with the kernel's other tests of rr -- k_merge_rows_bwd took 55 vector registers for 50.
#define SEL4(rr, a0, a1, a2, a3) ((rr) == 0 ? (a0) : ((rr) == 1 ? (a1) : ((rr) == 2 ? (a2) : (a3))))
// ---- broadcast: what lanes 0..3 hold of a per-lane value, as four wave-uniform scalars
__device__ __forceinline__ void lanes4(int my, int &a0, int &a1, int &a2, int &a3) {
    a0 = __builtin_amdgcn_readlane(my, 0), a1 = __builtin_amdgcn_readlane(my, 1);
    a2 = __builtin_amdgcn_readlane(my, 2), a3 = __builtin_amdgcn_readlane(my, 3);
}
__device__ __forceinline__ void lanes4(float my, float &a0, float &a1, float &a2, float &a3) {
    a0 = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(my), 0));
    a1 = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(my), 1));
    a2 = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(my), 2));
    a3 = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(my), 3));
}

// ---- forward slab facts (k_merge_rows_fast, k_merge_rows_ln_amp): the wave streams OUTPUT rows o0 .. o0+R-1 of group g.
// Lane L < R: the token row L is read from and its B-row number (-1: an unmerged A token, which receives nothing).  A
// wave whose rows are all destination (odd) tokens knows its tokens without reading an index -- its row loads depend
// on no earlier load; the others read unm_idx, which goes out together with the caller's first block of dst_idx.  The
// size entry is read unconditionally from size_src (the group's sizes, or the tokens themselves when there are none)
// and converted by the caller only after its row loads are out: two memory round trips (index -> rows), not three.
// vmask is handed back whole: bit rr says row rr exists.
template <typename TS> struct FwdSlab {
    int tok0, tok1, tok2, tok3, j0, j1, j2, j3;  // rows 0..3: token, B-row number
    unsigned long long vmask;
    bool my_valid;  // lane < R and its row exists
    TS my_s_raw;    // the lane's size entry, unconverted
};
template <typename TS>
__device__ __forceinline__ FwdSlab<TS> fwd_slab(const TS *__restrict__ size_src, const int64_t *__restrict__ unm_idx,
                                                int g, int o0, int R, int To, int U, int distill, int lane) {
    const bool my_valid = lane < R && (o0 + lane) < To;
    bool is_dst;
    int idx;
    decode_out_row(my_valid ? o0 + lane : 0, U, distill, is_dst, idx);
    int my_tok = 2 * idx + 1, my_j = idx;
    const bool all_dst = (!distill && o0 >= U) || o0 > U;
    if (U > 0 && !all_dst) {  // (wave-uniform; unm_idx may be absent when every even token is merged away)
        const int ut = 2 * (int)unm_idx[(int64_t)g * U + ((my_valid && !is_dst) ? idx : 0)];
        my_tok = is_dst ? my_tok : ut;
        my_j = is_dst ? my_j : -1;
    }
    my_tok = my_valid ? my_tok : 0;
    my_j = my_valid ? my_j : -1;
    FwdSlab<TS> f;
    f.my_s_raw = size_src[my_tok], f.vmask = __ballot(my_valid), f.my_valid = my_valid;
    lanes4(my_tok, f.tok0, f.tok1, f.tok2, f.tok3);
    lanes4(my_j, f.j0, f.j1, f.j2, f.j3);
    return f;
}

// ---- edge rows: which of the wave's four rows receive sources (B-row numbers j; d_first: dst_idx[lane] of the group's
// first 64 ranks, -2 beyond r).  Such rows are left to the edge waves.  Called AFTER the row loads have been issued: a
// row that turns out to be one was read for nothing (r of T rows), but no row load waits for dst_idx.
struct SlabEdges { bool e0, e1, e2, e3; };
__device__ __forceinline__ SlabEdges slab_edge_rows(int d_first, int j0, int j1, int j2, int j3,
                                                    const int64_t *__restrict__ dstg, int r, int lane) {
    bool e0 = __ballot(d_first == j0) != 0ull, e1 = __ballot(d_first == j1) != 0ull,
         e2 = __ballot(d_first == j2) != 0ull, e3 = __ballot(d_first == j3) != 0ull;
    for (int base = WAVE; base < r; base += WAVE) {
        const int k = base + lane;
        const int d = (k < r) ? (int)dstg[k] : -2;
        e0 = e0 || (__ballot(d == j0) != 0ull);
        e1 = e1 || (__ballot(d == j1) != 0ull);
        e2 = e2 || (__ballot(d == j2) != 0ull);
        e3 = e3 || (__ballot(d == j3) != 0ull);
    }
    return SlabEdges{e0, e1, e2, e3};
}

// ---- wavg of a row nothing merges into, (x * s) / s: x itself when s is 1, and also when s is a power of two and x
// came from a 16-bit format (the fp32 product cannot overflow) -- those rows move as raw bits; the others are rescaled
// in fp32 and rounded once.  RAW: the 16-byte chunk or the Slot, any whole number of TX.
template <typename TX> __device__ __forceinline__ bool wavg_moves_raw(float s) {
    return (s == 1.0f) || (sizeof(TX) == 2 && (__float_as_uint(s) & 0x007FFFFFu) == 0u && s >= 1.0f && s <= 65536.0f);
}
template <typename TX, typename RAW> __device__ __forceinline__ RAW wavg_rescaled(const RAW &raw, float s) {
    Pack<TX, sizeof(RAW) / sizeof(TX)> pk;
    __builtin_memcpy(&pk, &raw, sizeof(RAW));
#pragma unroll
    for (int e = 0; e < (int)(sizeof(RAW) / sizeof(TX)); ++e)
        pk.e[e] = from_f32<TX>(__fdiv_rn(__fmul_rn(to_f32(pk.e[e]), s), s));
    RAW o;
    __builtin_memcpy(&o, &pk, sizeof(RAW));
    return o;
}
// size' (and log size') of the streamed row a lane speaks for, at sout[at] -- unless its edge wave stores them
template <typename TS>
__device__ __forceinline__ void slab_store_size(bool mine_has_edges, TS *__restrict__ sout, TS *__restrict__ lsout,
                                                int64_t at, float my_s) {
    if (!mine_has_edges) store_size<TS>(sout + at, lsout ? lsout + at : nullptr, my_s);
}

// ---- backward slab facts (k_merge_rows_bwd, k_merge_ln_rows_bwd[_amp]): the wave owns INPUT-token rows t0 .. t0+R-1.
// the merged row of token t of group g, or -1 when the token has none (drop); clamped into [0, To)
__device__ __forceinline__ int bwd_row_of(int t, int g, int T1, int U, int To, int distill, int drop,
                                          const int *__restrict__ row_map) {
    int o;
    if (t & 1) o = out_row_dst(t >> 1, U, distill);
    else {
        o = row_map[(int64_t)g * T1 + (t >> 1)];
        o = o < 0 ? 0 : (o >= To ? To - 1 : o);
        if (drop) {
            bool is_dst;
            int idx;
            decode_out_row(o, U, distill, is_dst, idx);
            if (is_dst) return -1;
        }
    }
    return o < 0 ? 0 : (o >= To ? To - 1 : o);
}
// bwd_row_of and whether token t is the one that owns row o(t) in the parameter sums
__device__ __forceinline__ int bwd_row_owner(int t, int g, int T1, int U, int To, int distill, int drop,
                                             const int *__restrict__ row_map, bool &owns) {
    const int o = bwd_row_of(t, g, T1, U, To, distill, drop, row_map);
    owns = o >= 0;
    if (o >= 0 && !(t & 1)) {
        bool is_dst;
        int idx;
        decode_out_row(o, U, distill, is_dst, idx);
        owns = !is_dst;  // an even token in a destination row was merged into it: the odd token counts the row
    }
    return o;
}
// Lane L < R: the merged row of token t0 + L (o: -2 no such token, -1 a token without a row, whose gradient is zero;
// os0: row 0's, clamped to a real row -- where a lane without a chunk reads) and the two scales, read unconditionally
// (no branch between the index load and the row loads; 1 when a scale is absent) and broadcast by the caller after its
// row loads.  OWNER: my_owns says the lane's token exists and owns its row in the parameter sums.
struct BwdSlab { int o0, o1, o2, o3, os0; float my_d, my_m; bool my_owns; };
template <bool OWNER, typename TS>
__device__ __forceinline__ BwdSlab bwd_slab(const TS *__restrict__ out_div, const TS *__restrict__ in_mul,
                                            const int *__restrict__ row_map, int g, int t0, int R, int T_, int T1, int U,
                                            int To, int distill, int drop, int lane) {
    const bool my_valid = lane < R && (t0 + lane) < T_;
    const int my_t = my_valid ? t0 + lane : t0;
    bool my_owns = false;
    const int my_o = OWNER ? bwd_row_owner(my_t, g, T1, U, To, distill, drop, row_map, my_owns)
                           : bwd_row_of(my_t, g, T1, U, To, distill, drop, row_map);
    const int my_os = my_o < 0 ? 0 : my_o;
    float my_d = 1.0f, my_m = 1.0f;
    if (out_div) my_d = to_f32(out_div[(int64_t)g * To + my_os]);  // (wave-uniform conditions)
    if (in_mul) my_m = to_f32(in_mul[(int64_t)g * T_ + my_t]);
    const int my_row = my_valid ? my_o : -2;
    BwdSlab f;
    lanes4(my_row, f.o0, f.o1, f.o2, f.o3);
    f.os0 = __builtin_amdgcn_readlane(my_os, 0), f.my_d = my_d, f.my_m = my_m, f.my_owns = my_valid && my_owns;
    return f;
}

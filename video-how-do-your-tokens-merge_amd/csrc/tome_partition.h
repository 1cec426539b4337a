// tome_partition.h -- part of the single translation unit csrc/tome_kernels.hip ("partition matching": the two token
// sets are arbitrary ordered position lists and EVERY source row is merged into its best destination).
#pragma once
// ------------------------------------------------------------------------------------------------
// Serves kth_bipartite_soft_matching (merge.py:105-158) and random_bipartite_soft_matching (merge.py:161-212).
// Per group: an ordered source set A (Na positions) and an ordered destination set B (Nb positions);
//   dst_idx[i] = first-index row argmax of the cosine similarity A.B^T           (merge.py:131-135, :192-196)
//   merge      = B rows, each reduced with the A rows that name it               (merge.py:137-142, :198-203)
//   unmerge    = every position gets its own destination row / its source's      (merge.py:144-156, :205-210)
// Launch sequence of one matching (tome_match_partition):
//   k_unit_rows_part   unit vectors of both sets in the fragment-major workspace of tome_match.h
//   k_scores_rowmax    (tome_match.h, unchanged) with T1 = Na, T2 = Nb
//   k_part_fold        folds the column parts, puts the NaN rows back, writes dst_idx (int64)
//   k_part_lists       inverted list: per destination its sources in ascending source-row order
// and of one merge: k_merge_part (one wave per destination row), k_unmerge_part (one wave per set row).
//
// Order of the arithmetic: the destination's own row first, then its sources in ascending source-row order --
// the order in which torch's CPU scatter_reduce(include_self=True) walks the index dimension.
// ------------------------------------------------------------------------------------------------

// Which token position a set row stands for.  k > 0: the kth rule (merge.py:119-126: groups of k consecutive tokens,
// the first k-1 of a group are sources, the last one the destination; positions past (T/k)*k belong to neither set).
// k == 0: explicit position lists a_idx [n,Na] / b_idx [n,Nb] (merge.py:176-183).
struct PartSets {
    int k, Na, Nb;
    const int64_t *a_idx, *b_idx;
};

__device__ __forceinline__ int clamp_tok(int64_t t, int T_) { return t < 0 ? 0 : (t >= T_ ? T_ - 1 : (int)t); }

__device__ __forceinline__ int part_tok_a(const PartSets &S, int g, int i, int T_) {
    if (S.k > 0) {
        const int km = S.k - 1, q = i / km;
        return q * S.k + (i - q * km);
    }
    return clamp_tok(S.a_idx[(int64_t)g * S.Na + i], T_);  // (a position outside the sequence is never dereferenced)
}

__device__ __forceinline__ int part_tok_b(const PartSets &S, int g, int j, int T_) {
    if (S.k > 0) return j * S.k + S.k - 1;
    return clamp_tok(S.b_idx[(int64_t)g * S.Nb + j], T_);
}

// ------------------------------------------------------------------------------------------------
// k_unit_rows_part: k_unit_rows (tome_match.h) for set rows instead of even/odd tokens: work item w of a group is A
// row w (w < Na) or B row w - Na.  Same norm arithmetic (fma chain inside a block of 8 channels, blocks added in
// ascending order), same workspace layout, same NaN flags.
// ------------------------------------------------------------------------------------------------
template <typename T, int NCH>
__global__ __launch_bounds__(256) void k_unit_rows_part(const T *__restrict__ metric, int64_t stride_n,
                                                        int64_t stride_t, int n, int T_, int D, PartSets S,
                                                        float *__restrict__ unitA, float *__restrict__ unitB,
                                                        int64_t groupA_f4, int64_t groupB_f4,
                                                        uint8_t *__restrict__ badA, uint8_t *__restrict__ badB) {
    const int lane = threadIdx.x & 63;
    const int b8 = lane & 7;
    const int per = S.Na + S.Nb;
    const int64_t item = ((int64_t)blockIdx.x * (blockDim.x >> 3)) + (threadIdx.x >> 3);
    const int64_t nitem = (int64_t)n * per;
    const bool live = item < nitem;
    const int64_t it_ = live ? item : nitem - 1;
    const int g = (int)((uint32_t)it_ / (uint32_t)per);  // (the host keeps n * (Na + Nb) below 2^31)
    const int w = (int)((uint32_t)it_ - (uint32_t)g * (uint32_t)per);
    const bool isB = w >= S.Na;
    const int rowi = isB ? w - S.Na : w;
    const int t = isB ? part_tok_b(S, g, rowi, T_) : part_tok_a(S, g, rowi, T_);
    const T *row = metric + (int64_t)g * stride_n + (int64_t)t * stride_t;
    const int nblk = D >> 3;  // D % 8 == 0 on this path

    float v[NCH][8];
    float part[NCH];
#pragma unroll
    for (int it = 0; it < NCH; ++it) {
        const int b = b8 + 8 * it;
        part[it] = 0.0f;
        if (b < nblk) {
            Load8<T>::run(row + 8 * b, v[it]);
#pragma unroll
            for (int e = 0; e < 8; ++e) part[it] = __fmaf_rn(v[it][e], v[it][e], part[it]);
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) v[it][e] = 0.0f;
        }
    }
    float ss = 0.0f;
    const int base = lane & ~7;
#pragma unroll
    for (int it = 0; it < NCH; ++it) {
#pragma unroll
        for (int l = 0; l < 8; ++l) {
            const float p = __shfl(part[it], base + l);
            if (l + 8 * it < nblk) ss = __fadd_rn(ss, p);
        }
    }
    const float nr = __builtin_sqrtf(ss);
    f32x4 *dst = reinterpret_cast<f32x4 *>(isB ? unitB : unitA) + (int64_t)g * (isB ? groupB_f4 : groupA_f4);
    const int tile = rowi >> 5, slot = rowi & 31;
    bool nan_here = false;
#pragma unroll
    for (int it = 0; it < NCH; ++it) {
        const int b = b8 + 8 * it;
        f32x4 ev, od;
        if (b < nblk) {
            ev.x = __fdiv_rn(v[it][0], nr); od.x = __fdiv_rn(v[it][1], nr);
            ev.y = __fdiv_rn(v[it][2], nr); od.y = __fdiv_rn(v[it][3], nr);
            ev.z = __fdiv_rn(v[it][4], nr); od.z = __fdiv_rn(v[it][5], nr);
            ev.w = __fdiv_rn(v[it][6], nr); od.w = __fdiv_rn(v[it][7], nr);
            nan_here = nan_here || (ev.x != ev.x) || (ev.y != ev.y) || (ev.z != ev.z) || (ev.w != ev.w) ||
                       (od.x != od.x) || (od.y != od.y) || (od.z != od.z) || (od.w != od.w);
        } else {
            ev.x = ev.y = ev.z = ev.w = 0.0f;
            od = ev;
        }
        if (live) {
            const int64_t f = frag_index(tile, NCH, it, b8, slot);
            dst[f] = ev;
            dst[f + 32] = od;
        }
    }
    const unsigned long long nan_mask = __ballot(nan_here);
    if (live && b8 == 0) {
        const uint8_t flag = ((nan_mask >> (lane & ~7)) & 0xFFull) ? 1 : 0;
        if (isB) badB[(int64_t)g * S.Nb + rowi] = flag;
        else badA[(int64_t)g * S.Na + rowi] = flag;
    }
}

// Any D / alignment: one thread per set row, scalar accesses, same arithmetic order (k_unit_rows_generic).
template <typename T>
__global__ __launch_bounds__(256) void k_unit_rows_part_generic(const T *__restrict__ metric, int64_t stride_n,
                                                                int64_t stride_t, int n, int T_, int D, int Dp,
                                                                PartSets S, float *__restrict__ unitA,
                                                                float *__restrict__ unitB, int64_t groupA_f4,
                                                                int64_t groupB_f4, uint8_t *__restrict__ badA,
                                                                uint8_t *__restrict__ badB) {
    const int per = S.Na + S.Nb;
    const int64_t item = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (item >= (int64_t)n * per) return;
    const int g = (int)(item / per);
    const int w = (int)(item - (int64_t)g * per);
    const bool isB = w >= S.Na;
    const int rowi = isB ? w - S.Na : w;
    const int t = isB ? part_tok_b(S, g, rowi, T_) : part_tok_a(S, g, rowi, T_);
    const T *row = metric + (int64_t)g * stride_n + (int64_t)t * stride_t;
    float ss = 0.0f;
    for (int k0 = 0; k0 < D; k0 += 8) {
        float part = 0.0f;
        for (int k = k0; k < D && k < k0 + 8; ++k) {
            const float v = to_f32(row[k]);
            part = __fmaf_rn(v, v, part);
        }
        ss = __fadd_rn(ss, part);
    }
    const float nr = __builtin_sqrtf(ss);
    const int tile = rowi >> 5, slot = rowi & 31, nchunk = Dp >> 6;
    float *dst = (isB ? unitB : unitA) + 4 * (int64_t)g * (isB ? groupB_f4 : groupA_f4);
    bool nan_here = false;
    for (int k = 0; k < Dp; ++k) {
        const float u = (k < D) ? __fdiv_rn(to_f32(row[k]), nr) : 0.0f;
        nan_here = nan_here || (u != u);
        const int s = k >> 1, h = k & 1;
        const int64_t f = frag_index(tile, nchunk, s >> 5, (s & 31) >> 2, slot + 32 * h);
        dst[4 * f + (s & 3)] = u;
    }
    if (isB) badB[(int64_t)g * S.Nb + rowi] = nan_here ? 1 : 0;
    else badA[(int64_t)g * S.Na + rowi] = nan_here ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------
// k_part_fold: the WJ partial (max, index) pairs k_scores_rowmax left per source row -> dst_idx.  Larger value wins,
// equal values keep the smaller index.  NaN rule of torch.max (merge.py:134, :195), as in k_rowmax_given: a NaN
// score wins and the first NaN column keeps the row; NaN scores come only from rows whose unit vector is NaN (the
// flags of k_unit_rows_part), which the MFMA pass ignored.  grid (ceil(Na / 256), n).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_part_fold(const float *__restrict__ part_max,
                                                   const int *__restrict__ part_idx, int nparts, int Na, int Nb,
                                                   const uint8_t *__restrict__ badA,
                                                   const uint8_t *__restrict__ badB,
                                                   int64_t *__restrict__ dst_idx) {
    __shared__ int s_first_bad;
    const int g = blockIdx.y;
    if (threadIdx.x == 0) s_first_bad = 0x7fffffff;
    __syncthreads();
    {
        int fb = 0x7fffffff;
        for (int j = (int)threadIdx.x; j < Nb; j += blockDim.x)
            if (badB[(int64_t)g * Nb + j]) { fb = j; break; }
        if (fb != 0x7fffffff) atomicMin(&s_first_bad, fb);  // (a minimum: the arrival order does not matter)
    }
    __syncthreads();
    const int first_bad = s_first_bad;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= Na) return;
    const float *pm = part_max + (int64_t)g * nparts * Na;
    const int *pi = part_idx + (int64_t)g * nparts * Na;
    float best = pm[i];
    int bidx = pi[i];
    for (int p = 1; p < nparts; ++p) {
        const float v = pm[(int64_t)p * Na + i];
        const int j = pi[(int64_t)p * Na + i];
        const bool up = (v > best) || (v == best && j < bidx);
        best = up ? v : best;
        bidx = up ? j : bidx;
    }
    if (badA[(int64_t)g * Na + i]) bidx = 0;              // the whole row is NaN: its first column
    else if (first_bad != 0x7fffffff) bidx = first_bad;   // the first NaN column
    if (bidx < 0 || bidx >= Nb) bidx = 0;
    dst_idx[(int64_t)g * Na + i] = bidx;
}

// ------------------------------------------------------------------------------------------------
// k_part_lists: dst_idx [n,Na] -> offsets [n,Nb+1], sources [n,Na] (int32): sources[offsets[j] .. offsets[j+1])
// are the source rows merged into destination j, ascending.  One workgroup per group; a thread owns whole
// destinations: it counts the entries that name its destination, one wave turns the counts into offsets, and the
// thread walks the entries again, in ascending order, writing its own segment.  No atomics: the lists are the same
// bits on every run.  LDS = true keeps the group's dst_idx (as int32) and the counts in LDS; the generic form
// (groups too large for that) reads dst_idx from memory and counts in the offsets buffer itself.
// ------------------------------------------------------------------------------------------------
template <bool LDS>
__global__ __launch_bounds__(1024) void k_part_lists(const int64_t *__restrict__ dst_idx, int Na, int Nb,
                                                     int32_t *__restrict__ offsets, int32_t *__restrict__ sources) {
    extern __shared__ __attribute__((aligned(16))) int part_lds[];
    const int g = blockIdx.x, tid = threadIdx.x, nth = blockDim.x;
    const int64_t *dg = dst_idx + (int64_t)g * Na;
    int32_t *og = offsets + (int64_t)g * (Nb + 1);
    int32_t *sg = sources + (int64_t)g * Na;
    const int NaP = (Na + 3) & ~3;
    int *dl = part_lds;                        // [NaP] (LDS form)
    int *cnt = LDS ? part_lds + NaP : og;      // [Nb + 1]
    if (LDS) {
        for (int i = tid; i < NaP; i += nth) dl[i] = (i < Na) ? (int)dg[i] : -1;
        __syncthreads();
    }
    // 1. counts
    for (int j = tid; j < Nb; j += nth) {
        int c = 0;
        if (LDS) {
            const int4 *d4 = reinterpret_cast<const int4 *>(dl);
            for (int q = 0; q < (NaP >> 2); ++q) {
                const int4 d = d4[q];
                c += (d.x == j) + (d.y == j) + (d.z == j) + (d.w == j);
            }
        } else {
            for (int i = 0; i < Na; ++i) c += ((int)dg[i] == j);
        }
        cnt[j] = c;
    }
    __syncthreads();
    // 2. exclusive scan by the first wave: a lane sums a contiguous segment, the segment sums are scanned across the
    // lanes, the lane walks its segment again
    if (tid < WAVE) {
        const int seg = (Nb + WAVE - 1) / WAVE;
        const int j0 = tid * seg, j1 = (j0 + seg < Nb) ? j0 + seg : Nb;
        int s = 0;
        for (int j = j0; j < j1; ++j) s += cnt[j];
        int incl = s;
#pragma unroll
        for (int off = 1; off < WAVE; off <<= 1) {
            const int o = __shfl_up(incl, off);
            if (tid >= off) incl += o;
        }
        int run = incl - s;
        for (int j = j0; j < j1; ++j) {
            const int c = cnt[j];
            cnt[j] = run;
            run += c;
        }
        if (tid == WAVE - 1) cnt[Nb] = incl;
    }
    __syncthreads();
    // 3. placement, ascending source row inside every destination's segment
    for (int j = tid; j < Nb; j += nth) {
        int p = cnt[j];
        if (LDS) {
            const int4 *d4 = reinterpret_cast<const int4 *>(dl);
            for (int q = 0; q < (NaP >> 2); ++q) {
                const int4 d = d4[q];
                if (d.x == j) sg[p++] = 4 * q;
                if (d.y == j) sg[p++] = 4 * q + 1;
                if (d.z == j) sg[p++] = 4 * q + 2;
                if (d.w == j) sg[p++] = 4 * q + 3;
            }
        } else {
            for (int i = 0; i < Na; ++i)
                if ((int)dg[i] == j) sg[p++] = i;
        }
    }
    if (LDS) {
        for (int j = tid; j <= Nb; j += nth) og[j] = cnt[j];
    }
}

// ------------------------------------------------------------------------------------------------
// k_merge_part: merge.py:137-142 / :198-203 (+ :365-368 when OP_WAVG).  One wave per OUTPUT (= destination) row:
// its own row first, then its list.  fp32 accumulation, reduce_step<OP> of tome_merge.h; TOME_MEAN divides by
// count + 1; OP_WAVG: x*size summed, size summed, one division (the arithmetic of OP_WAVG in k_merge_rows).  A lane
// holds two packs of VEC channels, so a row of up to 128 packs (768 bf16 channels: 96) is one pass over the list.
// Every input row is read once, every output row written once.
// ------------------------------------------------------------------------------------------------
template <typename TX, typename TS, int VEC, int OP>
__global__ __launch_bounds__(256) void k_merge_part(const TX *__restrict__ x, const TS *__restrict__ size, int n,
                                                    int T_, int C, PartSets S,
                                                    const int32_t *__restrict__ offsets,
                                                    const int32_t *__restrict__ sources, TX *__restrict__ xout,
                                                    TS *__restrict__ sout, TS *__restrict__ lsout) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (row >= (int64_t)n * S.Nb) return;
    const int g = (int)(row / S.Nb);
    const int j = (int)(row - (int64_t)g * S.Nb);
    const TX *xg = x + (int64_t)g * T_ * C;
    const TS *sg = size ? size + (int64_t)g * T_ : nullptr;
    const int32_t *og = offsets + (int64_t)g * (S.Nb + 1);
    const int32_t *sl = sources + (int64_t)g * S.Na;
    int p0 = og[j], p1 = og[j + 1];
    p0 = p0 < 0 ? 0 : p0;
    p1 = p1 > S.Na ? S.Na : p1;
    const int tb = part_tok_b(S, g, j, T_);
    const TX *xr = xg + (int64_t)tb * C;
    TX *orow = xout + row * C;
    float s_own = 1.0f;
    if (OP == OP_WAVG) s_own = sg ? to_f32(sg[tb]) : 1.0f;
    float ssum = s_own;
    bool first_pass = true;
    for (int c0 = 0; c0 < C; c0 += 2 * WAVE * VEC) {
        const int ca = c0 + lane * VEC, cb = ca + WAVE * VEC;
        const bool a0 = ca < C, a1 = cb < C;
        float acc0[VEC], acc1[VEC];
        if (a0) load_pack<TX, VEC>(xr + ca, acc0);
        if (a1) load_pack<TX, VEC>(xr + cb, acc1);
        if (OP == OP_WAVG) {
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                if (a0) acc0[e] = __fmul_rn(acc0[e], s_own);
                if (a1) acc1[e] = __fmul_rn(acc1[e], s_own);
            }
        }
        for (int p = p0; p < p1; ++p) {
            int i = sl[p];
            i = (i < 0 || i >= S.Na) ? 0 : i;
            const int ts = part_tok_a(S, g, i, T_);
            const TX *xs = xg + (int64_t)ts * C;
            float s2 = 1.0f;
            if (OP == OP_WAVG) s2 = sg ? to_f32(sg[ts]) : 1.0f;
            float v0[VEC], v1[VEC];
            if (a0) load_pack<TX, VEC>(xs + ca, v0);
            if (a1) load_pack<TX, VEC>(xs + cb, v1);
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                if (a0) acc0[e] = reduce_step<OP>(acc0[e], (OP == OP_WAVG) ? __fmul_rn(v0[e], s2) : v0[e]);
                if (a1) acc1[e] = reduce_step<OP>(acc1[e], (OP == OP_WAVG) ? __fmul_rn(v1[e], s2) : v1[e]);
            }
            if (OP == OP_WAVG && first_pass) ssum = __fadd_rn(ssum, s2);
        }
        first_pass = false;
        if (OP == OP_WAVG) {
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                if (a0) acc0[e] = __fdiv_rn(acc0[e], ssum);
                if (a1) acc1[e] = __fdiv_rn(acc1[e], ssum);
            }
        } else if (OP == TOME_MEAN && p1 > p0) {
            const float fc = (float)(p1 - p0 + 1);
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                if (a0) acc0[e] = __fdiv_rn(acc0[e], fc);
                if (a1) acc1[e] = __fdiv_rn(acc1[e], fc);
            }
        }
        if (a0) store_pack<TX, VEC>(orow + ca, acc0);
        if (a1) store_pack<TX, VEC>(orow + cb, acc1);
    }
    if (OP == OP_WAVG && lane == 0) store_size<TS>(sout + row, lsout ? lsout + row : nullptr, ssum);
}

// ------------------------------------------------------------------------------------------------
// k_unmerge_part: merge.py:144-156 / :205-210.  One wave per set row: B row j copies merged row j to its own
// position, A row i copies merged row dst_idx[i] to its position.  The two sets are disjoint, so every output row
// is written exactly once and nothing is zero-filled (kth: out has (T/k)*k rows, random: T).
// ------------------------------------------------------------------------------------------------
template <typename TX, int VEC>
__global__ __launch_bounds__(256) void k_unmerge_part(const TX *__restrict__ x, int n, int T_, int Tout, int C,
                                                      PartSets S, const int64_t *__restrict__ dst_idx,
                                                      TX *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int per = S.Na + S.Nb;
    const int64_t item = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (item >= (int64_t)n * per) return;
    const int g = (int)(item / per);
    const int w = (int)(item - (int64_t)g * per);
    int t, j;
    if (w < S.Na) {
        t = part_tok_a(S, g, w, T_);
        const int64_t d = dst_idx[(int64_t)g * S.Na + w];
        j = (d < 0 || d >= S.Nb) ? 0 : (int)d;
    } else {
        j = w - S.Na;
        t = part_tok_b(S, g, j, T_);
    }
    if (t >= Tout) return;
    const TX *xr = x + ((int64_t)g * S.Nb + j) * C;
    TX *orow = out + ((int64_t)g * Tout + t) * C;
    for (int c = lane * VEC; c < C; c += WAVE * VEC) {
        float v[VEC];
        load_pack<TX, VEC>(xr + c, v);
        store_pack<TX, VEC>(orow + c, v);
    }
}

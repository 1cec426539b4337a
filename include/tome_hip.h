/*
 * tome_hip.h -- C ABI of the MI355X (gfx950) ToMe merge path.
 *
 * This is the drop-in boundary: plain pointers and sizes, no torch types.  Every entry point is
 * asynchronous on the caller's HIP stream, allocates nothing, never synchronises and returns a
 * status (0 = ok).  All pointers are DEVICE pointers owned by the caller.
 *
 * The reference (sjpollard/video-how-do-your-tokens-merge) is pure Python/PyTorch, so its "FFI"
 * for this path is the function interface of tome/merge.py; each entry below names the reference
 * lines it replaces.  INTEGRATION.md shows the ctypes binding a maintainer of the reference would
 * add (it is the binding video-how-do-your-tokens-merge_amd/tome/_abi.py uses).
 *
 * Index conventions (merge.py:52,64-73): tokens with even position are set A ("src
 * candidates", row i = t/2, T1 = ceil(T/2) rows), odd positions are set B ("dst", row j = t/2,
 * T2 = floor(T/2) rows).  src_idx / unm_idx hold A rows, dst_idx holds B rows, all int64 like the
 * reference's closure variables ([n,r,1] / [n,T1-r,1], trailing 1 implicit here).
 */
#ifndef TOME_HIP_H
#define TOME_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void *tome_stream_t; /* hipStream_t */

enum tome_dtype { TOME_F32 = 0, TOME_BF16 = 1, TOME_F16 = 2 };

/* reduce argument of torch.Tensor.scatter_reduce as used by merge(x, mode) -- merge.py:80 */
enum tome_mode { TOME_SUM = 0, TOME_MEAN = 1, TOME_AMAX = 2, TOME_PROD = 3, TOME_AMIN = 4 };

enum tome_status {
    TOME_OK = 0,
    TOME_EINVAL = 1,     /* bad argument (shape, dtype, null pointer, misaligned index buffer) */
    TOME_EWORKSPACE = 2, /* workspace smaller than tome_match_workspace_bytes() */
    TOME_ELAUNCH = 3     /* HIP reported a launch error (text in tome_last_error()) */
};

#define TOME_ABI_VERSION 11

int tome_abi_version(void);

/* Thread-local text of the last non-zero status returned on this thread. */
const char *tome_last_error(void);

/* merge.py:36-47 -- r clamped to half of the unprotected tokens; <= 0 means "do nothing". */
int64_t tome_effective_r(int64_t T, int64_t r, int class_token, int distill_token);

/* Bytes of scratch tome_match needs for a [n,T,D] metric. */
size_t tome_match_workspace_bytes(int64_t n, int64_t T, int64_t D);

/*
 * tome_match  <-  bipartite_soft_matching, index part (merge.py:49-73; identical code in
 *                 bipartite_soft_matching_drop :236-251 and _hybrid :296-311).
 *
 * metric: [n,T,D] of `dtype`, element strides (stride_n, stride_t, 1) -- a strided view such as
 *         timesformer.py:83 `k.mean(1)[:, 1:, :]` needs no copy.
 * r:      the caller's r; the call clamps it itself (tome_effective_r) and the index buffers must
 *         be sized for the clamped value: src_idx, dst_idx [n, r_eff], unm_idx [n, T1 - r_eff].
 * node_max: optional [n,T1] fp32 (row maxima of the similarity matrix, merge.py:64; needed by
 *         the hybrid threshold test merge.py:326).
 * row_map:  optional [n,T1] int32: for every A row the row of the MERGED sequence it ends up in
 *         (its own slot when unmerged, its destination's slot when merged).
 * Arithmetic: metric is converted to fp32; unit vectors, the A.B^T similarity (fp32 MFMA, k-ordered
 *         fma chain), first-index row argmax and a stable descending ranking -- the contract is
 *         written out in oracle/tome_oracle.c and DESIGN.md.
 * Returns TOME_OK also when r_eff <= 0 (nothing is written).
 */
int tome_match(const void *metric, int dtype, int64_t n, int64_t T, int64_t D, int64_t stride_n,
               int64_t stride_t, int64_t r, int class_token, int distill_token, int64_t *src_idx,
               int64_t *dst_idx, int64_t *unm_idx, float *node_max, int32_t *row_map,
               void *workspace, size_t workspace_bytes, tome_stream_t stream);

/*
 * tome_match_keys  <-  the metric producer fused in front of tome_match:
 *     metric = k.mean(1)   (tome/patch/videomae.py:72-73, timesformer.py:83, motionformer.py:143-144,
 *     vivit.py:123-124), then bipartite_soft_matching(metric, ...) (merge.py:49-73).
 *
 * keys: per-head attention keys [n,H,T,D] of `dtype`, element strides (stride_n, stride_h, stride_t, 1) --
 *       e.g. the k slice of the qkv projection buffer, no copy; every stride and the base must be 16-byte
 *       aligned; D must be 64.  The head mean is taken as torch does on CPU: fp32 sum in head order, one
 *       division by H, one rounding to `dtype`; everything after is tome_match.
 * inner, stride_inner: groups interleaved inside a clip (Motionformer's '(b h) (s f) d -> (b f) h s d',
 *       motionformer.py:143-144): group g = o * inner + f starts at o * stride_n + f * stride_inner, its tokens are
 *       stride_t apart (inner token rows).  inner = 1 (stride_inner ignored): n independent [H,T,D] blocks.
 */
int tome_match_keys(const void *keys, int dtype, int64_t n, int64_t H, int64_t T, int64_t D, int64_t stride_n,
                    int64_t inner, int64_t stride_inner, int64_t stride_h, int64_t stride_t, int64_t r,
                    int class_token, int distill_token,
                    int64_t *src_idx, int64_t *dst_idx, int64_t *unm_idx, float *node_max, int32_t *row_map,
                    void *workspace, size_t workspace_bytes, tome_stream_t stream);

/*
 * tome_match_scores  <-  the same selection from caller-made scores [n,T1,T2] fp32
 *                        (merge.py:54-57 random_merge / :239-242 random_drop, scores = torch.rand).
 */
int tome_match_scores(const float *scores, int64_t n, int64_t T, int64_t r, int class_token,
                      int distill_token, int64_t *src_idx, int64_t *dst_idx, int64_t *unm_idx,
                      float *node_max, int32_t *row_map, void *workspace, size_t workspace_bytes,
                      tome_stream_t stream);

/* merge.py:326 -- edge_keep[n,r] = (node_max[src_idx[k]] >= threshold) as 0/1 bytes. */
int tome_edge_keep(const float *node_max, const int64_t *src_idx, int64_t n, int64_t T, int64_t r,
                   float threshold, uint8_t *edge_keep, tome_stream_t stream);

/*
 * tome_merge_wavg  <-  merge_wavg (merge.py:355-369) fused: x*size, the two "sum" merges, x/size.
 *
 * x [n,T,C] of x_dtype, contiguous.  size: NULL (ones, :362-363) or [n,T] of size_dtype.
 * x_out [n,T-r,C] of x_dtype, size_out [n,T-r] of size_dtype.  r is the clamped r (> 0).
 * edge_keep: NULL, or the hybrid flags (merge.py:326).
 * log_size_out: NULL, or [n,T-r] of size_dtype receiving log(size_out) -- the proportional-attention bias the
 * next block adds to its logits (`size.log()`, tome/patch/videomae.py:62-63, timesformer.py:73-74,
 * motionformer.py:107-111, vivit.py:103-104): fp32 log of the stored size, rounded to size_dtype.  All four
 * tome_merge_wavg* entries take it.
 * Arithmetic in fp32 (products, then sequential adds from the destination's own term in src_idx
 * order, then one division); results rounded once to the output dtype.
 */
int tome_merge_wavg(const void *x, int x_dtype, const void *size, int size_dtype, int64_t n,
                    int64_t T, int64_t C, int64_t r, const int64_t *src_idx,
                    const int64_t *dst_idx, const int64_t *unm_idx, int distill_token,
                    const uint8_t *edge_keep, void *x_out, void *size_out, void *log_size_out,
                    tome_stream_t stream);

/*
 * tome_merge_wavg_ln  <-  merge_wavg followed by the block's second LayerNorm:
 *     x = merge_wavg(merge, x, size); ... self.norm2(x)      (tome/patch/videomae.py:25-27, vivit.py:38-41)
 * x_out as tome_merge_wavg; y_out [n,T-r,C] = LayerNorm(x_out) over the channels (weight, bias [C] of the token
 * dtype, eps), computed in fp32 from the stored x_out and rounded once -- so the MLP reads y_out and the
 * separate LayerNorm pass over the merged tokens disappears.  16-bit tokens, C <= 1024, C % 8 == 0.
 * addend: NULL, or [n,T,C] like x: the tokens that are merged are round_to_dtype(x + addend), i.e. the residual
 * `x = x + attn(norm1(x))` in front of the merge (videomae.py:20, vivit.py:35) is taken while loading and the
 * separate add pass disappears as well.
 * x_out_bias: NULL, or [C] of the token dtype: x_out is stored as round(x' + x_out_bias) while y_out stays
 * LayerNorm(x').  x' is the ROUNDED row, the x_out the same call stores without x_out_bias (the bias is added to the
 * 16-bit value, and the LayerNorm reads that 16-bit value: both roundings are visible in x_out).  For callers that let the MLP's second GEMM accumulate onto x_out in place
 * (`x = x + self.mlp(self.norm2(x))`, videomae.py:29, as `x_out.addmm_(h, W2^T)`): that GEMM's bias is in the buffer
 * beforehand, and the block's second residual add is no pass of its own.
 */
int tome_merge_wavg_ln(const void *x, int x_dtype, const void *size, int size_dtype, int64_t n, int64_t T,
                       int64_t C, int64_t r, const int64_t *src_idx, const int64_t *dst_idx,
                       const int64_t *unm_idx, int distill_token, const uint8_t *edge_keep,
                       const void *ln_weight, const void *ln_bias, float eps, const void *addend, void *x_out,
                       void *y_out, void *size_out, void *log_size_out, const void *x_out_bias,
                       tome_stream_t stream);

/*
 * tome_merge_wavg_regrouped  <-  the rearrange / merge_wavg / rearrange / cat sequence of
 *     timesformer_merge (tome/patch/timesformer.py:89-107) and motionformer_merge
 *     (tome/patch/motionformer.py:150-168), without the two permuted copies of x.
 *
 * x [B, has_cls + P*F, C]: token `has_cls + p*F + f` of clip b belongs to merge group b*F + f (n = B*F groups
 * of P tokens, the layout both patches regroup into); the index buffers and size [n,P] / size_out [n,P-r]
 * are those of the n groups.  x_out [B, has_cls + (P-r)*F, C] in the same interleaved layout, class token
 * rows copied through.  Arithmetic as tome_merge_wavg.  C * sizeof(dtype) must be a multiple of 16.
 */
int tome_merge_wavg_regrouped(const void *x, int x_dtype, const void *size, int size_dtype, int64_t B,
                              int64_t F, int64_t P, int64_t C, int64_t r, int has_cls,
                              const int64_t *src_idx, const int64_t *dst_idx, const int64_t *unm_idx,
                              const uint8_t *edge_keep, void *x_out, void *size_out, void *log_size_out,
                              tome_stream_t stream);

/* tome_merge_wavg_regrouped with the residual add in front and the block's norm2 behind it fused in, as
 * tome_merge_wavg_ln does for the plain layout (timesformer.py:52-56, motionformer.py:24-29).  The class-token
 * rows get the same add + LayerNorm.  16-bit tokens, C <= 1024.
 * addend: NULL, or the residual in x's layout [B, has_cls + P*F, C] (addend_grouped = 0), or -- addend_grouped = 1 --
 * in the GROUPED layout [B*F, has_cls + P, C] the spatial attention of TimeSformer leaves it in
 * (tome/patch/timesformer.py:32-52: `res_spatial`, whose '(b t) (h w) m -> b (h w t) m' rearrangement and `cat` with
 * the frame-averaged class token are then not made); its class rows are ignored and the class tokens' addend is
 * cls_addend [B, C] (NULL: none).  x_out_bias: as in tome_merge_wavg_ln (class-token rows included). */
int tome_merge_wavg_regrouped_ln(const void *x, int x_dtype, const void *size, int size_dtype, int64_t B,
                                 int64_t F, int64_t P, int64_t C, int64_t r, int has_cls,
                                 const int64_t *src_idx, const int64_t *dst_idx, const int64_t *unm_idx,
                                 const uint8_t *edge_keep, const void *ln_weight, const void *ln_bias, float eps,
                                 const void *addend, int addend_grouped, const void *cls_addend, void *x_out,
                                 void *y_out, void *size_out, void *log_size_out, const void *x_out_bias,
                                 tome_stream_t stream);

/* tome_drop (below) on the regrouped layout of tome_merge_wavg_regrouped: timesformer_drop / motionformer_drop
 * (tome/patch/timesformer.py:111-131, motionformer.py:172-193) without the permuted copies.
 * x [B, has_cls + P*F, C] -> x_out [B, has_cls + (P-r)*F, C]; und_idx [B*F, ceil(P/2)-r].
 * C * sizeof(dtype) must be a multiple of 16. */
int tome_drop_regrouped(const void *x, int dtype, int64_t B, int64_t F, int64_t P, int64_t C, int64_t r,
                        int has_cls, const int64_t *und_idx, void *x_out, tome_stream_t stream);

/*
 * tome_drop_ln  <-  the drop step of a patched block between its first residual and its second LayerNorm:
 *     x = x + attn; x = drop(x); ... self.norm2(x)      (videomae_drop, tome/patch/videomae.py:103-127, with the
 *     block around it, videomae.py:20-27; vivit_drop likewise)
 * one launch instead of an add pass, tome_drop and a LayerNorm pass.  Added to ABI v11 after its first release.
 * x [n,T,C], 16-bit, C % 8 == 0, C <= 1024; und_idx, distill_token and r as tome_drop.
 * addend: NULL, or [n,T,C] like x: the rows that are kept are round_to_dtype(x + addend).
 * x_out [n,T-r,C]: the rows tome_drop keeps of that sum, bit for bit.  y_out [n,T-r,C] = LayerNorm(x_out) (weight,
 * bias [C] of the token dtype, eps) in fp32 from the stored row, rounded once: the arithmetic of tome_add_layernorm.
 * x_out_bias: NULL, or [C]: as in tome_merge_wavg_ln -- stored into x_out, y_out is the norm of the row without it.
 * Every buffer 16-byte aligned.  Each refusal is made on the host, before any launch, with its own tome_last_error.
 */
int tome_drop_ln(const void *x, int dtype, int64_t n, int64_t T, int64_t C, int64_t r, const int64_t *und_idx,
                 int distill_token, const void *ln_weight, const void *ln_bias, float eps, const void *addend,
                 void *x_out, void *y_out, const void *x_out_bias, tome_stream_t stream);

/* tome_drop_ln on the interleaved layout of tome_drop_regrouped: timesformer_drop / motionformer_drop
 * (tome/patch/timesformer.py:111-131, motionformer.py:172-193) with the residual in front and norm2 behind them
 * (timesformer.py:52-56, motionformer.py:24-29) in one launch.  The class-token rows get the same add + LayerNorm.
 * addend / addend_grouped / cls_addend and x_out_bias: as in tome_merge_wavg_regrouped_ln.  Added to ABI v11 after its
 * first release. */
int tome_drop_regrouped_ln(const void *x, int dtype, int64_t B, int64_t F, int64_t P, int64_t C, int64_t r,
                           int has_cls, const int64_t *und_idx, const void *ln_weight, const void *ln_bias, float eps,
                           const void *addend, int addend_grouped, const void *cls_addend, void *x_out, void *y_out,
                           const void *x_out_bias, tome_stream_t stream);

/*
 * tome_prop_attention  <-  the proportional attention of the patched attention modules:
 *     attn = softmax(q k^T * scale + size.log()[:, None, None, :, 0]) ; x = attn @ v
 *     (ToMeAttention.forward, tome/patch/videomae.py:55-66; vivit.py:95-113; timesformer.py:66-78 with the bias
 *      on the non-class block only: bias_skip = 1)
 * q: [B, H, N, 64], k, v: [B, H, Nk, 64] views of 16-bit tensors, element strides {batch, head, token} each (channels
 * contiguous, rows 16-byte aligned) -- e.g. the three slices of a [B, N, 3, H, 64] qkv buffer, read in place.  Nk may
 * differ from N (Motionformer's trajectory attention attends from every token to the keys of one frame at a time,
 * tome/patch/motionformer.py:98-121).
 * log_size: NULL (plain attention) or fp32 [B, Nk - bias_skip] with row stride log_size_stride: log of the token
 * sizes, added to the logits of key j (bias_skip = 1, N == Nk: key 0 and query 0 carry no bias, entry j-1 belongs
 * to key j).
 * out: NULL strides -> [B, N, H*64] contiguous, the layout the output projection reads; else element strides
 * {batch, head, token} of out[b, q, h, 0..63] (rows 8-byte aligned).  fp32 softmax and accumulation.
 */
int tome_prop_attention(const void *q, const void *k, const void *v, int dtype, int64_t B, int64_t H, int64_t N,
                        int64_t Nk, int64_t D, const int64_t *q_strides, const int64_t *k_strides,
                        const int64_t *v_strides, const float *log_size, int64_t log_size_stride, int bias_skip,
                        float scale, void *out, const int64_t *out_strides, tome_stream_t stream);

/* tome_prop_attention_segments  <-  the per-frame stage of ToMeTrajectoryAttention.forward
 * (tome/patch/motionformer.py:98-121): every query attends to the keys of ONE frame at a time -- `nseg` independent
 * key ranges of Nk keys each with their own softmax -- in ONE launch.  Segment s reads k + s*seg_strides[0],
 * v + s*seg_strides[1], log_size + s*seg_strides[3] and writes out + s*seg_strides[2] (element offsets); the
 * other arguments are tome_prop_attention's (no bias_skip form).  The [B*H, N, nseg*Nk] logits never exist. */
int tome_prop_attention_segments(const void *q, const void *k, const void *v, int dtype, int64_t B, int64_t H,
                                 int64_t N, int64_t Nk, int64_t D, const int64_t *q_strides,
                                 const int64_t *k_strides, const int64_t *v_strides, const float *log_size,
                                 int64_t log_size_stride, float scale, void *out, const int64_t *out_strides,
                                 int64_t nseg, const int64_t *seg_strides, tome_stream_t stream);

/*
 * tome_trajectory_mix  <-  the temporal stage of ToMeTrajectoryAttention.forward (tome/patch/motionformer.py:122-139):
 *     attn = softmax(einsum('b h s d, b h s f d -> b h s f', q2 * scale, k2)); x = einsum('b h s f, b h s f d -> b h s d', attn, v2)
 * q2 [B, S, H*64]; k2, val [B, S, F, H*64] views whose (b, s, f) rows are k_row_stride / v_row_stride elements apart
 * (k2 = first half of the proj_kv output, val = the trajectory tokens or its second half); out [B, S, H*64] rows,
 * batch b starting out_batch_stride elements after batch b-1 (0 = S*H*64, contiguous; larger: `out` is a slice of
 * the [B, 1+S, C] buffer that also takes the class token's row, so that `torch.cat((cls_out, x), dim=1)` of
 * motionformer.py:138 needs no copy); tattn NULL or fp32 [B, H, S, F].  16-bit tensors, head dim 64, H <= 16,
 * F <= 8; fp32 arithmetic inside.
 */
int tome_trajectory_mix(const void *q2, const void *k2, const void *val, int dtype, int64_t B, int64_t S, int64_t F,
                        int64_t H, int64_t D, int64_t k_row_stride, int64_t v_row_stride, float scale, void *out,
                        int64_t out_batch_stride, float *tattn, tome_stream_t stream);

/*
 * tome_short_attention  <-  `self.temporal_attn(...)` in ToMeBlock.forward of the TimeSformer patch
 * (tome/patch/timesformer.py:25-27): the host model's attention over the T <= 8 copies of one spatial token,
 *     softmax(q k^T * scale) v        per (sequence, head), sequences = 'b (p t) m -> (b p) t m'
 * q, k, v: [B, H, N, 64] views ({batch, head, token} element strides; the heads of a token side by side: head
 * stride 64 -- the slices of a qkv projection read in place); out [B, N, H*64] contiguous.  16-bit tensors,
 * N <= 8, fp32 arithmetic inside.  No bias term: the temporal attention never sees token sizes.
 */
int tome_short_attention(const void *q, const void *k, const void *v, int dtype, int64_t B, int64_t H, int64_t N,
                         int64_t D, const int64_t *q_strides, const int64_t *k_strides, const int64_t *v_strides,
                         float scale, void *out, tome_stream_t stream);

/*
 * tome_add_layernorm  <-  the second residual of the patched block and the LayerNorm that consumes it:
 *     x = x + self.drop_path(self.mlp(self.norm2(x)))      (tome/patch/videomae.py:29)
 *     ... next ToMeBlock.forward: self.norm1(x)            (tome/patch/videomae.py:19)
 * x_out = round(x + addend), y_out = LayerNorm(x_out), both [rows, C] of `dtype` (16-bit, C <= 1024, C % 8 == 0).
 * addend NULL: y_out = LayerNorm(x) only -- x already holds the sum (the MLP's GEMM accumulated onto it, see
 * x_out_bias of tome_merge_wavg_ln); x_out is then ignored and may be NULL.
 */
int tome_add_layernorm(const void *x, const void *addend, int dtype, int64_t rows, int64_t C,
                       const void *ln_weight, const void *ln_bias, float eps, void *x_out, void *y_out,
                       tome_stream_t stream);

/* tome_add_layernorm for rows that come in `groups` groups of `group_rows` whose first row is a class token the
 * consumer of y does not read: x_out [groups*group_rows, C] as before, y_out [groups*(group_rows-1), C] holds the
 * LayerNorm of the other rows, compacted.  TimeSformer: `self.temporal_norm1(xt)` with `xt = x[:, 1:, :]`
 * (tome/patch/timesformer.py:24-26) -- the regrouping '(b p) t m' of y is then a view. */
int tome_add_layernorm_skip_first(const void *x, const void *addend, int dtype, int64_t groups, int64_t group_rows,
                                  int64_t C, const void *ln_weight, const void *ln_bias, float eps, void *x_out,
                                  void *y_out, tome_stream_t stream);

/*
 * tome_add_layernorm_regrouped  <-  the middle of TimeSformer's divided space-time ToMeBlock.forward
 * (tome/patch/timesformer.py:24-38): the temporal attention's residual, the regrouping of the tokens for the
 * spatial attention (class token replicated into every frame) and that attention's LayerNorm:
 *     xt = x[:, 1:, :] + res_temporal;  x1 = cat(cls, xt)
 *     xs = cat(cls repeated per frame, rearrange(xt, 'b (p t) m -> (b t) p m'));  y = self.norm1(xs)
 * x [B, 1 + P*F, C], addend [B, P*F, C] -> x_out = x1 [B, 1 + P*F, C] and y_out = norm1(xs) [B*F, 1 + P, C]
 * (16-bit, C <= 1024, C % 8 == 0): one pass, the regrouped un-normalised copy `xs` is never written.
 */
int tome_add_layernorm_regrouped(const void *x, const void *addend, int dtype, int64_t B, int64_t F, int64_t P,
                                 int64_t C, const void *ln_weight, const void *ln_bias, float eps, void *x_out,
                                 void *y_out, tome_stream_t stream);

/* tome_merge  <-  merge(x, mode) closure (merge.py:75-85; hybrid :313-334 when edge_keep). */
int tome_merge(const void *x, int dtype, int64_t n, int64_t T, int64_t C, int64_t r,
               const int64_t *src_idx, const int64_t *dst_idx, const int64_t *unm_idx,
               int distill_token, int mode, const uint8_t *edge_keep, void *out,
               tome_stream_t stream);

/* tome_drop  <-  drop(x) closure (merge.py:253-262): unmerged A rows then all B rows. */
int tome_drop(const void *x, int dtype, int64_t n, int64_t T, int64_t C, int64_t r,
              const int64_t *und_idx, int distill_token, void *out, tome_stream_t stream);

/* tome_unmerge  <-  unmerge(x) closure (merge.py:87-100): x [n,T-r,C] -> out [n,T,C]. */
int tome_unmerge(const void *x, int dtype, int64_t n, int64_t T, int64_t C, int64_t r,
                 const int64_t *src_idx, const int64_t *dst_idx, const int64_t *unm_idx, void *out,
                 tome_stream_t stream);

/*
 * tome_merge_backward  <-  what autograd derives from the merge closure and merge_wavg in the reference (only the
 *     matching is under no_grad, merge.py:49; models are patched for training, tools/train_net.py:727-741): the
 *     gradient with respect to the tokens of
 *         merge(x, "sum")                 merge.py:75-85        out_div = in_mul = NULL
 *         merge(x, "mean")                merge.py:75-85        out_div = 1 + number of sources of each merged row
 *         merge_wavg(merge, x, size)      merge.py:355-369      out_div = the returned size, in_mul = size (or NULL)
 *         drop(x)                         merge.py:253-262      drop != 0: merged-away tokens get a zero gradient
 *     as one gather:  grad_in[t, :] = (grad_out[row of t, :] / out_div[row of t]) * in_mul[t], fp32 arithmetic (division,
 *     then product: the order of the reference's chain x*size -> sum -> /size walked back), one rounding, no atomics,
 *     every row written once, same bits on every run.
 *     grad_out [n,T-r,C], grad_in [n,T,C] of x_dtype; out_div [n,T-r], in_mul [n,T] of size_dtype (= x_dtype or
 *     TOME_F32; ignored when both are NULL); row_map [n,ceil(T/2)] as tome_row_map / tome_match write it.
 *     The backward of unmerge (merge.py:87-100) is tome_merge in mode TOME_SUM, its adjoint.
 * tome_merge_backward_regrouped: the same on the layout of tome_merge_wavg_regrouped / tome_drop_regrouped
 *     (timesformer.py:89-107, :111-131; motionformer.py:150-168, :172-193): grad_out [B, has_cls + (P-r)*F, C] ->
 *     grad_in [B, has_cls + P*F, C], class rows copied through; out_div [B*F,P-r], in_mul [B*F,P], row_map
 *     [B*F,ceil(P/2)].  C * sizeof(dtype) must be a multiple of 16.
 */
int tome_merge_backward(const void *grad_out, int x_dtype, const void *out_div, const void *in_mul, int size_dtype,
                        int64_t n, int64_t T, int64_t C, int64_t r, const int32_t *row_map, int distill_token,
                        int drop, void *grad_in, tome_stream_t stream);
int tome_merge_backward_regrouped(const void *grad_out, int x_dtype, const void *out_div, const void *in_mul,
                                  int size_dtype, int64_t B, int64_t F, int64_t P, int64_t C, int64_t r, int has_cls,
                                  const int32_t *row_map, int drop, void *grad_in, tome_stream_t stream);

/*
 * tome_layernorm_backward  <-  what autograd derives from the LayerNorms of the patched block when the tokens require
 *     grad (additions to ABI v11, no entry changed; models are patched for training, tools/train_net.py:727-741):
 *         self.norm1(x) / self.norm2(x)                        tome/patch/videomae.py:19,29
 *         x = x + mlp(...); next block: self.norm1(x)          tome/patch/videomae.py:29,19
 *         self.temporal_norm1(x)[:, 1:]                        tome/patch/timesformer.py:24-26   (skip_first)
 *     i.e. the backward of tome_add_layernorm / tome_add_layernorm_skip_first.  With xs the STORED 16-bit rows the
 *     forward normalised (its x_out, or its x when there was no addend), gw = gy * weight, xhat = (xs - mean) * rstd:
 *         gx = gx_in + rstd * (gw - mean(gw) - xhat * mean(gw * xhat))              one rounding to `dtype`
 *         dweight[c] = sum over rows of gy * xhat,   dbias[c] = sum over rows of gy  one rounding to `dtype`
 *     mean and rstd are recomputed from xs with the forward's arithmetic: nothing is saved by the forward.  fp32
 *     arithmetic, no atomics, every row written once, same bits on every run.
 *     rows = groups * group_rows.  gy [rows, C], or with skip_first != 0 [groups * (group_rows - 1), C]: every group's
 *     first row (a class token) has no row in gy, gets gx = gx_in (0 without gx_in) and adds nothing to dweight / dbias.
 *     xs, gx [rows, C]; gx_in [rows, C] or NULL: the gradient that reaches xs through the residual stream.
 *     weight, dweight, dbias [C] of `dtype` (16-bit, C <= 1024, C % 8 == 0); dweight / dbias may be NULL one by one; both
 *     NULL (frozen LayerNorm): no parameter work at all and no workspace.  Otherwise workspace holds
 *     tome_layernorm_backward_workspace_bytes(rows, C) bytes (fp32 partial rows [parts, 2, C]; 0 for an illegal shape).
 */
size_t tome_layernorm_backward_workspace_bytes(int64_t rows, int64_t C);
int tome_layernorm_backward(const void *gy, const void *xs, const void *gx_in, int dtype, int64_t groups,
                            int64_t group_rows, int skip_first, int64_t C, const void *weight, float eps, void *gx,
                            void *dweight, void *dbias, void *workspace, tome_stream_t stream);

/*
 * tome_layernorm_backward_regrouped  <-  what autograd derives from the middle of TimeSformer's divided space-time
 *     ToMeBlock.forward (tome/patch/timesformer.py:24-38) when the tokens require grad (additions to ABI v11, no entry
 *     changed; models are patched for training, tools/train_net.py:727-741): the backward of
 *     tome_add_layernorm_regrouped.  xs is that entry's x_out [B, 1 + P*F, C], the stored rows it normalised; gx_in (or
 *     NULL) and gx have the same layout; gy [B*F, 1 + P, C] is the gradient of the regrouped, normalised tensor.
 *         token row 1 + p*F + t of clip b reads row (b*F + t)(1 + P) + 1 + p of gy;
 *         a clip's class row, which the forward stored F times, takes the fp32 sum of rows (b*F + t)(1 + P) of gy in
 *         frame order t = 0 .. F-1, not rounded (what `expand`'s backward computes, with F - 1 fewer roundings), and
 *         enters gx, dweight and dbias once;
 *     then tome_layernorm_backward's formula, statistics recomputed from xs, one rounding.  The gradient of the addend
 *     is the view gx[:, 1:], that of x is gx: no pass of its own.  Parameter gradients, workspace
 *     (tome_layernorm_backward_regrouped_workspace_bytes(B, F, P, C); 0 for an illegal shape), frozen LayerNorm, limits
 *     on C and alignment as in tome_layernorm_backward; at most 2^31 - 1 rows on either side.
 */
size_t tome_layernorm_backward_regrouped_workspace_bytes(int64_t B, int64_t F, int64_t P, int64_t C);
int tome_layernorm_backward_regrouped(const void *gy, const void *xs, const void *gx_in, int dtype, int64_t B, int64_t F,
                                      int64_t P, int64_t C, const void *weight, float eps, void *gx, void *dweight,
                                      void *dbias, void *workspace, tome_stream_t stream);

/*
 * tome_merge_ln_backward  <-  what autograd derives from the middle of the patched flat block when the tokens or the
 *     norm require grad (additions to ABI v11, no entry changed; models are patched for training,
 *     tools/train_net.py:727-741):
 *         x = x + attn; x, size = merge_wavg(merge, x, size); self.norm2(x)    tome/patch/videomae.py:20-29
 *         the same in the ViViT layer                                          tome/patch/vivit.py:35-41
 *     i.e. the backward of tome_merge_wavg_ln and tome_drop_ln (flat layout, no x_out_bias) as ONE launch.  xs is the
 *     forward's stored x_out [n,T-r,C], the rows it normalised; gy the gradient of y_out; gx_out (or NULL) the gradient
 *     that reaches x_out through the residual stream.  With o(t) the merged row of token t (row_map / distill_token as
 *     in tome_merge_backward), gw = gy * weight, xhat = (xs - mean) * rstd:
 *         gm[o] = gx_out[o] + rstd * (gw - mean(gw) - xhat * mean(gw * xhat))       fp32, not rounded
 *         gx[t] = (gm[o(t)] / out_div[o(t)]) * in_mul[t]                            one rounding to x_dtype
 *     -- one rounding fewer than tome_layernorm_backward followed by tome_merge_backward.  gx [n,T,C] is the gradient
 *     of x and of the addend alike.  out_div = size_out [n,T-r], in_mul = size [n,T] or NULL, of size_dtype (= x_dtype
 *     or TOME_F32; ignored when both are NULL).  drop != 0 (tome_drop_ln): no scales, a merged-away token gets 0.
 *     mean and rstd are recomputed from xs with the arithmetic of tome_layernorm_backward.
 *         dweight[c] = sum over the merged rows of gy * xhat,   dbias[c] = sum over the merged rows of gy
 *     every merged row once (a destination's term is computed once per token that landed in it, counted once), fp32
 *     partial rows in `workspace` summed in a fixed order, no atomics, same bits on every run, one rounding to x_dtype.
 *     dweight / dbias may be NULL one by one; both NULL (frozen LayerNorm): no parameter work and no workspace.
 *     Otherwise workspace holds tome_merge_ln_backward_workspace_bytes(n, T, C) bytes (0 for an illegal shape).
 *     16-bit tokens, C <= 1024, C % 8 == 0, 0 < r <= T/2, 16-byte aligned buffers; anything else is refused with a
 *     status and a tome_last_error text before any launch.
 */
size_t tome_merge_ln_backward_workspace_bytes(int64_t n, int64_t T, int64_t C);
int tome_merge_ln_backward(const void *gy, const void *gx_out, const void *xs, int x_dtype, const void *out_div,
                           const void *in_mul, int size_dtype, int64_t n, int64_t T, int64_t C, int64_t r,
                           const int32_t *row_map, int distill_token, int drop, const void *weight, float eps, void *gx,
                           void *dweight, void *dbias, void *workspace, tome_stream_t stream);

/*
 * tome_add_layernorm_amp  <-  tome_add_layernorm / tome_add_layernorm_skip_first for a model that runs under autocast
 *     with fp32 master weights (additions to ABI v11, no entry changed):
 *         with torch.cuda.amp.autocast(enabled=cfg.TRAIN.MIXED_PRECISION):   tools/train_net.py:123
 *         with torch.autocast(device.type, enabled=use_fp16):               tome/utils.py:54
 *     Under autocast the LayerNorm's weight and bias are fp32, its output feeds a 16-bit Linear, and the residual stream
 *     is fp32 (`x + self.pos_embed` promotes it) or 16-bit (`pos_embed.type_as(x)`,
 *     videomae_video_model_builder.py:278).  x' = x + addend (addend NULL: x' = x, x_out neither read nor written and
 *     may be NULL), y = LayerNorm(x'):
 *         x, x_out of x_dtype; y_out of y_dtype (16-bit); weight_f32, bias_f32 [C] fp32.
 *         x_dtype == y_dtype:  addend of the same dtype;  x' = round16(x + addend), the bits tome_add_layernorm stores.
 *         x_dtype == TOME_F32: addend of y_dtype or fp32; x' = the fp32 sum, one rounding (`x + addend.float()`).
 *     The statistics are taken in fp32 from the STORED x' (two passes, centred variance), y is rounded once.
 *     rows = groups * group_rows; skip_first != 0: y_out [groups * (group_rows - 1), C] leaves out every group's first
 *     row (tome_add_layernorm_skip_first).  C % 8 == 0, C <= 1024, 16-byte aligned buffers.  Any other dtype
 *     combination: TOME_EINVAL.
 */
int tome_add_layernorm_amp(const void *x, int x_dtype, const void *addend, int addend_dtype, int64_t groups,
                           int64_t group_rows, int skip_first, int64_t C, const void *weight_f32, const void *bias_f32,
                           float eps, void *x_out, void *y_out, int y_dtype, tome_stream_t stream);

/*
 * tome_merge_wavg_ln_amp  <-  tome_merge_wavg_ln for a model that runs under autocast with fp32 master weights
 *     (additions to ABI v11, no entry changed; tools/train_net.py:123, tome/utils.py:54 as for tome_add_layernorm_amp):
 *         x = x + attn; x, size = merge_wavg(merge, x, size); self.norm2(x)    tome/patch/videomae.py:20-27
 *         the same in the ViViT layer                                          tome/patch/vivit.py:35-41
 *     one launch: x' = x + addend (addend NULL: x' = x), x_out / size_out / log_size_out = tome_merge_wavg(x', size),
 *     y_out = LayerNorm(x_out).  Dtypes as in tome_add_layernorm_amp:
 *         x [n,T,C], x_out [n,T-r,C] of x_dtype; y_out [n,T-r,C] of y_dtype (16-bit); weight_f32, bias_f32 [C] fp32.
 *         x_dtype == y_dtype:  addend of the same dtype; x' = round16(x + addend), the bits tome_merge_wavg_ln merges.
 *         x_dtype == TOME_F32: addend of y_dtype or fp32; x' = the fp32 sum, one rounding (`x + addend.float()`).
 *         size, size_out, log_size_out of size_dtype (x_dtype or TOME_F32) as in tome_merge_wavg; size may be NULL (ones),
 *         log_size_out may be NULL.  Any other dtype combination: TOME_EINVAL.
 *     The merge is tome_merge_wavg's contract, bit for bit: fp32 products, the destination's own term first, then its
 *     sources in src_idx order, one division, one rounding to x_dtype (none for fp32); rows nothing merges into, of
 *     size 1, move as raw bits.  edge_keep and distill_token as in tome_merge_wavg_ln.  The LayerNorm's statistics are
 *     taken in fp32 from the STORED x_out (two passes, centred variance), y_out is rounded once.
 *     Flat layout only, no x_out_bias; the backward of this entry and of tome_drop_ln_amp is
 *     tome_merge_ln_backward_amp below.  C % 8 == 0, C <= 1024, 0 < r <= T/2, 16-byte aligned buffers; each
 *     refusal is made on the host before any launch, with its own tome_last_error.
 */
int tome_merge_wavg_ln_amp(const void *x, int x_dtype, const void *addend, int addend_dtype, const void *size,
                           int size_dtype, int64_t n, int64_t T, int64_t C, int64_t r, const int64_t *src_idx,
                           const int64_t *dst_idx, const int64_t *unm_idx, int distill_token, const uint8_t *edge_keep,
                           const void *weight_f32, const void *bias_f32, float eps, void *x_out, void *y_out, int y_dtype,
                           void *size_out, void *log_size_out, tome_stream_t stream);

/*
 * tome_drop_ln_amp  <-  tome_drop_ln under autocast with fp32 master weights (additions to ABI v11, no entry changed;
 *     tools/train_net.py:123, tome/utils.py:54): the drop step between the first residual and the second LayerNorm of
 *     the block (tome/patch/videomae.py:20-27, vivit.py:35-41 with videomae_drop / vivit_drop as the reduction).
 *     x' = x + addend as in tome_merge_wavg_ln_amp; x_out [n,T-r,C] of x_dtype: the rows tome_drop keeps of x', bit for
 *     bit; y_out [n,T-r,C] of y_dtype = LayerNorm(x_out) with the fp32 weight_f32 / bias_f32, statistics from the stored
 *     row, rounded once.  und_idx, distill_token and r as tome_drop.  Dtypes, limits and refusals as in
 *     tome_merge_wavg_ln_amp.
 */
int tome_drop_ln_amp(const void *x, int x_dtype, const void *addend, int addend_dtype, int64_t n, int64_t T, int64_t C,
                     int64_t r, const int64_t *und_idx, int distill_token, const void *weight_f32, const void *bias_f32,
                     float eps, void *x_out, void *y_out, int y_dtype, tome_stream_t stream);

/*
 * tome_layernorm_backward_amp  <-  the backward of tome_add_layernorm_amp: tome_layernorm_backward's formula for a model
 *     that trains under autocast with a GradScaler and fp32 master weights (additions to ABI v11, no entry changed;
 *     tools/train_net.py:123 and :680, tome/utils.py:54).
 *         gy of gy_dtype (16-bit): [rows, C], or with skip_first [groups * (group_rows - 1), C];
 *         xs (the stored x'), gx_in (or NULL), gx of x_dtype: gy_dtype, or TOME_F32 (gx is then the unrounded fp32 value);
 *         weight_f32, dweight_f32, dbias_f32 [C] fp32 (either or both gradients may be NULL: a frozen LayerNorm does no
 *         parameter work and needs no workspace; otherwise tome_layernorm_backward_amp_workspace_bytes(rows, C, x_dtype)
 *         bytes, 0 for an illegal shape or dtype);
 *         gx16 (x_dtype == TOME_F32 only, or NULL): [rows, C] of gy_dtype, round16(gx) from the same registers, bit-equal
 *         to a cast of gx -- the gradient of a 16-bit addend without a pass of its own.
 *     Statistics recomputed from xs with the forward's arithmetic; no atomics, same bits on every run.
 */
size_t tome_layernorm_backward_amp_workspace_bytes(int64_t rows, int64_t C, int x_dtype);
int tome_layernorm_backward_amp(const void *gy, int gy_dtype, const void *xs, const void *gx_in, int x_dtype,
                                int64_t groups, int64_t group_rows, int skip_first, int64_t C, const void *weight_f32,
                                float eps, void *gx, void *gx16, void *dweight_f32, void *dbias_f32, void *workspace,
                                tome_stream_t stream);

/*
 * tome_merge_ln_backward_amp  <-  the backward of tome_merge_wavg_ln_amp and tome_drop_ln_amp (flat layout) as ONE launch:
 *     tome_merge_ln_backward's formula for a model that trains under autocast with fp32 master weights (additions to ABI
 *     v11, no entry changed; tools/train_net.py:123 and :680, tome/utils.py:54).
 *         gy [n,T-r,C] of gy_dtype (16-bit); xs (the forward's stored x_out), gx_out (or NULL) [n,T-r,C] and gx [n,T,C] of
 *         x_dtype: gy_dtype or TOME_F32; weight_f32, dweight_f32, dbias_f32 [C] fp32; out_div = size_out [n,T-r],
 *         in_mul = size [n,T] or NULL, of size_dtype (x_dtype or TOME_F32; ignored when both are NULL); row_map,
 *         distill_token and drop as in tome_merge_ln_backward.
 *     With o(t) the merged row of token t, gw = gy * weight, xhat = (xs - mean) * rstd:
 *         gm[o] = gx_out[o] + rstd * (gw - mean(gw) - xhat * mean(gw * xhat))       fp32, not rounded
 *         gx[t] = (gm[o(t)] / out_div[o(t)]) * in_mul[t]      division first; one rounding to a 16-bit x_dtype, none to fp32
 *     drop != 0: no scales, a merged-away token gets 0.  gx16 (x_dtype == TOME_F32 only, or NULL): [n,T,C] of gy_dtype,
 *     round16(gx) from the same registers, bit-equal to a cast of gx -- the gradient of a 16-bit addend of an fp32 stream.
 *     mean and rstd are recomputed from xs with the arithmetic of tome_layernorm_backward_amp, and gm is that entry's
 *     expression term for term.
 *         dweight[c] = sum over the merged rows of gy * xhat,   dbias[c] = sum over the merged rows of gy
 *     every merged row once, counted by the token that owns it; fp32 partial rows in `workspace` summed in a fixed order,
 *     no atomics, same bits on every run.  Either gradient may be NULL; both NULL (frozen LayerNorm): no parameter work
 *     and no workspace.  Otherwise workspace holds tome_merge_ln_backward_amp_workspace_bytes(n, T, C, x_dtype) bytes (0
 *     for an illegal shape or dtype).  C % 8 == 0, C <= 1024, 0 < r <= T/2, 16-byte aligned buffers; each refusal is made
 *     on the host before any launch, with its own tome_last_error.
 */
size_t tome_merge_ln_backward_amp_workspace_bytes(int64_t n, int64_t T, int64_t C, int x_dtype);
int tome_merge_ln_backward_amp(const void *gy, int gy_dtype, const void *gx_out, const void *xs, int x_dtype,
                               const void *out_div, const void *in_mul, int size_dtype, int64_t n, int64_t T, int64_t C,
                               int64_t r, const int32_t *row_map, int distill_token, int drop, const void *weight_f32,
                               float eps, void *gx, void *gx16, void *dweight_f32, void *dbias_f32, void *workspace,
                               tome_stream_t stream);

/*
 * tome_prop_attention_backward  <-  what autograd derives from the proportional attention of the patched blocks when
 *     q, k or v require grad (additions to ABI v11, no entry changed; models are patched for training,
 *     tools/train_net.py:727-741):
 *         attn = softmax(q k^T * scale + log(size)); x = attn @ v      tome/patch/videomae.py:55-66, vivit.py:95-113
 *         the same with the bias on the non-class block only           tome/patch/timesformer.py:66-78  (bias_skip)
 *     i.e. the backward of tome_prop_attention (its plain form; the segmented form's is
 *     tome_prop_attention_segments_backward below).  With P the softmax and
 *     O = out the forward's stored 16-bit result:
 *         dV = P^T dO,  delta = rowsum(dO o O),  dS = P o (dO V^T - delta),  dQ = scale dS K,  dK = scale dS^T Q
 *     size gets no gradient.  The forward saves nothing: P is recomputed with the forward's definition of the logits
 *     (q * scale * log2 e rounded once to the 16-bit format, bias in log2 units, exp2).  fp32 softmax and accumulation,
 *     P and dS enter the matrix products in the 16-bit format, one rounding per output.  Two launches, no atomics,
 *     every row of dq, dk, dv written once, same bits on every run; no allocation, no synchronisation.
 *     q, out, dout, dq: [B, H, N, 64]; k, v, dk, dv: [B, H, Nk, 64]; each with element strides {batch, head, token}
 *     (multiples of 8, contiguous channels, 16-byte aligned base) -- the three slices of one [B, N, 3, H, 64] buffer
 *     are a legal source and a legal target; only the 64 channels of every row are written.  log_size as in
 *     tome_prop_attention (NULL: no bias; bias_skip needs N == Nk).  workspace: 16-byte aligned,
 *     tome_prop_attention_backward_workspace_bytes(B, H, N, Nk) bytes (fp32 row statistics; 0 for an illegal shape);
 *     NULL or workspace_bytes below that: TOME_EWORKSPACE.  Head dim 64 and TOME_BF16 / TOME_F16 only.
 */
size_t tome_prop_attention_backward_workspace_bytes(int64_t B, int64_t H, int64_t N, int64_t Nk);
int tome_prop_attention_backward(const void *q, const void *k, const void *v, const void *out, const void *dout,
                                 int dtype, int64_t B, int64_t H, int64_t N, int64_t Nk, int64_t D,
                                 const int64_t *q_strides, const int64_t *k_strides, const int64_t *v_strides,
                                 const int64_t *out_strides, const int64_t *dout_strides, const float *log_size,
                                 int64_t log_size_stride, int bias_skip, float scale, void *dq, void *dk, void *dv,
                                 const int64_t *dq_strides, const int64_t *dk_strides, const int64_t *dv_strides,
                                 void *workspace, size_t workspace_bytes, tome_stream_t stream);

/*
 * tome_prop_attention_segments_backward  <-  what autograd derives from the per-frame stage of
 *     ToMeTrajectoryAttention.forward (tome/patch/motionformer.py:98-121) when q, k or v require grad (additions to ABI
 *     v11, no entry changed): the backward of tome_prop_attention_segments.  For every segment s, with P_s its own softmax
 *     recomputed with the forward's definition of the logits (as in tome_prop_attention_backward) and O_s the forward's
 *     stored 16-bit result:
 *         dV_s = P_s^T dO_s,  delta_s = rowsum(dO_s o O_s),  dS_s = P_s o (dO_s V_s^T - delta_s),  dK_s = scale dS_s^T Q,
 *         dQ = scale * sum_s dS_s K_s
 *     The sum over the segments is taken in fp32 inside the workgroup that owns the query rows and rounded once when dq
 *     is stored.  Two launches, no atomics, every row of dq, dk, dv written exactly once and nothing beside its 64
 *     channels, same bits on every run; no allocation, no synchronisation.  size gets no gradient.
 *     q, k, v, log_size, nseg and seg_strides = {k, v, out, log_size}: the forward's arguments (Nk keys per segment).
 *     out and dout: the [B, N, nseg, H*64] layout the forward writes, each as {batch, head, token} element strides;
 *     segment s of out lies seg_strides[2] elements, of dout grad_seg_strides[0] elements behind segment s-1.
 *     dq [B, H, N, 64]; dk, dv [B, H, Nk, 64] per segment, each with strides of its own; segment s of dk / dv lies
 *     grad_seg_strides[1] / [2] elements behind segment s-1 (grad_seg_strides = {dout, dk, dv}) -- rows 1 .. of the
 *     three slices of one [B, N, 3, H, 64] gradient buffer are a legal target.  All strides and offsets multiples of 8,
 *     bases 16-byte aligned.  workspace: 16-byte aligned, tome_prop_attention_segments_backward_workspace_bytes(B, H, N,
 *     Nk, nseg) bytes (fp32 L and delta per segment and query row; 0 for an illegal shape); NULL or workspace_bytes
 *     below that: TOME_EWORKSPACE; anything else wrong: TOME_EINVAL with a message.  Head dim 64, TOME_BF16 / TOME_F16.
 */
size_t tome_prop_attention_segments_backward_workspace_bytes(int64_t B, int64_t H, int64_t N, int64_t Nk, int64_t nseg);
int tome_prop_attention_segments_backward(const void *q, const void *k, const void *v, const void *out, const void *dout,
                                          int dtype, int64_t B, int64_t H, int64_t N, int64_t Nk, int64_t D,
                                          const int64_t *q_strides, const int64_t *k_strides, const int64_t *v_strides,
                                          const int64_t *out_strides, const int64_t *dout_strides, const float *log_size,
                                          int64_t log_size_stride, float scale, int64_t nseg, const int64_t *seg_strides,
                                          const int64_t *grad_seg_strides, void *dq, void *dk, void *dv,
                                          const int64_t *dq_strides, const int64_t *dk_strides, const int64_t *dv_strides,
                                          void *workspace, size_t workspace_bytes, tome_stream_t stream);

/*
 * tome_trajectory_mix_backward  <-  what autograd derives from the temporal stage of ToMeTrajectoryAttention.forward
 *     (tome/patch/motionformer.py:122-139) when q2, k2 or val require grad (additions to ABI v11, no entry changed): the
 *     backward of tome_trajectory_mix.  Per (batch, token, head), with p = softmax_f(scale * q2 . k2[f]) recomputed as
 *     the forward computes it:
 *         dval[f] = p_f dout,  dp_f = dout . val[f],  delta = sum_f p_f dp_f,  ds_f = p_f (dp_f - delta),
 *         dq2 = scale sum_f ds_f k2[f],  dk2[f] = scale ds_f q2
 *     fp32 throughout, one rounding per output element; one streaming launch, no workspace, no atomics, same bits on
 *     every run.  The forward's `tattn` output gets NO gradient: the patched block never consumes the map; a caller that
 *     wants it under grad keeps the framework's ops.
 *     q2 [B, S, H*64] contiguous; k2, val [B, S, F, H*64] views with their row strides as in the forward (val may be
 *     the trajectory tokens themselves); dout [B, S, H*64] rows, batch b starting dout_batch_stride elements behind
 *     batch b-1 (0 = contiguous; larger: rows 1 .. of the [B, 1+S, C] gradient of the joined buffer); dq2 [B, S, H*64]
 *     contiguous; dk2, dval [B, S, F, H*64] with row strides of their own -- the two halves of one [B, S, F, 2C] buffer
 *     are a legal target -- each NULL when that gradient is not wanted.  Only the H*64 channels of every row are written.
 *     16-bit tensors, head dim 64, H <= 16, F <= 8, rows 16-byte aligned; anything else is TOME_EINVAL with a message.
 */
int tome_trajectory_mix_backward(const void *q2, const void *k2, const void *val, const void *dout, int dtype, int64_t B,
                                 int64_t S, int64_t F, int64_t H, int64_t D, int64_t k_row_stride, int64_t v_row_stride,
                                 int64_t dout_batch_stride, float scale, void *dq2, void *dk2, void *dval,
                                 int64_t dk_row_stride, int64_t dv_row_stride, tome_stream_t stream);

/*
 * tome_short_attention_backward  <-  what autograd derives from `self.temporal_attn(...)` in ToMeBlock.forward of the
 *     TimeSformer patch (tome/patch/timesformer.py:25-27) when the qkv projection requires grad (additions to ABI v11,
 *     no entry changed; models are patched for training, tools/train_net.py:727-741): the backward of
 *     tome_short_attention.  With P = softmax(q k^T * scale) recomputed with the forward's definition of the logits
 *     (packed 2-element dot products, scale * log2 e, exp2):
 *         dP = dO V^T,  delta_i = sum_j P_ij dP_ij,  dS = P o (dP - delta),  dQ = scale dS K,  dK = scale dS^T Q,
 *         dV = P^T dO
 *     fp32 throughout, one rounding per output; delta comes from the recomputed P, so the forward's output is not read
 *     and the forward saves nothing.  One launch, no workspace, no atomics, same bits on every run.
 *     q, k, v: as in tome_short_attention ([B, H, N <= 8, 64] views, head stride 64, 16-byte aligned rows); dout
 *     [B, N, H*64] contiguous, the layout the forward writes; dq, dk, dv: views with the same kind of strides -- the
 *     three slices of one [B, N, 3, H, 64] buffer are a legal target.  Every one of the 64 channels of every row is
 *     written exactly once and nothing else is, so the targets need no initialisation; their rows must not overlap.
 *     TOME_BF16 / TOME_F16 and D = 64 only; anything else is TOME_EINVAL with a message.
 */
int tome_short_attention_backward(const void *q, const void *k, const void *v, const void *dout, int dtype, int64_t B,
                                  int64_t H, int64_t N, int64_t D, const int64_t *q_strides, const int64_t *k_strides,
                                  const int64_t *v_strides, float scale, void *dq, void *dk, void *dv,
                                  const int64_t *dq_strides, const int64_t *dk_strides, const int64_t *dv_strides,
                                  tome_stream_t stream);

/* tome_gelu_erf  <-  the activation of the MLP the patched block calls between merge and second residual
 * (`x = x + self.drop_path(self.mlp(self.norm2(x)))`, tome/patch/videomae.py:29, timesformer.py:56,
 * motionformer.py:29; the models' `act_layer=nn.GELU`): y = x * 0.5 * (1 + erf(x / sqrt(2))) on `elements` 16-bit
 * values (a multiple of 8), fp32 arithmetic, bit-identical to the framework's kernel.  y may alias x. */
int tome_gelu_erf(const void *x, int dtype, int64_t elements, void *y, tome_stream_t stream);

/*
 * tome_token_mean  <-  the mean pooling in front of the head of a ViT without class token and the MLP in front of it
 *     (slowfast/models/videomae_video_model_builder.py, forward_features: `x = self.norm(x)` with norm = nn.Identity(),
 *     `return self.fc_norm(x.mean(1))`; the last block's `Mlp.forward`: `x = self.fc2(self.act(self.fc1(x)))`).  The
 *     last block's output is read only through that unweighted mean, and everything behind the activation is linear:
 *         mean_t(x'_t + b2 + W2 a_t) = mean_t(x'_t) + b2 + W2 mean_t(a_t)            a = gelu(fc1(norm2(x')))
 *     so the block needs two column means instead of fc2 over every token (addition to ABI v11, no entry changed):
 *         out[g, c] = (1 / tokens) * sum_t v[g, t, c]
 *     x: contiguous [groups, tokens, width] of `dtype` (TOME_BF16 / TOME_F16, width % 8 == 0), 16-byte aligned; out: fp32
 *     [groups, width].  act = 0: v = x.  act = 1: v = the 16-bit value tome_gelu_erf would have stored for x (rounded to
 *     `dtype`, then widened), so the mean is taken of exactly the bits fc2 used to read; nothing is written but out.
 *     fp32 sums in one fixed order (rows ascending per wave, the waves' sums added in wave order), one division by
 *     `tokens`: no atomics, the same bits on every run; no workspace, no allocation, no synchronisation.
 *     groups < 1, tokens < 1, width % 8 != 0, any other dtype or act, null or misaligned pointers: TOME_EINVAL.
 */
int tome_token_mean(const void *x, int dtype, int64_t groups, int64_t tokens, int64_t width, int act, float *out,
                    tome_stream_t stream);

/*
 * tome_gelu_erf_backward  <-  what autograd derives from the MLP of the patched block between its two Linear layers
 *     when its input or its parameters require grad (additions to ABI v11, no entry changed; models are patched for
 *     training, tools/train_net.py:727-741):
 *         x = x + self.drop_path(self.mlp(self.norm2(x)))      tome/patch/videomae.py:29, timesformer.py:56,
 *                                                              motionformer.py:29   (mlp = fc1, nn.GELU(), fc2)
 *     With h = fc1's output (the saved pre-activation), ga the gradient of the activation, v = h in fp32,
 *     Phi(v) = 0.5 (1 + erf(v / sqrt 2)), phi(v) = exp(-v^2 / 2) / sqrt(2 pi):
 *         gh = ga * (Phi(v) + v phi(v))                        one rounding to `dtype`; gh may be ga (in place)
 *         act = gelu(h)                 (act != NULL)          the bits tome_gelu_erf stored in the forward, for fc2's
 *                                                              weight gradient; a buffer of its own, never h
 *         dbias[c] = sum over rows of the ROUNDED gh[:, c]     (dbias != NULL) fc1's bias gradient: fp32 sums, one
 *                                                              rounding to `dtype`
 *     h, ga, gh, act: contiguous [rows, width] of `dtype` (TOME_BF16 / TOME_F16, width % 8 == 0, width <= 8192,
 *     1 <= rows < 2^31), 16-byte aligned; dbias [width].  One streaming launch (plus the sum of the partial rows when
 *     dbias is asked for), no atomics, same bits on every run; no allocation, no synchronisation.  Without dbias no
 *     workspace is read.  With it: workspace of tome_gelu_erf_backward_workspace_bytes(rows, width) bytes (fp32 partial
 *     rows [parts <= 512, width]; 0 for an illegal shape); NULL or workspace_bytes below that: TOME_EWORKSPACE.
 */
size_t tome_gelu_erf_backward_workspace_bytes(int64_t rows, int64_t width);
int tome_gelu_erf_backward(const void *h, const void *ga, int dtype, int64_t rows, int64_t width, void *gh, void *act,
                           void *dbias, void *workspace, size_t workspace_bytes, tome_stream_t stream);

/*
 * tome_gelu_tanh, tome_gelu_tanh_backward  <-  the MLP of ViViT's layer, forward and what autograd derives from it
 *     (additions to ABI v11, no entry changed):
 *         layer_output = self.layernorm_after(hidden_states)           tome/patch/vivit.py:39   the layer forward,
 *         layer_output = self.intermediate(layer_output)               tome/patch/vivit.py:40   ToMeVivitLayer.forward
 *         layer_output = self.output(layer_output, hidden_states)      tome/patch/vivit.py:43   (:18-47)
 *     where HF's VivitIntermediate is dense -> "gelu_fast" -> dropout and VivitOutput dense -> dropout -> + residual;
 *     gelu_fast (transformers.activations.FastGELUActivation) is 0.5 x (1 + tanh(0.7978845608 x (1 + 0.044715 x^2))).
 *     Arithmetic contract.  v = the stored 16-bit pre-activation in fp32, beta = 0.7978845608028654f, kappa = 0.044715f:
 *         u  = beta (v + kappa v^3)
 *         s  = sigma(2u) = 1 / (1 + exp(-2u))            ( = 0.5 (1 + tanh u) )
 *         a  = v s                                       the activation            (tome_gelu_tanh: y; backward: act)
 *         d  = s + v s (1 - s) * 2 beta (1 + 3 kappa v^2)     its derivative
 *         gh = round(ga * d)                             gh may be ga (in place), never h
 *         dbias[c] = sum over rows of the ROUNDED gh[:, c]
 *     fp32 throughout, one rounding per output.  s and 1 - s are each computed without cancellation: with
 *     e = exp(-2|u|) (one hardware exp2 of -2 log2(e) |u|) and r = 1 / (1 + e) (one hardware reciprocal, 1 ulp) they
 *     are r and e r, picked by the sign of u; 1 - s is never formed by subtraction and the framework's 1 + tanh(u),
 *     which has lost every bit below v = -4, is not used.  Every result is
 *     finite for every finite fp16 v and every bf16 v with |v| <= 2^20 (beyond that nothing is promised: the framework's
 *     own formula gives NaN there).  The forward and the backward evaluate s through the same inline function
 *     (csrc/tome_common.h gelu_tanh_sigmoid / gelu_tanh_value), so `act` has the bits tome_gelu_tanh stored.
 *     tome_gelu_tanh: `elements` 16-bit values (a multiple of 8), y may alias x; as tome_gelu_erf.
 *     tome_gelu_tanh_backward: arguments, shapes, refusals and error codes of tome_gelu_erf_backward (16-bit tensors
 *     only, width % 8 == 0, width <= 8192, act a buffer of its own, dbias needs the workspace).  The launch form is the
 *     erf entry's, and so is the workspace: size it with tome_gelu_erf_backward_workspace_bytes(rows, width) -- there is
 *     no second size function.
 */
int tome_gelu_tanh(const void *x, int dtype, int64_t elements, void *y, tome_stream_t stream);
int tome_gelu_tanh_backward(const void *h, const void *ga, int dtype, int64_t rows, int64_t width, void *gh, void *act,
                            void *dbias, void *workspace, size_t workspace_bytes, tome_stream_t stream);

/* tome_tubelet_rows  <-  the models' patch embedding, a convolution whose stride equals its kernel
 * (slowfast/models/videomae_video_model_builder.py:137-166 `PatchEmbed.proj`; TimeSformer's per-frame Conv2d; Motionformer
 * `PatchEmbed3D`; ViViT's tubelet Conv3d): its input side as the [B*N, C*kt*kh*kw] matrix the weight multiplies,
 *     rows[b, (t', h', w'), (c, dt, dh, dw)] = x[b, c, t'*kt + dt, h'*kh + dh, w'*kw + dw]      (a pure move)
 * x: any view [B, C, T, H, W] with unit stride along W, x_strides = element strides {b, c, t, h}; elem_bytes 2 or 4;
 * kw * elem_bytes and every stride a multiple of 16 bytes.  Token order (t', h', w') row-major =
 * `conv(x).flatten(2).transpose(1, 2)`; inner order = the flattened convolution weight's. */
int tome_tubelet_rows(const void *x, int elem_bytes, int64_t B, int64_t C, int64_t T, int64_t H, int64_t W,
                      const int64_t *x_strides, int64_t kt, int64_t kh, int64_t kw, void *rows,
                      tome_stream_t stream);

/* tome_row_map / tome_source_init  <-  merge_source(merge, x, source=None) (merge.py:372-384) and the drop modes'
 * `drop(eye)` (tome/patch/videomae.py:112-117): the first layer's source matrix.  The reference builds an
 * [n,T,T] identity and merges it with mode "max"; element (o, t) of the result is 1 exactly when token t lands in
 * merged row o, i.e. the matching's row map -- so the identity is never made.
 *   tome_row_map      row_map [n,T1] int32 from the index tensors (same values tome_match writes when asked to)
 *   tome_source_init  source_out [n,T-r,T] fp32, one coalesced pass; drop != 0: merged-away tokens get no row
 */
int tome_row_map(int64_t n, int64_t T, int64_t r, int distill_token, const int64_t *src_idx,
                 const int64_t *dst_idx, const int64_t *unm_idx, int32_t *row_map, tome_stream_t stream);
int tome_source_init(int64_t n, int64_t T, int64_t r, int distill_token, int drop, const int32_t *row_map,
                     float *source_out, tome_stream_t stream);

/*
 * Partition matchings  <-  kth_bipartite_soft_matching (merge.py:105-158) and random_bipartite_soft_matching
 * (merge.py:161-212).  Per group an ordered source set A (Na token positions) and an ordered destination set B (Nb
 * positions); EVERY source row is merged into its best destination and the merged sequence is the destination set
 * alone ([n,Nb,C]).  The sets are given either by
 *   k > 1:  the kth rule (merge.py:119-126): tokens in groups of k, the first k-1 of a group are sources (A row
 *           g*(k-1)+j), the last one the destination (B row g); tokens past (T/k)*k belong to neither set.
 *           Na = (T/k)*(k-1), Nb = T/k; a_idx / b_idx are ignored (may be null);
 *   k == 0: explicit position lists a_idx [n,Na], b_idx [n,Nb] (int64, values in [0,T), disjoint; merge.py:176-177).
 * k <= 1 otherwise, Nb <= 0, Na <= 0, null or misaligned buffers give TOME_EINVAL.
 *
 * tome_partition_workspace_bytes: scratch of tome_match_partition.
 * tome_match_partition  <-  merge.py:128-135 / :188-196.  metric [n,T,D], element strides (stride_n, stride_t, 1).
 *     out: dst_idx [n,Na] int64 = first-index row argmax of the cosine similarity A.B^T (same arithmetic contract as
 *          tome_match: fp32 unit vectors, k-ordered fma chain on the fp32 matrix pipe; torch.max's NaN rule);
 *          offsets [n,Nb+1], sources [n,Na] int32: the inverted list -- sources[offsets[j] .. offsets[j+1]) are the
 *          A rows merged into B row j, ascending.  Bit-identical on every run.
 * tome_merge_partition  <-  merge(x, mode) (merge.py:137-142 / :198-203): out [n,Nb,C]; a destination's own row
 *     first, then its sources in ascending A-row order (the order of torch's CPU scatter_reduce), fp32 accumulation.
 * tome_merge_wavg_partition  <-  merge_wavg(merge, x, size) (merge.py:355-369) on such a matching, one launch:
 *     x*size summed, size summed, one division; size may be null (all ones); log_size_out optional (log(size')).
 *     size / size_out / log_size_out [n,T,1] / [n,Nb,1] of size_dtype (= x_dtype or TOME_F32).
 * tome_unmerge_partition  <-  unmerge(x) (merge.py:144-156 / :205-210): x [n,Nb,C] -> out [n,Tout,C],
 *     Tout = (T/k)*k for the kth rule (the reference loses the tail too), T for lists; every row written once.
 * x / out are contiguous.
 */
size_t tome_partition_workspace_bytes(int64_t n, int64_t Na, int64_t Nb, int64_t D);
int tome_match_partition(const void *metric, int dtype, int64_t n, int64_t T, int64_t D, int64_t stride_n,
                         int64_t stride_t, int64_t k, const int64_t *a_idx, const int64_t *b_idx, int64_t Na,
                         int64_t Nb, int64_t *dst_idx, int32_t *offsets, int32_t *sources, void *workspace,
                         size_t workspace_bytes, tome_stream_t stream);
int tome_merge_partition(const void *x, int dtype, int64_t n, int64_t T, int64_t C, int64_t k, const int64_t *a_idx,
                         const int64_t *b_idx, int64_t Na, int64_t Nb, const int32_t *offsets,
                         const int32_t *sources, int mode, void *out, tome_stream_t stream);
int tome_merge_wavg_partition(const void *x, int x_dtype, const void *size, int size_dtype, int64_t n, int64_t T,
                              int64_t C, int64_t k, const int64_t *a_idx, const int64_t *b_idx, int64_t Na,
                              int64_t Nb, const int32_t *offsets, const int32_t *sources, void *x_out,
                              void *size_out, void *log_size_out, tome_stream_t stream);
int tome_unmerge_partition(const void *x, int dtype, int64_t n, int64_t T, int64_t C, int64_t k,
                           const int64_t *a_idx, const int64_t *b_idx, int64_t Na, int64_t Nb,
                           const int64_t *dst_idx, void *out, tome_stream_t stream);

#ifdef TOME_PROFILE_HOOKS
/*
 * MEASUREMENT BUILD ONLY (lib/libtome_hip_prof.so, compiled with -DTOME_PROFILE_HOOKS; not part of the product
 * ABI, not in libtome_hip.so): tome_profile_enable(reps > 0) makes tome_match on the calling thread record HIP
 * events between its stages on the caller's stream and launch every stage kernel `reps` times back to back (the
 * kernels are pure functions of their inputs, results are unchanged); tome_profile_read waits for the last
 * profiled call and returns the milliseconds PER LAUNCH of the stages {unit vectors, similarity+row max,
 * rank+select}.  bench.py's stage-timing leg is the only caller.  No reference counterpart.
 */
int tome_profile_enable(int on);
int tome_profile_read(float *stage_ms, int max_stages);
#endif

#ifdef __cplusplus
}
#endif
#endif /* TOME_HIP_H */

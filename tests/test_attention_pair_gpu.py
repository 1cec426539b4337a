"""k_prop_attention_stream<.., PAIR = true> (csrc/tome_attn_stream.h): the persistent attention kernel held to 128
registers, two workgroups per CU, forced through TOME_ATTN_STREAM=2 on inputs small enough to take seconds.  What
differs from the one-workgroup-per-CU form and is exercised here: the reference point carried by the matrix pipe
(two 16-bit terms in the bias k-step) instead of the accumulators' start values, the PV product taken in the step that
staged the tile, lane-derived addresses formed again at every use, and the grid of two workgroups per CU.

Every case, both 16-bit formats, without and with the per-key bias where the case allows it:
  * against the framework's attention on fp32 copies of the inputs, under the bound the stream-kernel tests of
    tests/test_hip_parity.py hold that format to (restated below with their lines);
  * against the one-workgroup-per-CU form of the kernel (TOME_ATTN_STREAM=1) under the same bound;
  * `out` is filled with NaN beforehand: a query row or head left unwritten shows as a non-finite value.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# tests/test_hip_parity.py:1364 (test_prop_attention_tile_edges_each_workgroup_shape, TOME_ATTN_WAVES=8: the stream
# kernel): absolute, the values are convex combinations of v ~ N(0, 1)
TOL = {torch.bfloat16: 1e-2, torch.float16: 2e-3}
# tests/test_hip_parity.py:1395 (test_prop_attention_rerun_path, the stream form among the others): the same inputs
# as the dominant-key test below -- q of norm 8 along one direction, a jump of 70 / 18 log2 units
TOL_RERUN = {torch.bfloat16: 2e-2, torch.float16: 4e-3}
SWITCHES = ("TOME_ATTN_RESIDENT", "TOME_ATTN_WAVES", "TOME_ATTN_STREAM", "TOME_ATTN_GRID")
PAIR = {"TOME_ATTN_RESIDENT": "0", "TOME_ATTN_WAVES": "8", "TOME_ATTN_STREAM": "2"}
OLD = {"TOME_ATTN_RESIDENT": "0", "TOME_ATTN_WAVES": "8", "TOME_ATTN_STREAM": "1"}


def _reference(q, k, v, log_bias, skip, scale=0.125):
    """The framework's attention on fp32 copies -> [B, N, H, 64]; the bias per key, or TimeSformer's skip form
    (query 0 and key 0 unbiased, log_bias[j - 1] on key j)."""
    B, H, N, _ = q.shape
    Nk = k.shape[2]
    mask = None
    if log_bias is not None:
        mask = torch.zeros(B, 1, N, Nk, device=q.device)
        if skip:
            mask[:, :, 1:, 1:] = log_bias[:, None, None, :]
        else:
            mask[:, :, :, :] = log_bias[:, None, None, :]
    out = F.scaled_dot_product_attention(q.float(), k.float(), v.float(), attn_mask=mask, scale=scale)
    return out.transpose(1, 2)


def _run(monkeypatch, env, grid, q, k, v, log_bias, skip):
    """One call under the switches of `env` (+ the forced workgroup count) into a NaN-filled out -> [B, N, H, 64]."""
    from tome import _abi
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    if grid:
        monkeypatch.setenv("TOME_ATTN_GRID", str(grid))
    B, H, N, _ = q.shape
    out = torch.full((B, N, H, 64), float("nan"), dtype=q.dtype, device=q.device)
    res = _abi.prop_attention(q, k, v, None, 0.125, bias_skip=skip, log_bias=log_bias, out=out)
    assert res.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    return out


def _check(monkeypatch, what, q, k, v, log_bias, skip, grid, tol):
    want = _reference(q, k, v, log_bias, skip)
    new = _run(monkeypatch, PAIR, grid, q, k, v, log_bias, skip)
    old = _run(monkeypatch, OLD, grid, q, k, v, log_bias, skip)
    for name, got in (("pair", new), ("one workgroup per CU", old)):
        bad = ~torch.isfinite(got.float())
        assert not bool(bad.any()), f"{what}: {name}: {int(bad.any(-1).sum())} (query, head) rows not written"
    e_ref = float((new.float() - want).abs().max())
    e_old = float((new.float() - old.float()).abs().max())
    e_old_ref = float((old.float() - want).abs().max())
    print(f"{what}: pair vs fp32 {e_ref:.3e}, pair vs old kernel {e_old:.3e}, old kernel vs fp32 {e_old_ref:.3e}, "
          f"bound {tol:.0e}")
    assert e_ref <= tol, (what, "against the fp32 reference", e_ref)
    assert e_old <= tol, (what, "against the one-workgroup-per-CU form", e_old)


def _heads(B, H, N, Nk, dtype, g):
    """q [B, H, N, 64] and k, v [B, H, Nk, 64] as the strided head views the patches pass (one buffer per tensor)."""
    q = torch.randn(B, N, H, 64, device=DEV, generator=g).to(dtype).permute(0, 2, 1, 3)
    k = torch.randn(B, Nk, H, 64, device=DEV, generator=g).to(dtype).permute(0, 2, 1, 3)
    v = torch.randn(B, Nk, H, 64, device=DEV, generator=g).to(dtype).permute(0, 2, 1, 3)
    return q, k, v


# (B, H, N, Nk, forced workgroups or None)
SHAPES = {
    # three key tiles, the last one masked down to one key; the second query block holds one row: a part-empty block
    # with seven helper waves.  The smallest N == Nk with a tile and a block boundary inside.
    "1-two-blocks-129": (1, 2, 129, 129, None),
    # 16 items over 8 workgroups: every workgroup walks a second item (the switch between items), whose block is the
    # 32-row tail (one computing wave, seven helpers)
    "2-second-item-288": (1, 2, 288, 288, 8),
    # N != Nk, two tiles, 33 keys in the last one (the full-width masked tile) ...
    "3-tall-256x97": (1, 2, 256, 97, None),
    # ... and 32 keys in the last one: `last_half`, the half-width masked tile
    "3b-tall-256x96": (1, 2, 256, 96, None),
    # 80 items over 8 workgroups, five tiles per item: the ring slot parity flips from item to item
    "4-ten-items-320": (3, 12, 320, 320, 8),
}


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("case", list(SHAPES))
def test_pair_kernel_shapes(case, dtype, monkeypatch):
    B, H, N, Nk, grid = SHAPES[case]
    g = torch.Generator(device=DEV).manual_seed(1000 + N + Nk)
    q, k, v = _heads(B, H, N, Nk, dtype, g)
    lb = torch.randint(1, 30, (B, Nk), device=DEV, generator=g).float().log()
    for bias in (None, lb):
        _check(monkeypatch, f"{case} {dtype} bias={bias is not None}", q, k, v, bias, False, grid, TOL[dtype])


@pytest.mark.parametrize("dtype,jump", [(torch.bfloat16, 70.0), (torch.float16, 18.0)], ids=["bf16", "fp16"])
@pytest.mark.parametrize("N", [200, 256])
def test_pair_kernel_dominant_key_in_last_tile(N, dtype, jump, monkeypatch):
    """The logits of every query sit near 0 up to the last tile and `jump` log2 units higher (beyond what the
    16-bit weights can hold against the first tile's reference point) on the keys of the last tile -- 8 keys of a
    half-width masked tile (N = 200) or a full tile (N = 256).  The guard must trip in that tile and the wave take
    it again on the general path, which moves the reference point that the matrix pipe carries."""
    B, H = 2, 3
    g = torch.Generator(device=DEV).manual_seed(N + int(jump))
    direction = torch.randn(B, H, 1, 64, device=DEV, generator=g)
    direction = direction / direction.norm(dim=-1, keepdim=True)
    amp = jump / 1.4426950408889634  # q . k * scale * log2(e) = jump: q = 8 d, k = amp d, scale = 1/8
    step = torch.zeros(1, 1, N, 1, device=DEV)
    step[:, :, 192:] = amp
    q = (8.0 * direction + 0.05 * torch.randn(B, H, N, 64, device=DEV, generator=g)).to(dtype)
    k = (step * direction + 0.05 * torch.randn(B, H, N, 64, device=DEV, generator=g)).to(dtype)
    v = torch.randn(B, H, N, 64, device=DEV, generator=g).to(dtype)
    lb = torch.randint(1, 9, (B, N), device=DEV, generator=g).float().log()
    # (not vacuous: against the first tile's maximum the late scores are out of the format's range)
    s2 = (q.float() @ k.float().transpose(-1, -2)) * (0.125 * 1.4426950408889634)
    assert float((s2 - s2[..., :64].amax(-1, keepdim=True)).amax()) > (60.0 if dtype == torch.bfloat16 else 15.0)
    for bias in (None, lb):
        _check(monkeypatch, f"dominant key N={N} {dtype} bias={bias is not None}", q, k, v, bias, False, None,
               TOL_RERUN[dtype])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("N,grid", [(129, None), (288, 8)])
def test_pair_kernel_timesformer_skip_form(N, grid, dtype, monkeypatch):
    """bias_skip = 1 -- key 0 and the whole of query row 0 unbiased, log_bias[j - 1] on key j; query row 0 is
    one lane of the first block's first wave, every later block has no such row."""
    B, H = 2, 3
    g = torch.Generator(device=DEV).manual_seed(6000 + N)
    q, k, v = _heads(B, H, N, N, dtype, g)
    lb = torch.randint(1, 30, (B, N - 1), device=DEV, generator=g).float().log()
    _check(monkeypatch, f"skip form N={N} {dtype}", q, k, v, lb, True, grid, TOL[dtype])

"""tests/ln_oracle.py on the CPU: `check` accepts honest fp32 LayerNorms of the inputs the GPU tests use, at every
width 8 .. 1024 in both 16-bit formats, and rejects what a slip in the rows-per-wave packing or in the arithmetic of
the fused kernels would produce.  The mutants are emulations in torch on the CPU; no kernel is altered anywhere."""
import pytest
import torch

import ln_oracle as lo

DTYPES = [torch.bfloat16, torch.float16]
IDS = ["bf16", "fp16"]
EPS = 1e-6
ROWS = 64
F32 = torch.float32


# ---------------------------------------------------------------------------------------------------------------------
# fp32 evaluations: an honest one whose summation order differs from the framework's, with switches for the slips
# ---------------------------------------------------------------------------------------------------------------------
def _tree(t):
    """pairwise fp32 sum over the last dimension"""
    while t.shape[-1] > 1:
        if t.shape[-1] % 2:
            t = torch.cat((t, torch.zeros_like(t[..., :1])), -1)
        t = t[..., 0::2] + t[..., 1::2]
    return t[..., 0]


def _chunk_tree(v, weight=None):
    """sums of 8 consecutive channels (sequential), then a pairwise tree over the chunks; weight [chunks] scales the
    chunk sums (0: chunk left out, 2: counted twice)"""
    rows, C = v.shape
    ch = v.reshape(rows, C // 8, 8)
    s = ch[..., 0].clone()
    for e in range(1, 8):
        s = s + ch[..., e]
    if weight is not None:
        s = s * weight
    return _tree(s)


def ln32(x, w, b, eps=EPS, mutant=None, chunk=None):
    """fp32 LayerNorm of the stored rows x [rows, C], rounded once to x.dtype.  mutant None is an honest evaluation
    (chunk sums, pairwise tree, 1/C as a product, two passes, y = d * (w * rstd) + b)."""
    dtype = x.dtype
    rows, C = x.shape
    cpr = C // 8
    j = (cpr // 2) if chunk is None else chunk
    xf, wf, bf = x.to(F32), w.to(F32), b.to(F32)
    inv_c = torch.tensor(1.0, dtype=F32) / torch.tensor(float(C), dtype=F32)
    cw = torch.ones(cpr, dtype=F32)
    mean_w = var_w = None
    if mutant == "mean_drops_chunk":
        mean_w = cw.clone(); mean_w[j] = 0.0
    if mutant == "mean_counts_chunk_twice":
        mean_w = cw.clone(); mean_w[j] = 2.0
    if mutant == "var_drops_chunk":
        var_w = cw.clone(); var_w[j] = 0.0
    if mutant == "var_counts_chunk_twice":
        var_w = cw.clone(); var_w[j] = 2.0
    m = (_chunk_tree(xf, mean_w) * inv_c)[:, None]
    d = xf - m
    if mutant == "var_uncentred":
        var = _chunk_tree(xf * xf) * inv_c - m[:, 0] * m[:, 0]
    elif mutant == "var_unbiased":
        var = _chunk_tree(d * d) / torch.tensor(float(C - 1), dtype=F32)
    else:
        var = _chunk_tree(d * d, var_w) * inv_c
    if mutant == "eps_missing":
        rs = 1.0 / torch.sqrt(var)
    elif mutant == "eps_after_sqrt":
        rs = 1.0 / (torch.sqrt(var) + eps)
    else:
        rs = 1.0 / torch.sqrt(var + eps)
    rs = rs[:, None]
    mm, rr = m.expand(rows, C).clone(), rs.expand(rows, C).clone()
    sl = slice(8 * j, 8 * j + 8)
    if mutant in ("neighbour_stats", "neighbour_mean"):
        mm[:, sl] = torch.roll(m, -1, 0).expand(rows, 8)
    if mutant in ("neighbour_stats", "neighbour_rstd"):
        rr[:, sl] = torch.roll(rs, -1, 0).expand(rows, 8)
    if mutant == "weight_from_next_column":
        wf = wf.clone(); wf[sl] = w.to(F32)[8 * (j + 1) % C:][:8] if 8 * (j + 1) < C else w.to(F32)[:8]
    if mutant == "bias_from_next_column":
        bf = bf.clone(); bf[sl] = b.to(F32)[8 * (j + 1) % C:][:8] if 8 * (j + 1) < C else b.to(F32)[:8]
    y = (xf - mm) * (wf * rr) + bf
    if mutant == "rounded_twice":  # fp32 -> fp16 -> bf16
        return y.to(torch.float16).to(dtype)
    if mutant == "truncated":
        bits = y.view(torch.int32)
        drop = 16 if dtype == torch.bfloat16 else 13
        t = (bits >> drop << drop).view(F32)  # fp16: exact for normal results, which is all these rows produce
        return t.to(dtype)
    return y.to(dtype)


def framework32(x, w, b, eps=EPS):
    return torch.nn.functional.layer_norm(x.to(F32), (x.shape[-1],), w.to(F32), b.to(F32), eps).to(x.dtype)


def framework_sums32(x, w, b, eps=EPS):
    """two passes with the framework's own fp32 reductions (its vectorised summation order), a true division by C,
    rsqrt, and the products associated the other way round"""
    xf, C = x.to(F32), x.shape[-1]
    m = xf.sum(-1, keepdim=True) / C
    d = xf - m
    rs = torch.rsqrt((d * d).sum(-1, keepdim=True) / C + eps)
    return (d * rs * w.to(F32) + b.to(F32)).to(x.dtype)


def rejected(y, x, w, b, signature=True, R=4):
    try:
        lo.check(y, x, w, b, EPS, R=R, signature=signature, label="mutant")
    except AssertionError as e:
        assert "outside the bound" in str(e), e  # the inputs' own condition must not be what fails
        return True
    return False


def _inputs(C, dtype, sign=1):
    return lo.signature_rows((ROWS, C), dtype, 1000 + C, sign=sign), *lo.affine(C, dtype, 7 + C)


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_honest_evaluations_are_accepted_at_every_width(dtype, capsys):
    """Three fp32 evaluations, each rounded once: the framework's LayerNorm, two passes over the framework's own
    reductions, and chunk sums of 8 followed by a pairwise tree with 1/C as a product.  The two that sum the row are
    inside the bound on signature rows of both signs with the 99 % / u/8 condition; the framework's LayerNorm keeps a
    running mean instead of a sum (ln_oracle, step 1c) and is inside the bound with the any-order mean term; all three
    on plain rows; at all 128 widths."""
    worst = 0.0
    for C in lo.WIDTHS:
        w, b = lo.affine(C, dtype, 7 + C)
        for name, x, sig in (("sig+", lo.signature_rows((ROWS, C), dtype, 1000 + C, 1), True),
                             ("sig-", lo.signature_rows((ROWS, C), dtype, 2000 + C, -1), True),
                             ("plain", lo.plain_rows((ROWS, C), dtype, 3000 + C), False)):
            for ev in (framework32, framework_sums32, ln32):
                sums = ev is not framework32
                st = lo.check(ev(x, w, b), x, w, b, EPS, R=4, signature=sig and sums, sums=sums,
                              label=f"{ev.__name__} {name} C={C}")
                worst = max(worst, st["worst"])
    capsys.readouterr()
    print(f"worst err / bound of the honest evaluations: {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_condition_holds_for_merged_signature_rows(dtype, capsys):
    """What the merge stores: rows of one class averaged two, three and five at a time with sizes 1 .. 4 (fp32
    products and sum, one division, one rounding), with and without a grid addend in front.  They are still exact-sum
    rows with e32 <= u/8 |ref| + 2^-14, at every width, and an honest LayerNorm of them is accepted."""
    gen = torch.Generator().manual_seed(5)
    for C in lo.WIDTHS:
        w, b = lo.affine(C, dtype, 7 + C)
        for k in (2, 3, 5):
            for sign in (1, -1):
                klass = torch.arange(ROWS)
                parts = []
                for i in range(k):
                    xi = lo.signature_rows((ROWS, C), dtype, 100 * C + 10 * k + i, sign, klass)
                    if i % 2:
                        xi = xi + lo.signature_rows((ROWS, C), dtype, 77 * C + i, sign, klass, 0.5, offset=False)
                    parts.append(xi.to(F32))
                sizes = torch.randint(1, 5, (k, ROWS, 1), generator=gen).to(F32)
                acc = parts[0] * sizes[0]
                for i in range(1, k):
                    acc = acc + parts[i] * sizes[i]
                merged = (acc / sizes.sum(0)).to(dtype)
                lo.assert_rows_in_a_wave_differ(merged, ROWS, f"merged k={k} C={C}")
                lo.check(ln32(merged, w, b), merged, w, b, EPS, R=4, signature=True, label=f"merged k={k} C={C}")
    capsys.readouterr()


CHUNK_MUTANTS = ["mean_drops_chunk", "mean_counts_chunk_twice", "var_drops_chunk", "var_counts_chunk_twice",
                 "neighbour_stats"]
COLUMN_MUTANTS = ["weight_from_next_column", "bias_from_next_column"]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("mutant", CHUNK_MUTANTS + COLUMN_MUTANTS)
def test_packing_slips_are_rejected_at_every_width(mutant, dtype, capsys):
    """One chunk of 8 channels left out of the mean / of the variance / counted twice; one chunk normalised with the
    mean and rstd of the next row; a weight or bias chunk taken from the next column -- on the signature rows, for the
    first, a middle and the last chunk of the row, at every width.  (A row of one chunk has no neighbouring column:
    the two column mutants start at C = 16.)"""
    missed = []
    for C in lo.WIDTHS:
        if mutant in COLUMN_MUTANTS and C == 8:
            continue
        x, w, b = _inputs(C, dtype)
        for chunk in sorted({0, C // 16, C // 8 - 1}):
            if not rejected(ln32(x, w, b, mutant=mutant, chunk=chunk), x, w, b):
                missed.append((C, chunk))
    capsys.readouterr()
    assert not missed, f"{mutant} accepted at (C, chunk) {missed}"


@pytest.mark.parametrize("mutant,dtype", [("rounded_twice", torch.bfloat16), ("truncated", torch.bfloat16),
                                          ("truncated", torch.float16)], ids=["twice-bf16", "trunc-bf16", "trunc-fp16"])
def test_a_second_rounding_is_rejected_at_every_width(mutant, dtype, capsys):
    """fp32 -> fp16 -> bf16 (for fp16 tokens that detour is a single rounding, so there is nothing to reject) and
    truncation instead of round to nearest even leave more than one unit roundoff on some element of 64 rows."""
    missed = []
    for C in lo.WIDTHS:
        x, w, b = _inputs(C, dtype)
        if not rejected(ln32(x, w, b, mutant=mutant), x, w, b):
            missed.append(C)
    capsys.readouterr()
    assert not missed, f"{mutant} accepted at C = {missed}"


def far_rows(C, dtype, seed):
    """Rows of one class far from zero: fp16 768 + 0.5 round(z), bf16 384 + 2 round(z) (the finest grids the formats
    hold there)."""
    M, s = (768.0, 0.5) if dtype == torch.float16 else (384.0, 2.0)
    z = torch.randn((ROWS, C), generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    rows = M + s * torch.round(z)
    assert torch.equal(rows.to(dtype).double(), rows)
    return rows.to(dtype)


def test_uncentred_variance_is_rejected_where_it_is_wrong(capsys):
    """Variance as E[x^2] - mean^2 in fp32.  Its error is 2^-24 mean^2 against a variance of about s^2, i.e.
    (M / s)^2 2^-24 relative.  fp16 rows at 768 + 0.5 round(z): 2^-24 * 1536^2 = 0.14 -- rejected at every width
    (asserted).  On bf16 no stored row can show it: a grid a format of 8 significant bits holds has M / s <= 2^8, so
    the error stays below 2^-8 of the variance, 2^-9 of the result: half a unit roundoff.  The same holds for the
    signature rows (M / s <= 33: below 2^-13 of the result, and for C below about 200 their squares and the sums of
    those are integers under 2^24, so the uncentred form is an exact evaluation there).  Those two are counted
    and printed, not asserted: a mutant that computes the right answer cannot be rejected."""
    missed, counts = [], {}
    for C in lo.WIDTHS:
        for dtype in DTYPES:
            w, b = lo.affine(C, dtype, 7 + C)
            x = far_rows(C, dtype, 4000 + C)
            lo.check(ln32(x, w, b), x, w, b, EPS, R=4, signature=False, label=f"far rows, honest, C={C}")
            rej = rejected(ln32(x, w, b, mutant="var_uncentred"), x, w, b, signature=False)
            if dtype == torch.float16 and not rej:
                missed.append(C)
            counts[("far", dtype)] = counts.get(("far", dtype), 0) + rej
            xs, _, _ = _inputs(C, dtype)
            rej = rejected(ln32(xs, w, b, mutant="var_uncentred"), xs, w, b)
            counts[("signature", dtype)] = counts.get(("signature", dtype), 0) + rej
    capsys.readouterr()
    print({f"{k[0]} {k[1]}": f"{v} of {len(lo.WIDTHS)} widths rejected" for k, v in counts.items()})
    assert not missed, f"uncentred variance accepted on fp16 rows far from zero at C = {missed}"


def flat_row(C, dtype):
    """A row of near-zero variance: 2^-6 everywhere, one element 2^-13 higher (both formats hold it): the variance is
    below 2^-26, far under eps = 1e-6."""
    row = torch.full((C,), 2.0 ** -6, dtype=torch.float64)
    row[C // 2] += 2.0 ** -13
    assert torch.equal(row.to(dtype).double(), row)
    return row.to(dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("mutant", ["eps_missing", "eps_after_sqrt"])
def test_eps_in_the_wrong_place_is_rejected_at_every_width(mutant, dtype, capsys):
    """eps left out, or added after the square root: invisible on rows of variance 1 or more, rejected on a row whose
    variance is far below eps (the signature rows plus one such row; the honest evaluation of them is accepted, with
    the condition on the inputs)."""
    missed = []
    for C in lo.WIDTHS:
        x, w, b = _inputs(C, dtype)
        x[0] = flat_row(C, dtype)
        lo.check(ln32(x, w, b), x, w, b, EPS, R=4, signature=True, label=f"with a flat row, C={C}")
        if not rejected(ln32(x, w, b, mutant=mutant), x, w, b):
            missed.append(C)
    capsys.readouterr()
    assert not missed, f"{mutant} accepted at C = {missed}"


def test_unbiased_variance_is_rejected_where_it_exceeds_a_rounding(capsys):
    """Divisor C - 1: the result grows by 1 / (2 C).  That is above the unit roundoff for C <= 64 in fp16 (2^-7 against
    2^-11) and C <= 16 in bf16 (2^-5 against 2^-8), and must be rejected there.  Above, it is at most a fraction of one
    rounding and is only caught where an element sits next to a rounding boundary; the count is printed, not
    asserted."""
    must, extra = [], {}
    for dtype, limit in ((torch.float16, 64), (torch.bfloat16, 16)):
        for C in lo.WIDTHS:
            x, w, b = _inputs(C, dtype)
            rej = rejected(ln32(x, w, b, mutant="var_unbiased"), x, w, b)
            if C <= limit and not rej:
                must.append((dtype, C))
            if C > limit:
                extra[dtype] = extra.get(dtype, 0) + rej
    capsys.readouterr()
    print({str(k): f"{v} widths above the limit rejected as well" for k, v in extra.items()})
    assert not must, f"divisor C - 1 accepted at {must}"


TABLE_MUTANTS = ["mean_drops_chunk", "var_drops_chunk", "mean_counts_chunk_twice", "neighbour_stats", "neighbour_mean",
                 "neighbour_rstd", "weight_from_next_column", "bias_from_next_column", "var_unbiased", "truncated"]


def old_criterion_accepts(y, x, w, b, dtype):
    """tests/test_hip_parity.py's LayerNorm assertion: |y - ref| / max(|ref|, 1) <= two unit roundoffs, against the
    framework's fp32 LayerNorm."""
    ref = torch.nn.functional.layer_norm(x.to(F32), (x.shape[-1],), w.to(F32), b.to(F32), EPS)
    tol = 2.0 ** -7 if dtype == torch.bfloat16 else 2.0 ** -10
    return float(((y.to(F32) - ref).abs() / ref.abs().clamp(min=1.0)).max()) <= tol


def test_old_criterion_next_to_the_oracle(capsys):
    """What the earlier criterion (relative to max(|ref|, 1), two unit roundoffs, N(0,1) rows) does with each mutant at
    C = 400, 768, 1024, next to `check` on the signature rows.  Only `check` is asserted.  As printed by this test
    ('old' = the old criterion ACCEPTS the mutant at that width, '-' = rejects; `check` rejects all of them):

        mutant                      bf16 400  768  1024   fp16 400  768  1024
        mean_drops_chunk                 -    -    -           -    -    -
        var_drops_chunk                  -    -    -           -    -    -
        mean_counts_chunk_twice          -    -    -           -    -    -
        neighbour_stats                  -    -    -           -    -    -
        neighbour_mean                   -    -    -           -    -    -
        neighbour_rstd                   -    -    -           -    -    -
        weight_from_next_column          -    -    -           -    -    -
        bias_from_next_column            -    -    -           -    -    -
        var_unbiased                     old  old  old         -    -    -
        truncated                        old  old  old         old  old  old

    So on these draws the old criterion caught every chunk slip, the finer neighbour forms included, and let through
    the two that stay under two unit roundoffs: the divisor C - 1 in bf16 and truncation in both formats.
    On N(0,1) rows the neighbour's mean differs by about 1 / sqrt(C) and its rstd by about 1 / sqrt(2 C) of the
    row's own, close to the old allowance, so whether it catches them depends on the draw; on the signature rows they
    move the chunk by 8 s or more."""
    lines = []
    for mutant in TABLE_MUTANTS:
        cells = []
        for dtype in DTYPES:
            for C in (400, 768, 1024):
                w, b = lo.affine(C, dtype, 7 + C)
                xn = torch.randn((ROWS, C), generator=torch.Generator().manual_seed(C), dtype=torch.float64).to(dtype)
                assert old_criterion_accepts(ln32(xn, w, b), xn, w, b, dtype)
                old = old_criterion_accepts(ln32(xn, w, b, mutant=mutant), xn, w, b, dtype)
                xs, _, _ = _inputs(C, dtype)
                assert rejected(ln32(xs, w, b, mutant=mutant), xs, w, b), (mutant, dtype, C)
                cells.append("old" if old else "-")
        lines.append(f"{mutant:28s}" + " ".join(f"{c:4s}" for c in cells))
    capsys.readouterr()
    print("\n".join(lines))


def test_forms_and_generators_are_what_the_gpu_tests_assume():
    """expected_form over the widths: the add entries only ever run three chunks per lane (R 4, 3, 2, 1 as the row
    grows), the merge entries three with an addend and six without (R 4 or 3); the signature classes keep four
    consecutive rows 8 max(s) apart, in both signs."""
    for entry in lo.ENTRIES:
        want = {(3, 4), (3, 3), (3, 2), (3, 1)}
        if entry.startswith("merge"):
            want |= {(6, 4), (6, 3)}
        assert lo.forms_that_exist(entry) == want, entry
    assert lo.expected_form("add_layernorm", 400) == (3, 3, False)
    assert lo.expected_form("add_layernorm", 520) == (3, 2, False)
    assert lo.expected_form("add_layernorm", 776) == (3, 1, False)
    assert lo.expected_form("merge_wavg_ln", 768, False, 392, 16) == (6, 4, False)
    assert lo.expected_form("merge_wavg_ln", 776, False, 196, 32) == (6, 3, True)
    assert lo.expected_form("merge_wavg_ln", 768, True, 197, 16) == (3, 2, False)
    assert lo.boundary_inside_iteration(512, 3) is False and lo.boundary_inside_iteration(400, 3) is True
    for sign in (1, -1):
        for dtype in DTYPES:
            x = lo.signature_rows((37, 64), dtype, 9, sign)
            lo.assert_rows_in_a_wave_differ(x, 37)
            k, sg = lo.row_class(x)
            assert torch.equal(k, torch.arange(37) % 8) and bool((sg == sign).all())

"""bench.py's command line and its --dump-outputs writer, without a GPU: a plain run switches every measurement but the
headline off, --full switches them back on (each still with its --no-* switch), and the dump is float32 / float64,
exact, and bounded by a fixed, seeded row sample."""
import numpy as np
import pytest
import torch

import bench


def test_plain_run_measures_the_headline_only():
    args = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (args.steps, args.warmup, args.full, args.dump_outputs) == (7, 2, False, None)
    assert args.no_roofline and args.no_also and args.no_cpu_baseline


def test_full_run_measures_everything_it_did_before():
    args = bench.parse(["--full"])
    assert args.full and not (args.no_roofline or args.no_also or args.no_cpu_baseline)
    args = bench.parse(["--full", "--no-also", "--no-cpu-baseline"])
    assert args.no_also and args.no_cpu_baseline and not args.no_roofline


@pytest.mark.parametrize("argv", [["--steps", "0"], ["--warmup", "-1"]])
def test_step_counts_are_checked(argv):
    with pytest.raises(SystemExit):
        bench.parse(argv)


def test_dump_outputs_writes_exact_float_arrays(tmp_path):
    g = torch.Generator().manual_seed(3)
    logits = torch.randn(6, 400, generator=g).bfloat16()
    counts = torch.tensor([2, 5, 6], dtype=torch.int64)
    bench.dump_outputs(str(tmp_path / "out"), {"logits": logits, "topk_counts": counts})
    got = np.load(tmp_path / "out" / "logits.npy")
    assert got.dtype == np.float32 and np.array_equal(got, logits.float().numpy())
    got = np.load(tmp_path / "out" / "topk_counts.npy")
    assert got.dtype == np.float64 and got.tolist() == [2.0, 5.0, 6.0]


def test_dump_outputs_samples_what_is_too_large(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 2 * 40 * 400 * 4)
    big = torch.arange(100 * 400, dtype=torch.float32).reshape(100, 400)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"logits": big, "topk_counts": torch.zeros(3, dtype=torch.int64)})
    a, b = np.load(tmp_path / "a" / "logits.npy"), np.load(tmp_path / "b" / "logits.npy")
    assert a.shape == (40, 400) and np.array_equal(a, b)  # the same rows every time
    rows = a[:, 0] / 400
    assert np.all(np.diff(rows) > 0) and np.array_equal(a, big.numpy()[rows.astype(int)])

"""tests/golden/models_*.npz and the sections of tests/golden/manifest.json that name them must agree: the model tests
are parametrised over the manifest, so a fixture file that no entry names is committed and never run (two drop fixtures
were lost this way by a partial regeneration), and an entry without its file fails only on the GPU.  Checked here without
one: every file is named by exactly one entry of `models` / `modes` / `full` / `config0`, every entry has its file, every
`certified` is true, and each file holds the arrays that the test of its section reads."""
import glob
import os

import numpy as np
import pytest

import golden_io as G

SECTIONS = ("models", "modes", "full", "config0")


def _entries():
    man = G.manifest()
    out = []
    for section in SECTIONS:
        got = man.get(section, [])
        out += [(section, m) for m in ([got] if isinstance(got, dict) else got)]
    return out


def _files():
    return sorted(os.path.basename(p)[len("models_"):-len(".npz")] for p in glob.glob(os.path.join(G.GOLDEN, "models_*.npz")))


def test_every_model_fixture_file_is_named_by_exactly_one_entry():
    named = [m["name"] for _, m in _entries()]
    files = _files()
    assert files, "no model fixtures found"
    orphans = [f for f in files if named.count(f) == 0]
    twice = sorted({n for n in named if named.count(n) > 1})
    missing = [n for n in named if n not in files]
    assert not orphans, f"fixture files that no manifest entry names (no test runs them): {orphans}"
    assert not twice, f"fixtures named by more than one manifest entry: {twice}"
    assert not missing, f"manifest entries without their models_<name>.npz: {missing}"


def test_the_mode_fixtures_cover_drop_and_hybrid_of_every_family():
    got = sorted((m["host"], m["mode"]) for s, m in _entries() if s == "modes")
    want = sorted((h, mode) for h in ("videomae", "timesformer", "motionformer", "vivit") for mode in ("drop", "hybrid"))
    assert got == want


def test_the_vivit_fixtures_are_the_seven_of_the_reference_patch():
    """ViViT's fixtures (tome/patch/vivit.py of the reference over tests/golden/vivit_tree.py): head dim 16, head dim 64
    with proportional attention off / on, the duplicate patch, `concat`, drop and hybrid -- each over 65 tokens (a
    class token in front of 4 x 4 x 4 tubelets), and each records that the matching protected row 0: `unm` starts with
    row 0 and is sorted, no source is row 0."""
    got = sorted(m["name"] for _, m in _entries() if m["host"] == "vivit")
    assert got == sorted(["vivit_prop1", "vivit_hd64_prop0", "vivit_hd64_prop1", "vivit_hd64_dup", "vivit_hd64_concat",
                          "vivit_hd64_drop", "vivit_hd64_hybrid"])
    for _, meta in _entries():
        if meta["host"] != "vivit":
            continue
        assert meta["tokens"][0] == 65 and all(t % 5 == 0 for t in meta["tokens"]) and meta["certified"] is True
        assert {"embed_dim", "num_heads", "depth"} <= set(meta["cfg"])
        z = np.load(os.path.join(G.GOLDEN, f"models_{meta['name']}.npz"))
        for i in range(len(meta["tokens"])):
            src, unm = z[f"L{i}_src"].astype(np.int64), z[f"L{i}_unm"].astype(np.int64)
            assert (src != 0).all() and (unm[:, 0] == 0).all() and (np.diff(unm, axis=1) > 0).all(), (meta["name"], i)
        if meta["cfg"]["embed_dim"] // meta["cfg"]["num_heads"] == 64 and "mode" not in meta:
            assert meta["l0_set_gap"] > 1e-2


@pytest.mark.parametrize("section,meta", _entries(), ids=lambda v: v["name"] if isinstance(v, dict) else v)
def test_entry_is_certified_and_its_file_holds_what_its_test_reads(section, meta):
    if "certified" in meta:
        assert meta["certified"] is True, "margins below the generator's tau: re-seed the fixture"
    path = os.path.join(G.GOLDEN, f"models_{meta['name']}.npz")
    assert os.path.exists(path), path
    z = np.load(path)
    layers = len(meta["tokens"])
    assert len(meta["r_eff"]) == layers and len(meta["seeds"]) == meta["clip_shape"][0]
    want = {"logits", "size"}
    if section in ("models", "modes"):
        want |= {f"L{i}_{k}" for i in range(layers) for k in ("src", "unm")}
    if section == "models" or meta.get("mode") == "hybrid":
        want |= {f"L{i}_dst" for i in range(layers)}
    if section == "modes":
        want |= {"source"}
        assert meta["mode"] in ("drop", "hybrid") and "size_dtype" in meta
        if meta["mode"] == "hybrid":
            want |= {f"L{i}_keep" for i in range(layers)}
            assert "threshold" in meta
    if section == "full":
        want |= {f"P{i}" for i in range(layers)}
        want |= {"L0_src", "L0_dst", "L0_unm", "L0_set_ok", "L0_src_ok", "L0_dst_ok", "L0_unm_ok", "L0_group_ok"}
    if section == "config0":
        want |= {"partitions", "L0_src", "L0_dst", "L0_unm", "L0_unm_certified"}
    lacking = sorted(want - set(z.files))
    assert not lacking, f"models_{meta['name']}.npz lacks {lacking}"
    assert z["logits"].shape[0] == meta["clip_shape"][0]
    for i in range(layers):  # one row of indices per group, r_eff sources, the rest unmerged (halves of the tokens)
        if section in ("models", "modes"):
            assert z[f"L{i}_src"].shape == (meta["groups"][i], meta["r_eff"][i]), i
            assert z[f"L{i}_unm"].shape == (meta["groups"][i], (meta["tokens"][i] + 1) // 2 - meta["r_eff"][i]), i
        if f"L{i}_keep" in want:
            assert z[f"L{i}_keep"].shape == z[f"L{i}_src"].shape, i
    if section == "config0":
        assert z["partitions"].shape[0] == layers
    if section == "full":
        assert all(z[f"P{i}"].shape == z["P0"].shape for i in range(layers))


def _has_spread(section, meta):
    return section != "models" or meta["cfg"]["embed_dim"] // meta["cfg"]["num_heads"] == 64


@pytest.mark.parametrize("section,meta", [e for e in _entries() if _has_spread(*e)],
                         ids=lambda v: v["name"] if isinstance(v, dict) else v)
def test_entry_records_the_spread_of_the_reference(section, meta):
    """`ref_spread` (generate_models.py --spread): the yardstick of the model tests' R1 - R3.  Logit errors are positive
    and the 16-bit one is the larger; per-layer agreement exactly where the fixture stores partitions."""
    spread = meta.get("ref_spread")
    assert spread, "no ref_spread: run tests/golden/generate_models.py --spread " + meta["name"]
    for key in ("fp64", "bf16"):
        assert 0.0 < spread[key]["logit_err"] < float("inf")
        if section in ("full", "config0"):
            agree = spread[key]["agree"]
            assert len(agree) == len(meta["tokens"]) and all(0.0 <= a <= 1.0 for a in agree)
            if key == "fp64":  # layer 0 of these fixtures is certified two orders above what fp32 evaluation moves
                assert agree[0] == 1.0
        else:
            assert "agree" not in spread[key]
    assert spread["fp64"]["logit_err"] < spread["bf16"]["logit_err"]

"""tools/update_measured.py on temporary files: tests/golden/measured.json is the build-to-build regression guard of the
model tests (a run is held to 1.5x the stored error and to the stored agreement minus 2 points), so folding a worse run
into it raises the guard's own tolerance.  Without --accept the tool must refuse such a fold and write nothing."""
import json
import os
import sys

TOOLS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
if TOOLS not in sys.path:
    sys.path.insert(0, TOOLS)

import update_measured as U  # noqa: E402

STORED = {"fx": {"agree": [1.0, 0.90, 0.80], "bf16_logit_err": 0.04, "fp32_logit_err": 0.01, "runs": 3}}


def _run(tmp_path, seen, *flags):
    out, src = tmp_path / "measured.json", tmp_path / "seen.json"
    if not out.exists():
        out.write_text(json.dumps(STORED))
    src.write_text(json.dumps(seen))
    before = out.read_text()
    code = U.main([*flags, "--out", str(out), str(src)])
    return code, before, out.read_text()


def test_a_run_inside_the_head_room_is_folded_with_max_and_min(tmp_path):
    seen = {"fx": {"agree": [1.0, 0.885, 0.85], "bf16_logit_err": 0.04 * 1.25, "fp32_logit_err": 0.005},
            "new": {"bf16_logit_err": 0.5}}
    code, _, after = _run(tmp_path, seen)
    assert code == 0
    got = json.loads(after)
    assert got["fx"] == {"agree": [1.0, 0.885, 0.80], "bf16_logit_err": 0.04 * 1.25, "fp32_logit_err": 0.01, "runs": 4}
    assert got["new"] == {"bf16_logit_err": 0.5, "runs": 1}  # (a fixture without a record has nothing to regress from)


def test_a_larger_error_is_refused_and_nothing_is_written(tmp_path, capsys):
    code, before, after = _run(tmp_path, {"fx": {"bf16_logit_err": 0.0501}})
    assert code == 1 and after == before
    said = capsys.readouterr().out
    assert "NOT written" in said and "fx: bf16_logit_err" in said and "--accept" in said


def test_a_lower_agreement_is_refused_and_nothing_is_written(tmp_path, capsys):
    code, before, after = _run(tmp_path, {"fx": {"agree": [1.0, 0.90, 0.779], "fp32_logit_err": 0.01}})
    assert code == 1 and after == before
    assert "fx: agree[2]" in capsys.readouterr().out


def test_one_refused_value_holds_back_the_whole_fold(tmp_path):
    code, before, after = _run(tmp_path, {"fx": {"fp32_logit_err": 0.02}, "new": {"bf16_logit_err": 0.5}})
    assert code == 1 and after == before and "new" not in json.loads(after)


def test_accept_records_the_regression(tmp_path):
    code, _, after = _run(tmp_path, {"fx": {"agree": [1.0, 0.5, 0.8], "bf16_logit_err": 0.4}}, "--accept")
    assert code == 0
    got = json.loads(after)["fx"]
    assert got["bf16_logit_err"] == 0.4 and got["agree"] == [1.0, 0.5, 0.8] and got["runs"] == 4


def test_the_tracked_file_is_the_default_target():
    assert os.path.normpath(U.OUT).endswith(os.path.join("tests", "golden", "measured.json"))

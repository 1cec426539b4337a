#!/usr/bin/env python3
"""Fold what GPU runs of the model tests measured (TOME_RECORD_MEASURED=1 -> gpurun_out/measured_seen.json) into the
tracked tests/golden/measured.json: per fixture the LARGEST logit errors and the SMALLEST per-layer group agreement seen
over all folded runs.  The tests hold a run to 1.5x / minus 2 points of these -- a guard against a change between two
builds, not a statement of what error is acceptable (that is `ref_spread` in tests/golden/manifest.json, which this tool
never touches).  A fold would raise the guard's own tolerance, so one that raises a stored error by more than 1.25x or
lowers a stored agreement by more than 2 points is refused, and nothing is written, unless --accept says that the
regression has been looked at.
    python tools/update_measured.py [--accept] [--out FILE] measured_seen.json [more ...]"""
import argparse
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "measured.json")
MAX_ERR_RATIO = 1.25
MAX_AGREE_DROP = 0.02


def fold(cur, seen, accept=False):
    """Folds one run's values into `cur` in place; returns the refused changes as strings (none under `accept`)."""
    refused = []
    for name, vals in seen.items():
        rec = cur.setdefault(name, {})
        for k, v in vals.items():
            if k == "agree":
                old = rec.get(k)
                if old is None or len(old) != len(v):
                    rec[k] = v
                    continue
                refused += [f"{name}: agree[{i}] {a:.4f} -> {b:.4f}" for i, (a, b) in enumerate(zip(old, v))
                            if a - b > MAX_AGREE_DROP]
                rec[k] = [min(a, b) for a, b in zip(old, v)]
            else:
                old = rec.get(k)
                if old is not None and v > MAX_ERR_RATIO * old:
                    refused.append(f"{name}: {k} {old:.4e} -> {v:.4e} ({v / old:.2f}x)" if old > 0 else
                                   f"{name}: {k} {old:.4e} -> {v:.4e}")
                rec[k] = v if old is None else max(old, v)
        rec["runs"] = rec.get("runs", 0) + 1
    return [] if accept else refused


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--accept", action="store_true", help="record a run that is worse than the stored values by more "
                    f"than {MAX_ERR_RATIO}x in an error or {MAX_AGREE_DROP:.2f} in an agreement")
    ap.add_argument("--out", default=OUT, help="the file to fold into (default: the tracked one)")
    ap.add_argument("paths", nargs="+", help="measured_seen.json of one or more recorded runs")
    args = ap.parse_args(argv)
    cur = json.load(open(args.out)) if os.path.exists(args.out) else {}
    refused = []
    for p in args.paths:
        refused += fold(cur, json.load(open(p)), args.accept)
    if refused:
        print(f"{args.out}: NOT written.  This run is worse than the record beyond the guard's own head-room:")
        for line in refused:
            print("  " + line)
        print("Find out why first; --accept records it once that is understood.")
        return 1
    with open(args.out, "w") as f:
        json.dump(cur, f, indent=1, sort_keys=True)
    print(f"{args.out}: {len(cur)} fixtures")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())

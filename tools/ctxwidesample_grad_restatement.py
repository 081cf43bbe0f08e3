#!/usr/bin/env python3
"""The float32 restatement of the sampling-direction walk (tests/ctxsample_restatement.py, from a float32 z) over the cases
of tests/ctxwidesample_restatement.py against float64 autograd through the oracle, on the CPU (no GPU needed): per case
the larger of the whole and the per-context-row error of each gradient, the worst per group, and the bar each group takes
in the tests -- BAR_P / BAR_Z of tests/domain_helpers.py, or 4 x the restatement's error where that alone exceeds a
quarter of the bar.  Writes --out (default profiles/r23_ctxwidesample_grad_errors.json)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
import flow_oracle as orc  # noqa: E402
import ctxwidesample_restatement as R  # noqa: E402
from domain_helpers import BAR_P, BAR_Z  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r23_ctxwidesample_grad_errors.json"))
args = ap.parse_args()

out = {"bars": {"params": BAR_P, "omega": BAR_Z}, "cases": {}, "groups": {}}
for group, cases in R.groups().items():
    worst = {"params": 0.0, "omega": 0.0}
    for c in cases:
        e = R.restatement_errors(orc, c)
        out["cases"][R.case_id(c)] = e
        worst = {k: max(worst[k], e[k]) for k in worst}
        print(group, R.case_id(c), e, flush=True)
    out["groups"][group] = {"restatement": worst, "bar": {k: R.group_bar(out["bars"][k], worst[k]) for k in worst}}
with open(args.out, "w") as f:
    json.dump(out, f, indent=1, sort_keys=True)
    f.write("\n")
print(json.dumps(out["groups"], indent=1, sort_keys=True))

#!/usr/bin/env python3
"""Records tests/golden/rollout_forms.json: the kernel_counts() delta of one rollout for every case of tests/test_rollout_forms.py.

Run ONCE on the GPU, on a build of the commit whose form selection is the reference (the table pins it for every later change):

    python tools/record_rollout_forms.py --commit $(git rev-parse HEAD) [--out tests/golden/rollout_forms.json]

The table is the reference's behaviour, not this tree's: re-record it only with a change that moves a handle to another form on purpose."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="full hash of the commit the loaded library was built from")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "rollout_forms.json"))
    args = ap.parse_args()
    assert len(args.commit) == 40, "--commit takes the full 40-character hash"
    from tests import test_rollout_forms as F

    def delenv(s):
        os.environ.pop(s, None)

    table = {"parent": args.commit, "T": F.T, "cases": {}}
    for name in sorted(F.ALL_CASES):
        F.set_switches(F.ALL_CASES[name], os.environ.__setitem__, delenv)
        table["cases"][name], _ = F.run_case(F.ALL_CASES[name])
        print(name, table["cases"][name], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()

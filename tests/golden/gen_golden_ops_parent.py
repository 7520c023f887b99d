"""Records tests/golden/ops_parent.json: the outputs of the operator-level API (tests/ops_parent_cases.py) at one commit, as
SHA-256 digests.  Run on the MI355X at the commit whose behaviour is to be pinned -- the parent of a change that must not
move a bit -- with the library built:

    python tests/golden/gen_golden_ops_parent.py [output.json]

The digests hold for the toolchain and GPU they were recorded on (both are written into the file)."""
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "yolo-compression-and-deployment-in-fpga_amd"), ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import ops_parent_cases as P  # noqa: E402


def main():
    import torch
    commit = os.environ.get("Y355_GOLDEN_COMMIT")
    if not commit:
        commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], text=True).strip()
    rec = {"commit": commit, "rocm": torch.version.hip, "gpu": torch.cuda.get_device_name(0), "cases": {}}
    for cid, fn in P.CASES:
        res = fn()
        for k, v in res.items():
            if k.startswith("none_"):
                assert v is None, (cid, k, "should have been declined")
                continue
            assert v is not None, (cid, k, "a forward_i8 that has to succeed returned None")
            if isinstance(v, np.ndarray):
                assert v.size > 1 and (v != v.flat[0]).any(), (cid, k, "constant array: a vacuous digest")
        if cid == "i8_fused":                                    # some outputs saturate, not all
            for c in ("c3", "c40"):
                assert 0 < res[c + "_saturated"] < res[c].size, (c, res[c + "_saturated"])
        rec["cases"][cid] = P.summarise(res)
        print(cid, "ok:", ", ".join(sorted(res)))
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "ops_parent.json")
    with open(out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    main()

"""
Record tests/golden/layered_parent.npz: what the layered entry points compute, launch and allocate for the cases of
tests/rgf_parent_cases.py.  The record is the yardstick of tests/test_rgf_parent_gpu.py (bit for bit), so it is taken
ONCE, on the GPU, from a build of the commit BEFORE a change to the orchestration of the recursion:

    NEGF_LIB_PATH=/path/to/parent/libnegf_hip.so python scripts/gen_layered_parent_fixture.py [out.npz]

It holds `keys` with one SHA-256 digest each (`sha`), and under `full:<key>` the arrays of the smallest case and every
integer item (info, launch counts, workspace bytes).
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import rgf_parent_cases as pc  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "layered_parent.npz")
    from gaunegf_amd import _lib
    from gaunegf_amd.engine import get_engine
    print("library:", _lib.LIB_PATH)
    eng = get_engine()
    items = {}
    for group in pc.GROUPS:
        got = pc.RUNNERS[group](eng)
        print(f"{group}: {len(got)} items")
        items.update(got)
    keys = sorted(items)
    rec = {"keys": np.array(keys), "sha": np.array([pc.digest(items[k]) for k in keys])}
    for k in keys:
        if pc.kept_in_full(k, items[k]):
            rec["full:" + k] = items[k]
    print("launches per family", pc.FAMILIES, "\n", items["counts/d"], "\nworkspace bytes", items["workspace/b"])
    np.savez_compressed(out, **rec)
    print("wrote", out, os.path.getsize(out), "bytes,", len(keys), "items,", len(rec) - 2, "in full")


if __name__ == "__main__":
    main()

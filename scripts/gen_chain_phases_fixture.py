"""
Record tests/golden/chain_phases_parent.npz: what the 1-D chain fixed-point kernel computes for the cases of
tests/chain_phases_cases.py.  The record is the yardstick of tests/test_chain_phases_gpu.py (bit for bit), so it is
taken ONCE, on the GPU, from a build of the commit BEFORE a change to the kernel:

    NEGF_LIB_PATH=/path/to/parent/libnegf_hip.so python scripts/gen_chain_phases_fixture.py [out.npz]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import chain_phases_cases as cs  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "chain_phases_parent.npz")
    from gaunegf_amd import _lib
    from gaunegf_amd.engine import get_engine
    print("library:", _lib.LIB_PATH)
    eng = get_engine()
    eng.set_chain_cache(0)                          # every evaluation runs its fixed points
    eng.set_chain_round_robin(-1, 0)
    rec = {}
    for ncL, ncR in cs.sizes():
        for fi in cs.FORCE:
            blk, its, cv = cs.run_fixed(ncL, ncR, fi)
            k = cs.key_fixed(ncL, ncR, fi)
            rec[k + "_sha"] = cs.digests(blk); rec[k + "_it"] = its; rec[k + "_cv"] = cv
            if (ncL, ncR, fi) in cs.FULL_FIXED:
                for m, row in enumerate(blk):
                    for c, b in enumerate(row):
                        rec[f"{k}_blk_{m}_{c}"] = b
    blk, its, cv = cs.run_free()
    rec["free_sha"] = cs.digests(blk); rec["free_it"] = its; rec["free_cv"] = cv
    capped = [m for m in range(len(blk)) if (cv[m] == 0).any()]
    stopped = [m for m in range(len(blk)) if (cv[m] == 1).any()]
    print("free-running sweep counts:\n", its, "\nflags:\n", cv)
    assert capped and stopped, "the free-running grid needs units that stop on the test and units that reach the cap"
    both = [m for m in stopped if m in capped]       # one energy with both kinds of unit, else one of each
    full = np.array(both[-1:]) if both else np.unique([stopped[-1], capped[0]])
    rec["free_full"] = full
    for m in full:
        for c in (0, 1):
            rec[f"free_blk_{m}_{c}"] = blk[m][c]
    np.savez(out, **rec)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()

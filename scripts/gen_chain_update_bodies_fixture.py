"""
Record tests/golden/chain_update_bodies_parent.npz: what the 1-D chain fixed-point kernel computes for the cases of
tests/chain_update_bodies_cases.py (a singular column in the first, a middle and the last panel, a pivot permutation that is
not the identity in any panel, leads scaled by 2^+-64; plain and round robin).  The record is the yardstick of
tests/test_chain_update_bodies_gpu.py (bit for bit, NaN positions included), so it is taken ONCE, on the GPU, from a build
of the commit BEFORE a change to the update bodies of the stage schedule:

    NEGF_LIB_PATH=/path/to/parent/libnegf_hip.so python scripts/gen_chain_update_bodies_fixture.py [out.npz]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import chain_update_bodies_cases as cs  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "chain_update_bodies_parent.npz")
    from gaunegf_amd import _lib
    from gaunegf_amd.engine import get_engine
    print("library:", _lib.LIB_PATH)
    eng = get_engine()
    eng.set_chain_cache(0)                          # every evaluation runs its fixed points
    rec = {}
    for ncL, ncR, fi, kind, mode in cs.cases():
        blk, its, cv = cs.run(eng, ncL, ncR, fi, kind, mode)
        k = cs.key(ncL, ncR, kind, mode)
        rec[k + "_sha"] = cs.digests(blk); rec[k + "_it"] = its; rec[k + "_cv"] = cv; rec[k + "_fin"] = cs.finite(blk)
        print(k, "sweeps", its.tolist(), "flags", cv.tolist(), "finite", rec[k + "_fin"].astype(int).tolist())
    eng.set_chain_round_robin(-1, 0)
    np.savez_compressed(out, **rec)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()

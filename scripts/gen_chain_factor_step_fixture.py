"""
Record tests/golden/chain_factor_step_parent.npz: what the 1-D chain fixed-point kernel computes for the cases of
tests/chain_factor_step_cases.py (pivot ties, a zero column, NaN / Inf in a pivot row, leads scaled by 2^+-64).  The
record is the yardstick of tests/test_chain_factor_step_gpu.py (bit for bit, NaN positions included), so it is taken
ONCE, on the GPU, from a build of the commit BEFORE a change to the column step:

    NEGF_LIB_PATH=/path/to/parent/libnegf_hip.so python scripts/gen_chain_factor_step_fixture.py [out.npz]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import chain_factor_step_cases as cs  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "chain_factor_step_parent.npz")
    from gaunegf_amd import _lib
    from gaunegf_amd.engine import get_engine
    print("library:", _lib.LIB_PATH)
    eng = get_engine()
    eng.set_chain_cache(0)                          # every evaluation runs its fixed points
    eng.set_chain_round_robin(-1, 0)
    rec = {}
    for ncL, ncR, fi, kind in cs.cases():
        blk, its, cv = cs.run(ncL, ncR, fi, kind)
        k = cs.key(ncL, ncR, kind)
        rec[k + "_sha"] = cs.digests(blk); rec[k + "_it"] = its; rec[k + "_cv"] = cv
        nonfinite = sum(int((~np.isfinite(b.view(np.float64))).sum()) for row in blk for b in row)
        print(k, "sweeps", its.tolist(), "flags", cv.tolist(), "non-finite values", nonfinite)
        if (ncL, ncR) in cs.FULL:
            for m, row in enumerate(blk):
                for c, b in enumerate(row):
                    rec[f"{k}_blk_{m}_{c}"] = b
    np.savez_compressed(out, **rec)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()

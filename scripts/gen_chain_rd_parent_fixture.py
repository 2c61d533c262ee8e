"""
Record tests/golden/chain_rd_parent.npz: what the renormalisation-decimation kernel (k_chain1d_rd.hip) computes for the
cases of tests/test_chain_rd_parent_gpu.py -- free-running decimations at the default tolerance, both sides of every
pitch class.  The record is that test's yardstick (bit for bit), so it is taken ONCE, on the GPU, from a build of the
commit BEFORE the shared inverse (chain_rs_inverse.h) was restructured:

    NEGF_LIB_PATH=/path/to/parent/libnegf_hip.so python scripts/gen_chain_rd_parent_fixture.py [out.npz]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import chain_phases_cases as cs  # noqa: E402
import test_chain_rd_parent_gpu as rp  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else rp.GOLDEN
    from gaunegf_amd import _lib
    from gaunegf_amd.engine import get_engine
    print("library:", _lib.LIB_PATH)
    get_engine().set_chain_cache(0)                 # every evaluation runs its decimation steps
    rec = {}
    for ncL, ncR in rp.SIZES:
        blk, its, cv = rp.run(ncL, ncR)
        k = rp.key(ncL, ncR)
        rec[k + "_sha"] = cs.digests(blk); rec[k + "_it"] = its; rec[k + "_cv"] = cv
        print(k, "steps", its.ravel().tolist(), "flags", cv.ravel().tolist())
    np.savez(out, **rec)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()

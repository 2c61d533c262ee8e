"""
Record tests/golden/chain_lazy_stop_parent.npz: what the 1-D chain fixed-point kernel computes for the cases of
tests/chain_lazy_stop_cases.py -- free-running fixed points that stop on the test, at three tolerances.  The record is
the yardstick of tests/test_chain_lazy_stop_gpu.py (bit for bit), so it is taken ONCE, on the GPU, from a build of the
commit BEFORE the stopping test was changed:

    NEGF_LIB_PATH=/path/to/parent/libnegf_hip.so python scripts/gen_chain_lazy_stop_fixture.py [out.npz]

Two conditions on the cases are checked on the CPU (the numpy oracle's iterates, the lane map of
gaunegf_amd/csrc/chain_mix_map.h) and asserted before anything is recorded (--check-only: nothing else, no GPU):
  (i)  in at least one case some sweep has a wave whose slot-0 elements all pass the test while another element of the
       workgroup fails it: that wave must run the full test, and the launch must go on;
  (ii) at least one unit of every size class stops on the test below the sweep cap.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import chain_lazy_stop_cases as lz  # noqa: E402
import chain_phases_cases as cs  # noqa: E402
from oracle.negf_oracle import inv  # noqa: E402

LANES, WAVE = 256, 64                               # RS_MIX_LANES, lanes of a wave


def mix_map(n):
    """rs_mix_map of chain_mix_map.h: (row groups, slots per lane); lane t < rg n holds the elements s rg n + t"""
    rg = min(LANES // n, 64)
    return rg, (n + rg - 1) // rg


def oracle_sweeps(E, lead, conv, relFactor=0.1):
    """the reference's fixed point (oracle.chain1d_g), yielding per sweep the elements' test results (True = passes)"""
    alpha, Salpha, beta, Sbeta = lead
    z = E + 1j * cs.ETA
    A = z * Salpha - alpha
    B = z * Sbeta - beta
    Bd = B.conj().T
    g = inv(A)
    for count in range(1, lz.MAX_ITER + 1):
        g_new = inv(A - B @ g @ Bd)
        ok = np.abs(g_new - g) ** 2 <= conv * conv * np.maximum(np.abs(g_new) ** 2, 1e-24)
        g = g_new * relFactor + g * (1 - relFactor)
        yield count, ok
        if ok.all():
            return


def mixed_sweep(n, ok):
    """a wave whose slot-0 elements all pass while another element of the workgroup fails?"""
    if ok.all():
        return False
    rg, _ = mix_map(n)
    flat = ok.ravel()[: rg * n]                     # slot 0: elements t of the lanes t < rg n
    return any(flat[w:w + WAVE].all() for w in range(0, rg * n, WAVE))


def check_conditions():
    # (ii) per size class, cheapest first: the energy off the axis at the loosest tolerance
    for ncL, ncR in lz.SIZES:
        lead = lz.leads(ncL, ncR)[0]
        stopped = None
        for ci, conv in enumerate(lz.CONVS):
            for E in (lz.ES[1], lz.ES[0], lz.ES[2], lz.ES[3]):
                last = 0
                for last, ok in oracle_sweeps(E, lead, conv):
                    pass
                if ok.all() and last < lz.MAX_ITER:
                    stopped = (ci, E, last)
                    break
            if stopped:
                break
        assert stopped, f"(ii) no unit of size class {ncL} stops on the test below the cap"
        print(f"(ii) n_c = {ncL}: conv {lz.CONVS[stopped[0]]:g}, E = {stopped[1]}: stops after {stopped[2]} sweeps")
    # (i) any case
    for ncL, ncR in lz.SIZES:
        for c, n in enumerate((ncL, ncR)):
            if mix_map(n)[1] < 2:
                continue                            # (one slot per lane: slot 0 is the whole test)
            lead = lz.leads(ncL, ncR)[c]
            for ci, conv in enumerate(lz.CONVS):
                for E in lz.ES:
                    for count, ok in oracle_sweeps(E, lead, conv):
                        if mixed_sweep(n, ok):
                            print(f"(i) sizes ({ncL}, {ncR}), contact {c}, conv {conv:g}, E = {E}: sweep {count} has a wave that passes "
                                  f"on slot 0 while {int((~ok).sum())} elements fail")
                            return
    raise AssertionError("(i) no case has a sweep with a wave that passes on slot 0 while another element fails")


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    check_conditions()
    if "--check-only" in sys.argv:
        return
    out = args[0] if args else os.path.join(ROOT, "tests", "golden", "chain_lazy_stop_parent.npz")
    from gaunegf_amd import _lib
    from gaunegf_amd.engine import get_engine
    print("library:", _lib.LIB_PATH)
    eng = get_engine()
    eng.set_chain_cache(0)                          # every evaluation runs its fixed points
    eng.set_chain_round_robin(-1, 0)
    rec = {}
    for ncL, ncR, ci in lz.cases():
        blk, its, cv = lz.run(ncL, ncR, ci)
        k = lz.key(ncL, ncR, ci)
        rec[k + "_sha"] = cs.digests(blk); rec[k + "_it"] = its; rec[k + "_cv"] = cv
        print(k, "sweeps", its.ravel().tolist(), "flags", cv.ravel().tolist())
    for ncL, ncR in lz.SIZES:                       # (ii) once more, on what the kernel did
        assert any(((rec[lz.key(ncL, ncR, ci) + "_cv"] == 1) & (rec[lz.key(ncL, ncR, ci) + "_it"] < lz.MAX_ITER)).any()
                   for ci in range(len(lz.CONVS))), (ncL, ncR)
    np.savez(out, **rec)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()

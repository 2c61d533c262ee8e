"""
The cases of tests/test_chain_stage_sched_gpu.py: the compile-time stage schedule of the chain kernel's small inverse
(rs_inverse_sched, remainder-strip classes) against the generic loop (rs_inverse) of the SAME build.  The generic loop
runs when the wave roles follow the wave numbers, NEGF_CHAIN1D_ROLES=0, which the library reads once per process (as it
does NEGF_CHAIN1D_OCC), so that side is computed by a child process running this file:

    python chain_stage_sched_cases.py <group> <out.npz>

Every case yields the Sigma blocks of both contacts, the sweep counts and the convergence flags.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))

import chain_phases_cases as cs                     # noqa: E402
from helpers import chain_lead                      # noqa: E402

# ---- the launcher's class rule (launch_chain1d_lds, chain_mix_map.h), restated
PITCHES = [17, 19, 25, 33, 35, 41, 49, 51, 57, 65]


def class_tiles(P):
    return (P - 1 + 15) // 16


def class_nmax(P):                                  # rs_class_nmax
    return P if P < 16 * class_tiles(P) else 16 * class_tiles(P)


def is_strip_class(P):                              # REM of the kernel
    return class_tiles(P) >= 2 and P - 16 * (class_tiles(P) - 1) <= 4


def class_edge_sizes():
    """Every n of every strip class -- last panels of every width the class holds, both ends of its range -- and one
    step outside on each side (the class without strips below, the next class above)."""
    out = []
    for P in PITCHES:
        if is_strip_class(P):
            lo = 16 * (class_tiles(P) - 1) + 1
            out += list(range(lo - 1, class_nmax(P) + 2))
    return out


FORCE = cs.FORCE                                    # 0 / 1 / 3 sweeps
UNEQUAL = [(50, 49), (50, 40)]                      # inside a strip class; the guarded class
BAD = [(50, d) for d in ("zero_column", "nan_entry")] + [(18, d) for d in ("zero_column", "nan_entry")]
BAD_E = np.array([0.3, 0.1 + 0.2j])


def free_energies():
    """Two energies of the free-running grid of chain_phases_cases: one with a unit that stops on the test, one with a
    unit that reaches the cap (read off the committed record of that grid)."""
    rec = np.load(os.path.join(HERE, "golden", "chain_phases_parent.npz"), allow_pickle=False)
    it, cv = rec["free_it"], rec["free_cv"]
    stops = int(np.argmax((cv == 1).any(axis=1)))
    capped = int(np.argmax(((cv == 0) & (it == it.max())).any(axis=1)))
    assert (cv[stops] == 1).any() and (cv[capped] == 0).any() and stops != capped
    return cs.FREE_E[[stops, capped]]


def fixed_names():
    return [f"fx_{n}_{n}_{f}" for n in class_edge_sizes() for f in FORCE] + [f"fx_{a}_{b}_{f}" for a, b in UNEQUAL for f in FORCE]


def bad_names():
    return [f"bad_{n}_{d}" for n, d in BAD]


GROUPS = {
    "main": lambda: fixed_names() + ["free", "rr"] + bad_names(),
    "occ2": lambda: ["fx_50_50_3"],                 # (run with NEGF_CHAIN1D_OCC=2)
}


def _pack(out, name, blk, its, cv):
    out[name + "_it"] = np.asarray(its); out[name + "_cv"] = np.asarray(cv)
    for m, row in enumerate(blk):
        for c, b in enumerate(row):
            out[f"{name}_blk_{m}_{c}"] = b


def _bad_leads(n, defect):
    good = (chain_lead(n, 801), chain_lead(n, 802))
    alpha, Salpha = good[1][0].copy(), good[1][1].copy()
    if defect == "zero_column":
        alpha[:, n // 2] = 0.0; Salpha[:, n // 2] = 0.0
    else:
        alpha[1, 2] = np.nan
    return good[0], (alpha, Salpha, good[1][2], good[1][3])


def run_case(engine, name):
    """-> (blocks [energy][contact], sweep counts, flags) of one case, by a cold plain launch unless the case says otherwise"""
    engine.set_chain_cache(0); engine.set_chain_round_robin(-1, 0)
    try:
        kind = name.split("_")[0]
        if kind == "fx":
            ncL, ncR, f = map(int, name.split("_")[1:])
            return cs.run_fixed(ncL, ncR, f)
        if kind == "free":
            engine.set_chain_round_robin(0, 0)
            g, inds = cs.provider(cs.FREE_NC, cs.FREE_NC, 55)
            sig, its, cv = g.sigma_batch(free_energies())
            return cs.blocks(sig, inds), its, cv
        if kind == "rr":                            # 5 slots, quantum 7: every job of the grid is set aside and resumed
            engine.set_chain_round_robin(7, 5)
            return cs.run_free()
        if kind == "bad":
            n, defect = int(name.split("_")[1]), name.split("_", 2)[2]
            g, inds = cs.provider(n, n, 800, leads=_bad_leads(n, defect))
            sig, its, cv = g.sigma_batch(BAD_E)
            return cs.blocks(sig, inds), its, cv
        raise KeyError(name)
    finally:
        engine.set_chain_round_robin(-1, 0); engine.set_chain_cache(512)


def run_group(engine, group):
    out = {}
    for name in GROUPS[group]():
        _pack(out, name, *run_case(engine, name))
    return out


if __name__ == "__main__":
    from gaunegf_amd.engine import get_engine
    np.savez(sys.argv[2], **run_group(get_engine(), sys.argv[1]))

"""
The cases of tests/test_env_retired_gpu.py and of part (ii) of tests/test_env_switches_host.py: what a process computes
must not depend on the environment variables the library no longer reads.  RETIRED lists them with the values that used
to change the most -- wrong-result ablations, other window kernels, the vector-unit products, the element form of the
permuted accumulate, the eager gather, the blocking wait, no round robin; a child process runs this file with all of
them set:

    python env_retired_cases.py plans <out.npz>       (no GPU)
    python env_retired_cases.py gpu <out.npz>
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))

RETIRED = {
    "NEGF_GJ_DEBUG": "32", "NEGF_GJ_STRIP_DBG": "15",
    "NEGF_GJ_LARGE_MIN": "999", "NEGF_GJ_SMALL_WIN_MIN": "1", "NEGF_GJ_WINLA": "0", "NEGF_GJ_STRIP": "0",
    "NEGF_GJ_STRIP_MIN": "1", "NEGF_GJ_STRIP_CFG": "3", "NEGF_GJ_PAIR": "0", "NEGF_GJ_PAIR_MIN": "1",
    "NEGF_GJ_FAT_MAX": "1", "NEGF_GJ_FAT_TOTAL_MAX": "1", "NEGF_GJ_SPLIT_MAX": "0", "NEGF_GJ_GROUP_MAX": "2",
    "NEGF_GJ_GROUP_MIN": "1",
    "NEGF_ZGEMM_ALGO": "valu", "NEGF_ZGEMM_HERM": "0", "NEGF_ZGEMM_FLEX": "2",
    "NEGF_ACC_PERM_ROWS": "0", "NEGF_GATHER_FUSED": "0", "NEGF_SYNC_SPIN": "0", "NEGF_CHAIN_RR": "0",
    "NEGF_SPECULATIVE_ONE_CU": "7", "NEGF_SPECULATIVE_SMALL": "7", "NEGF_REFINE_ON_DEVICE": "0",
}

PLAN_SHAPES = [(100, 257), (209, 6), (300, 256), (513, 640), (900, 644)]

# six energies, one of them complex
ENERGIES = np.array([-0.9, -0.35, 0.1, 0.2 + 0.05j, 0.55, 0.8])
WEIGHTS = np.array([0.3, 0.1 - 0.2j, 0.25, 0.2 + 0.1j, 0.05, 0.1])
# (n, negf_set_inverse_algo, calls, window-kernel bit the launch must record: 10 single workgroup, 1 strip<1,32,4,2,4>,
#  8 look-ahead of 12 waves)
GPU_CASES = [
    (40, 2, ("gr_batch",), 10),
    (72, 3, ("gr_batch", "gr_int", "gless_int"), 1),
    (300, 0, ("gr_int",), 8),
]


def plans():
    """every plan of PLAN_SHAPES (auto rule, gather run and deferred) as one integer table"""
    from gaunegf_amd.engine import Engine
    out = {}
    for n, nb in PLAN_SHAPES:
        for defer in (False, True):
            p = Engine.inverse_plan(n, nb, 0, defer)
            rows = [[g[k] for k in ("first", "count", "wk", "pairs", "upd_full", "upd_single", "mask")] for g in p["groups"]]
            head = [p["path"], *p["cls"], p["nblk"], len(rows), int(p["gather"]), int(p["deferred"])]
            out[f"plan_{n}_{nb}_{int(defer)}"] = np.array(head + [v for r in rows for v in r], dtype=np.int64)
    return out


def system(n):
    """F, S and the constant self-energies of two contacts of six orbitals at the ends"""
    rng = np.random.default_rng(4000 + n)
    A = rng.standard_normal((n, n)); F = (A + A.T) / np.sqrt(2 * n) * 2
    B = rng.standard_normal((n, n)); S = np.eye(n) + 0.1 * (B + B.T) / np.sqrt(2 * n)
    sig = np.zeros((2, n, n), dtype=np.complex128)
    for c, idx in enumerate((np.arange(6), np.arange(n - 6, n))):
        H = rng.standard_normal((6, 6))
        sig[c][np.ix_(idx, idx)] = 0.1 * (H + H.T) - 0.05j * (np.eye(6) + 0.1 * H @ H.T)
    return F, S, sig


def run_gpu(engine):
    out = {}
    try:
        for n, algo, calls, bit in GPU_CASES:
            F, S, sig = system(n)
            engine.set_system(F, S)
            h = engine.sigma_const(sig)
            engine.set_inverse_algo(algo)
            for call in calls:
                if call == "gr_batch":
                    r = engine.gr_batch(h, ENERGIES)
                elif call == "gr_int":
                    r = engine.gr_int(h, ENERGIES, WEIGHTS)
                else:
                    r = engine.gless_int(h, -1, ENERGIES, WEIGHTS)
                out[f"{call}_{n}"] = r
                out[f"{call}_{n}_info"] = np.array(engine.last_info)
                out[f"{call}_{n}_masks"] = np.array(engine.inverse_last()["masks"], dtype=np.int64)
            engine.sigma_free(h)
    finally:
        engine.set_inverse_algo(0)
    return out


if __name__ == "__main__":
    if sys.argv[1] == "plans":
        np.savez(sys.argv[2], **plans())
    else:
        from gaunegf_amd.engine import get_engine
        np.savez(sys.argv[2], **run_gpu(get_engine()))

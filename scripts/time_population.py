"""Time the projected DOS against the reference-parity DOS, and a contact's share against GrLessInt, on the same grid:
N = 500 with constant self-energies on two contacts of 50 orbitals, 1000 real energies.

  dos              Engine.dos (negf_dos: -Im diag G / pi, host-pointer form, [m, n] per-site values come back)
  pdos             Engine.population(RETARDED, rows=True): the same G, one pass over it with S -> [m, n]
  pdos groups      the same with 50 groups of 10 orbitals -> [m, 50]
  coop table       Engine.population(RETARDED) with the 50 groups -> [m, 50, 50]
  proj             Engine.projected_dos(RETARDED) on 16 vectors
  gless_int        Engine.gless_int_dev(ind = 0): the products up to A_c = G Gamma_c G^H, then the weighted sum
  pdos contact     Engine.population_dev(ind = 0, rows=True): the same products, then one pass over A_c with S

--passes alternating passes, wall time from call to the end of the call / negf_sync (best and median) and the library's
per-family kernel times.  --baseline-only times dos and gless_int alone (runs on a checkout that predates the feature)."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests.helpers import random_system                     # noqa: E402
from gaunegf_amd.engine import get_engine                   # noqa: E402

FAMILIES = ("small", "assemble", "inverse", "gamma", "zgemm", "accumulate", "trace", "pop")


def const_handle(eng, N, K):
    F, S = random_system(N, 500)
    rng = np.random.default_rng(500)
    sig = []
    for idx in (np.arange(K), np.arange(N - K, N)):
        A = rng.standard_normal((idx.size, idx.size)) + 1j * rng.standard_normal((idx.size, idx.size))
        s = np.zeros((N, N), complex); s[np.ix_(idx, idx)] = -0.05j * (A @ A.conj().T) / idx.size
        sig.append(s)
    eng.set_system(F, S)
    return F, S, eng.sigma_const(sig)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=500)
    ap.add_argument("--energies", type=int, default=1000)
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--baseline-only", action="store_true")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("time_population.py needs a GPU (the engine has no CPU path)")
    torch.cuda.set_device(0)
    eng = get_engine()
    n, m = a.n, a.energies
    F, S, h = const_handle(eng, n, 50)
    E = np.linspace(-2.0, 2.0, m)
    dev = torch.device("cuda", eng.device)
    groups = np.arange(n) // 10
    ng = int(groups.max()) + 1
    E_t = torch.from_numpy(np.ascontiguousarray(E, dtype=np.complex128)).to(dev)
    w_t = torch.full((m,), 0.01 + 0.0j, dtype=torch.complex128, device=dev)
    out_c = torch.zeros((n, n), dtype=torch.complex128, device=dev)
    out_r = torch.zeros((m, n), dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)

    def synced(fn):
        def call():
            fn(); eng.sync()
        return call
    calls = {"dos": lambda: eng.dos(h, E),
             "gless_int": synced(lambda: eng.gless_int_dev(h, 0, m, E_t.data_ptr(), w_t.data_ptr(), out_c.data_ptr()))}
    if not a.baseline_only:
        W = np.ascontiguousarray(np.random.default_rng(1).standard_normal((16, n)) + 0j)
        calls.update({
            "pdos": lambda: eng.population(h, eng.RETARDED, E, 'S', rows=True),
            "pdos groups": lambda: eng.population(h, eng.RETARDED, E, 'S', groups, rows=True),
            "coop table": lambda: eng.population(h, eng.RETARDED, E, 'S', groups),
            "proj": lambda: eng.projected_dos(h, eng.RETARDED, E, W),
            "pdos contact": synced(lambda: eng.population_dev(h, 0, m, E_t.data_ptr(), out_r.data_ptr(), 'S', None, rows=True)),
            "pdos contact groups": synced(lambda: eng.population_dev(h, 0, m, E_t.data_ptr(), out_r.data_ptr(), 'S', groups, rows=True)),
        })
    eng.profile(True)
    for fn in calls.values():                                # warm: workspace, staging, code objects
        fn()
    times = {k: [] for k in calls}
    fams = {}
    for _ in range(a.passes):                                # alternating passes
        for k, fn in calls.items():
            eng.profile_reset()
            t0 = time.perf_counter(); fn(); t = time.perf_counter() - t0
            if not times[k] or t < min(times[k]):
                fams[k] = {f: eng.profile_read(f) for f in FAMILIES}
            times[k].append(t)
    eng.profile(False)
    print(f"N = {n}, CONST Sigma (K = 50 / 50), {m} energies, batch {eng.get_batch()}, {a.passes} alternating passes")
    for k, ts in times.items():
        base = min(times["gless_int" if "contact" in k or k == "gless_int" else "dos"])
        print(f"  {k:20s} best {min(ts) * 1e3:8.2f} ms, median {np.median(ts) * 1e3:8.2f} ms, ratio (best) {min(ts) / base:.3f}")
        print("    kernels: " + ", ".join(f"{f} {ms:.3f} ms/{cnt}" for f, (ms, cnt) in fams[k].items() if cnt))
    if not a.baseline_only:
        moved = m * 16.0 * n * n                              # G or A_c once per energy; S from L2
        for k in ("pdos", "pdos groups", "pdos contact", "pdos contact groups"):
            ms = fams[k]["pop"][0]
            print(f"  pop family in {k}: {ms:.3f} ms for {moved / 1e9:.2f} GB of G / A_c (from shapes) = {moved / ms / 1e9:.2f} TB/s")
    eng.sigma_free(h)


if __name__ == "__main__":
    main()

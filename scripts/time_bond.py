"""Time the local (bond) transmission against GrLessInt on the same warm grid: BASELINE C3 size (N = 500, two 1-D chain
leads of n_c = 50, 2000 real energies, g(E) cache warm) and N = 60 with constant self-energies.  The three calls --
gless_int(ind = 0), local_transmission with groups of 10 orbitals, bond_int -- do identical work up to A_c = G Gamma G^H;
GrLessInt then reads A_c once in launch_accumulate, which is what the "bond" kernels replace.  Device-resident entry
points (grid and results in HBM), --passes alternating passes, wall time from call to the end of negf_sync (best and
median), the library's per-family kernel times, and the bytes the "bond" family moves (from shapes) over its time.
--baseline-only times gless_int alone (runs on a checkout that predates the feature)."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests.helpers import chain_lead, random_system        # noqa: E402
from gaunegf_amd.engine import get_engine                   # noqa: E402
from gaunegf_amd.surfG1D import surfG                       # noqa: E402

FAMILIES = ("chain1d", "chain1d_hit", "small", "assemble", "inverse", "gamma", "zgemm", "accumulate", "bond")


def c3_handle(eng, N=500, nc=50, eta=1e-4):
    F, S = random_system(N, 3)
    aL, aR = chain_lead(nc, 31), chain_lead(nc, 32)
    g = surfG(F, S, [list(range(nc)), list(range(N - nc, N))], taus=[aL[2].copy(), aR[2].copy()],
              staus=[aL[3].copy(), aR[3].copy()], alphas=[aL[0], aR[0]], aOverlaps=[aL[1], aR[1]],
              betas=[aL[2], aR[2]], bOverlaps=[aL[3], aR[3]], eta=eta)
    eng.set_system(F, S)
    return g, g._negf_lower(eng)


def const_handle(eng, N=60):
    F, S = random_system(N, 60)
    rng = np.random.default_rng(60)
    sig = []
    for idx in (np.arange(10), np.arange(N - 12, N)):
        A = rng.standard_normal((idx.size, idx.size)) + 1j * rng.standard_normal((idx.size, idx.size))
        s = np.zeros((N, N), complex); s[np.ix_(idx, idx)] = -0.05j * (A @ A.conj().T) / idx.size
        sig.append(s)
    eng.set_system(F, S)
    return None, eng.sigma_const(sig)


def run(eng, label, h, E, passes, baseline_only):
    import torch
    dev = torch.device("cuda", eng.device)
    n, m = eng.n, E.size
    groups = np.arange(n) // 10
    ng = int(groups.max()) + 1
    E_t = torch.view_as_complex(torch.from_numpy(np.ascontiguousarray(E, dtype=np.complex128).view(np.float64).reshape(-1, 2).copy())).to(dev)
    wc_t = torch.full((m,), 0.01 + 0.0j, dtype=torch.complex128, device=dev)
    wr_t = torch.full((m,), 0.01, dtype=torch.float64, device=dev)
    out_c = torch.zeros((n, n), dtype=torch.complex128, device=dev)
    out_r = torch.zeros((n, n), dtype=torch.float64, device=dev)
    out_g = torch.zeros((m, ng, ng), dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    calls = {"gless_int": lambda: eng.gless_int_dev(h, 0, m, E_t.data_ptr(), wc_t.data_ptr(), out_c.data_ptr())}
    if not baseline_only:
        calls["local_transmission"] = lambda: eng.local_transmission_dev(h, 0, m, E_t.data_ptr(), groups, out_g.data_ptr())
        calls["bond_int"] = lambda: eng.bond_int_dev(h, 0, m, E_t.data_ptr(), wr_t.data_ptr(), out_r.data_ptr())
    eng.profile(True)
    for fn in calls.values():                                # warm: workspace, g(E) cache, code objects
        fn(); eng.sync()
    times = {k: [] for k in calls}
    fams = {}
    for _ in range(passes):                                  # alternating passes
        for k, fn in calls.items():
            eng.profile_reset()
            t0 = time.perf_counter(); fn(); eng.sync(); t = time.perf_counter() - t0
            if not times[k] or t < min(times[k]):
                fams[k] = {f: eng.profile_read(f) for f in FAMILIES}
            times[k].append(t)
    eng.profile(False)
    base = min(times["gless_int"])
    print(f"{label}: {m} energies, batch {eng.get_batch()}, {passes} alternating passes")
    for k, ts in times.items():
        print(f"  {k:18s} best {min(ts) * 1e3:8.2f} ms, median {np.median(ts) * 1e3:8.2f} ms, ratio to gless_int (best) "
              f"{min(ts) / base:.3f}")
        parts = ", ".join(f"{f} {ms:.2f} ms/{cnt}" for f, (ms, cnt) in fams[k].items() if cnt)
        print(f"    kernels: {parts}")
    if baseline_only:
        return
    # bytes from shapes: A once per energy (16 n^2), the output; S and F come from L2 (counted once per launch)
    nb = max(eng.get_batch(), 1)
    launches = -(-m // nb)
    moved = {"local_transmission": m * 16.0 * n * n + m * 8.0 * ng * ng + launches * 32.0 * n * n,
             "bond_int": m * 16.0 * n * n + launches * (32.0 * n * n + 8.0 * n * n * (2 * (-(-nb // 32) + 1) + 2))}
    for k, b in moved.items():
        ms = fams[k]["bond"][0]
        print(f"  bond family in {k}: {ms:.3f} ms for {b / 1e9:.3f} GB (from shapes) = {b / ms / 1e9:.2f} TB/s; "
              f"accumulate in gless_int: {fams['gless_int']['accumulate'][0]:.3f} ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--energies", type=int, default=2000)
    ap.add_argument("--passes", type=int, default=10)
    ap.add_argument("--only", choices=("c3", "n60"), default=None)
    ap.add_argument("--baseline-only", action="store_true")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("time_bond.py needs a GPU (the engine has no CPU path)")
    torch.cuda.set_device(0)                                 # torch's runtime first, then the engine's context
    eng = get_engine()
    E = np.linspace(-2.0, 2.0, a.energies)
    if a.only in (None, "c3"):
        g, h = c3_handle(eng)
        run(eng, "C3 (N = 500, chain leads n_c = 50, g(E) cache warm)", h, E, a.passes, a.baseline_only)
    if a.only in (None, "n60"):
        _, h = const_handle(eng)
        run(eng, "N = 60, CONST Sigma (K_L = 10, K_R = 12)", h, E, a.passes, a.baseline_only)
        eng.sigma_free(h)


if __name__ == "__main__":
    main()

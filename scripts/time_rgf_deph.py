"""Time the lesser Green's function's weighted sum with floating dephasing probes on a layered device against what a user
ran without it, in one process: 20 layers of 100, const terminals of 50 orbitals on the two end layers, a 10-orbital probe
on every tenth of every layer (200 probes, K_tot = N, C = 202), 256 real energies, contact 0.

  layered gless_int_probes   Engine.layered_gless_int_probes_dev(h, 0): two strip passes with the strips kept, T, R, D, Y,
                             the blocks of G D_0 G^H on the pattern
  layered tmatrix + gless    Engine.layered_transmission_matrix_dev with the probes, then layered_gless_int_dev(h, 0): the
                             device work of the path without the feature (it does not give the floating density; the host
                             solve and the transfers are not counted)
  dense gless_int_probes     Engine.gless_int_probes_dev(h, 0) on to_dense(): the N x N inverse, G D_0 G^H in full

Device-resident calls (grid and results in HBM), warm-up, --passes alternating passes, wall time from the call to the end
of negf_sync (best and median), the library's per-family kernel times of the best pass ("deph": the response solve, the
coupling kernel and the block-diagonal product) and the workspace bytes of every side."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gaunegf_amd.engine import get_engine                                        # noqa: E402
from gaunegf_amd.layered import LayeredSystem, dephasing_probes_layered          # noqa: E402

FAMILIES = ("rgf", "assemble", "inverse", "gamma", "zgemm", "tmat", "deph", "accumulate")


def layered_blocks(L, n, seed=20):
    rng = np.random.default_rng(seed)
    Fd, Sd, Fu, Su = [], [], [], []
    for _ in range(L):
        a = rng.standard_normal((n, n)); s = rng.standard_normal((n, n))
        Fd.append((a + a.T) / np.sqrt(2 * n)); Sd.append(np.eye(n) + 0.1 * (s + s.T) / np.sqrt(2 * n))
    for _ in range(L - 1):
        Fu.append(0.6 * rng.standard_normal((n, n)) / np.sqrt(n)); Su.append(0.05 * rng.standard_normal((n, n)) / np.sqrt(n))
    return Fd, Fu, Sd, Su


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=20)
    ap.add_argument("--n", type=int, default=100)
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--probe", type=int, default=10, help="orbitals per probe; the probes tile every layer")
    ap.add_argument("--energies", type=int, default=256)
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--no-dense", action="store_true", help="leave the dense side out (it takes 16 N^2 bytes per energy, three times)")
    ap.add_argument("--json", default=None, help="write the figures to this file as well")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("time_rgf_deph.py needs a GPU (the engine has no CPU path)")
    torch.cuda.set_device(0)
    eng = get_engine()
    L, n, K, m = a.layers, a.n, a.k, a.energies
    N = L * n
    Fd, Fu, Sd, Su = layered_blocks(L, n)
    ls = LayeredSystem(Fd, Fu, Sd, Su)
    rng = np.random.default_rng(21)
    sig = []
    for _ in range(2):
        A = rng.standard_normal((K, K)) + 1j * rng.standard_normal((K, K))
        sig.append(-0.05j * (A @ A.conj().T) / K)
    probes = dephasing_probes_layered(ls, [np.arange(s0, min(s0 + a.probe, (s0 // n + 1) * n)) for i in range(L)
                                           for s0 in range(i * n, (i + 1) * n, a.probe)], 0.1)
    h = eng.layered_create(Fd, Fu, Sd, Su)
    eng.layered_terminal_const(h, 0, np.arange(K), sig[0])
    eng.layered_terminal_const(h, L - 1, np.arange(n - K, n), sig[1])
    C = 2 + len(probes)
    dev = torch.device("cuda", eng.device)
    E_t = torch.from_numpy(np.linspace(-1.0, 1.0, m).astype(np.complex128)).to(dev)
    w_t = torch.full((m,), 2.0 / m + 0.0j, dtype=torch.complex128, device=dev)
    out_p = torch.zeros(eng.layered_pattern_size(h), dtype=torch.complex128, device=dev)
    out_l = torch.zeros_like(out_p)
    TC = torch.zeros((m, C, C), dtype=torch.float64, device=dev)
    hd, out_d = None, None
    if not a.no_dense:
        F, S = ls.to_dense()
        eng.set_system(F, S)
        dense_sig = []
        for idx, blk in ((np.arange(K), sig[0]), (np.arange(N - K, N), sig[1])):
            s = np.zeros((N, N), complex); s[np.ix_(idx, idx)] = blk
            dense_sig.append(s)
        hd = eng.sigma_const(dense_sig)
        out_d = torch.zeros((N, N), dtype=torch.complex128, device=dev)
    torch.cuda.synchronize(dev)
    work = {}

    def layered_probes():
        eng.layered_gless_int_probes_dev(h, 0, m, E_t.data_ptr(), w_t.data_ptr(), out_p.data_ptr(), probes); eng.sync()
        work["layered gless_int_probes"] = eng.layered_workspace_bytes(h)

    def layered_today():
        eng.layered_transmission_matrix_dev(h, m, E_t.data_ptr(), TC.data_ptr(), probes)
        w0 = eng.layered_workspace_bytes(h)
        eng.layered_gless_int_dev(h, 0, m, E_t.data_ptr(), w_t.data_ptr(), out_l.data_ptr()); eng.sync()
        work["layered tmatrix + gless"] = max(w0, eng.layered_workspace_bytes(h))

    def dense_probes():
        eng.gless_int_probes_dev(hd, 0, m, E_t.data_ptr(), w_t.data_ptr(), out_d.data_ptr(), probes); eng.sync()
        work["dense gless_int_probes"] = eng.workspace_bytes()[0]

    calls = {"layered gless_int_probes": layered_probes, "layered tmatrix + gless": layered_today}
    if hd is not None:
        calls["dense gless_int_probes"] = dense_probes
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
    print(f"{L} layers of {n} (N = {N}), const terminals of {K}, {len(probes)} probes of {a.probe} (C = {C}), {m} energies, "
          f"{a.passes} alternating passes")
    if hd is not None:                                       # the two sides agree on the pattern
        P = out_d.cpu().numpy()
        d, u, l = eng._lsplit(h, out_p.cpu().numpy())
        dif = max(max(np.abs(d[i] - P[i * n:(i + 1) * n, i * n:(i + 1) * n]).max() for i in range(L)),
                  max(np.abs(u[i] - P[i * n:(i + 1) * n, (i + 1) * n:(i + 2) * n]).max() for i in range(L - 1)),
                  max(np.abs(l[i] - P[(i + 1) * n:(i + 2) * n, i * n:(i + 1) * n]).max() for i in range(L - 1)))
        print(f"  max |layered - dense| on the pattern {dif:.3g} (max |dense| {np.abs(P).max():.3g})")
    base = min(times["layered gless_int_probes"])
    report = {"layers": L, "n": n, "k": K, "probes": len(probes), "energies": m, "passes": a.passes, "calls": {}}
    for k, ts in times.items():
        print(f"  {k:26s} best {min(ts) * 1e3:9.2f} ms, median {np.median(ts) * 1e3:9.2f} ms, "
              f"ratio to gless_int_probes (best) {min(ts) / base:.3f}, workspace {work[k] / 1e6:10.1f} MB")
        print("    kernels: " + ", ".join(f"{f} {ms:.3f} ms/{cnt}" for f, (ms, cnt) in fams[k].items() if cnt))
        report["calls"][k] = {"best_ms": min(ts) * 1e3, "median_ms": float(np.median(ts)) * 1e3, "ratio_best": min(ts) / base,
                              "workspace_bytes": int(work[k]), "kernels_ms": {f: ms for f, (ms, cnt) in fams[k].items() if cnt}}
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(report, f, indent=1)
    if hd is not None:
        eng.sigma_free(hd)
    eng.layered_free(h)


if __name__ == "__main__":
    main()

"""Time the transmission matrix of a layered device against the dense engine on to_dense(): 20 layers of 100, const
terminals of 50 orbitals on the two end layers, 256 real energies, device-resident entry points in one process.

  layered tmatrix, probes   Engine.layered_transmission_matrix_dev with a probe of 10 orbitals on every tenth of every
                            layer (K_tot = N, C = 202): two passes of forward and backward sweep with the column strips
  layered tmatrix           the same call without probes (C = 2)
  layered transmission      Engine.layered_transmission_dev: one forward sweep with the corner block
  dense tmatrix, probes     Engine.transmission_matrix_dev on to_dense() with the same probes: the N x N inverse
  dense tmatrix             ... without probes

Host clock around a stream synchronisation, warm-up, --passes alternating passes (best and median), the library's
per-family kernel times of the best pass, and the workspace bytes of both sides.  --json writes the raw figures."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gaunegf_amd.engine import get_engine                   # noqa: E402
from time_layered_less import layered_blocks                # noqa: E402

FAMILIES = ("rgf", "assemble", "inverse", "zgemm", "tmat", "trace", "gamma")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=20)
    ap.add_argument("--n", type=int, default=100)
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--probe", type=int, default=10)
    ap.add_argument("--energies", type=int, default=256)
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("time_layered_tmatrix.py needs a GPU (the engine has no CPU path)")
    torch.cuda.set_device(0)
    eng = get_engine()
    L, n, K, m, kp = a.layers, a.n, a.k, a.energies, a.probe
    N = L * n
    Fd, Fu, Sd, Su = layered_blocks(L, n)
    rng = np.random.default_rng(21)
    sig = []
    for _ in range(2):
        A = rng.standard_normal((K, K)) + 1j * rng.standard_normal((K, K))
        sig.append(-0.05j * (A @ A.conj().T) / K)
    h = eng.layered_create(Fd, Fu, Sd, Su)
    tl = eng.layered_terminal_const(h, 0, np.arange(K), sig[0])
    tr = eng.layered_terminal_const(h, L - 1, np.arange(n - K, n), sig[1])
    F = np.zeros((N, N)); S = np.zeros((N, N))
    for i in range(L):
        F[i * n:(i + 1) * n, i * n:(i + 1) * n] = Fd[i]; S[i * n:(i + 1) * n, i * n:(i + 1) * n] = Sd[i]
    for i in range(L - 1):
        F[i * n:(i + 1) * n, (i + 1) * n:(i + 2) * n] = Fu[i]; F[(i + 1) * n:(i + 2) * n, i * n:(i + 1) * n] = Fu[i].T
        S[i * n:(i + 1) * n, (i + 1) * n:(i + 2) * n] = Su[i]; S[(i + 1) * n:(i + 2) * n, i * n:(i + 1) * n] = Su[i].T
    eng.set_system(F, S)
    dense_sig = []
    for idx, blk in ((np.arange(K), sig[0]), (np.arange(N - K, N), sig[1])):
        s = np.zeros((N, N), complex); s[np.ix_(idx, idx)] = blk
        dense_sig.append(s)
    hd = eng.sigma_const(dense_sig)
    # a dephasing probe (gamma = 0.1) on every kp orbitals of every layer
    probes = []
    for s0 in range(0, N, kp):
        idx = np.arange(s0, min(s0 + kp, (s0 // n + 1) * n))
        probes.append((idx, -0.05j * S[np.ix_(idx, idx)].astype(complex)))
    C = 2 + len(probes)
    dev = torch.device("cuda", eng.device)
    E_t = torch.from_numpy(np.linspace(-1.0, 1.0, m).astype(np.complex128)).to(dev)
    T_lp = torch.zeros((m, C, C), dtype=torch.float64, device=dev)
    T_dp = torch.zeros_like(T_lp)
    T_l0 = torch.zeros((m, 2, 2), dtype=torch.float64, device=dev)
    T_d0 = torch.zeros_like(T_l0)
    T_1 = torch.zeros(m, dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    work = {}

    def layered_probes():
        eng.layered_transmission_matrix_dev(h, m, E_t.data_ptr(), T_lp.data_ptr(), probes); eng.sync()
        work["layered tmatrix, probes"] = eng.layered_workspace_bytes(h)

    def layered_none():
        eng.layered_transmission_matrix_dev(h, m, E_t.data_ptr(), T_l0.data_ptr()); eng.sync()
        work["layered tmatrix"] = eng.layered_workspace_bytes(h)

    def layered_t():
        eng.layered_transmission_dev(h, tr, tl, m, E_t.data_ptr(), T_1.data_ptr()); eng.sync()
        work["layered transmission"] = eng.layered_workspace_bytes(h)

    def dense_probes():
        eng.transmission_matrix_dev(hd, m, E_t.data_ptr(), T_dp.data_ptr(), probes); eng.sync()
        work["dense tmatrix, probes"] = eng.workspace_bytes()[0]

    def dense_none():
        eng.transmission_matrix_dev(hd, m, E_t.data_ptr(), T_d0.data_ptr()); eng.sync()
        work["dense tmatrix"] = eng.workspace_bytes()[0]

    calls = {"layered tmatrix, probes": layered_probes, "layered tmatrix": layered_none, "layered transmission": layered_t,
             "dense tmatrix, probes": dense_probes, "dense tmatrix": dense_none}
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
    lp, dp = T_lp.cpu().numpy(), T_dp.cpu().numpy()
    l0, d0, t1 = T_l0.cpu().numpy(), T_d0.cpu().numpy(), T_1.cpu().numpy()
    dif_p = float(np.linalg.norm(lp - dp) / np.linalg.norm(dp))
    dif_0 = float(np.linalg.norm(l0 - d0) / np.linalg.norm(d0))
    dif_1 = float(np.linalg.norm(l0[:, 1, 0] - t1) / np.linalg.norm(t1))
    print(f"{L} layers of {n} (N = {N}), const terminals of {K}, {len(probes)} probes of {kp} (C = {C}), {m} energies, "
          f"{a.passes} alternating passes; |layered - dense| / |dense|: {dif_p:.3g} with probes, {dif_0:.3g} without; "
          f"T[right][left] against layered_transmission {dif_1:.3g}")
    rows = {}
    for k, ts in times.items():
        rows[k] = dict(best_ms=min(ts) * 1e3, median_ms=float(np.median(ts)) * 1e3, workspace_bytes=int(work[k]),
                       kernels_ms={f: [ms, cnt] for f, (ms, cnt) in fams[k].items() if cnt})
        print(f"  {k:26s} best {min(ts) * 1e3:9.2f} ms, median {np.median(ts) * 1e3:9.2f} ms, workspace {work[k] / 1e6:10.1f} MB")
        print("    kernels: " + ", ".join(f"{f} {ms:.3f} ms/{cnt}" for f, (ms, cnt) in fams[k].items() if cnt))
    b = {k: r["best_ms"] for k, r in rows.items()}
    ratios = {"dense / layered, probes": b["dense tmatrix, probes"] / b["layered tmatrix, probes"],
              "dense / layered, no probes": b["dense tmatrix"] / b["layered tmatrix"],
              "layered tmatrix (no probes) / layered transmission": b["layered tmatrix"] / b["layered transmission"],
              "layered tmatrix (probes) / layered transmission": b["layered tmatrix, probes"] / b["layered transmission"]}
    for k, v in ratios.items():
        print(f"  {k}: {v:.2f}")
    if a.json:
        with open(a.json, "w") as f:
            json.dump(dict(layers=L, n=n, N=N, lead_k=K, probes=len(probes), probe_k=kp, C=C, energies=m, passes=a.passes,
                           agreement=dict(probes=dif_p, no_probes=dif_0, against_layered_transmission=dif_1),
                           rows=rows, ratios=ratios), f, indent=1)
            f.write("\n")
    eng.sigma_free(hd)
    eng.layered_free(h)


if __name__ == "__main__":
    main()

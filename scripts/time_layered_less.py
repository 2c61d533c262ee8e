"""Time G Gamma G^H of a layered device against the dense engine on to_dense(): 20 layers of 100, const terminals of 50
orbitals on the two end layers, 256 real energies, device-resident entry points in one process.

  layered gless_int   Engine.layered_gless_int_dev(ind = all): the two sweeps with the leads' columns, blocks on the pattern
  layered gr_int      Engine.layered_gr_int_dev on the same system: the sweeps alone
  dense gless_int     Engine.gless_int_dev(ind = all) on to_dense(): the N x N inverse, G Gamma G^H in full

Host clock around a stream synchronisation, warm-up, --passes alternating passes (best and median), the library's
per-family kernel times of the best pass, and the workspace bytes of both sides."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gaunegf_amd.engine import get_engine                   # noqa: E402

FAMILIES = ("rgf", "assemble", "inverse", "gamma", "zgemm", "accumulate")


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
    ap.add_argument("--energies", type=int, default=256)
    ap.add_argument("--passes", type=int, default=7)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("time_layered_less.py needs a GPU (the engine has no CPU path)")
    torch.cuda.set_device(0)
    eng = get_engine()
    L, n, K, m = a.layers, a.n, a.k, a.energies
    N = L * n
    Fd, Fu, Sd, Su = layered_blocks(L, n)
    rng = np.random.default_rng(21)
    sig = []
    for _ in range(2):
        A = rng.standard_normal((K, K)) + 1j * rng.standard_normal((K, K))
        sig.append(-0.05j * (A @ A.conj().T) / K)
    h = eng.layered_create(Fd, Fu, Sd, Su)
    eng.layered_terminal_const(h, 0, np.arange(K), sig[0])
    eng.layered_terminal_const(h, L - 1, np.arange(n - K, n), sig[1])
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
    dev = torch.device("cuda", eng.device)
    E_t = torch.from_numpy(np.linspace(-1.0, 1.0, m).astype(np.complex128)).to(dev)
    w_t = torch.full((m,), 2.0 / m + 0.0j, dtype=torch.complex128, device=dev)
    out_l = torch.zeros(eng.layered_pattern_size(h), dtype=torch.complex128, device=dev)
    out_g = torch.zeros_like(out_l)
    out_d = torch.zeros((N, N), dtype=torch.complex128, device=dev)
    torch.cuda.synchronize(dev)
    work = {}

    def layered_less():
        eng.layered_gless_int_dev(h, None, m, E_t.data_ptr(), w_t.data_ptr(), out_l.data_ptr()); eng.sync()
        work["layered gless_int"] = eng.layered_workspace_bytes(h)

    def layered_gr():
        eng.layered_gr_int_dev(h, m, E_t.data_ptr(), w_t.data_ptr(), out_g.data_ptr()); eng.sync()
        work["layered gr_int"] = eng.layered_workspace_bytes(h)

    def dense_less():
        eng.gless_int_dev(hd, None, m, E_t.data_ptr(), w_t.data_ptr(), out_d.data_ptr()); eng.sync()
        work["dense gless_int"] = eng.workspace_bytes()[0]

    calls = {"layered gless_int": layered_less, "layered gr_int": layered_gr, "dense gless_int": dense_less}
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
    # the two sides agree on the pattern
    P = out_d.cpu().numpy()
    d, u, l = eng._lsplit(h, out_l.cpu().numpy())
    dif = max(max(np.abs(d[i] - P[i * n:(i + 1) * n, i * n:(i + 1) * n]).max() for i in range(L)),
              max(np.abs(u[i] - P[i * n:(i + 1) * n, (i + 1) * n:(i + 2) * n]).max() for i in range(L - 1)),
              max(np.abs(l[i] - P[(i + 1) * n:(i + 2) * n, i * n:(i + 1) * n]).max() for i in range(L - 1)))
    print(f"{L} layers of {n} (N = {N}), const terminals of {K}, {m} energies, {a.passes} alternating passes; "
          f"max |layered - dense| on the pattern {dif:.3g} (max |dense| {np.abs(P).max():.3g})")
    for k, ts in times.items():
        print(f"  {k:20s} best {min(ts) * 1e3:9.2f} ms, median {np.median(ts) * 1e3:9.2f} ms, workspace {work[k] / 1e6:10.1f} MB")
        print("    kernels: " + ", ".join(f"{f} {ms:.3f} ms/{cnt}" for f, (ms, cnt) in fams[k].items() if cnt))
    eng.sigma_free(hd)
    eng.layered_free(h)


if __name__ == "__main__":
    main()

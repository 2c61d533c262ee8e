"""Time the bond currents and the local transmission of a layered device against layered_gless_int and against the dense
engine on to_dense(): 20 layers of 100, const terminals of 50 orbitals on the two end layers, 256 real energies,
device-resident entry points in one process, the left terminal injecting.

  layered local orbital   Engine.layered_local_transmission_dev, every orbital its own group: [m, pattern] doubles
  layered local 10/layer  ... with 10 groups per layer (atoms)
  layered local 1/layer   ... with one group per layer (calculate_interlayer_transmission)
  layered bond_int        Engine.layered_bond_int_dev: sum_k w_k flow(E_k) at orbital level
  layered gless_int       Engine.layered_gless_int_dev on the same system and ind: the call whose accumulate pass the flow replaces
  dense local 10/layer    Engine.local_transmission_dev on to_dense() with the same 200 groups
  dense bond_int          Engine.bond_int_dev on to_dense()

Host clock around a stream synchronisation, warm-up, --passes alternating passes (best and median), the library's
per-family kernel times of the best pass, and the workspace bytes of every call.  --json writes the raw values."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gaunegf_amd.engine import get_engine                   # noqa: E402
from time_layered_less import layered_blocks                # noqa: E402

FAMILIES = ("rgf", "assemble", "inverse", "gamma", "zgemm", "accumulate", "bond")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=20)
    ap.add_argument("--n", type=int, default=100)
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--energies", type=int, default=256)
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--no-dense", action="store_true", help="skip the dense engine's calls")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("time_layered_bond.py needs a GPU (the engine has no CPU path)")
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
    ind = 0
    ten = (np.full(L, 10, np.int32), np.tile(np.arange(n) * 10 // n, L).astype(np.int32))
    one = (np.ones(L, np.int32), np.zeros(N, np.int32))
    dev = torch.device("cuda", eng.device)
    E_t = torch.from_numpy(np.linspace(-1.0, 1.0, m).astype(np.complex128)).to(dev)
    w_t = torch.full((m,), 2.0 / m + 0.0j, dtype=torch.complex128, device=dev)
    wr_t = torch.full((m,), 2.0 / m, dtype=torch.float64, device=dev)
    npat = eng.layered_pattern_size(h)
    out_orb = torch.zeros((m, npat), dtype=torch.float64, device=dev)
    out_ten = torch.zeros((m, eng.layered_table_size((10,) * L)), dtype=torch.float64, device=dev)
    out_one = torch.zeros((m, eng.layered_table_size((1,) * L)), dtype=torch.float64, device=dev)
    out_int = torch.zeros(npat, dtype=torch.float64, device=dev)
    out_less = torch.zeros(npat, dtype=torch.complex128, device=dev)
    work = {}

    def layered(key, fn):
        def call():
            fn(); eng.sync()
            work[key] = eng.layered_workspace_bytes(h)
        return call
    calls = {
        "layered local orbital": layered("layered local orbital", lambda: eng.layered_local_transmission_dev(
            h, ind, m, E_t.data_ptr(), out_orb.data_ptr())),
        "layered local 10/layer": layered("layered local 10/layer", lambda: eng.layered_local_transmission_dev(
            h, ind, m, E_t.data_ptr(), out_ten.data_ptr(), *ten)),
        "layered local 1/layer": layered("layered local 1/layer", lambda: eng.layered_local_transmission_dev(
            h, ind, m, E_t.data_ptr(), out_one.data_ptr(), *one)),
        "layered bond_int": layered("layered bond_int", lambda: eng.layered_bond_int_dev(
            h, ind, m, E_t.data_ptr(), wr_t.data_ptr(), out_int.data_ptr())),
        "layered gless_int": layered("layered gless_int", lambda: eng.layered_gless_int_dev(
            h, ind, m, E_t.data_ptr(), w_t.data_ptr(), out_less.data_ptr())),
    }
    hd = None
    if not a.no_dense:
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
        dense_groups = (np.repeat(10 * np.arange(L), n) + ten[1]).astype(np.int32)
        out_dten = torch.zeros((m, 10 * L, 10 * L), dtype=torch.float64, device=dev)
        out_dint = torch.zeros((N, N), dtype=torch.float64, device=dev)

        def dense_local():
            eng.local_transmission_dev(hd, ind, m, E_t.data_ptr(), dense_groups, out_dten.data_ptr(), n_groups=10 * L); eng.sync()
            work["dense local 10/layer"] = eng.workspace_bytes()[0]

        def dense_int():
            eng.bond_int_dev(hd, ind, m, E_t.data_ptr(), wr_t.data_ptr(), out_dint.data_ptr()); eng.sync()
            work["dense bond_int"] = eng.workspace_bytes()[0]
        calls["dense local 10/layer"] = dense_local
        calls["dense bond_int"] = dense_int
    torch.cuda.synchronize(dev)
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
    print(f"{L} layers of {n} (N = {N}), const terminals of {K}, {m} energies, {a.passes} alternating passes")
    # the sides agree: the integral is the weighted sum of the tables, one group per layer is the blocks' sums, and the
    # dense tables are the layered ones
    orb = out_orb.cpu().numpy()
    dif = np.abs(out_int.cpu().numpy() - (2.0 / m) * orb.sum(axis=0)).max()
    d, u, l = eng._lsplit_tables(eng._lsizes(h), orb)
    cut = np.stack([b.sum(axis=(1, 2)) for b in u], axis=1)
    cut1 = np.stack(eng._lsplit_tables((1,) * L, out_one.cpu().numpy())[1], axis=1)[:, :, 0, 0]
    print(f"  max |bond_int - sum w flow| {dif:.3g} (max |flow| {np.abs(orb).max():.3g}); cuts: spread over the boundaries "
          f"{np.abs(cut - cut[:, :1]).max():.3g}, max |one group per layer - block sums| {np.abs(cut - cut1).max():.3g}")
    if hd is not None:
        td, tu, tl = eng._lsplit_tables((10,) * L, out_ten.cpu().numpy())
        D = out_dten.cpu().numpy()
        dd = max(max(np.abs(td[i] - D[:, 10 * i:10 * i + 10, 10 * i:10 * i + 10]).max() for i in range(L)),
                 max(np.abs(tu[i] - D[:, 10 * i:10 * i + 10, 10 * i + 10:10 * i + 20]).max() for i in range(L - 1)),
                 max(np.abs(tl[i] - D[:, 10 * i + 10:10 * i + 20, 10 * i:10 * i + 10]).max() for i in range(L - 1)))
        print(f"  max |layered - dense| over the group tables {dd:.3g} (max |dense| {np.abs(D).max():.3g})")
    raw = {"layers": L, "n": n, "k": K, "energies": m, "passes": a.passes, "calls": {}}
    for k, ts in times.items():
        print(f"  {k:24s} best {min(ts) * 1e3:9.2f} ms, median {np.median(ts) * 1e3:9.2f} ms, workspace {work[k] / 1e6:10.1f} MB")
        print("    kernels: " + ", ".join(f"{f} {ms:.3f} ms/{cnt}" for f, (ms, cnt) in fams[k].items() if cnt))
        raw["calls"][k] = {"seconds": ts, "workspace_bytes": work[k],
                           "kernel_ms_and_launches_of_the_best_pass": {f: list(v) for f, v in fams[k].items() if v[1]}}
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(raw, f, indent=1)
    if hd is not None:
        eng.sigma_free(hd)
    eng.layered_free(h)


if __name__ == "__main__":
    main()

"""Time the eigenchannel scattering states against the transmission eigenchannels on the same warm grid: 1-D chain leads
(N = 500, n_c = 50) and BASELINE C2's size with constant self-energies (N = 200, a CONST pair of K = 50), 256 real
energies each.  Both calls do identical work up to H; the states then run the eigenvector form of the Jacobi kernel and
the back-transformation Psi = G[:, I_s] L U.  Device-resident entry points (grid and results in HBM), --passes
alternating passes, wall time from call to the end of negf_sync (median, best, spread) and the library's "eig" / "zgemm"
family times of the best pass.  --baseline-only times transmission_channels alone (runs on a library that predates the
states); interleave such runs with full ones to compare the values-only "eig" time across two builds."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests.helpers import chain_lead, random_system        # noqa: E402
from gaunegf_amd.engine import get_engine                   # noqa: E402
from gaunegf_amd.surfG1D import surfG                       # noqa: E402

FAMILIES = ("chain1d", "chain1d_hit", "assemble", "inverse", "gamma", "zgemm", "eig")


def chain_handle(eng, N=500, nc=50, eta=1e-4):
    F, S = random_system(N, 3)
    aL, aR = chain_lead(nc, 31), chain_lead(nc, 32)
    g = surfG(F, S, [list(range(nc)), list(range(N - nc, N))], taus=[aL[2].copy(), aR[2].copy()],
              staus=[aL[3].copy(), aR[3].copy()], alphas=[aL[0], aR[0]], aOverlaps=[aL[1], aR[1]],
              betas=[aL[2], aR[2]], bOverlaps=[aL[3], aR[3]], eta=eta)
    eng.set_system(F, S)
    return g, g._negf_lower(eng)


def const_handle(eng, N=200, K=50):
    F, S = random_system(N, 200)
    rng = np.random.default_rng(200)
    sig = []
    for idx in (np.arange(K), np.arange(N - K, N)):
        A = rng.standard_normal((K, K)) + 1j * rng.standard_normal((K, K))
        s = np.zeros((N, N), complex); s[np.ix_(idx, idx)] = -0.05j * (A @ A.conj().T) / K
        sig.append(s)
    eng.set_system(F, S)
    return None, eng.sigma_const(sig)


def run(eng, label, h, E, K, passes, baseline_only):
    import torch
    dev = torch.device("cuda", eng.device)
    n, m = eng.n, E.size
    E_t = torch.view_as_complex(torch.from_numpy(np.ascontiguousarray(E, dtype=np.complex128).view(np.float64).reshape(-1, 2).copy())).to(dev)
    T_c = torch.zeros((m, K), dtype=torch.float64, device=dev)
    T_s = torch.zeros((m, K), dtype=torch.float64, device=dev)
    psi = torch.zeros((m, K, n), dtype=torch.complex128, device=dev)
    torch.cuda.synchronize(dev)
    calls = {"transmission_channels": lambda: eng.transmission_channels_dev(h, 1, 0, m, E_t.data_ptr(), K, T_c.data_ptr())}
    if not baseline_only:
        calls["channel_states"] = lambda: eng.channel_states_dev(h, 0, 1, m, E_t.data_ptr(), K, T_s.data_ptr(), psi.data_ptr())
    eng.profile(True)
    for fn in calls.values():                                # warm: workspace, g(E) cache, code objects
        fn(); eng.sync()
    times = {k: [] for k in calls}
    fams = {k: [] for k in calls}
    for _ in range(passes):                                  # alternating passes
        for k, fn in calls.items():
            eng.profile_reset()
            t0 = time.perf_counter(); fn(); eng.sync(); t = time.perf_counter() - t0
            times[k].append(t)
            fams[k].append({f: eng.profile_read(f) for f in FAMILIES})
    eng.profile(False)
    print(f"{label}: {m} energies, K = {K}, batch {eng.get_batch()}, {passes} alternating passes")
    med = {}
    for k, ts in times.items():
        ts = np.array(ts) * 1e3
        med[k] = np.median(ts)
        print(f"  {k:22s} wall median {np.median(ts):8.3f} ms, best {ts.min():8.3f}, worst {ts.max():8.3f}")
        for f in FAMILIES:
            v = np.array([p[f][0] for p in fams[k]])
            if fams[k][0][f][1]:
                print(f"    {f:12s} median {np.median(v):8.3f} ms, min {v.min():8.3f}, max {v.max():8.3f}  ({fams[k][0][f][1]} launches)")
    if not baseline_only:
        print(f"  channel_states / transmission_channels (median wall): {med['channel_states'] / med['transmission_channels']:.3f}")
        assert torch.equal(T_c.isnan(), T_s.isnan())
        print(f"  max |T_states - T_channels| = {float((T_s - T_c).abs().nan_to_num().max()):.2e}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--energies", type=int, default=256)
    ap.add_argument("--passes", type=int, default=10)
    ap.add_argument("--only", choices=("chain", "c2"), default=None)
    ap.add_argument("--baseline-only", action="store_true")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("time_channel_states.py needs a GPU (the engine has no CPU path)")
    torch.cuda.set_device(0)                                 # torch's runtime first, then the engine's context
    eng = get_engine()
    E = np.linspace(-2.0, 2.0, a.energies)
    if a.only in (None, "chain"):
        g, h = chain_handle(eng)
        run(eng, "chain leads (N = 500, n_c = 50, g(E) cache warm)", h, E, 50, a.passes, a.baseline_only)
    if a.only in (None, "c2"):
        _, h = const_handle(eng)
        run(eng, "C2 size (N = 200, CONST pair, K = 50)", h, E, 50, a.passes, a.baseline_only)
        eng.sigma_free(h)


if __name__ == "__main__":
    main()

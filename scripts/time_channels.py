"""Time the transmission eigenchannels (negf_transmission_channels) against the transmission (negf_transmission) on the
same warm grid: BASELINE C3 size (N = 500, two 1-D chain leads of n_c = 50, 2000 energies, g(E) cache warm) and N = 60
with constant self-energies (K = 10 + 12 contact orbitals).  Wall time of the host call (best of --reps) and the
library's per-family kernel times (negf_profile_read), the new "eig" family included."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests.helpers import chain_lead, random_system        # noqa: E402
from gaunegf_amd.engine import get_engine                   # noqa: E402
from gaunegf_amd.surfG1D import surfG                       # noqa: E402

FAMILIES = ("chain1d", "chain1d_hit", "small", "assemble", "inverse", "gamma", "zgemm", "trace", "eig")


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


def run(eng, label, h, E, reps):
    def timed(fn):
        best, out = 1e30, None
        for _ in range(reps):
            eng.profile_reset()
            t0 = time.perf_counter(); out = fn(); t = time.perf_counter() - t0
            if t < best:
                best, fam = t, {f: eng.profile_read(f) for f in FAMILIES}
        return best, fam, out
    eng.profile(True)
    T = eng.transmission(h, 0, -1, E)                       # warm: workspace, g(E) cache, code objects
    C = eng.transmission_channels(h, 0, -1, E)
    tT, famT, T = timed(lambda: eng.transmission(h, 0, -1, E))
    tC, famC, C = timed(lambda: eng.transmission_channels(h, 0, -1, E))
    eng.profile(False)
    sr = np.max(np.abs(C.sum(axis=1) - T) / np.maximum(np.abs(T), 1e-3))
    print(f"{label}: {E.size} energies, {C.shape[1]} channels; transmission {tT * 1e3:.2f} ms, channels {tC * 1e3:.2f} ms "
          f"(ratio {tC / tT:.3f}); sum rule max rel {sr:.1e}")
    for name, fam in (("transmission", famT), ("channels", famC)):
        parts = ", ".join(f"{f} {ms:.2f} ms/{n}" for f, (ms, n) in fam.items() if n)
        print(f"  {name:12s} kernels: {parts}")
    print(f"  eig family: {famC['eig'][0]:.3f} ms in {famC['eig'][1]} launches")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--energies", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", choices=("c3", "n60"), default=None)
    a = ap.parse_args()
    eng = get_engine()
    E = np.linspace(-2.0, 2.0, a.energies)
    if a.only in (None, "c3"):
        g, h = c3_handle(eng)
        run(eng, "C3 (N = 500, chain leads n_c = 50, g(E) cache warm)", h, E, a.reps)
    if a.only in (None, "n60"):
        _, h = const_handle(eng)
        run(eng, "N = 60, CONST Sigma (K_L = 10, K_R = 12)", h, E, a.reps)
        eng.sigma_free(h)


if __name__ == "__main__":
    main()

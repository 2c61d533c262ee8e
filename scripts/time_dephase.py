"""Time the lesser Green's function's weighted sum with floating dephasing probes against the paths without them, on the
same grid at the same commit: N = 500, two 1-D chain leads of n_c = 50 (renormalisation-decimation solver), 50 dephasing
probes of 9 orbitals, 256 real energies.

  gless_int              Engine.gless_int_dev(h, 0): one inverse, G Gamma_0 G^H, no probes at all
  tmatrix + gless_int    Engine.transmission_matrix_dev with the 50 probes, then gless_int_dev: what the path without the
                         feature runs on the device (two inverses; the host solve and the transfers are not counted)
  gless_int_probes       Engine.gless_int_probes_dev(h, 0) with the 50 probes: one inverse, T, R, D_0, G D_0 G^H

Device-resident calls (grid and results in HBM), --passes alternating passes, wall time from the call to the end of
negf_sync (best and median), and the library's per-family kernel times ("deph": the response solve and the coupling)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests.helpers import chain_lead, random_system         # noqa: E402
from gaunegf_amd.engine import get_engine                   # noqa: E402
from gaunegf_amd.transport import dephasing_probes          # noqa: E402

FAMILIES = ("chain1d_rd", "chain1d_rd_hit", "assemble", "inverse", "gamma", "zgemm", "trace", "tmat", "deph", "accumulate")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=500)
    ap.add_argument("--nc", type=int, default=50)
    ap.add_argument("--probes", type=int, default=50)
    ap.add_argument("--energies", type=int, default=256)
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--json", default=None, help="write the figures to this file as well")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("time_dephase.py needs a GPU (the engine has no CPU path)")
    torch.cuda.set_device(0)
    from gaunegf_amd.surfG1D import surfG
    eng = get_engine()
    n, nc, m = a.n, a.nc, a.energies
    F, S = random_system(n, 500)
    lead = [chain_lead(nc, 40 + k) for k in range(2)]
    ci = [list(range(nc)), list(range(n - nc, n))]
    rng = np.random.default_rng(500)
    taus = [0.2 * rng.standard_normal((nc, nc)) for _ in range(2)]
    staus = [0.02 * rng.standard_normal((nc, nc)) for _ in range(2)]
    g = surfG(F, S, ci, taus=taus, staus=staus, alphas=[l[0] for l in lead], aOverlaps=[l[1] for l in lead],
              betas=[l[2] for l in lead], bOverlaps=[l[3] for l in lead], eta=1e-3, solver='doubling')
    # probes of 9 consecutive orbitals spread over the device region between the leads
    starts = np.linspace(nc, n - nc - 9, a.probes).astype(int)
    probes = dephasing_probes(S, [np.arange(s0, s0 + 9) for s0 in starts], 0.1)
    eng.set_system(F, S)
    h = g._negf_lower(eng)
    C = 2 + len(probes)
    dev = torch.device("cuda", eng.device)
    E_t = torch.from_numpy(np.ascontiguousarray(np.linspace(-2.0, 2.0, m), dtype=np.complex128)).to(dev)
    w_t = torch.from_numpy(np.ascontiguousarray(np.cos(np.arange(m)) + 1.5, dtype=np.complex128)).to(dev)
    TC = torch.zeros((m, C, C), dtype=torch.float64, device=dev)
    out = torch.zeros((n, n), dtype=torch.complex128, device=dev)
    torch.cuda.synchronize(dev)

    def synced(fn):
        def call():
            fn(); eng.sync()
        return call
    calls = {
        "gless_int": synced(lambda: eng.gless_int_dev(h, 0, m, E_t.data_ptr(), w_t.data_ptr(), out.data_ptr())),
        "tmatrix + gless_int": synced(lambda: (eng.transmission_matrix_dev(h, m, E_t.data_ptr(), TC.data_ptr(), probes),
                                               eng.gless_int_dev(h, 0, m, E_t.data_ptr(), w_t.data_ptr(), out.data_ptr()))),
        "gless_int_probes": synced(lambda: eng.gless_int_probes_dev(h, 0, m, E_t.data_ptr(), w_t.data_ptr(), out.data_ptr(),
                                                                    probes)),
    }
    eng.profile(True)
    for fn in calls.values():                                # warm: workspace, staging, code objects, the g(E) cache
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
    base = min(times["gless_int"])
    print(f"N = {n}, chain leads n_c = {nc} (doubling), {len(probes)} probes of 9, {m} energies, batch {eng.get_batch()}, "
          f"{a.passes} alternating passes")
    report = {"n": n, "nc": nc, "probes": len(probes), "energies": m, "batch": eng.get_batch(), "passes": a.passes, "calls": {}}
    for k, ts in times.items():
        print(f"  {k:20s} best {min(ts) * 1e3:8.2f} ms, median {np.median(ts) * 1e3:8.2f} ms, ratio to gless_int (best) {min(ts) / base:.3f}")
        print("    kernels: " + ", ".join(f"{f} {ms:.3f} ms/{cnt}" for f, (ms, cnt) in fams[k].items() if cnt))
        report["calls"][k] = {"best_ms": min(ts) * 1e3, "median_ms": float(np.median(ts)) * 1e3, "ratio_best": min(ts) / base,
                              "kernels_ms": {f: ms for f, (ms, cnt) in fams[k].items() if cnt}}
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()

"""Time the two solvers of the 1-D chain surface Green's function against each other on C3 (N = 500, n_c = 50,
eta = 1e-4, 2000 Legendre points on [-2, 2]): the GrInt step and the chain phase alone (the library's hipEvents, families
"chain1d" and "chain1d_rd"), g(E) cache off, one process.  After warming both, the two solvers' passes ALTERNATE
(>= 10 each), so that clock and thermal drift hit both alike; medians and spread are reported, with the mean step /
sweep counts, how many units the default solver leaves unconverged, and the flop ratio counted from negf_last_iters
(a sweep is one inverse and two products, 24 n^3; a doubling step one inverse and six products, 56 n^3).

    python scripts/time_chain_rd.py [passes]          (default 10)
"""
import os
import sys
import time

os.environ.setdefault("NEGF_CHAIN_CACHE", "0")      # time the solvers, not the g(E) cache
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import oracle
from scripts.bench_configs import _c3_system
from gaunegf_amd.engine import get_engine
from gaunegf_amd.integrate import GrInt

passes = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 10
M = 2000
F, S, g_fp, _ = _c3_system()
_, _, g_rd, _ = _c3_system()
g_rd.solver = "doubling"
E, _ = oracle.real_axis_grid(-2.0, 2.0, M, 0.0)
w = np.ones_like(E) * (4.0 / M)
eng = get_engine()
eng.set_chain_cache(0)
solvers = {"fixed-point": (g_fp, "chain1d"), "doubling": (g_rd, "chain1d_rd")}
counts, result = {}, {}
for name, (g, fam) in solvers.items():               # warm: allocations, code objects, the job order of the default solver
    for _ in range(2):
        result[name] = GrInt(F, S, g, E, w)
    it, cv = eng.last_iters_dev(g._negf_lower(eng), M, 2)
    counts[name] = (it.astype(np.float64), cv)
eng.profile(True)
step = {k: [] for k in solvers}
chain = {k: [] for k in solvers}
for _ in range(passes):
    for name, (g, fam) in solvers.items():
        eng.profile_reset()
        t0 = time.perf_counter()
        GrInt(F, S, g, E, w)
        step[name].append((time.perf_counter() - t0) * 1e3)
        chain[name].append(eng.profile_read(fam)[0])
eng.profile(False)


def stat(v):
    v = np.asarray(v)
    return f"median {np.median(v):8.2f} ms  (min {v.min():8.2f}, max {v.max():8.2f}, n = {v.size})"


n = 50
for name in solvers:
    it, cv = counts[name]
    print(f"{name:12s} GrInt step   {stat(step[name])}")
    print(f"{name:12s} chain phase  {stat(chain[name])}")
    print(f"{name:12s} mean {'steps' if name == 'doubling' else 'sweeps'} per unit {it.mean():.1f} (max {int(it.max())}), "
          f"units not converged {int((cv == 0).sum())} of {cv.size}")
flops_fp = 24.0 * n ** 3 * counts["fixed-point"][0].sum()
flops_rd = 56.0 * n ** 3 * counts["doubling"][0].sum()
r_chain = np.median(chain["fixed-point"]) / np.median(chain["doubling"])
print(f"counted flop ratio fixed-point / doubling {flops_fp / flops_rd:.1f}; measured chain-phase ratio {r_chain:.1f}; "
      f"step ratio {np.median(step['fixed-point']) / np.median(step['doubling']):.2f}")
print(f"algorithmic rate: fixed-point {flops_fp / np.median(chain['fixed-point']) / 1e9:.2f} TFLOP/s, "
      f"doubling {flops_rd / np.median(chain['doubling']) / 1e9:.2f} TFLOP/s")
d = np.linalg.norm(result["fixed-point"] - result["doubling"]) / np.linalg.norm(result["doubling"])
print(f"relative Frobenius distance of the two GrInt results {d:.3g} (the default solver's unconverged units)")

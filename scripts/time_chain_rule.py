"""Which schedule the repeated evaluation of the C3 grid (2000 energies x 2 leads of n_c = 50) should run under:
  (a) the launcher's default rule, negf_set_chain_round_robin(-1, 0),
  (b) the job queue started in the learned order, (100, 0),
  (c) the job queue started in launch order -- what the first evaluation of a fresh provider runs.
(a) and (b) are the third and fourth evaluation of a provider, (c) the first evaluation of every fresh provider.  One
fresh provider per series, the series alternate; GrInt through the device-pointer entry point, workspace allocated
beforehand, g(E) cache off, a fence around each call.  Prints every run, then median and spread (max - min) of each rule.

    python scripts/time_chain_rule.py [runs, default 6]
"""
import os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch, bench
from gaunegf_amd.engine import Engine
from gaunegf_amd.surfG1D import surfG

RUNS = int(sys.argv[1]) if len(sys.argv) > 1 else 6
N, NC, M = 500, 50, 2000
F, S, inds, kw = bench.c3_system(N, NC, 1e-4)
Eg, wg = bench.legendre_grid(M, -2.0, 2.0)
torch.cuda.init()
eng = Engine(0)
stream = torch.cuda.current_stream(); eng.set_stream(stream.cuda_stream)
eng.set_system(F, S); eng.set_chain_cache(0)
dev = torch.device("cuda", 0)
to_dev = lambda a: torch.view_as_complex(torch.from_numpy(np.ascontiguousarray(a, dtype=np.complex128).view(np.float64).reshape(-1, 2).copy())).to(dev)
E_dev, w_dev = to_dev(Eg), to_dev(wg)
out = torch.zeros((N, N), dtype=torch.complex128, device=dev)

def evaluate(h):
    torch.cuda.synchronize(); t = time.perf_counter()
    eng.gr_int_dev(h, M, E_dev.data_ptr(), w_dev.data_ptr(), out.data_ptr())
    torch.cuda.synchronize(); return (time.perf_counter() - t) * 1e3

def series(rule):
    """first, third and fourth evaluation of a fresh provider under `rule`"""
    eng.set_chain_round_robin(*rule)
    lead = surfG(F, S, inds, **kw); h = lead._negf_lower(eng)       # (the handle lives as long as the lead)
    t = [evaluate(h) for _ in range(4)]
    return t[0], t[2], t[3], bool(torch.equal(out, ref))

lead0 = surfG(F, S, inds, **kw); evaluate(lead0._negf_lower(eng))       # allocations
ref = out.clone()
times = {"a": [], "b": [], "c": []}
for run in range(RUNS):
    for name, rule in (("a", (-1, 0)), ("b", (100, 0))):
        t1, t3, t4, same = series(rule)
        times["c"].append(t1); times[name] += [t3, t4]
        print(f"run {run} rule {rule}: first (c) {t1:.1f} ms  third ({name}) {t3:.1f} ms  fourth ({name}) {t4:.1f} ms   identical to the reference run: {same}", flush=True)
eng.set_chain_round_robin(-1, 0)
label = {"a": "(a) default rule, repeated evaluation", "b": "(b) queue, learned order", "c": "(c) queue, launch order"}
for name in "abc":
    t = np.array(times[name])
    print(f"{label[name]:40s} median {np.median(t):.1f} ms  spread {t.max() - t.min():.1f} ms  (min {t.min():.1f}, max {t.max():.1f}, {t.size} evaluations)")

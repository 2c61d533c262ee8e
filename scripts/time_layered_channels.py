"""Time the layered transmission eigenchannels against the layered transmission on the same grid: README's layered
shape (20 layers of 100 orbitals, const terminals on all 100 orbitals of either end layer, 256 real energies), and one
line for K = 512 (two layers of 512, 16 energies).  Both calls do the same corner sweep, Gamma blocks and gather; the
transmission then takes two products and a trace, the channel call the Cholesky factor, three products and the
eigensolver -- the difference is the "eig" family.  Device-resident entry points (grid and results in HBM, buffers of the
HIP runtime the library is linked against), --passes alternating passes after a warm-up, wall time from the call to the
end of negf_sync, the library's per-family kernel times of the best pass, and the work areas of each call.  Writes one
JSON document (--out)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gaunegf_amd import layered as ly                        # noqa: E402
from gaunegf_amd.engine import get_engine                    # noqa: E402

FAMILIES = ("rgf", "inverse", "gamma", "zgemm", "trace", "eig")


def wire(L, n, seed, complex_h=False):
    rng = np.random.default_rng(seed)

    def rnd(a, b):
        x = rng.standard_normal((a, b))
        return x + 1j * rng.standard_normal((a, b)) if complex_h else x
    Fd, Sd, Fu, Su = [], [], [], []
    for _ in range(L):
        a = rnd(n, n); s = rnd(n, n)
        Fd.append((a + a.conj().T) / np.sqrt(2 * n))
        Sd.append(np.eye(n) + 0.1 * (s + s.conj().T) / np.sqrt(2 * n))
    for _ in range(L - 1):
        Fu.append(0.6 * rnd(n, n) / np.sqrt(n)); Su.append(0.05 * rnd(n, n) / np.sqrt(n))
    sig = []
    for _ in range(2):
        A = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
        B = rng.standard_normal((n, n))
        sig.append(0.05 * (B + B.T) - 0.5j * (0.3 * np.eye(n) + 0.4 * (A @ A.conj().T) / (2 * n)))
    return Fd, Fu, Sd, Su, sig


class Hip:
    def __init__(self):
        self.lib = C.CDLL("libamdhip64.so.7")
        self.lib.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.lib.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.lib.hipFree.argtypes = [C.c_void_p]
        self.bufs = []

    def buf(self, nbytes, src=None):
        p = C.c_void_p()
        assert self.lib.hipMalloc(C.byref(p), nbytes) == 0
        self.bufs.append(p)
        if src is not None:
            assert self.lib.hipMemcpy(p, src.ctypes.data_as(C.c_void_p), nbytes, 1) == 0
        return p.value

    def fetch(self, ptr, out):
        assert self.lib.hipMemcpy(out.ctypes.data_as(C.c_void_p), ptr, out.nbytes, 2) == 0
        return out

    def free(self):
        for p in self.bufs:
            self.lib.hipFree(p)
        self.bufs = []


def measure(eng, hip, L, n, m, passes, seed):
    Fd, Fu, Sd, Su, sig = wire(L, n, seed)
    E = np.ascontiguousarray(np.linspace(-1.0, 1.0, m), dtype=np.complex128)
    h = eng.layered_create(Fd, Fu, Sd, Su)
    out = {"layers": L, "n": n, "k": n, "energies": m, "passes": passes, "calls": {}}
    try:
        tl = eng.layered_terminal_const(h, 0, np.arange(n), sig[0])
        tr = eng.layered_terminal_const(h, L - 1, np.arange(n), sig[1])
        dE, dT, dC = hip.buf(E.nbytes, E), hip.buf(8 * m), hip.buf(8 * m * n)
        calls = {"layered_transmission_dev": lambda: eng.layered_transmission_dev(h, tr, tl, m, dE, dT),
                 "layered_transmission_channels_dev": lambda: ly.layered_transmission_channels_dev(eng, h, tr, tl, m, dE, n, dC)}
        res = {k: {"seconds": [], "workspace_bytes": 0, "kernel_ms_and_launches_of_the_best_pass": {}} for k in calls}
        eng.profile(True)
        for name, fn in calls.items():                             # warm-up: code objects, work areas
            fn(); eng.sync()
            res[name]["workspace_bytes"] = eng.layered_workspace_bytes(h)
        for _ in range(passes):
            for name, fn in calls.items():
                eng.profile_reset()
                t0 = time.perf_counter()
                fn(); eng.sync()
                dt = time.perf_counter() - t0
                r = res[name]
                if not r["seconds"] or dt < min(r["seconds"]):
                    r["kernel_ms_and_launches_of_the_best_pass"] = {f: list(eng.profile_read(f)) for f in FAMILIES
                                                                    if eng.profile_read(f)[1]}
                r["seconds"].append(dt)
        eng.profile(False)
        T = hip.fetch(dT, np.zeros(m)); Tn = hip.fetch(dC, np.zeros((m, n)))
        out["sum_rule_worst_relative"] = float(np.max(np.abs(Tn.sum(axis=1) - T) / np.abs(T)))
        for name, r in res.items():
            r["best_s"], r["median_s"] = float(np.min(r["seconds"])), float(np.median(r["seconds"]))
        out["calls"] = res
        # what the dense engine would hold for the same grid: three N x N work areas per energy in flight
        N = L * n
        out["dense_transmission_workspace_bytes_per_energy"] = 3 * 16 * N * N
    finally:
        eng.layered_free(h)
        hip.free()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--out", default="layered_channels_timing.json")
    args = ap.parse_args()
    eng, hip = get_engine(), Hip()
    doc = {"readme_shape": measure(eng, hip, 20, 100, 256, args.passes, 1),
           "k512": measure(eng, hip, 2, 512, 16, max(3, args.passes // 2), 2)}
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    for key, d in doc.items():
        for name, r in d["calls"].items():
            print(f"{key} {name}: best {r['best_s'] * 1e3:.2f} ms, median {r['median_s'] * 1e3:.2f} ms, "
                  f"workspace {r['workspace_bytes'] / 1e6:.1f} MB, kernels {r['kernel_ms_and_launches_of_the_best_pass']}")
        print(f"{key} sum rule {d['sum_rule_worst_relative']:.2e}")

"""
The floating dephasing probes on the CPU: transport.probe_response (the host form of the response R) against
tests/dephase_ref.py and its extended-precision truth, the identities it shares with effective_transmission, the
calibration of the bar the device is held to (C_DEPH, the procedure of test_tmatrix_host.test_calibration), and the
energy sharding of the front ends (gloo, world_size 2, a stub engine: no GPU in these processes).
"""
import os
import socket

import numpy as np
import pytest

import dephase_ref as dr
import tmatrix_ref as tr


def _T64(c, E):
    return tr.tmatrix(c.F, c.S, c.terms, E)


def _host(T, n_real):
    from gaunegf_amd.transport import probe_response
    return probe_response(np.asarray(T)[None], n_real)[0]


# --------------------------------------------------------------------------- the host form
@pytest.mark.parametrize("idx", range(len(dr.cases())))
def test_host_form_against_restatement_rows_and_identity(idx):
    from gaunegf_amd.transport import effective_transmission
    c = dr.cases()[idx]
    P = len(c.probes)
    for E in c.energies:
        T = _T64(c, E)
        R = _host(T, c.n_c)
        ref = dr.response(T, c.n_c)
        assert R.shape == (P, c.n_c)
        par = np.abs(R - ref).max()
        on = np.array([np.any(blk) for _, blk in c.probes])
        sums = np.abs(R[on].sum(axis=1) - 1.0).max()
        print(f"dephase host {c.name} E={E:.6g}: |R - restatement| {par:.3g}, |row sum - 1| {sums:.3g}, min R {R.min():.3g}")
        assert par <= 1e-10, (c.name, E, par)
        assert sums <= 1e-10, (c.name, E, sums)
        assert not np.any(R[~on])                              # decoupled probes: exact zeros
        assert R.min() >= -1e-10 and R.max() <= 1 + 1e-10
        # (I2) T_eff[d][s] = T[d][s] + sum_p T[d][p] R[p][s] is effective_transmission's on the same T
        tmax = np.abs(T).max()
        for s in range(c.n_c):
            for d in range(c.n_c):
                if d == s:
                    continue
                mine = T[d, s] + T[d, c.n_c:] @ R[:, s]
                theirs = effective_transmission(T[None], c.n_c, source=s, drain=d)[0]
                assert abs(mine - theirs) <= 1e-12 * tmax, (c.name, E, d, s, mine, theirs)


def test_nan_matrices_give_nan_and_shapes():
    from gaunegf_amd.transport import probe_response
    c = dr.shape_a()
    T = np.stack([_T64(c, E) for E in c.energies[:3]])
    T[1] = np.nan
    R = probe_response(T, c.n_c)
    assert np.all(np.isnan(R[1])) and np.all(np.isfinite(R[[0, 2]]))
    assert np.array_equal(R[0], _host(T[0], c.n_c))
    assert probe_response(T[:0], c.n_c).shape == (0, len(c.probes), c.n_c)
    assert probe_response(T[:, :2, :2], 2).shape == (3, 0, 2)
    with pytest.raises(ValueError):
        probe_response(T, 0)


def test_host_form_against_truth():
    for tag, c, E, R, _, _, ea, eb in dr.truth_table():
        err = dr.rel_err(_host(_T64(c, E), c.n_c), R)
        bar = dr.C_DEPH * max(ea, eb)
        print(f"dephase host {tag}: error {err:.3g} (bar {bar:.3g}, float64 forms {ea:.3g} / {eb:.3g})")
        assert err <= bar, (tag, err, bar)
        on = np.array([np.any(blk) for _, blk in c.probes])
        assert abs(np.asarray(R[on].sum(axis=1) - 1, dtype=float)).max() <= 1e-15, tag     # the truth's own row sums


def test_gless_restatement_against_truth():
    """dephase_ref.gless_probes (float64) against the clongdouble form, every contact and the total, on shape (a)"""
    c = dr.shape_a()
    E = c.energies[:2]
    w = np.array([0.75, 1.25])
    for s in (0, 1, None):
        ref = dr.gless_probes(c.F, c.S, c.terms, c.n_c, s, E, w)
        truth = sum(dr.LD(wk) * dr.truth_row(c, float(e))[1][-1 if s is None else s] for e, wk in zip(E, w))
        err = dr.rel_err(ref, truth)
        print(f"dephase host gless a24 s={s}: float64 restatement error {err:.3g}")
        assert err <= 1e-12, (s, err)
        assert np.abs(ref - ref.conj().T).max() <= 1e-13 * np.abs(ref).max()


def test_singular_w_gives_nan_for_that_energy_only():
    """probes that see only each other: W is singular -- NaN for that energy, the others as they are without it"""
    from gaunegf_amd.transport import probe_response
    c = dr.shape_a()
    T = np.stack([_T64(c, E) for E in c.energies[:3]])
    lone = np.zeros_like(T[1])
    lone[0, 1] = lone[1, 0] = 0.5
    lone[3, 4] = lone[4, 3] = 0.25                           # probes 1 and 2 exchange with each other alone
    T[1] = lone
    R = probe_response(T, c.n_c)
    assert np.all(np.isnan(R[1]))
    assert np.array_equal(R[[0, 2]], probe_response(T[[0, 2]], c.n_c))


def test_size_class_constants_agree():
    """Engine.DEPH_LDS_MAX_P / DEPH_LDS_MAX_RHS are copies of negf_common.h's: the GPU tests take their edge sizes from them"""
    import re
    from gaunegf_amd.engine import Engine
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(here, "gaunegf_amd", "csrc", "negf_common.h")).read()
    m = re.search(r"constexpr int DEPH_LDS_MAX_P = (\d+), DEPH_LDS_MAX_RHS = (\d+);", text)
    assert m, "negf_common.h no longer declares the size-class limits in this form"
    assert (int(m.group(1)), int(m.group(2))) == (Engine.DEPH_LDS_MAX_P, Engine.DEPH_LDS_MAX_RHS)


# --------------------------------------------------------------------------- the calibration of the device's bar
def test_calibration():
    r, worst, at, r_at, least = 1.0, 0.0, None, None, np.inf
    for tag, *_, ea, eb in dr.truth_table():
        if max(ea / eb, eb / ea) > r:
            r, r_at = max(ea / eb, eb / ea), tag
        if max(ea, eb) > worst:
            worst, at = max(ea, eb), tag
        least = min(least, ea, eb)
    c_deph = 2.0 ** np.ceil(np.log2(2.0 * r))
    print(f"dephase calibration: R {r:.3g} (at {r_at}) -> C {c_deph:g} (dephase_ref.C_DEPH = {dr.C_DEPH}); float64 errors "
          f"{least:.3g} ... {worst:.3g} (worst at {at})")
    assert c_deph == dr.C_DEPH, (r, c_deph, dr.C_DEPH)


# --------------------------------------------------------------------------- sharded = single process (gloo, two ranks)
class _StubEngine:
    """What the front ends ask of an engine, answered by the numpy restatement (no GPU in these processes)."""
    device = None                                          # host only: the integrals take the host sum under active ranks

    def __init__(self):
        self.n, self.F, self.S, self.contacts, self.generation = 0, None, None, {}, 0

    def set_system(self, F, S):
        self.F, self.S, self.n = np.asarray(F, dtype=complex), np.asarray(S, dtype=complex), np.asarray(F).shape[0]

    def sigma_const(self, mats):
        terms = []
        for s in mats:
            s = np.asarray(s)
            ix = np.nonzero(np.abs(s).sum(axis=0) + np.abs(s).sum(axis=1))[0]
            terms.append((ix, s[np.ix_(ix, ix)]))
        self.contacts[len(self.contacts)] = terms
        return len(self.contacts) - 1

    def sigma_free(self, h):
        pass

    def terminal_count(self, h, probes=None):
        return len(self.contacts[h]) + (len(probes) if probes else 0)

    def _terms(self, h, probes):
        return self.contacts[h] + [(np.asarray(i), np.asarray(b)) for i, b in probes]

    def probe_response(self, h, E, probes):
        nc = len(self.contacts[h])
        return np.stack([dr.response(tr.tmatrix(self.F, self.S, self._terms(h, probes), e), nc) for e in np.real(E)]
                        ).reshape(-1, len(probes), nc)

    def gless_int_probes(self, h, ind, E, w, probes):
        nc = len(self.contacts[h])
        s = None if ind is None else ind % nc
        return dr.gless_probes(self.F, self.S, self._terms(h, probes), nc, s, np.real(E), w)


class _StubProvider:
    def __init__(self, sigmas):
        self.sigmas = sigmas

    def _negf_lower(self, engine):
        return engine.sigma_const(self.sigmas)


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _evaluate():
    from gaunegf_amd import integrate, transport
    c = dr.shape_a()
    E = np.linspace(-1.5, 1.5, 7)                          # 7 energies on 2 ranks: ragged shards
    w = np.cos(np.arange(E.size)) + 1.5
    stub = _StubEngine()
    keep = integrate.get_engine, transport.get_engine
    integrate.get_engine = transport.get_engine = lambda: stub
    try:
        g = _StubProvider(c.contact_sigmas())
        sig = c.contact_sigmas()
        sc = transport.SigmaCalculator(sig[0], sig[1])
        return (integrate.GrLessIntProbes(c.F, c.S, g, E, w, c.probes, ind=0),
                integrate.GrLessIntProbes(c.F, c.S, g, E, w, c.probes),
                transport.calculate_probe_response(c.F, c.S, sc, E, c.probes))
    finally:
        integrate.get_engine, transport.get_engine = keep


def _worker(rank, world, port, q):
    import torch.distributed as dist
    from gaunegf_amd import distributed as D
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        D.enable()
        assert D.is_active() and D.rank_world() == (rank, world)
        res = _evaluate()
        if rank == 0:
            q.put(res)
    finally:
        D.disable()
        dist.destroy_process_group()


def test_sharded_matches_single_process():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = q.get(timeout=120)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    ref = _evaluate()
    c = dr.shape_a()
    assert ref[0].shape == (c.n, c.n) and ref[2].shape == (7, len(c.probes), c.n_c)
    assert np.array_equal(got[2], ref[2])                  # an all-gather of the shards moves the values, exactly
    for a, b in zip(got[:2], ref[:2]):                     # a sum over two ranks' partial sums: another order of additions
        assert np.abs(a - b).max() <= 1e-13 * np.abs(b).max()
    assert np.abs(ref[0] - dr.gless_probes(c.F, c.S, c.terms, c.n_c, 0, np.linspace(-1.5, 1.5, 7), np.cos(np.arange(7)) + 1.5)).max() == 0

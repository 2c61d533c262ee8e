"""Eigenchannel scattering states without a GPU: the entry points are bound and refuse to run on the host (no CPU
fallback), the numpy restatement the GPU tests compare against satisfies the states' identities on those tests' inputs,
the constant of the eigh bounds is what the calibration rule gives, and calculate_channel_states shards its energy grid
over ranks and returns the rows in grid order."""
import os
import socket

import numpy as np
import pytest

import channel_states_ref as R


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def test_channel_state_symbols_bound():
    from gaunegf_amd import _lib
    names = ("negf_eigh_batched", "negf_channel_states_count", "negf_channel_states", "negf_channel_states_dev")
    for name in names:
        assert name in _lib.SIGNATURES
    lib = _lib.load()
    for name in names:
        assert hasattr(lib, name)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "negf.h")).read()
    for name in names:
        assert f"int {name}(negf_ctx* ctx" in header


def test_no_cpu_fallback_for_channel_states():
    from gaunegf_amd import _lib
    if _lib.load().negf_device_count() > 0:
        pytest.skip("GPU present")
    from gaunegf_amd.engine import Engine
    from gaunegf_amd.transport import SigmaCalculator, calculate_channel_states, cohTransChannelStates
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Engine().eigh(np.eye(3)[None])
    n = 6
    F = np.zeros((n, n)); S = np.eye(n)
    s1 = np.zeros((n, n), complex); s1[0, 0] = -0.1j
    s2 = np.zeros((n, n), complex); s2[-1, -1] = -0.1j
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        calculate_channel_states(F, S, SigmaCalculator(s1, s2), np.array([0.1, 0.2]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cohTransChannelStates([0.1], F, S, s1, s2, nchan=1)


@pytest.mark.parametrize("c", R.CONST_CASES + ["rank3"])
def test_reference_satisfies_the_identities(c):
    """psi_a^H Gamma_d psi_b = T_a delta_ab, sum T_n = Re Tr[Gamma_d G Gamma_s G^H], Psi Psi^H = G Gamma_s G^H, and the
    nonzero T_n are the eigenvalues of t^H t (t = Gamma_d^1/2 G[I_d, I_s] Gamma_s^1/2), all to <= 1e-12 relative."""
    case = R.rank_deficient_case() if c == "rank3" else R.const_case(*c)
    gs, gd = R.gamma(case["ss"]), R.gamma(case["sd"])
    Is, Id = case["Is"], case["Id"]

    def psd_sqrt(M):
        w, V = np.linalg.eigh(0.5 * (M + M.conj().T))
        return (V * np.sqrt(np.clip(w, 0.0, None))) @ V.conj().T

    for e in case["E"]:
        G = R.case_green(case, e)
        T, psi = R.channel_states_ref(G, gs, gd, Is, Id)
        assert len(T) == (3 if c == "rank3" else len(Is)) and psi.shape == (len(T), G.shape[0])
        orth, srule, spec = R.identity_errors(T, psi, G, gs, gd)
        assert orth <= 1e-12 and srule <= 1e-12 and spec <= 1e-12, (c, e, orth, srule, spec)
        t = psd_sqrt(gd[np.ix_(Id, Id)]) @ G[np.ix_(Id, Is)] @ psd_sqrt(gs[np.ix_(Is, Is)])
        tt = np.sort(np.linalg.eigvalsh(t.conj().T @ t))[::-1][:len(T)]
        assert np.max(np.abs(tt - T)) <= 1e-12 * T[0]
        assert np.all(np.diff(T) <= 0)
        for s in psi:                                            # the gauge
            i = int(np.argmax(np.abs(s) ** 2))
            assert abs(s[i].imag) <= 1e-14 * abs(s[i]) and s[i].real > 0
        # the parity test needs singleton clusters to say anything
        assert sum(len(g) == 1 for g in R.clusters(T, 1e-3 * T[0])) >= 2


def test_eigh_constant_is_calibrated():
    """EIGH_C is at least twice the worst residual / orthonormality ratio of numpy.linalg.eigh and of the numpy
    restatement of the device's Jacobi on the GPU test's inputs, and the smallest such power of two."""
    worst = 0.0
    mats = [A for K in R.EIGH_KS for A in R.eigh_random(K)] + R.eigh_special()
    for A in mats:
        w, V = np.linalg.eigh(A)
        wj, Vj = R.jacobi_eigh(A)
        assert np.max(np.abs(wj - w)) <= 1e-12 * max(np.linalg.norm(A), 1e-300)
        worst = max(worst, *R.eigh_ratios(A, w, V), *R.eigh_ratios(A, wj, Vj))
    assert 2.0 * worst <= R.EIGH_C, worst
    assert R.EIGH_C == 2.0 ** np.ceil(np.log2(2.0 * 19.53))      # the recorded worst ratio (channel_states_ref.py)


def test_pivoted_cholesky_restatement():
    rng = np.random.default_rng(2)
    A = rng.standard_normal((9, 3)) + 1j * rng.standard_normal((9, 3))
    G = A @ A.conj().T
    L = R.pivoted_cholesky(G)
    assert L.shape == (9, 3) and np.linalg.norm(L @ L.conj().T - G) <= 1e-13 * np.linalg.norm(G)
    assert R.pivoted_cholesky(np.zeros((4, 4))).shape == (4, 0)


def _fake_states(F, S, calc, E, spin, nchan, source):
    """Stands in for the GPU: T row of an energy E is (E, 2E, ...), psi[k, c, i] = E (c + 1) + 1j (i + 1) E."""
    E = np.asarray(E).real
    N = np.asarray(F).shape[0] // (2 if spin in ('u', 'ro') else 1)
    T = E[:, None] * np.arange(1, nchan + 1)[None, :]
    psi = T[:, :, None] + 1j * E[:, None, None] * np.arange(1, N + 1)[None, None, :]
    return ((T, psi), (-T, -psi)) if spin in ('u', 'ro') else (T, psi)


def _worker(rank, world, port, q):
    import torch.distributed as dist
    from gaunegf_amd import distributed as D
    from gaunegf_amd import transport
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        D.enable()
        transport._channel_states_batch = _fake_states
        n = 4
        F = np.zeros((n, n)); S = np.eye(n)
        calc = transport.SigmaCalculator(np.zeros((n, n)), np.zeros((n, n)))
        E = np.linspace(-1.0, 1.0, 13)                        # 13 energies over 2 ranks: ragged shards
        r = transport.calculate_channel_states(F, S, calc, E, nchan=3)
        u = transport.calculate_channel_states(F, S, calc, E, spin='u', nchan=2)
        if rank == 0:
            q.put((r, u))
    finally:
        D.disable()
        dist.destroy_process_group()


def test_sharded_channel_states_in_grid_order():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    (T, psi), ((Tu, pu), (Td, pd)) = q.get(timeout=120)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    E = np.linspace(-1.0, 1.0, 13)
    n = 4
    eT, ep = _fake_states(np.zeros((n, n)), None, None, E, 'r', 3, 0)
    assert T.shape == (13, 3) and psi.shape == (13, 3, n) and psi.dtype == np.complex128
    assert np.array_equal(T, eT) and np.array_equal(psi, ep)
    (eTu, epu), (eTd, epd) = _fake_states(np.zeros((n, n)), None, None, E, 'u', 2, 0)
    assert pu.shape == (13, 2, n // 2)
    assert np.array_equal(Tu, eTu) and np.array_equal(pu, epu) and np.array_equal(Td, eTd) and np.array_equal(pd, epd)

"""Transmission eigenchannels without a GPU: the entry points are bound, refuse to run on the host (no CPU fallback),
and calculate_transmission_channels shards its energy grid over ranks and returns the rows in grid order."""
import os
import socket

import numpy as np
import pytest


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def test_channel_symbols_bound():
    from gaunegf_amd import _lib
    for name in ("negf_eigvalsh_batched", "negf_channel_count", "negf_transmission_channels",
                 "negf_transmission_channels_dev"):
        assert name in _lib.SIGNATURES
    lib = _lib.load()
    assert hasattr(lib, "negf_transmission_channels") and hasattr(lib, "negf_eigvalsh_batched")


def test_no_cpu_fallback_for_channels():
    from gaunegf_amd import _lib
    if _lib.load().negf_device_count() > 0:
        pytest.skip("GPU present")
    from gaunegf_amd.engine import Engine
    from gaunegf_amd.transport import SigmaCalculator, calculate_transmission_channels, cohTransChannels
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Engine().eigvalsh(np.eye(3)[None])
    n = 6
    F = np.zeros((n, n)); S = np.eye(n)
    s1 = np.zeros((n, n), complex); s1[0, 0] = -0.1j
    s2 = np.zeros((n, n), complex); s2[-1, -1] = -0.1j
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        calculate_transmission_channels(F, S, SigmaCalculator(s1, s2), np.array([0.1, 0.2]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cohTransChannels([0.1], F, S, s1, s2, nchan=1)


def _fake_batch(F, S, calc, E, spin, nchan):
    """Stands in for the GPU: row k of an energy E is (E, 2E, ... nchan E) -- which rows come back where is visible."""
    rows = np.asarray(E).real[:, None] * np.arange(1, nchan + 1)[None, :]
    return (rows, -rows) if spin in ('u', 'ro') else rows


def _worker(rank, world, port, q):
    import torch.distributed as dist
    from gaunegf_amd import distributed as D
    from gaunegf_amd import transport
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        D.enable()
        transport._channels_batch = _fake_batch
        n = 4
        F = np.zeros((n, n)); S = np.eye(n)
        calc = transport.SigmaCalculator(np.zeros((n, n)), np.zeros((n, n)))
        E = np.linspace(-1.0, 1.0, 13)                        # 13 energies over 2 ranks: ragged shards
        T = transport.calculate_transmission_channels(F, S, calc, E, nchan=3)
        up, down = transport.calculate_transmission_channels(F, S, calc, E, spin='u', nchan=2)
        if rank == 0:
            q.put((T, up, down))
    finally:
        D.disable()
        dist.destroy_process_group()


def test_sharded_channels_in_grid_order():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    T, up, down = q.get(timeout=120)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    E = np.linspace(-1.0, 1.0, 13)
    assert np.array_equal(T, E[:, None] * np.arange(1, 4)[None, :])
    assert np.array_equal(up, E[:, None] * np.arange(1, 3)[None, :]) and np.array_equal(down, -up)

"""
The energy sharding of the transmission-matrix front ends on the CPU (gloo, world_size 2, the harness of
test_population_sharded_cpu.py): transport._pop_sharded with rows of C^2 doubles -- flattened, all-gathered, unflattened --
must reproduce the single-process result exactly.  The per-shard evaluation is the numpy restatement here (no GPU in this
process); on the GPU box the same function wraps the HIP engine (test_tmatrix_gpu.test_sharded_equals_local).
"""
import os
import socket

import numpy as np

import tmatrix_ref as tr


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _inputs():
    c = tr.cases()[1]
    return c, np.linspace(-1.5, 1.5, 11)                           # 11 energies on 2 ranks: ragged shards


def _evaluate():
    """T [m, C, C] of one system and (up, down) of two, through _pop_sharded; T_eff from the gathered matrices"""
    from gaunegf_amd import transport as T
    c, E = _inputs()
    C = len(c.terms)

    def mats(idx, scale):
        return np.stack([scale * tr.tmatrix(c.F, c.S, c.terms, e) for e in E[idx]]).reshape(-1, C, C)
    one = T._pop_sharded([None], len(E), (C, C), lambda idx: np.stack([mats(idx, 1.0)]))
    up, down = T._pop_sharded([None, None], len(E), (C, C), lambda idx: np.stack([mats(idx, 1.0), mats(idx, 0.5)]))
    return one, up, down, T.effective_transmission(one, c.n_c)


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


def test_tmatrix_sharded_matches_single_process():
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
    c, E = _inputs()
    C = len(c.terms)
    assert ref[0].shape == (len(E), C, C) and ref[3].shape == (len(E),)
    for a, b in zip(got, ref):
        assert np.array_equal(a, b)                 # an all-gather of the shards moves the values, exactly

"""
The energy sharding of the population front ends on the CPU (gloo, world_size 2, the harness of test_distributed_cpu.py):
transport._pop_sharded -- per-energy rows of one or two systems, flattened, all-gathered, unflattened -- must reproduce
the single-process result exactly.  The per-shard evaluation is the numpy restatement here (no GPU in this process); on
the GPU box the same function wraps the HIP engine (test_population_gpu.test_sharded_equals_local).
"""
import os
import socket

import numpy as np

import population_ref as pr


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _inputs():
    c = pr.const_cases()[0]
    return c, np.linspace(-1.5, 1.5, 11), c.atom_groups()         # 11 energies on 2 ranks: ragged shards


def _evaluate(sharded):
    """tables [m, ng, ng] of one system and rows ([m, ng], [m, ng]) of two, through _pop_sharded"""
    from gaunegf_amd import transport as T
    c, E, groups = _inputs()
    ng = int(groups.max()) + 1

    def tab(idx, scale):
        return np.stack([scale * pr.group_table(pr.table(c.F, c.S, c.sigmas, e, 0, 'F'), groups) for e in E[idx]]).reshape(-1, ng, ng)

    def rows(idx, scale):
        return np.stack([scale * pr.group_rows(pr.table(c.F, c.S, c.sigmas, e), groups) for e in E[idx]]).reshape(-1, ng)
    one = T._pop_sharded([None], len(E), (ng, ng), lambda idx: np.stack([tab(idx, 1.0)]))
    up, down = T._pop_sharded([None, None], len(E), (ng,), lambda idx: np.stack([rows(idx, 1.0), rows(idx, -2.0)]))
    empty = T._pop_sharded([None], 1, (ng,), lambda idx: np.stack([rows(idx, 1.0)[:len(np.arange(1)[idx])]]))
    return one, up, down, empty


def _worker(rank, world, port, q):
    import torch.distributed as dist
    from gaunegf_amd import distributed as D
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        D.enable()
        assert D.is_active() and D.rank_world() == (rank, world)
        res = _evaluate(True)
        if rank == 0:
            q.put(res)
    finally:
        D.disable()
        dist.destroy_process_group()


def test_pop_sharded_matches_single_process():
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
    ref = _evaluate(False)
    c, E, groups = _inputs()
    ng = int(groups.max()) + 1
    assert ref[0].shape == (len(E), ng, ng) and ref[1].shape == (len(E), ng)
    for a, b in zip(got, ref):
        assert np.array_equal(a, b)                 # an all-gather of the shards moves the values, exactly

"""The grid-chunked weighted sum with carry (launch_accumulate_grid, k_elementwise.hip; negf_gless_int_probes), as a float64
model on the CPU (accumulate_ref.model_grid_sum): whatever the sweeps, the bits are those of one sweep over the whole grid,
and every defect a carry can have changes them under at least one of the cuts the GPU tests run (test_batch_cut_gpu.py)."""
import numpy as np
import pytest

import accumulate_ref as ar

M = 70                                    # two full chunks of 32 and a third of 6
CUTS = (1, 3, 31, 32, 33, 64, 70)         # below, at and above the chunk; two chunks; the whole grid


@pytest.fixture(scope="module")
def operands():
    rng = np.random.default_rng(70)
    n = 5
    X = rng.standard_normal((M, n, n)) + 1j * rng.standard_normal((M, n, n))
    X *= 10.0 ** rng.uniform(-3, 3, (M, 1, 1))             # terms of very different sizes: every order has its own bits
    _, w = ar.grid(M, 71)
    return w, X


def test_one_sweep_is_the_segment_model(operands):
    """a grid in one sweep: launch_accumulate's order, which model_segments holds for one segment"""
    w, X = operands
    assert np.array_equal(ar.model_grid_sum(w, X, M), ar.model_segments(w, X, [M], M)[0])
    assert np.array_equal(ar.model_grid_sum(w, X, 4096), ar.model_segments(w, X, [M], M)[0])


@pytest.mark.parametrize("batch", CUTS)
def test_every_cut_gives_the_same_bits(operands, batch):
    w, X = operands
    assert np.array_equal(ar.model_grid_sum(w, X, batch), ar.model_grid_sum(w, X, M))


def test_the_sum_is_within_the_bar(operands):
    """the order is a chunked sum of at most 32 terms and 3 records: accumulate_ref's bar with the one-sweep k"""
    w, X = operands
    got = ar.model_grid_sum(w, X, 33)
    assert ar.ratio(got, w, X, ar.k_of([M])) <= 1.0


@pytest.mark.parametrize("defect", ar.GRID_DEFECTS)
def test_planted_defect_changes_bits(operands, defect):
    w, X = operands
    good = ar.model_grid_sum(w, X, M)
    changed = [b for b in CUTS if not np.array_equal(ar.model_grid_sum(w, X, b, defect), good)]
    print(f"{defect}: changes bits under cuts {changed}")
    assert changed, f"{defect} passes every cut"
    assert M not in changed                                  # (one sweep has no boundary for any of them to act at)


def test_sweeps_of():
    assert ar.sweeps_of(7, 3) == [(0, 3), (3, 3), (6, 1)]
    assert ar.sweeps_of(7, 9) == [(0, 7)]
    assert [ar.k_of([nb for _, nb in ar.sweeps_of(M, b)]) for b in (1, 33, 70)] == [2 + 70 + 2, 64 + 5 + 2, 64 + 3 + 2]

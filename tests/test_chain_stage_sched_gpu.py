"""
The compile-time stage schedule of the chain kernel's small inverse (chain_rs_inverse.h: rs_inverse_sched, rs_stage_sched;
the job table of chain_rs_sched.h) against the generic loop of the same build.  The schedule changes control flow, guards
and addressing only -- every stored element comes from the same operations on the same operands in the same order -- so
Sigma blocks, sweep counts and flags are compared with np.array_equal.  The generic loop runs in the launches with the
roles by wave number (NEGF_CHAIN1D_ROLES=0, read once per process): that side is computed once, by a child process
(tests/chain_stage_sched_cases.py), and shared by all tests below; results do not depend on the roles.
  * class edges: every n of every remainder-strip class (last panels 1, 2 and 3 columns wide: the strip classes hold no
    wider one) and one step outside on each side -- the non-strip class below, the next class above -- two energies
    (one complex), 0 / 1 / 3 forced sweeps;
  * contacts of unequal size inside a strip class, (50, 49), and in the guarded class, (50, 40);
  * n_c = 50, eta = 1e-4 free running at two energies of the chain_phases_cases grid: a unit that stops on the test, a
    unit that reaches the cap;  the whole grid round robin on 5 slots with a quantum of 7 sweeps (the persistent
    instantiation, every job set aside and resumed);
  * two workgroups per CU (NEGF_CHAIN1D_OCC=2, also read once per process: a child process each), n = 50, 3 sweeps;
  * a singular column and a NaN lead element at n = 50 and n = 18: converged = 0 and a non-finite block, the same on
    both paths, the other contact's block equal.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import chain_stage_sched_cases as sc

pytestmark = pytest.mark.gpu

CASES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "chain_stage_sched_cases.py")


def _child(tmp, group, tag, **env):
    """results of a case group by a fresh process with `env` set"""
    out = str(tmp / f"{tag}.npz")
    cmd = [sys.executable, *(["-s"] if sys.flags.no_user_site else []), CASES, group, out]
    r = subprocess.run(cmd, env={**os.environ, **env}, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, f"{tag}: exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    with np.load(out, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def generic(tmp_path_factory):
    """every case by the generic loop (roles by wave number)"""
    return _child(tmp_path_factory.mktemp("stage_sched"), "main", "generic", NEGF_CHAIN1D_ROLES="0")


@pytest.fixture(scope="module")
def sched(engine):
    """every case by this process: roles by SIMD, the stage schedule in the strip classes"""
    assert os.environ.get("NEGF_CHAIN1D_ROLES", "1") != "0" and os.environ.get("NEGF_CHAIN1D_OCC", "0") != "2"
    return sc.run_group(engine, "main")


def _keys(res, name):
    return sorted(k for k in res if k.startswith(name + "_") and k[len(name) + 1:].split("_")[0] in ("it", "cv", "blk"))


def _assert_same(a, b, name, equal_nan=False):
    ka = _keys(a, name)
    assert ka and ka == _keys(b, name), name
    for k in ka:
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k], equal_nan=equal_nan and "_blk_" in k), k


@pytest.mark.parametrize("name", sc.fixed_names())
def test_forced_sweeps_equal_generic_loop(sched, generic, name):
    _assert_same(sched, generic, name)
    assert np.all(sched[name + "_it"] == int(name.rsplit("_", 1)[1]))
    assert all(np.all(np.isfinite(sched[k].view(np.float64))) for k in _keys(sched, name) if "_blk_" in k)


def test_free_running_equal_generic_loop(sched, generic):
    it, cv = sched["free_it"], sched["free_cv"]
    assert (cv == 1).any() and ((cv == 0) & (it == it.max())).any()         # a unit that stops, a unit at the cap
    _assert_same(sched, generic, "free")


def test_round_robin_equal_generic_loop(sched, generic):
    _assert_same(sched, generic, "rr")


@pytest.mark.parametrize("name", sc.bad_names())
def test_bad_unit_reported_the_same(sched, generic, name):
    _assert_same(sched, generic, name, equal_nan=True)
    for m in range(sc.BAD_E.size):
        bad, good = sched[f"{name}_blk_{m}_1"], sched[f"{name}_blk_{m}_0"]
        assert int(sched[name + "_cv"][m, 1]) == 0 and not np.any(np.isfinite(bad.real) & np.isfinite(bad.imag)), m
        assert np.all(np.isfinite(good.view(np.float64))), m


def test_two_per_cu_equal_generic_loop(tmp_path):
    a = _child(tmp_path, "occ2", "occ2_sched", NEGF_CHAIN1D_OCC="2")
    b = _child(tmp_path, "occ2", "occ2_generic", NEGF_CHAIN1D_OCC="2", NEGF_CHAIN1D_ROLES="0")
    _assert_same(a, b, "fx_50_50_3")

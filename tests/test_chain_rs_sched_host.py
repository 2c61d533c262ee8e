"""
The compile-time stage schedule of the chain kernels' small inverse (gaunegf_amd/csrc/chain_rs_sched.h, used by
rs_inverse_sched in chain_rs_inverse.h) against the rule it replaces: the walk over the column tiles that the generic
loop (rs_inverse) makes at run time -- clo / chi of every tile, the half-tile test, ownership by cnt % team -- written
out here in a few lines of Python.  tests/chain_rs_sched_check.cpp prints the table as the kernel decodes it, built
plainly and with the address and undefined-behaviour sanitizers.
"""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "gaunegf_amd", "csrc")
NB, WAVES = 8, 4
WHOLE, HALF, STRIP = 1, 2, 3


def _compiler():
    for cand in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        if cand and shutil.which(cand):
            return shutil.which(cand)
    return None


def generic_walk(n, TR):
    """rs_inverse with the factoring wave fixed (fw = 3) in the strip class with TR full tiles:
    {(stage, role): [(kind, tile, upper half), ...]} for the full stages, and the same for the last stage."""
    npanels, ntiles = (n + NB - 1) // NB, (n + 15) >> 4
    fw = WAVES - 1
    full, last = {}, {}
    for sgi in range(npanels):
        has_next = sgi + 1 < npanels
        p0, pw, n0 = sgi * NB, min(NB, n - sgi * NB), (sgi + 1) * NB
        tp, tl = p0 >> 4, n0 >> 4
        team = WAVES - 1 if has_next else WAVES
        cnt = 0
        for tj in range(ntiles):
            clo, chi = tj * 16, tj * 16 + 16
            if tj == tp:
                if p0 & 8:
                    chi = p0
                else:
                    clo = p0 + NB
            if has_next and tj == tl:
                if n0 & 8:
                    chi = min(chi, n0)
                else:
                    clo = max(clo, n0 + NB)
            if clo >= chi or clo >= n:
                continue
            owner = cnt % team                      # me = (wave - fw - 1) & 3 = wave for the waves 0 .. 2; me = wave at the end
            cnt += 1
            if chi - clo == 8 and chi <= n and tj != TR:
                job = (HALF, tj, (clo - tj * 16) // 8)
            else:
                assert (clo, chi) == (tj * 16, tj * 16 + 16), (n, sgi, tj, clo, chi)
                job = (STRIP if tj == TR else WHOLE, tj, 0)
            if has_next:
                assert pw == NB and owner != fw
                full.setdefault((sgi, owner), []).append(job)
            else:
                assert pw == n - 16 * TR
                last.setdefault((sgi, owner), []).append(job)
    assert npanels == 2 * TR + 1
    return full, last


@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")],
                         ids=["plain", "asan_ubsan"])
def test_stage_schedule_matches_generic_walk(tmp_path, flags):
    cxx = _compiler()
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "chain_rs_sched_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", *flags, "-I", CSRC,
                    os.path.join(HERE, "chain_rs_sched_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failures" in r.stdout
    table = {}
    for line in r.stdout.splitlines():
        f = line.split()
        if f[0] == "job":
            TR, sgi, role, slot, kind, tj, hi = map(int, f[1:])
            jobs = table.setdefault(TR, {}).setdefault((sgi, role), [])
            assert slot == len(jobs)
            jobs.append((kind, tj, hi))
    for TR in (1, 2, 3):
        for width in (1, 2, 3, 4):                  # every last panel a strip can hold
            n = 16 * TR + width
            full, last = generic_walk(n, TR)
            assert table[TR] == full, (TR, n)
            # the last stage (not in the table): whole tile tj by role tj, which rs_inverse_sched writes out
            assert last == {(2 * TR, tj): [(WHOLE, tj, 0)] for tj in range(TR)}, (TR, n)
    # n_c = 50: 20 jobs under the full panels, 3 under the last
    assert sum(len(v) for v in table[3].values()) == 20

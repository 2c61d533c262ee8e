"""
The lane map of the chain kernel's mixing step (gaunegf_amd/csrc/chain_mix_map.h) is pure index arithmetic that the
kernel includes: tests/chain_mix_map_check.cpp checks it exhaustively on the host -- every element of the n x n iterate
held by exactly one (lane, slot), none outside, the multiply-shift division, the LDS / global split against the
storage the kernel has -- built plainly and with the address and undefined-behaviour sanitizers.
"""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "gaunegf_amd", "csrc")


def _compiler():
    for cand in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        if cand and shutil.which(cand):
            return shutil.which(cand)
    return None


@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")],
                         ids=["plain", "asan_ubsan"])
def test_mix_map_host_program(tmp_path, flags):
    cxx = _compiler()
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "chain_mix_map_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", *flags, "-I", CSRC,
                    os.path.join(HERE, "chain_mix_map_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failures" in r.stdout

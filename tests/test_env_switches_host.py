"""
The environment variables of the package (no GPU).
  (i)  The names the sources read -- getenv( in gaunegf_amd/csrc/*.{hip,h}, os.environ in gaunegf_amd/*.py -- are the
       names of the table "Environment variables" of INTEGRATION.md, no more and no fewer.
  (ii) The launch rule of the blocked inverse reads none of the retired NEGF_GJ_* switches: a child process with every
       retired variable set to a value that used to change the plan (env_retired_cases.RETIRED) gets the plans of this
       process.  negf_inverse_plan needs no device.
"""
import glob
import os
import re
import subprocess
import sys

import numpy as np

import env_retired_cases as rc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "gaunegf_amd")


def _read(path):
    with open(path, encoding="utf-8") as f:
        return f.read()


def names_read_by_the_sources():
    names, unnamed = set(), []
    for path in sorted(glob.glob(os.path.join(PKG, "csrc", "*.hip")) + glob.glob(os.path.join(PKG, "csrc", "*.h"))):
        text = _read(path)
        found = re.findall(r'getenv\(\s*"([^"]+)"', text)
        names.update(found)
        # a getenv( whose argument is no string literal would hide a name from this test
        if len(found) != len(re.findall(r"\bgetenv\(", text)):
            unnamed.append(os.path.basename(path))
    for path in sorted(glob.glob(os.path.join(PKG, "*.py"))):
        text = _read(path)
        found = re.findall(r'os\.environ(?:\.get|\.setdefault|\.pop)?[\(\[]\s*"([^"]+)"', text)
        names.update(found)
        if len(found) != len(re.findall(r"\bos\.environ\b", text)) or re.search(r"\bgetenv\b", text):
            unnamed.append(os.path.basename(path))
    return names, unnamed


def names_of_the_table():
    text = _read(os.path.join(ROOT, "INTEGRATION.md"))
    m = re.search(r"^## \d+\. Environment variables$(.*?)(?=^## |\Z)", text, re.S | re.M)
    assert m, "INTEGRATION.md has no section 'Environment variables'"
    rows = [ln for ln in m.group(1).splitlines() if ln.startswith("|")]
    assert rows[0].count("|") == 5 and rows[1].startswith("|---"), "name | default | what it does | can results change?"
    names = []
    for ln in rows[2:]:
        cells = [c.strip() for c in ln.strip().strip("|").split("|")]
        assert len(cells) == 4 and all(cells), ln
        assert re.fullmatch(r"`[A-Z][A-Z0-9_]*`", cells[0]), ln
        names.append(cells[0].strip("`"))
    return names


def test_table_lists_exactly_the_variables_the_sources_read():
    read, unnamed = names_read_by_the_sources()
    assert not unnamed, f"environment reads without a literal name: {unnamed}"
    table = names_of_the_table()
    assert len(table) == len(set(table)), "a variable is listed twice"
    assert set(table) == read, f"only in the table: {sorted(set(table) - read)}; only in the sources: {sorted(read - set(table))}"
    assert {"LOCAL_RANK", "HIPCC"} <= read
    assert not read & set(rc.RETIRED), sorted(read & set(rc.RETIRED))


def test_retired_switches_do_not_move_the_plan(tmp_path):
    assert not any(k in os.environ for k in rc.RETIRED)
    here = rc.plans()
    out = str(tmp_path / "plans.npz")
    cmd = [sys.executable, *(["-s"] if sys.flags.no_user_site else []), os.path.join(HERE, "env_retired_cases.py"), "plans", out]
    r = subprocess.run(cmd, env={**os.environ, **rc.RETIRED}, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, f"exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    with np.load(out, allow_pickle=False) as z:
        there = {k: z[k] for k in z.files}
    assert sorted(here) == sorted(there) and len(here) == 2 * len(rc.PLAN_SHAPES)
    for k in sorted(here):
        assert np.array_equal(here[k], there[k]), f"{k}: {here[k].tolist()} here, {there[k].tolist()} with the retired variables set"

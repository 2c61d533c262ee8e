"""
The layered entry points against what the commit before the recursion was folded into one forward and one backward
sweep computed: tests/golden/layered_parent.npz, recorded on the GPU by scripts/gen_layered_parent_fixture.py from a
build of that commit.  The fold keeps every kernel, its arguments and the order of the launches, so every output and
its `info` is compared bit for bit (through its SHA-256 digest, and in full where the record keeps the array), and the
launch counts per profile family and the workspace bytes are equal as integers.  The cases: rgf_parent_cases.py.
"""
import os

import numpy as np
import pytest

import rgf_parent_cases as pc

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "layered_parent.npz")


@pytest.fixture(scope="module")
def parent():
    rec = np.load(GOLDEN, allow_pickle=False)
    sha = dict(zip(rec["keys"].tolist(), rec["sha"]))
    return rec, sha


def test_the_record_covers_every_group(parent):
    rec, sha = parent
    for group in pc.GROUPS:
        assert any(k.startswith(group + "/") for k in sha), group
    assert any(k.startswith("full:") and f"/{pc.FULL_CASE}/" in k for k in rec.files)


@pytest.mark.parametrize("group", pc.GROUPS)
def test_equal_parent(engine, parent, group):
    rec, sha = parent
    got = pc.RUNNERS[group](engine)
    assert sorted(got) == sorted(k for k in sha if k.startswith(group + "/"))
    bad = []
    for k, x in got.items():
        if "full:" + k in rec.files:
            want = rec["full:" + k]
            assert x.dtype == want.dtype and np.array_equal(x, want, equal_nan=True), (k, x, want)
        if not np.array_equal(pc.digest(x), sha[k]):
            bad.append(k)
    assert not bad, bad

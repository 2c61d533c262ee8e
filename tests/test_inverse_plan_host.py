"""
The launch rule of the blocked Gauss-Jordan inverse as negf_inverse_plan states it (no GPU): both sides of every
threshold of the rule with the expectation written out by hand, the plan against an independent restatement of the
rule over a sweep of (n, nb, algo, defer), and the structural properties every plan must have.  The rule's thresholds
are the defaults, so no NEGF_GJ_* switch may be set in the environment of this test.
"""
import os

import pytest

from gaunegf_amd import _lib
from gaunegf_amd.engine import Engine


@pytest.fixture(autouse=True)
def _default_thresholds():
    on = sorted(k for k in os.environ if k.startswith("NEGF_GJ_"))
    assert not on, f"the plan is checked at the rule's default thresholds: unset {on}"

plan = Engine.inverse_plan

# window kernel ids (include/negf.h)
STRIP_256, STRIP_512, STRIP_1024, LA_6, LA_12, TEAM, SINGLE = 1, 5, 6, 7, 8, 9, 10
STRIPS = (1, 2, 3, 4, 5, 6)
UPD4, UPD8, UPD2, GATHER = 1 << 12, 1 << 13, 1 << 14, 1 << 15


def wks(p):
    return [g["wk"] for g in p["groups"]]


def counts(p):
    return [g["count"] for g in p["groups"]]


# --------------------------------------------------------------------------- #
# both sides of every threshold, expectations by hand
# --------------------------------------------------------------------------- #
def test_n_thresholds_path_and_class():
    # 31 / 32: below 32 no blocked kernel; from 32 the single-workgroup kernel
    assert plan(31, 6)["path"] == 0 and plan(31, 6)["groups"] == []
    p = plan(32, 6)
    assert p["path"] == 1 and wks(p) == [SINGLE] and counts(p) == [6] and p["groups"][0]["mask"] == 1 << SINGLE
    # 63 / 64: the strip family (algo 3) goes windowed from 64; auto and algo 4 stay on one workgroup
    assert plan(63, 6, 3)["path"] == 1
    p = plan(64, 6, 3)
    assert p["path"] == 2 and p["cls"] == (16, 1) and p["nblk"] == 1 and wks(p) == [STRIP_256]
    assert p["groups"][0]["upd_full"] == 0 and p["groups"][0]["mask"] == (1 << STRIP_256 | GATHER)   # one window: no update
    assert plan(64, 6)["path"] == 1 and plan(64, 6, 4)["path"] == 1
    # 99 / 100 with 257 matrices, 256 / 257 matrices at n = 100
    assert plan(99, 257)["path"] == 1 and plan(100, 256)["path"] == 1
    p = plan(100, 257)
    assert p["path"] == 2 and p["cls"] == (16, 1) and p["nblk"] == 2 and counts(p) == [65, 65, 65, 62]
    assert wks(p) == [STRIP_256] * 4 and all(g["upd_full"] == 8 and not g["pairs"] for g in p["groups"])
    # 208 / 209
    assert plan(208, 6)["path"] == 1 and plan(208, 256)["path"] == 1
    p = plan(208, 257)
    assert p["path"] == 2 and p["nblk"] == 4 and wks(p) == [STRIP_256] * 4
    p = plan(209, 6)
    assert p["path"] == 2 and p["cls"] == (16, 1) and p["nblk"] == 4 and wks(p) == [STRIP_256]
    # 256 / 257: always strip up to 256, by the group's count above; algo 4: one workgroup up to 256
    assert wks(plan(256, 6)) == [STRIP_256] and plan(256, 6)["nblk"] == 4
    assert wks(plan(257, 6)) == [LA_12] and plan(257, 6)["nblk"] == 5
    assert plan(256, 6, 4)["path"] == 1 and wks(plan(257, 6, 4)) == [LA_12]
    assert wks(plan(256, 6, 3)) == [STRIP_256] and wks(plan(257, 6, 3)) == [STRIP_512]
    # 512 / 513
    p, q = plan(512, 6), plan(513, 6)
    assert p["cls"] == (16, 1) and wks(p) == [LA_12] and p["nblk"] == 8
    assert q["cls"] == (16, 2) and wks(q) == [STRIP_1024] and q["nblk"] == 9
    assert wks(plan(512, 6, 3)) == [STRIP_512] and wks(plan(513, 6, 3)) == [STRIP_1024]
    assert wks(plan(512, 6, 4)) == [LA_12] and wks(plan(513, 6, 4)) == [TEAM]
    # 899 / 900: groups of 161 take the team kernel below 900 and the strip kernel from 900
    assert wks(plan(899, 644)) == [TEAM] * 4 and wks(plan(900, 644)) == [STRIP_1024] * 4
    assert wks(plan(899, 6)) == [STRIP_1024] and wks(plan(900, 6)) == [STRIP_1024]
    # 1024 / 1025 and the classes above: no strip kernel beyond sub-panels of 16, also by force
    assert plan(1024, 6)["cls"] == (16, 2) and wks(plan(1024, 6)) == [STRIP_1024]
    for algo in (0, 2, 3, 4):
        assert plan(1025, 6, algo)["cls"] == (8, 4) and wks(plan(1025, 6, algo)) == [TEAM]
    assert plan(2048, 2)["cls"] == (8, 4) and plan(2049, 2)["cls"] == (4, 8)
    assert plan(4096, 2)["cls"] == (4, 8) and plan(4097, 2)["cls"] == (2, 16)
    assert plan(8192, 2)["cls"] == (2, 16) and plan(8192, 2)["path"] == 2 and wks(plan(8192, 2)) == [TEAM]
    assert plan(8193, 2)["path"] == 0 and plan(8193, 2)["groups"] == []
    assert plan(1030, 2)["cls"] == (8, 4)            # (what test_accuracy_gpu.test_auto_1030_pairs runs)


def test_nb_thresholds_groups():
    for nb, want in ((23, [23]), (24, [12, 12]), (35, [18, 17]), (36, [12, 12, 12]), (47, [16, 16, 15]),
                     (48, [12, 12, 12, 12]), (37, [13, 13, 11]), (255, [64, 64, 64, 63]), (641, [161, 161, 161, 158]),
                     (25, [13, 12])):
        assert counts(plan(513, nb)) == want, nb
    # the single-workgroup kernel has one group whatever the batch
    assert counts(plan(200, 256)) == [256]


def test_count_thresholds_window_kernel():
    # 257 ... 512: the lean strip kernel from 64 matrices per group
    assert wks(plan(300, 252)) == [LA_12] * 4 and counts(plan(300, 252)) == [63] * 4
    assert wks(plan(300, 256)) == [STRIP_512] * 4
    assert wks(plan(257, 255)) == [STRIP_512] * 3 + [LA_12]
    assert wks(plan(512, 63)) == [LA_12] * 4 and wks(plan(300, 23)) == [LA_12]
    # 513 ... 899: the strip kernel up to 160 matrices per group
    assert wks(plan(513, 640)) == [STRIP_1024] * 4 and counts(plan(513, 640)) == [160] * 4
    assert wks(plan(513, 644)) == [TEAM] * 4
    assert wks(plan(513, 641)) == [TEAM] * 3 + [STRIP_1024]


def test_pair_threshold():
    """count * (nblk - 2) >= 256.  255 = 85 x 3, 256 = 64 x 4 = 256 x 1, 257 = 257 x 1, 258 = 86 x 3."""
    pairs = lambda p: [g["pairs"] for g in p["groups"]]
    assert pairs(plan(257, 340)) == [0] * 4 and counts(plan(257, 340)) == [85] * 4          # 255
    assert pairs(plan(257, 344)) == [1] * 4                                                  # 258
    assert pairs(plan(257, 343)) == [1, 1, 1, 0]
    assert pairs(plan(384, 252)) == [0] * 4 and pairs(plan(384, 256)) == [1] * 4             # 63 x 4 = 252, 64 x 4 = 256
    assert pairs(plan(150, 1020, 3)) == [0] * 4                                              # 255 x 1
    assert pairs(plan(150, 1024, 3)) == [1] * 4                                              # 256 x 1
    assert pairs(plan(150, 1028, 3)) == [1] * 4                                              # 257 x 1
    assert pairs(plan(513, 147)) == [1, 1, 1, 0] and pairs(plan(513, 148)) == [1] * 4        # 36 x 7 = 252, 37 x 7 = 259
    assert pairs(plan(128, 4000, 3)) == [0] * 4                                              # two windows: never
    # a pair's launches: single-block updates; a launch over all other blocks only for an odd last window
    g = plan(257, 344)["groups"][0]
    assert (g["upd_single"], g["upd_full"]) == (8, 4) and g["mask"] == (1 << STRIP_512 | UPD4 | UPD8 | UPD2 | GATHER)
    g = plan(384, 256)["groups"][0]
    assert (g["upd_single"], g["upd_full"]) == (8, 0) and g["mask"] == (1 << STRIP_512 | UPD8 | UPD2 | GATHER)


def test_fat_lean_thresholds():
    """Lean where count * blocks > 256 or nb * nblk > 2000.  Products of the first kind below the second threshold:
    255 = 85 x 3, 256 = 128 x 2, 258 = 86 x 3 = 129 x 2 (257 is prime, and 257 groups' worth of single-block launches
    already exceed 2000 in total); of the second kind 2000 = 400 x 5, 2001 = 87 x 23, 2005 = 401 x 5."""
    full = lambda p: [g["upd_full"] for g in p["groups"]]
    single = lambda p: [g["upd_single"] for g in p["groups"]]
    assert full(plan(250, 340)) == [8] * 4 and counts(plan(250, 340)) == [85] * 4            # 85 x 3 = 255
    assert full(plan(250, 344)) == [4] * 4                                                   # 86 x 3 = 258
    assert full(plan(150, 512, 3)) == [8] * 4                                                # 128 x 2 = 256
    assert full(plan(150, 516, 3)) == [4] * 4                                                # 129 x 2 = 258
    assert full(plan(250, 343)) == [4, 4, 4, 8]                                              # 86, 86, 86, 85
    # nb * nblk: the single-block launches of a pair (100 workgroups) turn lean with the whole batch
    assert single(plan(257, 400)) == [8] * 4 and full(plan(257, 400)) == [4] * 4             # 2000
    assert single(plan(257, 401)) == [4] * 4                                                 # 2005
    p, q = plan(1409, 86), plan(1409, 87)
    assert p["nblk"] == 23 and single(p) == [8] * 4 and single(q) == [4] * 4                 # 1978 / 2001
    assert full(plan(1025, 25)) == [8, 8] and full(plan(900, 6)) == [8]


@pytest.mark.parametrize("algo", [0, 1, 2, 3, 4])
def test_algo(algo):
    for n in (17, 40, 100, 200, 256, 300, 600, 1030):
        p = plan(n, 30, algo)
        if algo == 1:
            assert p["path"] == 0 and p["groups"] == [] and not p["gather"]
            continue
        want_single = n >= 32 and {0: n < 209, 2: n < 209, 3: n < 64, 4: n <= 256}[algo]
        assert p["path"] == (0 if n < 32 else 1 if want_single else 2), (n, algo)
        if p["path"] == 2:
            strip = {0: None, 2: None, 3: True, 4: False}[algo]
            for g in p["groups"]:
                if strip is not None:
                    assert (g["wk"] in STRIPS) == (strip and p["cls"][0] == 16), (n, algo, g)
    assert plan(300, 30, 0) == plan(300, 30, 2)


def test_gather_and_deferral():
    p = plan(300, 30, defer=True)
    assert p["deferred"] and not p["gather"] and all(not g["mask"] & GATHER for g in p["groups"])
    q = plan(300, 30)
    assert q["gather"] and not q["deferred"] and all(g["mask"] & GATHER for g in q["groups"])
    assert [dict(g, mask=0) for g in p["groups"]] == [dict(g, mask=0) for g in q["groups"]]
    for n, nb in ((200, 30), (100, 256), (40, 3), (17, 3)):      # one workgroup / unblocked: nothing to defer
        p = plan(n, nb, defer=True)
        assert not p["deferred"] and not p["gather"], (n, nb)


def test_invalid_arguments():
    lib = _lib.load()
    for n, nb, algo in ((0, 1, 0), (-3, 1, 0), (10, 0, 0), (10, -1, 0), (10, 1, -1), (10, 1, 5)):
        assert lib.negf_inverse_plan(n, nb, algo, 0, *([None] * 8)) == _lib.NEGF_EINVAL, (n, nb, algo)
    assert lib.negf_inverse_plan(300, 30, 0, 0, *([None] * 8)) == 0
    assert lib.negf_inverse_last(None, None, None, None) == _lib.NEGF_EINVAL


# --------------------------------------------------------------------------- #
# the rule, restated from its description, against the plan over a sweep
# --------------------------------------------------------------------------- #
def _rule(n, nb, algo, defer):
    if algo == 1 or n < 32:
        return dict(path=0)
    single = {0: n < 209 and not (n >= 100 and nb >= 257), 2: n < 209 and not (n >= 100 and nb >= 257),
              3: n < 64, 4: n <= 256}[algo]
    if single and n <= 256:
        return dict(path=1, counts=[nb])
    if n > 8192:
        return dict(path=0)
    cls = next(c for top, c in ((512, (16, 1)), (1024, (16, 2)), (2048, (8, 4)), (4096, (4, 8)), (8192, (2, 16))) if n <= top)
    nblk = -(-n // 64)
    groups = max(1, min(4, nb // 12))
    per = -(-nb // groups)
    cnt = [min(per, nb - g * per) for g in range(groups)]
    out = []
    for c in cnt:
        if cls[0] != 16 or algo == 4:
            strip = False
        elif algo == 3:
            strip = True
        else:
            strip = n <= 256 or (c >= 64 if n <= 512 else (c <= 160 or n >= 900))
        if strip:
            wk = STRIP_256 if n <= 256 else STRIP_512 if n <= 512 else STRIP_1024
        elif cls == (16, 1):
            wk = LA_6 if n <= 256 else LA_12
        else:
            wk = TEAM
        pairs = int(nblk >= 3 and c * (nblk - 2) >= 256)
        waves = lambda blocks: 4 if (c * blocks > 256 or nb * nblk > 2000) else 8
        full = waves(nblk - 1) if nblk > 1 and (not pairs or nblk % 2) else 0
        sing = waves(1) if pairs else 0
        mask = 1 << wk | (UPD4 if 4 in (full, sing) else 0) | (UPD8 if 8 in (full, sing) else 0) | (UPD2 if pairs else 0)
        out.append(dict(wk=wk, pairs=pairs, upd_full=full, upd_single=sing, mask=mask | (0 if defer else GATHER)))
    return dict(path=2, cls=cls, nblk=nblk, counts=cnt, groups=out)


_N = sorted(set(list(range(1, 1101, 13)) + [t + d for t in (32, 64, 100, 128, 192, 209, 256, 257, 320, 384, 512, 513, 576,
                                                           640, 900, 1024, 1025, 1088) for d in (-1, 0, 1)] + [1100]))


def test_plan_equals_the_restated_rule_and_is_well_formed():
    for algo, defer in ((0, False), (0, True), (3, False), (4, False), (1, False)):
        nbs = range(1, 701) if algo == 0 and not defer else list(range(1, 60)) + list(range(60, 701, 7))
        for n in _N:
            for nb in nbs:
                p = plan(n, nb, algo, defer)
                r = _rule(n, nb, algo, defer)
                key = (n, nb, algo, defer)
                assert p["path"] == r["path"], key
                # the groups tile [0, nb) exactly once, in order, none empty
                if p["path"] == 0:
                    assert p["groups"] == [] and not p["gather"] and not p["deferred"], key
                    continue
                first = 0
                for g in p["groups"]:
                    assert g["first"] == first and g["count"] >= 1, key
                    first += g["count"]
                assert first == nb and 1 <= len(p["groups"]) <= 4, key
                assert counts(p) == r["counts"], key
                # deferred gather only on the windowed path
                assert p["deferred"] == (defer and p["path"] == 2) and p["gather"] == (p["path"] == 2 and not defer), key
                if p["path"] == 1:
                    assert wks(p) == [SINGLE] and p["groups"][0]["mask"] == 1 << SINGLE, key
                    continue
                assert p["cls"] == r["cls"] and p["nblk"] == r["nblk"], key
                for g, rg in zip(p["groups"], r["groups"]):
                    assert {k: g[k] for k in rg} == rg, (key, g, rg)
                    assert not g["pairs"] or p["nblk"] >= 3, key                       # pairs imply three windows
                    assert g["wk"] not in STRIPS or p["cls"][0] == 16, key             # strip only with sub-panels of 16


def test_large_classes_keep_the_team_kernel():
    """The classes no accuracy test reaches at an affordable size: <4,8> and <2,16> (their residual tests stay in
    test_gpu_parity.py)."""
    for n, cls in ((2049, (4, 8)), (3000, (4, 8)), (4097, (2, 16)), (8192, (2, 16))):
        for nb in (1, 2, 24, 48):
            for algo in (0, 3, 4):
                p = plan(n, nb, algo)
                assert p["path"] == 2 and p["cls"] == cls and set(wks(p)) == {TEAM}, (n, nb, algo)

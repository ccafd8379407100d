"""FrozenLake maps of up to 1024 cells (rl_map_register_wide), the host side: the
registry, the tables decoded from the wide words, the FrozenLakeObs features and
the rejections.  No GPU needed.

The tables are compared with tests/maps_model.py (the rectangular restatement
tests/test_maps.py ties to tests/golden/faithful_py.py), which does not depend on
the map's size; the maps are tests/wide_maps.py's.
"""
import ctypes as C

import numpy as np
import pytest

import maps_model as mm
import wide_maps as wm
from golden import faithful_py as fp

KINDS = ("frozen_lake", "frozen_lake_edited")
RL_E_ARG = 2


def _register_wide_raw(rl, rows):
    arr = (C.c_char_p * max(len(rows), 1))(*[r.encode() for r in rows])
    mid = C.c_int32(-7)
    rc = rl.lib().rl_map_register_wide(arr, len(rows), C.byref(mid))
    return rc, rl.lib().rl_last_error().decode(), mid.value


def test_the_helper_builds_the_maps_the_issue_names():
    assert [(len(m), len(m[0])) for m in wm.LMAPS.values()] == [(5, 13), (16, 16), (3, 100), (32, 32)]
    for rows, starts, goal in ((wm.L65, {64, 30}, 0), (wm.L256, {5, 130, 255}, 132), (wm.L300, {299, 150}, 296),
                               (wm.L1024, {1023, 512}, 990)):
        flat = "".join(rows)
        assert {i for i, ch in enumerate(flat) if ch == "S"} == starts and flat[goal] == "G" and flat.count("G") == 1
    assert "".join(wm.L65)[3] == "H" and "".join(wm.L1024)[6] == "H"
    assert len(wm.M2) == 20 and all(len(r) == 20 for r in wm.M2)
    flat1, flat2 = "".join(wm.M1), "".join(wm.M2)
    assert all(flat2[wm.rel(s)] == flat1[s] for s in range(64)) and flat2.count("F") == 400 - 64 + flat1.count("F")


@pytest.mark.parametrize("rows", [["S" + "F" * 1024], ["S" + "F" * 40] + ["F" * 41] * 24], ids=["1x1025", "25x41"])
def test_more_than_the_cap_is_rejected(rl, rows):
    assert sum(len(r) for r in rows) == 1025
    rc, msg, mid = _register_wide_raw(rl, rows)
    assert rc == RL_E_ARG and "RL_MAP_WIDE_MAX_CELLS" in msg, (rc, msg)
    assert mid == -7, "a rejected map must not hand out an id"


@pytest.mark.parametrize("rows, word", [
    ([], "row"), ([""], "zero columns"), (["SFF", "FG"], "ragged"), (["SFF", "FFFG"], "ragged"),
    (["SFX", "FFG"], "SFHG"),
], ids=["no-rows", "no-columns", "ragged-short", "ragged-long", "bad-letter"])
def test_wide_register_validates_what_register_validates(rl, rows, word):
    rc, msg, mid = _register_wide_raw(rl, rows)
    assert rc == RL_E_ARG and word in msg and mid == -7, (rc, msg, mid)


def test_null_arguments_are_rejected(rl):
    mid, w = C.c_int32(-7), C.c_int32(-7)
    assert rl.lib().rl_map_register_wide(None, 1, C.byref(mid)) == RL_E_ARG and mid.value == -7
    arr = (C.c_char_p * 1)(b"SG")
    assert rl.lib().rl_map_register_wide(arr, 1, None) == RL_E_ARG
    assert rl.lib().rl_map_is_wide(0, None) == RL_E_ARG
    assert rl.lib().rl_map_is_wide(1 << 20, C.byref(w)) == RL_E_ARG and "map id" in rl.lib().rl_last_error().decode()


def test_the_cap_is_accepted_in_every_shape(rl):
    assert rl.MAP_WIDE_MAX_CELLS == 1024 and rl.MAP_MAX_CELLS == 64
    for rows in (wm.L1024, ["S" + "F" * 1022 + "G"], ["S"] + ["F"] * 1022 + ["G"]):
        mid = rl.register_map(rows, wide=True)
        assert mid >= 2 and rl.map_is_wide(mid)
        assert rl.map_info(mid) == rows
        for kind in KINDS:
            assert rl.env_dims(dict(env=kind, map8x8=mid)) == (1024, 4)


def test_wide_ids_are_distinct_stable_and_in_the_one_registry(rl):
    assert not rl.map_is_wide(0) and not rl.map_is_wide(1)
    seen = set()
    for rows in (fp.MAP4, fp.MAP8, mm.MAP_A, wm.M1, wm.L65):
        wide = rl.register_map(rows, wide=True)
        assert wide >= 2 and rl.map_is_wide(wide), "always a wide-format map, whatever the size"
        assert rl.register_map(rows, wide=True) == wide, "the same rows must give the same id again"
        assert rl.map_info(wide) == rows
        if len(rows) * len(rows[0]) <= rl.MAP_MAX_CELLS:
            small = rl.register_map(rows)
            assert small >= 2 and small != wide and not rl.map_is_wide(small)
            assert rl.register_map(rows) == small and rl.register_map(rows, wide=True) == wide
        seen.add(wide)
    assert len(seen) == 5
    # rl_map_register keeps its limit
    with pytest.raises(Exception, match="RL_MAP_MAX_CELLS"):
        rl.register_map(wm.L65)
    # default_params(map=rows, wide=True) registers wide; the default is unchanged
    p = rl.default_params(map=wm.L65, wide=True, slippery=1)
    assert p["map8x8"] == rl.register_map(wm.L65, wide=True) and "map" not in p and "wide" not in p
    assert rl.default_params(map=mm.MAP_A)["map8x8"] == rl.register_map(mm.MAP_A)
    assert rl.default_params()["map8x8"] == 0


def _assert_tables_equal_model(got, want):
    assert np.array_equal(got["prob"].view(np.uint64), np.array(want["prob"], np.float64).view(np.uint64))
    assert np.array_equal(got["next"], np.array(want["next"], np.uint32))
    assert np.array_equal(got["reward"], np.array(want["reward"], np.float64))
    assert np.array_equal(got["term"], np.array(want["term"], np.uint8))
    assert np.array_equal(got["start"].view(np.uint64), np.array(want["start"], np.float64).view(np.uint64))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("slip", (0, 1))
@pytest.mark.parametrize("name", list(wm.LMAPS))
def test_env_table_equals_the_restatement(rl, name, slip, kind):
    rows = wm.LMAPS[name]
    p = dict(env=kind, map8x8=rl.register_map(rows, wide=True), slippery=slip, max_steps=100)
    assert rl.env_dims(p) == (len(rows) * len(rows[0]), 4)
    got = rl.env_table(p)
    _assert_tables_equal_model(got, mm.table_of(mm.make_env(kind, rows, slip, 100)))
    assert np.count_nonzero(got["start"]) == "".join(rows).count("S")
    assert got["next"].max() > 63 or name == "L65"          # next states past the packed table's 6 bits
    assert got["next"].max() == len(rows) * len(rows[0]) - 1


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("slip", (0, 1))
@pytest.mark.parametrize("m8", (0, 1))
def test_wide_copy_of_a_built_in_map_gives_the_built_in_tables(rl, kind, slip, m8):
    mid = rl.register_map(fp.MAP8 if m8 else fp.MAP4, wide=True)
    a = dict(env=kind, map8x8=m8, slippery=slip, max_steps=100)
    b = dict(a, map8x8=mid)
    assert rl.env_dims(a) == rl.env_dims(b)
    ta, tb = rl.env_table(a), rl.env_table(b)
    for k in ("prob", "next", "reward", "term"):
        assert np.array_equal(ta[k], tb[k]), k
    assert np.array_equal(ta["start"].view(np.uint64), tb["start"].view(np.uint64))
    assert np.array_equal(rl.net_features(dict(a, net_input="fl_obs")), rl.net_features(dict(b, net_input="fl_obs")))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ("L65", "L300"))
def test_fl_obs_features_equal_the_restatement(rl, name, kind):
    rows = wm.LMAPS[name]
    p = dict(env=kind, map8x8=rl.register_map(rows, wide=True), slippery=0, max_steps=100, net_input="fl_obs")
    got = rl.net_features(p)
    assert np.array_equal(got, np.array(mm.fl_obs_features(rows), np.float64))
    S = len(rows) * len(rows[0])
    assert got[S - 1, 4] == len(rows) - 1 and got[S - 1, 5] == len(rows[0]) - 1

"""Caller-supplied FrozenLake maps (rl_map_register), the host side: the registry,
the tables, the FrozenLakeObs features and the rejections.  No GPU needed.

The reference takes any map (src/env/frozen_lake.rs:48-102,
src/env/frozen_lake_edited.rs:168-224); oracle/ knows the two built-in ones, so the
tables of custom maps are compared with tests/maps_model.py, a rectangular
restatement that is first tied to tests/golden/faithful_py.py (the model
tests/test_oracle_cross.py pins to the oracle) on both built-in maps.
"""
import ctypes as C

import numpy as np
import pytest

import maps_model as mm
from golden import faithful_py as fp

KINDS = ("frozen_lake", "frozen_lake_edited")
RL_E_ARG, RL_E_HIP = 2, 3


def test_restatement_equals_faithful_py_on_the_built_in_maps():
    for m8, rows in ((False, fp.MAP4), (True, fp.MAP8)):
        for slip in (False, True):
            want, got = fp.FrozenLake(m8, slip), mm.RectLake(rows, slip)
            assert got.probs == want.probs and got.start == want.start


def test_register_is_idempotent_and_info_round_trips(rl):
    ids = {}
    for name, rows in mm.MAPS.items():
        ids[name] = rl.register_map(rows)
        assert ids[name] >= 2
        assert rl.register_map(rows) == ids[name], "the same rows must give the same id again"
        assert rl.register_map([r.encode() for r in rows]) == ids[name]
        assert rl.map_info(ids[name]) == rows
    assert len(set(ids.values())) == len(ids), "distinct maps share an id"
    assert rl.map_info(0) == fp.MAP4 and rl.map_info(1) == fp.MAP8
    # dimensions alone, and a cells buffer of the wrong size
    nr, nc = C.c_uint32(), C.c_uint32()
    assert rl.lib().rl_map_info(ids["B2"], C.byref(nr), C.byref(nc), None, 0) == 0
    assert (nr.value, nc.value) == (2, 5)
    buf = C.create_string_buffer(9)
    assert rl.lib().rl_map_info(ids["B2"], None, None, buf, 9) == RL_E_ARG
    # default_params(map=rows) registers and sets the id
    p = rl.default_params(map=mm.MAP_A, slippery=1)
    assert p["map8x8"] == ids["A"] and "map" not in p


def test_registry_is_safe_from_many_threads(rl):
    """eight threads register the same 24 maps in different orders (ctypes releases
    the GIL in the call): one id per map, the same in every thread, none shared"""
    import threading
    maps = [["S" + "F" * i + "G", "F" * (i + 1) + "H"] for i in range(24)]
    rl.lib()
    got = [None] * 8

    def work(t):
        order = maps[t * 3:] + maps[:t * 3]
        got[t] = {"".join(m): rl.register_map(m) for m in order}

    threads = [threading.Thread(target=work, args=(t,)) for t in range(8)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert all(g == got[0] for g in got)
    assert len(set(got[0].values())) == len(maps) and min(got[0].values()) >= 2
    for m in maps:
        assert rl.map_info(got[0]["".join(m)]) == m


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("slip", (0, 1))
@pytest.mark.parametrize("m8", (0, 1))
def test_registered_copy_of_a_built_in_map_gives_the_built_in_tables(rl, kind, slip, m8):
    mid = rl.register_map(fp.MAP8 if m8 else fp.MAP4)
    assert mid >= 2
    a = dict(env=kind, map8x8=m8, slippery=slip, max_steps=100)
    b = dict(a, map8x8=mid)
    assert rl.env_dims(a) == rl.env_dims(b)
    ta, tb = rl.env_table(a), rl.env_table(b)
    for k in ("prob", "next", "reward", "term", "start"):
        assert np.array_equal(ta[k], tb[k]), k
    fa, fb = rl.net_features(dict(a, net_input="fl_obs")), rl.net_features(dict(b, net_input="fl_obs"))
    assert np.array_equal(fa, fb)
    if kind == "frozen_lake":
        assert np.array_equal(rl.net_features(dict(a, net_input="scalar")), rl.net_features(dict(b, net_input="scalar")))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("slip", (0, 1))
@pytest.mark.parametrize("name", list(mm.MAPS))
def test_env_table_equals_the_restatement(rl, name, slip, kind):
    rows = mm.MAPS[name]
    p = dict(env=kind, map8x8=rl.register_map(rows), slippery=slip, max_steps=100)
    assert rl.env_dims(p) == (len(rows) * len(rows[0]), 4)
    got, want = rl.env_table(p), mm.table_of(mm.make_env(kind, rows, slip, 100))
    assert np.array_equal(got["prob"].view(np.uint64), np.array(want["prob"], np.float64).view(np.uint64))
    assert np.array_equal(got["next"], np.array(want["next"], np.uint32))
    assert np.array_equal(got["reward"], np.array(want["reward"], np.float64))
    assert np.array_equal(got["term"], np.array(want["term"], np.uint8))
    assert np.array_equal(got["start"].view(np.uint64), np.array(want["start"], np.float64).view(np.uint64))
    n_s = "".join(rows).count("S")
    assert np.count_nonzero(got["start"]) == n_s
    if name == "N":
        assert not got["start"].any()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(mm.MAPS))
def test_fl_obs_features_equal_the_restatement(rl, name, kind):
    rows = mm.MAPS[name]
    p = dict(env=kind, map8x8=rl.register_map(rows), slippery=0, max_steps=100, net_input="fl_obs")
    got = rl.net_features(p)
    assert np.array_equal(got, np.array(mm.fl_obs_features(rows), np.float64))
    # x is the row and y the column: they differ on a map that is not square
    S = len(rows) * len(rows[0])
    assert got[S - 1, 4] == len(rows) - 1 and got[S - 1, 5] == len(rows[0]) - 1


def _register_raw(rl, rows):
    arr = (C.c_char_p * max(len(rows), 1))(*[r.encode() for r in rows])
    mid = C.c_int32(-7)
    rc = rl.lib().rl_map_register(arr, len(rows), C.byref(mid))
    return rc, rl.lib().rl_last_error().decode(), mid.value


@pytest.mark.parametrize("rows, word", [
    ([], "row"),                                           # zero rows
    ([""], "zero columns"),                                # zero columns
    (["SFF", "FG"], "ragged"),
    (["SFF", "FFFG"], "ragged"),
    (["SFX", "FFG"], "SFHG"),
    (["sff", "ffg"], "SFHG"),
    (["SFFFFFFFF"] * 8, "RL_MAP_MAX_CELLS"),               # 72 cells
    (["S" + "F" * 64], "RL_MAP_MAX_CELLS"),                # one row of 65
], ids=["no-rows", "no-columns", "ragged-short", "ragged-long", "bad-letter", "lower-case", "72-cells", "65-wide"])
def test_register_rejections_name_the_problem(rl, rows, word):
    rc, msg, mid = _register_raw(rl, rows)
    assert rc == RL_E_ARG and word in msg, (rc, msg)
    assert mid == -7, "a rejected map must not hand out an id"


def test_sixty_four_cells_are_accepted(rl):
    for rows in (["S" + "F" * 62 + "G"], ["S", "F"] + ["F"] * 61 + ["G"], mm.MAP_C):
        assert rl.register_map(rows) >= 2
        assert rl.env_dims(dict(env="frozen_lake", map8x8=rl.register_map(rows))) == (64, 4)


def test_unknown_map_id_is_an_argument_error_before_any_hip_call(rl):
    """RL_E_ARG with a message, also where no GPU exists (RL_E_HIP would mean a HIP call came first)"""
    for bad in (-1, 1 << 20):
        c = rl.env_config(dict(env="frozen_lake", map8x8=bad))
        S, A = C.c_uint32(), C.c_uint32()
        assert rl.lib().rl_env_dims(C.byref(c), C.byref(S), C.byref(A)) == RL_E_ARG
        assert "map id" in rl.lib().rl_last_error().decode()
        assert rl.lib().rl_env_table(C.byref(c), None, None, None, None, None) == RL_E_ARG
        out = np.zeros(6 * 64)
        assert rl.lib().rl_net_features(C.byref(c), 1, out.ctypes.data, out.size) == RL_E_ARG
        h = C.c_void_p()
        assert rl.lib().rl_env_create(C.byref(c), 4, 1, 0, 0, C.byref(h)) == RL_E_ARG
        for kind in KINDS:
            cfg = rl.agent_config(rl.default_params(env=kind, map8x8=bad, n_lanes=4))
            assert rl.lib().rl_agent_create(C.byref(cfg), C.byref(h)) == RL_E_ARG
            assert "map id" in rl.lib().rl_last_error().decode()
        nr = C.c_uint32()
        assert rl.lib().rl_map_info(bad, C.byref(nr), None, None, 0) == RL_E_ARG
    # the other envs ignore the field, as before
    assert rl.env_dims(dict(env="taxi", map8x8=12345)) == (500, 6)

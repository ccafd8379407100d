"""CPU: rl_population_create_maps' argument checks (rl.h).  No GPU: every RL_E_ARG case
is decided before the first HIP call, so it reads the same on a machine without a
device; rl_population_create keeps rejecting registered maps, and the ABI stays 7.
"""
import ctypes as C
import re
import subprocess

import pytest

import maps_model as mm
import population_map_cases as pmc

RL_E_ARG, RL_E_HIP, RL_E_STATE = 2, 3, 5
M, G = 3, 80
MAPS_SYMBOLS = ("rl_population_create_maps", "rl_population_maps")


def _base(rl, **kw):
    kw.setdefault("env", "frozen_lake")
    kw.setdefault("group_size", G)
    kw.setdefault("n_lanes", M * kw["group_size"])
    return rl.default_params(**kw)


def _create(rl, p, ids, n_members=M, members="default", base_null=False, out_null=False):
    """rl_population_create_maps' (code, message) for the raw arguments"""
    cfg = rl.agent_config(p)
    mc = rl.member_configs(p, [dict(seed=i) for i in range(max(n_members, 1))]) if members == "default" else members
    arr = None if ids is None else (C.c_int32 * max(len(ids), 1))(*ids)
    h = C.c_void_p()
    rc = rl.lib().rl_population_create_maps(None if base_null else C.byref(cfg), mc, arr, n_members,
                                            None if out_null else C.byref(h))
    msg = rl.lib().rl_last_error().decode()
    if rc == 0:
        rl.lib().rl_agent_destroy(h)
    return rc, msg


@pytest.fixture(scope="module")
def ids(rl):
    """three narrow 4x4 ids, a narrow 2x5 one, and wide copies of a 4x4 and the 10x10"""
    return dict(q4=[0, rl.register_map(mm.MAP_A), rl.register_map(pmc.Q4_MID)],
                r25=rl.register_map(mm.MAP_B2),
                q4_wide=rl.register_map(mm.MAP_A, wide=True),
                w10=rl.register_map(pmc.W10_ONE, wide=True))


def test_null_map_ids(rl):
    rc, msg = _create(rl, _base(rl), None)
    assert rc == RL_E_ARG and "map_ids" in msg and "null" in msg, (rc, msg)


@pytest.mark.parametrize("bad", [-1, 1 << 30])
def test_unknown_id_names_the_member(rl, ids, bad):
    rc, msg = _create(rl, _base(rl), [ids["q4"][1], 0, bad])
    assert rc == RL_E_ARG and "map_ids[2]" in msg and str(bad) in msg, (rc, msg)
    rc, msg = _create(rl, _base(rl), [bad, 0, 0])
    assert rc == RL_E_ARG and "map_ids[0]" in msg, (rc, msg)


def test_different_dimensions_name_both_members_and_shapes(rl, ids):
    rc, msg = _create(rl, _base(rl), [ids["q4"][1], ids["q4"][2], ids["r25"]])
    assert rc == RL_E_ARG and "dimensions" in msg, (rc, msg)
    assert "member 0" in msg and "member 2" in msg and "4x4" in msg and "2x5" in msg, msg
    rc, msg = _create(rl, _base(rl), [0, 1, 0])             # the two built-ins: 4x4 and 8x8
    assert rc == RL_E_ARG and "member 0" in msg and "member 1" in msg and "4x4" in msg and "8x8" in msg, msg
    rc, msg = _create(rl, _base(rl), [ids["q4_wide"], ids["w10"], ids["q4_wide"]])
    assert rc == RL_E_ARG and "4x4" in msg and "10x10" in msg, msg


def test_mixed_table_formats(rl, ids):
    rc, msg = _create(rl, _base(rl), [ids["q4"][1], ids["q4_wide"], ids["q4"][2]])
    assert rc == RL_E_ARG and "table formats" in msg and "member 1" in msg, (rc, msg)
    rc, msg = _create(rl, _base(rl), [ids["q4_wide"], 0, ids["q4_wide"]])   # a built-in is narrow
    assert rc == RL_E_ARG and "table formats" in msg and "narrow" in msg and "wide" in msg, (rc, msg)


@pytest.mark.parametrize("env", ["cliff_walking", "taxi", "blackjack"])
def test_other_envs_point_to_rl_population_create(rl, ids, env):
    rc, msg = _create(rl, _base(rl, env=env), ids["q4"])
    assert rc == RL_E_ARG and "env.kind" in msg and "rl_population_create" in msg, (rc, msg)


V1_CASES = [
    ("n_members-0", dict(), dict(n_members=0), "n_members"),
    ("group_size-1", dict(group_size=1, n_lanes=M), dict(), "group_size"),
    ("group_size-1025", dict(group_size=1025, n_lanes=M * 1025), dict(), "group_size"),
    ("n_lanes-short", dict(n_lanes=M * G - 1), dict(), "n_lanes"),
    ("n_lanes-long", dict(n_lanes=M * G + G), dict(), "n_lanes"),
    ("sync_every-0", dict(sync_every=0), dict(), "sync_every"),
    ("traces", dict(agent="traces"), dict(), "agent"),
    ("neural", dict(policy="neural"), dict(), "policy"),
    ("ucb-expected_sarsa", dict(selector="ucb", algo="expected_sarsa"), dict(), "selector"),
    ("null-base", dict(), dict(base_null=True), "base"),
    ("null-members", dict(), dict(members=None), "members"),
    ("null-out", dict(), dict(out_null=True), "out"),
]


@pytest.mark.parametrize("name,kw,call,field", V1_CASES, ids=[c[0] for c in V1_CASES])
def test_every_v1_error_as_today(rl, ids, name, kw, call, field):
    rc, msg = _create(rl, _base(rl, **kw), ids["q4"], **call)
    assert rc == RL_E_ARG, (rc, msg)
    assert field in msg, msg


def test_lds_guard_rejects_a_large_wide_map_before_any_hip_call(rl):
    """32 x 32 cells, double policy under UCB: 2 x 4096 entries of Q and sums and 4096
    counters pass the 160 KiB a workgroup can carve, as for rl_agent_create"""
    rows = ["S" + "F" * 31] + ["F" * 32] * 30 + ["F" * 31 + "G"]
    big = rl.register_map(rows, wide=True)
    rc, msg = _create(rl, _base(rl, policy="double", selector="ucb"), [big] * M)
    assert rc == RL_E_ARG and "exceed the 160 KiB LDS" in msg, (rc, msg)


@pytest.mark.parametrize("env", ["frozen_lake", "frozen_lake_edited"])
@pytest.mark.parametrize("which", ["narrow", "wide", "repeated"])
def test_valid_arguments_reach_the_device(rl, ids, env, which):
    """the checks reject nothing valid: a supported population passes them all and gets
    as far as the device (no GPU here: RL_E_HIP, as rl_agent_create); env.map8x8 of the
    base is ignored, even an unknown one"""
    n = C.c_int(0)
    gpu = rl.lib().rl_device_count(C.byref(n)) == 0 and n.value > 0
    m = {"narrow": ids["q4"], "wide": [ids["q4_wide"]] * M, "repeated": [ids["r25"]] * M}[which]
    rc, msg = _create(rl, _base(rl, env=env, map8x8=123456), m)
    assert rc == (0 if gpu else RL_E_HIP), (rc, msg)


@pytest.mark.parametrize("wide", [False, True], ids=["registered", "wide"])
def test_rl_population_create_still_rejects_registered_maps(rl, wide):
    mid = rl.register_map(mm.MAP_A, wide=wide)
    p = _base(rl, map8x8=mid)
    cfg = rl.agent_config(p)
    mc = rl.member_configs(p, [dict(seed=i) for i in range(M)])
    h = C.c_void_p()
    rc = rl.lib().rl_population_create(C.byref(cfg), mc, M, C.byref(h))
    msg = rl.lib().rl_last_error().decode()
    assert rc == RL_E_ARG and "env.map8x8" in msg and "not supported" in msg, (rc, msg)
    p = _base(rl, env="frozen_lake_edited")
    cfg = rl.agent_config(p)
    rc = rl.lib().rl_population_create(C.byref(cfg), mc, M, C.byref(h))
    assert rc == RL_E_ARG and "FrozenLakeEdited is not supported" in rl.lib().rl_last_error().decode()


def test_null_handles_need_no_gpu(rl):
    out = (C.c_int32 * 4)()
    assert rl.lib().rl_population_maps(None, 0, 1, out, 1) == RL_E_ARG
    assert b"null" in rl.lib().rl_last_error()


def test_python_binding_checks_the_list_length(rl):
    with pytest.raises(ValueError, match="one entry per member"):
        rl.Population(_base(rl), [dict(seed=1), dict(seed=2)], maps=[0])


def test_library_exports_the_symbols_and_the_abi_stays_7(rl):
    out = subprocess.run(["nm", "-D", "--defined-only", rl.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r" T (rl_[a-z0-9_]+)$", out, flags=re.M))
    assert set(MAPS_SYMBOLS) <= exported, set(MAPS_SYMBOLS) - exported
    assert set(MAPS_SYMBOLS) <= set(rl.SIGNATURES)
    assert rl.lib().rl_abi_version() == 7

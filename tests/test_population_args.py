"""CPU: the population ABI's argument checks, struct layout and exports (rl.h
rl_population_create).  No GPU: every RL_E_ARG case is decided before the first HIP
call, so it reads the same on a machine without a device.
"""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RL_E_ARG, RL_E_HIP, RL_E_STATE = 2, 3, 5
POP_SYMBOLS = ("rl_population_create", "rl_population_size", "rl_population_get_q", "rl_population_get_q_raw",
               "rl_population_get_ucb", "rl_population_stats")
M, G = 3, 80


def _base(rl, **kw):
    kw.setdefault("env", "frozen_lake")
    kw.setdefault("map8x8", 1)
    kw.setdefault("group_size", G)
    kw.setdefault("n_lanes", M * kw["group_size"])
    return rl.default_params(**kw)


def _create(rl, p, n_members=M, members="default", base_null=False, out_null=False):
    """rl_population_create's (code, message) for the raw arguments"""
    cfg = rl.agent_config(p)
    mc = rl.member_configs(p, [dict(seed=i) for i in range(max(n_members, 1))]) if members == "default" else members
    h = C.c_void_p()
    rc = rl.lib().rl_population_create(None if base_null else C.byref(cfg), mc, n_members,
                                       None if out_null else C.byref(h))
    msg = rl.lib().rl_last_error().decode()
    if rc == 0:
        rl.lib().rl_agent_destroy(h)
    return rc, msg


ARG_CASES = [
    ("n_members-0", dict(), dict(n_members=0), "n_members"),
    ("group_size-1", dict(group_size=1, n_lanes=M), dict(), "group_size"),
    ("group_size-1025", dict(group_size=1025, n_lanes=M * 1025), dict(), "group_size"),
    ("n_lanes-short", dict(n_lanes=M * G - 1), dict(), "n_lanes"),
    ("n_lanes-long", dict(n_lanes=M * G + G), dict(), "n_lanes"),
    ("traces", dict(agent="traces"), dict(), "agent"),
    ("neural", dict(policy="neural"), dict(), "policy"),
    ("ucb-expected_sarsa", dict(selector="ucb", algo="expected_sarsa"), dict(), "selector"),
    ("frozen_lake_edited", dict(env="frozen_lake_edited"), dict(), "env.kind"),
    ("null-base", dict(), dict(base_null=True), "base"),
    ("null-members", dict(), dict(members=None), "members"),
    ("null-out", dict(), dict(out_null=True), "out"),
]


@pytest.mark.parametrize("name,kw,call,field", ARG_CASES, ids=[c[0] for c in ARG_CASES])
def test_create_rejects_bad_arguments_before_any_hip_call(rl, name, kw, call, field):
    rc, msg = _create(rl, _base(rl, **kw), **call)
    assert rc == RL_E_ARG, (rc, msg)
    assert field in msg, msg


@pytest.mark.parametrize("wide", [False, True], ids=["registered", "wide"])
def test_create_rejects_registered_maps(rl, wide):
    mid = rl.register_map(["SFFF", "FHFH", "FFFH", "HFFG"], wide=wide)
    rc, msg = _create(rl, _base(rl, map8x8=mid))
    assert rc == RL_E_ARG and "env.map8x8" in msg, (rc, msg)


def test_member_times_group_must_stay_below_2_pow_32(rl):
    # 2^22 members of 1024 lanes: n_lanes (u32) cannot even state it
    p = _base(rl, group_size=1024, n_lanes=0)
    cfg = rl.agent_config(p)
    mc = (rl.MemberConfig * 1)()
    h = C.c_void_p()
    rc = rl.lib().rl_population_create(C.byref(cfg), mc, 1 << 22, C.byref(h))
    assert rc == RL_E_ARG and b"2^32" in rl.lib().rl_last_error()


def test_lds_guard_rejects_blackjack_double_ucb_before_any_hip_call(rl):
    rc, msg = _create(rl, _base(rl, env="blackjack", policy="double", selector="ucb"))
    assert rc == RL_E_ARG and "exceed the 160 KiB LDS" in msg, (rc, msg)


def test_valid_arguments_reach_the_device(rl):
    """the checks above reject nothing valid: a supported population passes them all
    and gets as far as the device (no GPU here: RL_E_HIP, as rl_agent_create)"""
    n = C.c_int(0)
    gpu = rl.lib().rl_device_count(C.byref(n)) == 0 and n.value > 0
    rc, msg = _create(rl, _base(rl))
    assert rc == (0 if gpu else RL_E_HIP), (rc, msg)


def test_window_and_handle_errors_need_no_gpu(rl):
    """null handles are RL_E_ARG on every rl_population_* call"""
    L = rl.lib()
    m, g = C.c_uint32(), C.c_uint32()
    assert L.rl_population_size(None, C.byref(m), C.byref(g)) == RL_E_ARG
    assert L.rl_population_get_q(None, 0, 1, None, 0) == RL_E_ARG
    assert L.rl_population_get_q_raw(None, 0, 1, None, 0) == RL_E_ARG
    assert L.rl_population_get_ucb(None, 0, 1, None, 0, None, 0) == RL_E_ARG
    assert L.rl_population_stats(None, 0, 1, None) == RL_E_ARG
    assert b"null" in L.rl_last_error()


def test_member_config_layout_matches_the_header(rl, tmp_path):
    """sizeof(rl_member_config) and every field offset, from a compiled C probe over
    include/rl.h, equal the ctypes struct's"""
    fields = [f for f, _ in rl.MemberConfig._fields_]
    prog = tmp_path / "layout.c"
    prog.write_text(
        "#include <stddef.h>\n#include <stdio.h>\n#include \"rl.h\"\n"
        "int main(void) {\n"
        "    printf(\"%zu\", sizeof(rl_member_config));\n" +
        "".join(f"    printf(\" %zu\", offsetof(rl_member_config, {f}));\n" for f in fields) +
        "    printf(\"\\n\");\n    return 0;\n}\n")
    exe = tmp_path / "layout"
    cc = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I",
                         os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-3000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60, check=True).stdout.split()
    assert int(out[0]) == C.sizeof(rl.MemberConfig) == 64
    assert [int(x) for x in out[1:]] == [getattr(rl.MemberConfig, f).offset for f in fields]


def test_library_exports_the_population_symbols(rl):
    out = subprocess.run(["nm", "-D", "--defined-only", rl.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r" T (rl_[a-z0-9_]+)$", out, flags=re.M))
    assert set(POP_SYMBOLS) <= exported, set(POP_SYMBOLS) - exported
    assert set(POP_SYMBOLS) <= set(rl.SIGNATURES)
    assert rl.lib().rl_abi_version() == 7


def test_member_params_apply_the_eps_decay_default_rule(rl):
    base = _base(rl, n_episodes_for_decay=40)
    m = rl.member_params(base, dict(eps0=0.5))
    assert m["eps_decay"] == 0.5 / (base["exploration_time"] * 40)
    assert rl.member_params(base, dict(eps0=0.5, eps_decay=0.01))["eps_decay"] == 0.01
    assert rl.member_params(base, dict(lr=0.1))["eps_decay"] == base["eps_decay"]
    with pytest.raises(ValueError):
        rl.member_params(base, dict(q_default=1.0))

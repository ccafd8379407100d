"""The device's private agents against the exact lane model (tests/private_model.py):
the cases, inputs, liveness conditions and helpers of tests/test_private_model.py
with rl.Agent as the side under test.  No oracle agent runs here; the oracle
library only supplies exp, tanh and ln, the model's checked inputs, which the
device's contract is to equal bit for bit.

Shapes are the smallest that reach each kernel's edges, and the Python model
replays only the named lanes:
  k_train_private_lds  (tables of at most 4096 bytes on FrozenLake, CliffWalking,
                       FrozenLakeEdited): 37 lanes, one full block of 32 and a partial
                       one; lanes 0, 7, 8 (a wave's last and the next wave's first
                       lane), 31, 32, 36
  k_train_private      (Taxi, Blackjack, networks off the bin's shape): 260 lanes,
                       across the 256-thread block; lanes 0, 63, 64, 255, 256, 259
  k_train_private_net  (the bin's 1-32-4 network): 300 lanes; 0, 63, 64, 255, 256, 299
Where the host reads an override at rl_agent_create (RLAMD_PRIV_LPW=0: the table
stays in HBM; RLAMD_NET_REGS=0: the parameters stay in HBM) the case runs through
both kernels: the default routing is held to the model's prediction and the
forced one must then equal the default in every record and every state word.
"""
import numpy as np
import pytest

import matrix_cases as mc
import private_model as pm
import test_private_model as tp

pytestmark = pytest.mark.gpu

LDS_LANES = (0, 7, 8, 31, 32, 36)
HBM_LANES = (0, 63, 64, 255, 256, 259)
NET_LANES = (0, 63, 64, 255, 256, 299)
MATRIX_GPU_LANES = (0, 5) + LDS_LANES[1:]          # the CPU test's lanes and the LDS kernel's edges
LDS_BLOCK_LANES = 32                                # 4 waves of 8 lanes (rl_host.cpp agent_select_kernel)


def small_table(kw):
    """the host's rule for k_train_private_lds"""
    S = {"frozen_lake": 64 if kw.get("map8x8") else 16, "frozen_lake_edited": 64 if kw.get("map8x8") else 16,
         "cliff_walking": 48}.get(kw["env"])
    P = 2 if kw.get("policy") == "double" else 1
    return S is not None and kw.get("policy") != "neural" and P * S * 4 * 8 <= 4096


def bin_network(kw):
    """the host's rule for k_train_private_net"""
    return (kw.get("policy") == "neural" and kw["env"] == "frozen_lake" and kw.get("agent", "one_step") == "one_step"
            and kw.get("net_input", "scalar") == "scalar" and kw["net_hidden"] == 32
            and kw["net_act1"] == "leaky_relu6" and kw["net_act2"] == "linear")


def funcs(oracle):
    return tp.oracle_funcs(oracle)


def _same_state(a, b):
    for j in a:
        for k, v in a[j].items():
            w = b[j][k]
            if k == "q":
                if not all(pm.same_bits(x, y) for x, y in zip(v, w)):
                    return False
            elif k in ("w", "eps"):
                x, y = np.atleast_1d(np.asarray(v, np.float64)), np.atleast_1d(np.asarray(w, np.float64))
                if not np.array_equal(x.view(np.uint64)[x == x], y.view(np.uint64)[y == y]) or \
                        not np.array_equal(x != x, y != y):
                    return False
            elif v != w:
                return False
    return True


def assert_kept_equal(kept, other):
    """the forced kernel's launches against the default one's: records byte for byte
    (td NaN as NaN), every state word of the named lanes"""
    assert len(kept) == len(other)
    for li, ((b0, r0, a0), (b1, r1, a1)) in enumerate(zip(kept, other)):
        for f in ("kind", "mode", "s", "a", "s2", "a2", "term"):
            assert np.array_equal(r0[f], r1[f]), f"launch {li}: record field {f} differs between the two kernels"
        for f in ("r", "td"):
            assert np.array_equal(r0[f], r1[f], equal_nan=True), f"launch {li}: {f} differs between the two kernels"
        assert _same_state(b0, b1) and _same_state(a0, a1), f"launch {li}: state differs between the two kernels"


def both_kernels(rl, monkeypatch, p, var, run, lds_block_words=None):
    """run(dev, keep) on the default routing (held to the model inside run) and on the
    forced one; lds_block_words: P*S*A + 2 where occupancy()'s LDS bytes tell the
    two apart"""
    monkeypatch.delenv(var, raising=False)
    dev = rl.Agent(p)
    try:
        occ = dev.occupancy()
        kept = []
        run(dev, kept)
    finally:
        dev.close()
    monkeypatch.setenv(var, "0")
    dev = rl.Agent(p)
    try:
        forced = dev.occupancy()
        other = []
        run(dev, other, check=False)
    finally:
        dev.close()
    if lds_block_words is not None:
        want = ((forced["lds_bytes"] + 15) & ~15) + LDS_BLOCK_LANES * lds_block_words * 8
        assert occ["lds_bytes"] == want and forced["lds_bytes"] < LDS_BLOCK_LANES * lds_block_words * 8, (occ, forced)
    assert_kept_equal(kept, other)


# ---------------------------------------------------------------- the matrix
@pytest.mark.parametrize("c", tp.MATRIX, ids=mc.case_id)
def test_device_matrix_case_equals_lane_model(rl, oracle, monkeypatch, c):
    kw = tp.matrix_kw(c)
    p = mc.device_params(rl, kw, c)
    fx = funcs(oracle)

    def run(dev, keep, check=True):
        tp.prepare_tabular(dev, p, kw)
        if check:
            models = tp.check_private(dev, p, kw, MATRIX_GPU_LANES, fx, keep=keep)
            tp.assert_matrix_live(models, p)
        else:
            keep += tp.run_and_keep(dev, p, MATRIX_GPU_LANES, 2)[0]

    if small_table(kw):
        P = 2 if kw["policy"] == "double" else 1
        S = 64 if kw.get("map8x8") else (48 if kw["env"] == "cliff_walking" else 16)
        both_kernels(rl, monkeypatch, p, "RLAMD_PRIV_LPW", run, P * S * 4 + 2)
    else:
        monkeypatch.delenv("RLAMD_PRIV_LPW", raising=False)
        dev = rl.Agent(p)
        try:
            run(dev, [])
        finally:
            dev.close()


# ---------------------------------------------------------------- Dyna
@pytest.mark.parametrize("name,plan", tp.DYNA, ids=[f"{e}-plan{n}" for e, n in tp.DYNA])
def test_device_dyna_case_equals_lane_model(rl, oracle, monkeypatch, name, plan):
    lds = small_table(tp.DYNA_ENVS[name])
    lanes = LDS_LANES if lds else HBM_LANES
    kw = tp.dyna_kw(name, n_lanes=lanes[-1] + 1)
    p = rl.default_params(**kw)
    fx = funcs(oracle)
    launches = tp.DYNA_LAUNCHES.get(name, 2)

    def run(dev, keep, check=True):
        if check:
            tp.check_dyna_case(dev, p, kw, name, plan, fx, lanes, keep=keep)
        else:
            tp.prepare_tabular(dev, p, kw, plan)
            keep += tp.run_and_keep(dev, p, lanes, launches)[0]

    if lds:
        P = 2 if kw.get("policy") == "double" else 1
        S = 64 if kw.get("map8x8") else (48 if kw["env"] == "cliff_walking" else 16)
        both_kernels(rl, monkeypatch, p, "RLAMD_PRIV_LPW", run, P * S * 4 + 2)
    else:
        dev = rl.Agent(p)
        try:
            run(dev, [])
        finally:
            dev.close()


@pytest.mark.parametrize("name", list(tp.DYNA_EXTRA))
def test_device_dyna_extra_case_equals_lane_model(rl, oracle, monkeypatch, name):
    lds = small_table(tp.DYNA_EXTRA[name][0])
    lanes = LDS_LANES if lds else HBM_LANES
    kw = tp.dyna_extra_kw(name, n_lanes=lanes[-1] + 1)
    p = rl.default_params(**kw)
    fx = funcs(oracle)

    def run(dev, keep, check=True):
        if check:
            tp.check_dyna_extra(dev, p, kw, name, fx, lanes, keep=keep)
        else:
            tp.prepare_tabular(dev, p, kw, tp.DYNA_EXTRA[name][1])
            keep += tp.run_and_keep(dev, p, lanes, 2)[0]

    if lds:
        S = 64 if kw.get("map8x8") else (48 if kw["env"] == "cliff_walking" else 16)
        both_kernels(rl, monkeypatch, p, "RLAMD_PRIV_LPW", run, S * 4 + 2)
    else:
        dev = rl.Agent(p)
        try:
            run(dev, [])
        finally:
            dev.close()


# ---------------------------------------------------------------- neural
@pytest.mark.parametrize("name", list(tp.NEURAL))
def test_device_neural_case_equals_lane_model(rl, oracle, monkeypatch, name):
    regs = bin_network(tp.neural_kw(name))
    lanes = NET_LANES if regs else HBM_LANES
    kw = tp.neural_kw(name, n_lanes=lanes[-1] + 1)
    p = rl.default_params(**kw)
    fx = tp.neural_fx(funcs(oracle), rl.net_features(p))
    opt = tp.NEURAL[name][1]

    def run(dev, keep, check=True):
        if check:
            tp.check_neural_case(dev, p, kw, name, fx, lanes, keep=keep)
        else:
            if opt.get("plan"):
                dev.set_planning(opt["plan"])
            dev.set_weights(tp.neural_weights(p["n_lanes"], len(fx["features"][0]), p["net_hidden"], dev.A, opt["w1"]))
            dev.set_recording(True)
            keep += tp.run_and_keep(dev, p, lanes, 2)[0]

    if regs:
        both_kernels(rl, monkeypatch, p, "RLAMD_NET_REGS", run)
    else:
        monkeypatch.delenv("RLAMD_NET_REGS", raising=False)
        dev = rl.Agent(p)
        try:
            run(dev, [])
        finally:
            dev.close()


def test_the_routing_rules_cover_all_three_kernels():
    """the case lists reach every private kernel by the host's own rules"""
    assert sum(small_table(tp.DYNA_ENVS[e]) for e in tp.DYNA_ENVS) == 4
    assert [n for n in tp.NEURAL if bin_network(tp.neural_kw(n))] == ["fl4-bin-1-32-4", "fl4-bin-plan17"]
    assert sum(small_table(tp.matrix_kw(c)) for c in tp.MATRIX) == 8 * 24

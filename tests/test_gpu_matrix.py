"""The parity matrix on the device: every case of tests/matrix_cases.py against the
CPU oracle, bit for bit, in every kernel family launch_train can pick for it.

Shared cases (learner groups of 64, a ragged last group of 2):
  (a) recording on, run():      k_train_shared<INSTR>        records, raw Q, UCB counters, stats
  (b) plain run():              k_train_shared_run / the 8-wave kernels (EPI 0)   raw Q, counters, stats
      and again forced to f64 wherever AUTO chose the fixed point
  (c) train() with the eval interleave: the episodic forms   raw Q, stats, per-lane epsilon
Private cases (37 agents: one full 32-lane block of k_train_private_lds and a
partial one): train() with records, Q bits, epsilon, counters and stats.

Blackjack with the double policy under UCB does not fit a learner group's LDS and
is rejected at create (matrix_cases.shared_rejected): asserted as such.

tests/test_matrix_coverage.py asserts on the CPU that every case here is live
(non-zero finite TD errors, entries that move, shared contributions, resets,
terminal steps); this file only compares.
"""
import numpy as np
import pytest

import matrix_cases as mc
from test_gpu_parity import _assert_q_equal, _assert_records_equal, _assert_stats_equal

pytestmark = pytest.mark.gpu
COMBOS = mc.combos()
RL_E_ARG = 2


def _shared_device(rl, c, q_mode=None):
    dev = rl.Agent(mc.device_params(rl, mc.shared_kw(c), c))
    if q_mode:
        dev.set_q_mode(q_mode)
    if mc.presets_ucb(c):
        dev.set_ucb(*mc.ucb_preset(dev.S, dev.A))
    return dev


def _assert_shared_state_equal(dev, ref):
    assert dev.q_repr() == ref.q_repr()
    assert np.array_equal(dev.q_raw(), ref.q_raw())
    dn, dt = dev.ucb()
    rn, rt = ref.ucb()
    assert np.array_equal(dn, rn) and dt == rt
    _assert_stats_equal(dev, ref)


@pytest.mark.parametrize("c", COMBOS, ids=mc.case_id)
def test_shared_case_matches_oracle(rl, oracle, c):
    if mc.shared_rejected(c):
        with pytest.raises(rl.RLError, match="exceed the 160 KiB LDS") as ex:
            _shared_device(rl, c)
        assert ex.value.code == RL_E_ARG
        return
    # (a) recording; the oracle's result also serves (b): recording changes nothing
    _, ref = mc.shared_oracle(oracle, c)
    ref.set_record(True)
    ref.run(mc.SHARED_LAUNCHES)
    dev = _shared_device(rl, c)
    try:
        dev.set_recording(True)
        dev.run(mc.SHARED_LAUNCHES)
        _assert_records_equal(dev.records(), ref.records())
        _assert_shared_state_equal(dev, ref)
    finally:
        dev.close()
    # (b) the throughput kernels
    dev = _shared_device(rl, c)
    try:
        dev.run(mc.SHARED_LAUNCHES)
        _assert_shared_state_equal(dev, ref)
    finally:
        dev.close()
    if ref.q_repr() == "fixed40":
        _, ref64 = mc.shared_oracle(oracle, c, q_mode="f64")
        ref64.run(mc.SHARED_LAUNCHES)
        dev = _shared_device(rl, c, q_mode="f64")
        try:
            assert dev.q_repr() == "f64"
            dev.run(mc.SHARED_LAUNCHES)
            _assert_shared_state_equal(dev, ref64)
        finally:
            dev.close()
    # (c) episodes with the eval interleave
    _, ref = mc.shared_oracle(oracle, c)
    ref.train_episodes(*mc.SHARED_TRAIN)
    dev = _shared_device(rl, c)
    try:
        dev.train(*mc.SHARED_TRAIN)
        _assert_shared_state_equal(dev, ref)
        assert np.array_equal(dev.epsilon().view(np.uint64), ref.lane_eps().view(np.uint64))
    finally:
        dev.close()


@pytest.mark.parametrize("c", COMBOS, ids=mc.case_id)
def test_private_case_matches_oracle(rl, oracle, c):
    n = mc.private_episodes(c)
    p, ref = mc.private_oracle(oracle, c)
    ref.set_record(True)
    ref.train_episodes(n, n // 3)
    dev = rl.Agent(mc.device_params(rl, mc.private_kw(c), c))
    try:
        if mc.presets_ucb(c):
            dev.set_ucb(*mc.ucb_preset(dev.S, dev.A, lanes=p["n_lanes"]))
        dev.set_recording(True)
        dev.train(n, n // 3)
        _assert_records_equal(dev.records(), ref.records())
        _assert_q_equal(dev.q(), ref.q())
        assert np.array_equal(dev.epsilon().view(np.uint64), ref.lane_eps().view(np.uint64))
        if c[3] == "ucb":
            dn, dt = dev.ucb()
            rn, rt = ref.ucb()
            assert np.array_equal(dn, rn) and np.array_equal(dt, rt)
        _assert_stats_equal(dev, ref)
    finally:
        dev.close()


# ---------------------------------------------------------------- the proven bound's edge
def _bound_pair(rl, oracle, case):
    p = rl.default_params(**mc.bound_kw(case))
    dev, ref = rl.Agent(p), oracle.Batch(p)
    q = mc.bound_table(case, ref.P, ref.S, ref.A)
    dev.set_q(q)
    ref.set_q(q)
    return dev, ref


def _assert_bound_state_equal(dev, ref):
    assert dev.q_repr() == ref.q_repr() == "fixed40"
    assert np.array_equal(dev.q_raw(), ref.q_raw())
    _assert_stats_equal(dev, ref)
    assert dev.stats()["q_clamp_hits"] == 0 and dev.stats()["delta_saturations"] == 0


@pytest.mark.parametrize("case", mc.BOUND_CASES, ids="-".join)
def test_updates_at_the_proven_bound_match_oracle(rl, oracle, case):
    """|lr * td| within 5 % of delta_bound (asserted on the oracle's records in
    tests/test_matrix_coverage.py), on both sides of the packed form's G * delta_bound
    < 2000: recording, throughput and episodic kernels stay in the fixed point, never
    clamp, and equal the oracle"""
    for what in ("record", "run", "train"):
        dev, ref = _bound_pair(rl, oracle, case)
        try:
            assert dev.q_repr() == ref.q_repr() == "fixed40"
            assert np.array_equal(dev.q_raw(), ref.q_raw())
            if what == "record":
                dev.set_recording(True)
                ref.set_record(True)
            if what == "train":
                dev.train(*mc.BOUND_TRAIN)
                ref.train_episodes(*mc.BOUND_TRAIN)
            else:
                dev.run(mc.BOUND_LAUNCHES)
                ref.run(mc.BOUND_LAUNCHES)
            if what == "record":
                _assert_records_equal(dev.records(), ref.records())
            _assert_bound_state_equal(dev, ref)
        finally:
            dev.close()

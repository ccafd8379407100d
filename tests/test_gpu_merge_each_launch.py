"""The one-process fixed-point merge (the delta replicas folded and applied to Q_base
after every launch) and the per-launch counters of the 8-wave throughput kernels,
against the CPU oracle's batched schedule.  No recording, so rl_agent_run takes the
EPI 0 kernels.  Bar: raw fixed-point Q EQUAL to the oracle's after every launch — a
stale replica word left by one launch shows in the next — and the counters (training
steps and episodes are summed from per-lane counts after the step loop) at the end.
"""
import numpy as np
import pytest

from test_gpu_parity import _assert_records_equal, _assert_stats_equal

pytestmark = pytest.mark.gpu

FL8 = dict(env="frozen_lake", map8x8=1, algo="qlearning", group_size=512, q_default=0.25, sync_every=16)


def _pair(rl, oracle, **kw):
    p = rl.default_params(**kw)
    return rl.Agent(p), oracle.Batch(p)


def _launches_match(dev, ref, n):
    for i in range(n):
        dev.run(1)
        ref.run(1)
        assert np.array_equal(dev.q_raw(), ref.q_raw()), f"Q differs after launch {i + 1}"
    _assert_stats_equal(dev, ref)


# 1 and 3 groups; 65 groups share the 64 replicas (group 64 adds into replica 0); the
# last group is partial in each (512, 1536, 33180 lanes)
@pytest.mark.parametrize("n_lanes", [512, 1536, 33180])
def test_merge_matches_oracle_every_launch(rl, oracle, n_lanes):
    dev, ref = _pair(rl, oracle, n_lanes=n_lanes, **FL8)
    _launches_match(dev, ref, 4)
    q = ref.q_raw()
    assert (q != q.flat[0]).any(), "the oracle's Q never moved: the case checks nothing"


# the other 8-wave fixed-point kernels with this merge and these counters, 3 groups
@pytest.mark.parametrize("case", [dict(env="cliff_walking", algo="sarsa"), dict(env="blackjack", algo="qlearning")],
                         ids=["cliff_walking-sarsa", "blackjack-qlearning"])
def test_merge_other_kernels(rl, oracle, case):
    dev, ref = _pair(rl, oracle, n_lanes=1536, group_size=512, q_default=0.25, sync_every=16, **case)
    _launches_match(dev, ref, 4)


def test_merge_alternates_with_train(rl, oracle):
    """run / train / run on one agent: the throughput kernel and the episodic one (its
    own kernel, its merges between its launches) leave each other a clean merge state"""
    dev, ref = _pair(rl, oracle, n_lanes=1536, **FL8)
    for step in ("run", "train", "run"):
        if step == "run":
            dev.run(2)
            ref.run(2)
        else:
            dev.train(12, 4)
            ref.train_episodes(12, 4)
        assert np.array_equal(dev.q_raw(), ref.q_raw()), step
        _assert_stats_equal(dev, ref)


def test_merge_is_deterministic(rl):
    """the order of the groups' atomics varies from run to run; the result must not"""
    qs = []
    for _ in range(2):
        a = rl.Agent(rl.default_params(n_lanes=33180, **FL8))
        a.run(4)
        qs.append(a.q_raw())
        a.close()
    assert np.array_equal(qs[0], qs[1])


def test_epsilon_decays_to_final_inside_the_window(rl, oracle):
    """lanes pass from the initial eps to eps_final within 6 launches (decay over 4
    episodes): records, Q and every lane's eps bits against the oracle's"""
    p = rl.default_params(env="frozen_lake", map8x8=1, algo="qlearning", n_lanes=600, group_size=256,
                          sync_every=16, q_default=0.25, n_episodes_for_decay=4)
    dev, ref = rl.Agent(p), oracle.Batch(p)
    dev.set_recording(True)
    ref.set_record(True)
    dev.run(6)
    ref.run(6)
    _assert_records_equal(dev.records(), ref.records())
    assert np.array_equal(dev.q_raw(), ref.q_raw())
    de, re_ = dev.epsilon(), ref.lane_eps()
    assert np.array_equal(de.view(np.uint64), re_.view(np.uint64))
    assert (re_ == p["eps_final"]).any(), "no lane reached eps_final: the window is too short"

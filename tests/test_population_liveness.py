"""CPU: the population tests' cases are live, on the oracle alone.

A comparison of tables that never move, or of members that all learn the same table,
shows nothing: every member of every case of tests/test_gpu_population.py changes at
least matrix_cases.SHARED_NEED["entries_changed"] entries, no two members end with
the same table, and the train() case has members that finish in different launches
(else no member ever idles while the others still run).
"""
import numpy as np
import pytest

import matrix_cases as mc
import population_cases as pc


def _members_after_run(oracle, c, members, G, launches, **over):
    base = oracle.default_params(**pc.base_kw(c, G, **over))
    refs = pc.member_oracles(oracle, base, members)
    mode = pc.population_q_mode(refs)
    for r in refs:
        if mode:
            r.set_q_mode(mode)
        r.run(launches)
    return refs, mode


def _assert_live(refs):
    tabs = [r.q() for r in refs]
    for m, q in enumerate(tabs):
        assert int((q != mc.Q_DEFAULT).sum()) >= pc.NEED_CHANGED, f"member {m} barely moved"
    for i in range(len(tabs)):
        for j in range(i):
            assert not np.array_equal(tabs[i], tabs[j]), f"members {j} and {i} learned the same table"


@pytest.mark.parametrize("c", pc.MATRIX, ids=mc.case_id)
def test_matrix_case_is_live_and_has_the_expected_representation(oracle, c):
    refs, mode = _members_after_run(oracle, c, pc.matrix_members(c), pc.MATRIX_G, pc.MATRIX_LAUNCHES)
    assert ("f64" if mode else "fixed40") == pc.expected_repr(c)
    _assert_live(refs)


@pytest.mark.parametrize("selector,members", [("eps_greedy", pc.HETERO), ("ucb", pc.HETERO_UCB)], ids=["eps_greedy", "ucb"])
def test_heterogeneous_members_are_live_and_all_fixed_point(oracle, selector, members):
    c = ("fl8", "one_step", "tabular", selector, "qlearning")
    refs, mode = _members_after_run(oracle, c, members, 80, 4)
    assert mode is None
    _assert_live(refs)


def test_supported_slice_is_what_the_header_states():
    assert len(pc.MATRIX) == 5 * 2 * (2 * 3 - 1)
    assert sum(pc.rejected(c) for c in pc.MATRIX) == 2      # Blackjack, double, UCB: SARSA and Q-learning


@pytest.mark.parametrize("env", ["fl8", "bj"])
def test_train_case_has_members_that_finish_in_different_launches(oracle, env):
    c = (env, "one_step", "tabular", "eps_greedy", "qlearning")
    base = oracle.default_params(**pc.base_kw(c, 80))
    refs = pc.member_oracles(oracle, base, pc.train_members(env))
    launches = [r.train_episodes(*mc.SHARED_TRAIN) for r in refs]
    assert len(set(launches)) > 1, launches


def test_weakest_member_decides_the_representation(oracle):
    """CliffWalking, gamma 0.95: delta_bound = lr * (100 + 1.95 * 100 / (1 - 0.95)), proven
    only below 2000.  Exactly 2000 at lr 0.5 — but 1 - 0.95 is 0.05 + 4.4e-17 in f64, the
    bound evaluates to 1999.9999999999982 and lr 0.5 is still proven; lr 0.75 (3000) is not"""
    c = ("cw", "one_step", "tabular", "eps_greedy", "qlearning")
    base = oracle.default_params(**pc.base_kw(c, 80))
    assert 0.5 * (100.0 + 1.95 * (100.0 / (1.0 - 0.95))) == 1999.9999999999982
    members = [dict(lr=0.05), dict(lr=0.1), dict(lr=0.5), dict(lr=0.75)]
    reprs = [r.q_repr() for r in pc.member_oracles(oracle, base, members)]
    assert reprs == ["fixed40", "fixed40", "fixed40", "f64"]

"""The parity matrix on the CPU: every case of tests/matrix_cases.py, the live
siblings of tests/test_gpu_parity.py and the proven-bound cases meet their
coverage conditions on the ORACLE's records (tests/coverage.py), and lane 5 of
every private combination is the faithful single-agent loop.

tests/test_gpu_matrix.py and tests/test_gpu_parity.py compare the device with the
oracle on the same cases; a case that stopped exercising its edge fails here,
without a GPU.
"""
import numpy as np
import pytest

import coverage as cov
import matrix_cases as mc
import test_gpu_parity as gp

COMBOS = mc.combos()


# ---------------------------------------------------------------- coverage.py itself
def _recs(rows, L):
    import oracle_ffi
    out = np.zeros(len(rows), oracle_ffi.RECORD_DTYPE)
    for i, (kind, s, a, td, mode, term) in enumerate(rows):
        out[i] = (s, 0, a, 0, term, mode, kind, (0, 0, 0), 0.0, td)
    return out.reshape(-1, L)


def test_measure_on_hand_made_records():
    nan = float("nan")
    recs = _recs([
        # step 0: lanes 0, 1 (group 0) hit (3, 1); lane 2 (group 1) too; lane 3 resets
        (2, 3, 1, 0.5, 0, 0), (2, 3, 1, -0.5, 0, 0), (2, 3, 1, 1.0, 0, 0), (1, 0, 0, 0.0, 0, 0),
        # step 1: a zero td, a NaN td, an eval step (not counted), a kind-3 terminal
        (2, 4, 0, 0.0, 0, 0), (2, 4, 0, nan, 0, 0), (2, 9, 9, 7.0, 1, 1), (3, 5, 2, -2.0, 0, 1),
        # step 2 (second launch): both groups move (3, 1) again; idle lanes
        (2, 3, 1, 0.25, 0, 0), (0, 0, 0, 0.0, 0, 0), (2, 3, 1, 0.25, 0, 0), (0, 0, 0, 0.0, 0, 0),
        (0, 0, 0, 0.0, 0, 0), (0, 0, 0, 0.0, 0, 0), (0, 0, 0, 0.0, 0, 0), (0, 0, 0, 0.0, 0, 0),
    ], 4)
    q = np.full((1, 6, 3), 0.25)
    q[0, 3, 1], q[0, 4, 0] = 0.5, nan
    m = cov.measure(recs, 2, 0.25, q=q, sync_every=2)
    assert m["train_steps"] == 8 and m["live_share"] == 6 / 8
    assert m["entries_changed"] == 2
    assert m["multi_contrib"] == 2 and m["max_contrib"] == 2        # (0, g0, 3, 1) and (1, g0, 4, 0)
    assert m["changed_by_2_groups"] == 2                            # (3, 1) in launch 0 and in launch 1
    assert m["resets"] == 1 and m["terminals"] == 1 and m["kind3"] == 1
    assert m["max_abs_td"] == 2.0
    cov.assert_live(m, live_share=0.75, entries_changed=2, multi_contrib=2, resets=1, terminals=1, kind3=1)
    with pytest.raises(AssertionError, match="live_share"):
        cov.assert_live(m, live_share=0.9, entries_changed=2, multi_contrib=2)
    with pytest.raises(AssertionError, match="max_contrib"):
        cov.assert_live(m, live_share=0.75, entries_changed=2, multi_contrib=2, max_contrib=3)


def test_matrix_reaches_every_combination():
    assert len(COMBOS) == 240 and len({mc.case_id(c) for c in COMBOS}) == 240
    units = {(kw["env"], reg) for kw, reg in mc.ENV_VARIANTS.values()}
    # rl_train_{frozen_lake, frozen_lake_edited}{, _map, _wide}, cliff_walking, taxi, blackjack
    assert units == {(e, r) for e in ("frozen_lake", "frozen_lake_edited") for r in (None, "map", "wide")} | {
        ("cliff_walking", None), ("taxi", None), ("blackjack", None)}


# ---------------------------------------------------------------- shared matrix
@pytest.mark.parametrize("c", COMBOS, ids=mc.case_id)
def test_shared_case_is_live_on_the_oracle(oracle, c):
    p, ref = mc.shared_oracle(oracle, c)
    ref.set_record(True)
    ref.run(mc.SHARED_LAUNCHES)
    recs = ref.records()
    assert recs.shape == (mc.SHARED_LAUNCHES * p["sync_every"], p["n_lanes"])
    m = cov.measure(recs, p["group_size"], p["q_default"], q=ref.q(), sync_every=p["sync_every"])
    cov.assert_live(m, terminals=1, **mc.SHARED_NEED)
    assert m["changed_by_2_groups"] >= 6, m
    if p["env"] == "taxi":      # truncation, not only the drop-off, inside the window
        assert (recs["term"] != 0).sum() >= p["n_lanes"], "max_steps no longer truncates inside the window"
    st = ref.stats().view(np.int64)
    assert st[8] == 0 and st[9] == 0, "clamp hits / saturations: the case left the fixed point's range"


def test_fixed_point_share_of_the_shared_matrix(oracle):
    """AUTO keeps the fixed point for the one-step single-table combinations without
    UCB + expected SARSA (5 of 24) on every non-slippery env: these also run forced
    to f64 on the device"""
    fixed = {}
    for c in COMBOS:
        _, ref = mc.shared_oracle(oracle, c)
        fixed.setdefault(c[0], []).append(ref.q_repr() == "fixed40")
    for var, (kw, _) in mc.ENV_VARIANTS.items():
        assert sum(fixed[var]) == (0 if kw.get("slippery") else 5), var


# ---------------------------------------------------------------- private matrix
@pytest.mark.parametrize("c", COMBOS, ids=mc.case_id)
def test_private_case_is_live_and_lane_5_is_the_faithful_loop(oracle, c):
    n = mc.private_episodes(c)
    p, ref = mc.private_oracle(oracle, c)
    ref.set_record(True)
    ref.train_episodes(n, n // 3)
    m = cov.measure(ref.records(), 1, p["q_default"], q=ref.q())
    assert m["live_share"] == 1.0 and m["train_steps"] >= 3000, m
    assert m["terminals"] >= n * p["n_lanes"] and m["entries_changed"] >= 500, m
    if mc.presets_ucb(c):
        # the faithful loop has no counter preset: it is compared from fresh counters
        # (NaN == NaN, as before), the device from preset ones
        p, ref = mc.private_oracle(oracle, c, preset=False)
        ref.train_episodes(n, n // 3)
    f = oracle.Faithful(dict(p, lane_offset=mc.FAITHFUL_LANE))
    f.train(n, n // 3)
    gp._assert_q_equal(ref.q()[mc.FAITHFUL_LANE], f.q())
    assert np.float64(ref.lane_eps()[mc.FAITHFUL_LANE]).tobytes() == np.float64(f.epsilon()).tobytes()


# ---------------------------------------------------------------- live siblings of test_gpu_parity.py
def _sibling_runs():
    """(id, case, n_lanes, sync_every, launches, reset_step, need) of every live sibling,
    cases and shapes from the tables the GPU tests iterate"""
    out = []
    for case, L, K, launches, need in gp.SHARED_LIVE_CASES:
        out.append(("shared", case, L, K, launches, False, need))
    sh = gp.THROUGHPUT_SHAPE
    for case in gp.THROUGHPUT_LIVE:
        out.append(("throughput", case, sh["n_lanes"], sh["sync_every"], sh["launches"], False, {}))
    sh = gp.LPW_SHAPE
    out.append(("lanes-per-wave", gp.LPW_LIVE, sh["n_lanes"], sh["sync_every"], sh["launches"], False, {}))
    sh = gp.RESET_STEP_SHAPE
    out.append(("reset-step", gp.RESET_STEP_LIVE, sh["n_lanes"], sh["sync_every"], sh["launches"], True,
                dict(resets=0, kind3=sh["n_lanes"])))
    sh = gp.TINY_SHAPE
    for L, G, case, need in gp.TINY_LIVE:
        out.append(("tiny", dict(case, group_size=G), L, sh["sync_every"], sh["launches"], False, need))
    return out


SIBLINGS = _sibling_runs()


@pytest.mark.parametrize("what,case,L,K,launches,reset_step,need", SIBLINGS,
                         ids=[f"{r[0]}-" + "-".join(f"{v}" for v in r[1].values()) for r in SIBLINGS])
def test_live_sibling_is_live_on_the_oracle(oracle, what, case, L, K, launches, reset_step, need):
    p = oracle.default_params(n_lanes=L, sync_every=K, n_episodes_for_decay=40, **gp._case_kw(case))
    ref = oracle.Batch(p)
    gp._preset_ucb(case, ref)
    if reset_step:
        ref.set_reset_step(True)
    ref.set_record(True)
    ref.run(launches)
    gp._oracle_is_live(ref, ref.records(), p, **need)


# ---------------------------------------------------------------- the proven bound's edge
@pytest.mark.parametrize("case", mc.BOUND_CASES, ids="-".join)
def test_bound_case_reaches_the_proven_bound_on_the_oracle(oracle, case):
    p = oracle.default_params(**mc.bound_kw(case))
    ref = oracle.Batch(p)
    ref.set_q(mc.bound_table(case, ref.P, ref.S, ref.A))
    assert ref.q_repr() == "fixed40", "the preset table is not exact in the fixed point"
    delta, G = mc.bound_delta(case), p["group_size"]
    assert delta < 2000.0                                                   # fix_proven
    mc.bound_packed(case)                                                   # pack_proven, as the table says
    ref.set_record(True)
    ref.run(mc.BOUND_LAUNCHES)
    m = cov.measure(ref.records(), G, 0.0, q=ref.q(), sync_every=p["sync_every"])
    assert p["lr"] * m["max_abs_td"] >= 0.95 * delta, (p["lr"] * m["max_abs_td"], delta)
    assert p["lr"] * m["max_abs_td"] <= delta
    assert m["live_share"] >= 0.9 and m["multi_contrib"] >= 10, m
    ref.train_episodes(*mc.BOUND_TRAIN)
    st = ref.stats().view(np.int64)
    assert ref.q_repr() == "fixed40" and st[8] == 0 and st[9] == 0

"""A population on the device (rl.h rl_population_create) against the CPU oracle:
member m is, bit for bit, the one-group oracle Batch of n_lanes = group_size = G with
member m's seed, lane offset and hyper-parameters (tests/population_cases.py).

Raw Q words are compared after every launch; stats, UCB counters and t, epsilon bits
and — against a lone device agent, the oracle exposing no lane records — every lane's
core and aux record at the end.
"""
import ctypes as C

import numpy as np
import pytest

import matrix_cases as mc
import population_cases as pc

pytestmark = pytest.mark.gpu
RL_E_ARG, RL_E_STATE = 2, 5
STAT_KEYS = ("train_steps", "eval_steps", "train_episodes", "eval_episodes", "reward_sum_q16")


def _make(rl, oracle, kw, members, G):
    """(population, its members' oracles in the population's representation)"""
    refs = pc.member_oracles(oracle, oracle.default_params(**kw), members)
    mode = pc.population_q_mode(refs)
    if mode:
        for r in refs:
            r.set_q_mode(mode)
    pop = rl.Population(rl.default_params(**kw), members)
    assert pop.size() == (len(members), G)
    assert pop.q_repr() == ("f64" if mode else "fixed40")
    assert all(r.q_repr() == pop.q_repr() for r in refs)
    return pop, refs


def _assert_q_equal(pop, refs):
    q = pop.q_raw()
    for m, ref in enumerate(refs):
        assert np.array_equal(q[m], ref.q_raw()), f"member {m}: raw Q differs"


def _assert_state_equal(pop, refs):
    _assert_q_equal(pop, refs)
    cnt, t = pop.ucb()
    eps = pop.epsilon()
    st = pop.member_stats()
    total = {k: 0 for k in STAT_KEYS}
    for m, ref in enumerate(refs):
        rn, rt = ref.ucb()
        assert np.array_equal(cnt[m], rn) and int(t[m]) == rt, f"member {m}: UCB counters"
        assert np.array_equal(eps[m].view(np.uint64), ref.lane_eps().view(np.uint64)), f"member {m}: epsilon"
        r = ref.stats().view(np.int64)
        for i, k in enumerate(STAT_KEYS):
            assert st[m][k] == int(r[i]), (m, k, st[m][k], int(r[i]))
            total[k] += int(r[i])
    tot = pop.stats()
    assert {k: tot[k] for k in STAT_KEYS} == total
    # the values are the raw words' (either representation)
    q, raw = pop.q(), pop.q_raw()
    want = raw.view(np.float64) if pop.q_repr() == "f64" else raw.astype(np.float64) * 2.0 ** -40
    assert np.array_equal(q.view(np.uint64), want.view(np.uint64))


def _lone(rl, pop, m, q_mode):
    """member m as rl_agent_create builds it alone"""
    dev = rl.Agent(dict(pop.members[m], n_lanes=pop.G, group_size=pop.G))
    if q_mode == "f64":
        dev.set_q_mode("f64")
    return dev


def _assert_lanes_equal_lone(rl, pop, calls):
    """every member's lane records (and words, counters, stats) equal the lone device
    agent's put through the same calls"""
    core, aux = pop.lane_state()
    raw = pop.q_raw()
    cnt, t = pop.ucb()
    st = pop.member_stats()
    for m in range(pop.M):
        dev = _lone(rl, pop, m, pop.q_repr())
        try:
            calls(dev)
            assert dev.q_repr() == pop.q_repr()
            lc, la = dev.lane_state()
            assert np.array_equal(core[m], lc), f"member {m}: core records"
            assert np.array_equal(aux[m], la), f"member {m}: aux records"
            assert np.array_equal(raw[m], dev.q_raw())
            dn, dt = dev.ucb()
            assert np.array_equal(cnt[m], dn) and int(t[m]) == dt
            ds = dev.stats()
            assert all(st[m][k] == ds[k] for k in STAT_KEYS), (st[m], ds)
        finally:
            dev.close()


def _assert_live(refs, q_default):
    tabs = [r.q() for r in refs]
    for m, q in enumerate(tabs):
        assert int((q != q_default).sum()) >= pc.NEED_CHANGED, f"member {m} barely moved"
    for i in range(len(tabs)):
        for j in range(i):
            assert not np.array_equal(tabs[i], tabs[j]), f"members {j} and {i} learned the same table"


# ---------------------------------------------------------------- 1. the matrix
@pytest.mark.parametrize("c", pc.MATRIX, ids=mc.case_id)
def test_matrix_case_members_match_their_oracles(rl, oracle, c):
    kw = pc.base_kw(c, pc.MATRIX_G)
    members = pc.matrix_members(c)
    if pc.rejected(c):
        with pytest.raises(rl.RLError, match="exceed the 160 KiB LDS") as ex:
            rl.Population(rl.default_params(**kw), members)
        assert ex.value.code == RL_E_ARG
        return
    pop, refs = _make(rl, oracle, kw, members, pc.MATRIX_G)
    try:
        assert pop.q_repr() == pc.expected_repr(c)
        for _ in range(pc.MATRIX_LAUNCHES):
            pop.run(1)
            for r in refs:
                r.run(1)
            _assert_q_equal(pop, refs)
        _assert_live(refs, mc.Q_DEFAULT)
        _assert_state_equal(pop, refs)
        _assert_lanes_equal_lone(rl, pop, lambda d: d.run(pc.MATRIX_LAUNCHES))
    finally:
        pop.close()


# ---------------------------------------------------------------- 2. heterogeneous members
@pytest.mark.parametrize("selector,members", [("eps_greedy", pc.HETERO), ("ucb", pc.HETERO_UCB)], ids=["eps_greedy", "ucb"])
def test_members_with_their_own_hyper_parameters(rl, oracle, selector, members):
    c = ("fl8", "one_step", "tabular", selector, "qlearning")
    kw = pc.base_kw(c, 80)
    pop, refs = _make(rl, oracle, kw, members, 80)
    try:
        assert pop.q_repr() == "fixed40"
        for _ in range(4):
            pop.run(1)
            for r in refs:
                r.run(1)
            _assert_q_equal(pop, refs)
        _assert_live(refs, mc.Q_DEFAULT)
        _assert_state_equal(pop, refs)
        _assert_lanes_equal_lone(rl, pop, lambda d: d.run(4))
    finally:
        pop.close()


# ---------------------------------------------------------------- 3. one representation
@pytest.mark.parametrize("lrs,want", [((0.05, 0.5), "fixed40"), ((0.05, 0.1), "fixed40"), ((0.05, 0.75), "f64")],
                         ids=["lr0.5-at-the-edge", "all-fixed", "weakest-f64"])
def test_representation_follows_the_weakest_member(rl, oracle, lrs, want):
    """CliffWalking, gamma 0.95: delta_bound = lr * (100 + 1.95 * 100 / (1 - 0.95)), proven
    for the fixed point only below 2000.  In exact arithmetic that is 200 / 400 / 2000 /
    3000 for lr 0.05 / 0.1 / 0.5 / 0.75, so lr 0.5 would just fail; in the host's and
    the oracle's f64 arithmetic 1 - 0.95 = 0.05 + 4.4e-17, the bound at lr 0.5 comes to
    1999.9999999999982 and is proven (the same edge as matrix_cases' cw-lr0.05-G10).
    A lone agent with lr 0.5 therefore runs in the fixed point, and so must the
    population that holds it: the representation is the fixed point iff every
    member's lone oracle is.  lr 0.75 (3000) is the member that forces f64."""
    c = ("cw", "one_step", "tabular", "eps_greedy", "qlearning")
    kw = pc.base_kw(c, 80)
    members = [dict(lr=lr, seed=21 + i, lane_offset=100 * i) for i, lr in enumerate(lrs)]
    lone = [r.q_repr() for r in pc.member_oracles(oracle, oracle.default_params(**kw), members)]
    assert lone[0] == "fixed40"
    assert want == ("fixed40" if all(x == "fixed40" for x in lone) else "f64"), lone
    pop, refs = _make(rl, oracle, kw, members, 80)
    try:
        assert pop.q_repr() == want
        for _ in range(4):
            pop.run(1)
            for r in refs:
                r.run(1)
            _assert_q_equal(pop, refs)
        _assert_state_equal(pop, refs)
        if want == "fixed40":   # rl_agent_set_q_mode follows the same rule, both ways
            def both(mode):
                pop.set_q_mode(mode)
                for r in refs:
                    r.set_q_mode(mode)
            both("f64")
            assert pop.q_repr() == "f64"
            _assert_q_equal(pop, refs)
            both("auto")        # every value still exact in the fixed point: back to it
            assert pop.q_repr() == "fixed40" and all(r.q_repr() == "fixed40" for r in refs)
            _assert_q_equal(pop, refs)
            both("f64")
            pop.run(1)
            for r in refs:
                r.run(1)
            _assert_q_equal(pop, refs)
            # AUTO returns only when every value of EVERY member is exact in the fixed
            # point: after an f64 launch they are not, and the population stays in f64
            # exactly when some member's lone oracle does
            both("auto")
            mode = pc.population_q_mode(refs)
            assert pop.q_repr() == ("f64" if mode else "fixed40")
            if mode:
                for r in refs:
                    r.set_q_mode(mode)
            _assert_q_equal(pop, refs)
            pop.run(1)
            for r in refs:
                r.run(1)
            _assert_state_equal(pop, refs)
    finally:
        pop.close()


# ---------------------------------------------------------------- 4. shapes
@pytest.mark.parametrize("c,M,G,K,launches", [
    (("taxi", "one_step", "tabular", "eps_greedy", "sarsa"), 66, 64, 8, 2),      # members 64.. share stats replicas with 0..
    (("fl8", "one_step", "tabular", "eps_greedy", "qlearning"), 2, 512, 16, 2),  # eight waves: the headline group shape
], ids=["66x64-taxi", "2x512-fl8"])
def test_shapes(rl, oracle, c, M, G, K, launches):
    kw = pc.base_kw(c, G, sync_every=K)
    pop, refs = _make(rl, oracle, kw, pc.seed_members(M), G)
    try:
        for _ in range(launches):
            pop.run(1)
            for r in refs:
                r.run(1)
            _assert_q_equal(pop, refs)
        _assert_state_equal(pop, refs)
    finally:
        pop.close()


# ---------------------------------------------------------------- 5. train / evaluate
@pytest.mark.parametrize("env", ["fl8", "bj"])
def test_train_run_evaluate(rl, oracle, env):
    c = (env, "one_step", "tabular", "eps_greedy", "qlearning")
    kw = pc.base_kw(c, 80)
    pop, refs = _make(rl, oracle, kw, pc.train_members(env), 80)
    try:
        launches = [r.train_episodes(*mc.SHARED_TRAIN) for r in refs]
        assert len(set(launches)) > 1, f"every member finishes in launch {launches[0]}: no member idles"
        pop.train(*mc.SHARED_TRAIN)
        _assert_state_equal(pop, refs)
        pop.run(2)
        for r in refs:
            r.run(2)
        _assert_state_equal(pop, refs)
        pop.evaluate(3)
        for r in refs:
            r.evaluate(3)
        _assert_state_equal(pop, refs)

        def calls(d):
            d.train(*mc.SHARED_TRAIN)
            d.run(2)
            d.evaluate(3)
        _assert_lanes_equal_lone(rl, pop, calls)
    finally:
        pop.close()


# ---------------------------------------------------------------- 6. independence, determinism
def _run_words(rl, kw, members, launches=3):
    pop = rl.Population(rl.default_params(**kw), members)
    try:
        pop.run(launches)
        return pop.q_raw(), pop.ucb(), pop.lane_state(), pop.member_stats()
    finally:
        pop.close()


def test_members_do_not_depend_on_their_neighbours_or_the_run(rl):
    c = ("cw", "one_step", "tabular", "ucb", "sarsa")
    kw = pc.base_kw(c, 80)
    A, B, Cm = (dict(seed=31, lr=0.05), dict(seed=32, lr=0.1, lane_offset=7), dict(seed=33, lr=0.02, ucb_c=1.5))
    q1, u1, l1, s1 = _run_words(rl, kw, [A, B, Cm])
    q2, u2, l2, s2 = _run_words(rl, kw, [Cm, A])
    for i1, i2 in ((0, 1), (2, 0)):     # A, then C
        assert np.array_equal(q1[i1], q2[i2])
        assert np.array_equal(u1[0][i1], u2[0][i2]) and u1[1][i1] == u2[1][i2]
        assert np.array_equal(l1[0][i1], l2[0][i2]) and np.array_equal(l1[1][i1], l2[1][i2])
        assert all(s1[i1][k] == s2[i2][k] for k in STAT_KEYS)
    q3, u3, l3, s3 = _run_words(rl, kw, [A, B, Cm])
    assert np.array_equal(q1, q3) and np.array_equal(u1[0], u3[0]) and np.array_equal(u1[1], u3[1])
    assert np.array_equal(l1[0], l3[0]) and np.array_equal(l1[1], l3[1])
    assert not np.array_equal(q1[0], q1[1])


# ---------------------------------------------------------------- 7. reset
def test_reset_gives_every_member_a_fresh_table_and_its_own_eps0(rl, oracle):
    """rl_agent_reset is Agent::reset: policy to default, selector fresh.  The lanes keep
    their RNG streams and env positions over it, on a lone agent and in the oracle
    alike, so run / reset / run is compared with the members' oracles put through the
    same calls (the contract), not with a fresh population's first run — which the
    oracle shows to differ (asserted below)."""
    c = ("fl8", "one_step", "tabular", "eps_greedy", "expected_sarsa")
    kw = pc.base_kw(c, 80)
    members = [dict(seed=41, eps0=1.0), dict(seed=42, eps0=0.6, lr=0.2), dict(seed=43, eps0=0.25)]
    pop, refs = _make(rl, oracle, kw, members, 80)
    try:
        pop.run(3)
        for r in refs:
            r.run(3)
        first = [r.q_raw() for r in refs]
        _assert_state_equal(pop, refs)
        pop.reset()
        for r in refs:
            r.reset()
        assert np.array_equal(pop.epsilon(), np.repeat([[1.0], [0.6], [0.25]], 80, axis=1))
        assert np.all(pop.q() == mc.Q_DEFAULT)
        cnt, t = pop.ucb()
        assert not cnt.any() and np.all(t == 1)
        _assert_state_equal(pop, refs)
        pop.run(3)
        for r in refs:
            r.run(3)
        _assert_state_equal(pop, refs)
        assert all(not np.array_equal(a, r.q_raw()) for a, r in zip(first, refs)), "streams go on over a reset"

        def calls(d):
            d.run(3)
            d.reset()
            d.run(3)
        _assert_lanes_equal_lone(rl, pop, calls)
    finally:
        pop.close()


# ---------------------------------------------------------------- 8. state and window errors
def test_unsupported_calls_and_windows(rl):
    c = ("fl8", "one_step", "tabular", "ucb", "qlearning")
    kw = pc.base_kw(c, 80)
    pop = rl.Population(rl.default_params(**kw), pc.seed_members(3))
    L, h = rl.lib(), pop.h
    buf = np.zeros(1 << 16, np.float64)
    p, n = buf.ctypes.data, buf.size
    u32, u64, i32, f64 = C.c_uint32(), C.c_uint64(), C.c_int32(), C.c_double()
    hp = C.c_void_p()
    calls = {
        "rl_agent_get_q": lambda: L.rl_agent_get_q(h, p, n),
        "rl_agent_set_q": lambda: L.rl_agent_set_q(h, p, n),
        "rl_agent_get_q_raw": lambda: L.rl_agent_get_q_raw(h, p, n),
        "rl_agent_get_ucb": lambda: L.rl_agent_get_ucb(h, p, n, p, n),
        "rl_agent_set_ucb": lambda: L.rl_agent_set_ucb(h, p, n, p, n),
        "rl_agent_set_recording": lambda: L.rl_agent_set_recording(h, 1),
        "rl_agent_take_records": lambda: L.rl_agent_take_records(h, None, 0, C.byref(u64)),
        "rl_agent_set_episode_log": lambda: L.rl_agent_set_episode_log(h, 4),
        "rl_agent_take_episodes": lambda: L.rl_agent_take_episodes(h, None, 0, C.byref(u64), C.byref(u64)),
        "rl_agent_set_reset_step": lambda: L.rl_agent_set_reset_step(h, 1),
        "rl_agent_set_planning": lambda: L.rl_agent_set_planning(h, 2),
        "rl_agent_set_future_q_value_func": lambda: L.rl_agent_set_future_q_value_func(h, 0),
        "rl_agent_set_action_selector": lambda: L.rl_agent_set_action_selector(h, 0, 1.0, 0.1, 0.0, 0, 0.5),
        "rl_agent_set_comm": lambda: L.rl_agent_set_comm(h, None),
        "rl_agent_sync": lambda: L.rl_agent_sync(h),
        "rl_agent_peer_handle": lambda: L.rl_agent_peer_handle(h, p),
        "rl_agent_peer_attach": lambda: L.rl_agent_peer_attach(h, 0, 1, p),
        "rl_agent_merge_path": lambda: L.rl_agent_merge_path(h, C.byref(i32)),
        "rl_agent_delta_words": lambda: L.rl_agent_delta_words(h, C.byref(u64)),
        "rl_agent_delta_max_words": lambda: L.rl_agent_delta_max_words(h, C.byref(u64)),
        "rl_agent_delta_cap_words": lambda: L.rl_agent_delta_cap_words(h, C.byref(u64)),
        "rl_agent_set_delta_buffer": lambda: L.rl_agent_set_delta_buffer(h, None, 0),
        "rl_agent_set_merge_groups": lambda: L.rl_agent_set_merge_groups(h, 4),
        "rl_agent_launch_train": lambda: L.rl_agent_launch_train(h),
        "rl_agent_launch_fold": lambda: L.rl_agent_launch_fold(h),
        "rl_agent_launch_apply": lambda: L.rl_agent_launch_apply(h),
        "rl_agent_get_action": lambda: L.rl_agent_get_action(h, 0, 0, C.byref(u32)),
        "rl_agent_update": lambda: L.rl_agent_update(h, 0, 0, 0, 0.0, 0, 1, 0, C.byref(f64)),
        "rl_agent_get_actions": lambda: L.rl_agent_get_actions(h, p, p, pop.L),
        "rl_agent_updates": lambda: L.rl_agent_updates(h, p, p, p, p, p, p, p, pop.L),
        "rl_agent_env": lambda: L.rl_agent_env(h, C.byref(hp)),
        "rl_agent_net_dims": lambda: L.rl_agent_net_dims(h, C.byref(u32), C.byref(u32), C.byref(u32)),
        "rl_agent_get_weights": lambda: L.rl_agent_get_weights(h, p, n),
        "rl_agent_set_weights": lambda: L.rl_agent_set_weights(h, p, n),
        "rl_agent_get_q_lanes": lambda: L.rl_agent_get_q_lanes(h, 0, 1, p, n),
        "rl_agent_get_weights_lanes": lambda: L.rl_agent_get_weights_lanes(h, 0, 1, p, n),
        "rl_agent_trace_items": lambda: L.rl_agent_trace_items(h, C.byref(u64)),
    }
    try:
        for name, call in calls.items():
            assert call() == RL_E_STATE, name
            assert b"population" in L.rl_last_error(), name
        for name in ("rl_agent_get_q", "rl_agent_get_q_raw", "rl_agent_get_ucb"):
            calls[name]()
            assert name.replace("rl_agent", "rl_population").encode() in L.rl_last_error()
        # the population went through all of that unharmed
        pop.run(1)
        assert pop.stats()["train_steps"] > 0
        # member windows and buffer lengths: RL_E_ARG, nothing written
        psa, sa = pop.P * pop.S * pop.A, pop.S * pop.A
        st = (rl.Stats * 4)()
        assert L.rl_population_get_q(h, 2, 2, p, 2 * psa) == RL_E_ARG and b"m0" in L.rl_last_error()
        assert L.rl_population_get_q_raw(h, 3, 1, p, psa) == RL_E_ARG
        assert L.rl_population_get_ucb(h, 0, 4, p, 4 * sa, p, 4) == RL_E_ARG
        assert L.rl_population_stats(h, 4, 0, st) == RL_E_ARG
        assert L.rl_population_stats(h, 0xFFFFFFFF, 2, st) == RL_E_ARG
        assert L.rl_population_get_q(h, 0, 3, p, 3 * psa - 1) == RL_E_ARG and b"n_out" in L.rl_last_error()
        assert L.rl_population_get_q_raw(h, 0, 1, p, psa + 1) == RL_E_ARG
        assert L.rl_population_get_ucb(h, 0, 2, p, 2 * sa, p, 1) == RL_E_ARG and b"n_t" in L.rl_last_error()
        assert L.rl_population_get_ucb(h, 0, 2, p, sa, p, 2) == RL_E_ARG and b"n_counts" in L.rl_last_error()
        assert L.rl_population_get_q(h, 0, 1, None, psa) == RL_E_ARG
        assert L.rl_population_stats(h, 0, 1, None) == RL_E_ARG
        assert L.rl_population_get_q(h, 1, 2, p, 2 * psa) == 0
    finally:
        pop.close()
    # and the population calls on a plain agent
    dev = rl.Agent(rl.default_params(**kw))
    try:
        m, g = C.c_uint32(), C.c_uint32()
        st = (rl.Stats * 1)()
        assert L.rl_population_size(dev.h, C.byref(m), C.byref(g)) == RL_E_STATE
        assert L.rl_population_get_q(dev.h, 0, 1, p, n) == RL_E_STATE
        assert L.rl_population_get_q_raw(dev.h, 0, 1, p, n) == RL_E_STATE
        assert L.rl_population_get_ucb(dev.h, 0, 1, p, n, p, n) == RL_E_STATE
        assert L.rl_population_stats(dev.h, 0, 1, st) == RL_E_STATE
    finally:
        dev.close()

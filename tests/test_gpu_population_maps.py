"""A population on maps of the members' own (rl.h rl_population_create_maps) on the
device: member m is, bit for bit, the lone device agent rl_agent_create builds on
map_ids[m] with n_lanes = group_size = G and member m's fields, put into the
population's representation (tests/population_map_cases.py; the lone map kernels are
pinned to tests/maps_model.py and the oracle by test_gpu_maps.py / test_gpu_wide_maps.py).

Raw Q words are compared after every launch; UCB counters and t, epsilon bits, core
and aux lane records, per-member stats and the totals at the end.
"""
import ctypes as C

import numpy as np
import pytest

import matrix_cases as mc
import population_cases as pc
import population_map_cases as pmc

pytestmark = pytest.mark.gpu
RL_E_ARG, RL_E_STATE = 2, 5
STAT_KEYS = ("train_steps", "eval_steps", "train_episodes", "eval_episodes", "reward_sum_q16")


class Pair:
    """a map population and its members' lone agents, in one representation"""

    def __init__(self, rl, kw, members, ids):
        self.pop = rl.Population(rl.default_params(**kw), members, maps=ids)
        self.lone = []
        try:
            for m, mid in enumerate(ids):
                self.lone.append(rl.Agent(dict(self.pop.members[m], n_lanes=self.pop.G, group_size=self.pop.G,
                                               map8x8=mid)))
            own = [d.q_repr() for d in self.lone]
            self.want = "fixed40" if all(r == "fixed40" for r in own) else "f64"
            if self.want == "f64":
                for d in self.lone:
                    d.set_q_mode("f64")
            assert self.pop.size() == (len(ids), self.pop.G)
            assert list(self.pop.maps()) == list(ids)
        except BaseException:
            self.close()
            raise

    def close(self):
        self.pop.close()
        for d in self.lone:
            d.close()

    def both(self, call):
        call(self.pop)
        for d in self.lone:
            call(d)

    def assert_repr(self):
        assert self.pop.q_repr() == self.want, (self.pop.q_repr(), self.want)
        assert all(d.q_repr() == self.want for d in self.lone)

    def assert_q_equal(self):
        q = self.pop.q_raw()
        for m, d in enumerate(self.lone):
            assert np.array_equal(q[m], d.q_raw()), f"member {m}: raw Q differs"

    def assert_state_equal(self):
        self.assert_repr()
        self.assert_q_equal()
        pop = self.pop
        cnt, t = pop.ucb()
        eps = pop.epsilon()
        core, aux = pop.lane_state()
        st = pop.member_stats()
        total = {k: 0 for k in STAT_KEYS}
        for m, d in enumerate(self.lone):
            dn, dt = d.ucb()
            assert np.array_equal(cnt[m], dn) and int(t[m]) == dt, f"member {m}: UCB counters"
            assert np.array_equal(eps[m].view(np.uint64), d.epsilon().view(np.uint64)), f"member {m}: epsilon"
            lc, la = d.lane_state()
            assert np.array_equal(core[m], lc), f"member {m}: core records"
            assert np.array_equal(aux[m], la), f"member {m}: aux records"
            ds = d.stats()
            for k in STAT_KEYS:
                assert st[m][k] == ds[k], (m, k, st[m][k], ds[k])
                total[k] += ds[k]
        tot = pop.stats()
        assert {k: tot[k] for k in STAT_KEYS} == total


def _run_case(rl, kw, members, ids, launches=pmc.LAUNCHES):
    pr = Pair(rl, kw, members, ids)
    try:
        pr.assert_repr()
        for _ in range(launches):
            pr.both(lambda h: h.run(1))
            pr.assert_q_equal()
        pr.assert_state_equal()
        assert pr.pop.stats()["train_steps"] > 0
        return pr.want, pr.pop.q_raw()
    finally:
        pr.close()


def _id(v):
    return "-".join(v)


# ---------------------------------------------------------------- 1. Q4 on ENV_FL_MAP: the ten variants
@pytest.mark.parametrize("slippery", [0, 1], ids=["det", "slippery"])
@pytest.mark.parametrize("variant", pmc.TEN, ids=_id)
def test_q4_every_variant(rl, variant, slippery):
    kw = pmc.base_kw("frozen_lake", *variant, slippery)
    ids = pmc.map_ids(rl, "Q4")
    want, _ = _run_case(rl, kw, pmc.seed_members(len(ids)), ids)
    # a slippery lake and the double policy run in f64; the tabular policy is proven
    assert want == ("f64" if slippery or variant[0] == "double" else "fixed40")


# ---------------------------------------------------------------- 2. the other env ids
OTHER = [("fle-q4", "frozen_lake_edited", "Q4", False), ("fl-q4-wide", "frozen_lake", "Q4", True),
         ("fle-q4-wide", "frozen_lake_edited", "Q4", True), ("fl-w10", "frozen_lake", "W10", True),
         ("fle-w10", "frozen_lake_edited", "W10", True)]


@pytest.mark.parametrize("slippery", [0, 1], ids=["det", "slippery"])
@pytest.mark.parametrize("variant", pmc.THREE, ids=_id)
@pytest.mark.parametrize("name,env,mapset,wide", OTHER, ids=[o[0] for o in OTHER])
def test_edited_and_wide_env_ids(rl, name, env, mapset, wide, variant, slippery):
    kw = pmc.base_kw(env, *variant, slippery)
    ids = pmc.map_ids(rl, mapset, wide=wide)
    assert all(rl.map_is_wide(i) == wide for i in ids)
    _run_case(rl, kw, pmc.seed_members(len(ids)), ids)


# ---------------------------------------------------------------- 3. a non-square shape, fixed and drawn starts
@pytest.mark.parametrize("slippery", [0, 1], ids=["det", "slippery"])
def test_r25_fixed_and_drawn_start_in_one_launch(rl, slippery):
    kw = pmc.base_kw("frozen_lake", "tabular", "eps_greedy", "qlearning", slippery)
    ids = pmc.map_ids(rl, "R25")
    # the two-start member first and last: blocks with a longer and a shorter start list
    # than their neighbours' on both sides
    order = [ids[1], ids[0], ids[1]]
    _run_case(rl, kw, pmc.seed_members(3), order)


# ---------------------------------------------------------------- 4. only the maps part the members
@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
def test_one_seed_distinct_maps_learn_distinct_tables(rl, wide):
    kw = pmc.base_kw("frozen_lake", "tabular", "eps_greedy", "qlearning", 0)
    ids = pmc.map_ids(rl, "Q4", wide=wide)
    names = [m[0] for m in pmc.SETS["Q4"]]
    _, q = _run_case(rl, kw, pmc.same_members(len(ids)), ids)
    default = int(mc.Q_DEFAULT * 2 ** 40)
    for m, name in enumerate(names):
        assert int((q[m] != default).sum()) >= mc.SHARED_NEED["entries_changed"], f"{name} barely moved"
    same = {frozenset(p) for p in pmc.SAME_ENV["Q4"]}
    for i, a in enumerate(names):
        for j, b in enumerate(names[:i]):
            if frozenset((a, b)) in same:
                assert np.array_equal(q[i], q[j]), f"{a} and {b} are one env"
            else:
                assert not np.array_equal(q[i], q[j]), f"{a} and {b} learned the same table"


# ---------------------------------------------------------------- 5. the oracle parity carried over
@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
@pytest.mark.parametrize("slippery", [0, 1], ids=["fixed40", "slippery-f64"])
def test_copies_of_the_builtin_8x8_equal_the_builtin_population(rl, slippery, wide):
    """rl.Population on map8x8 = 1 runs the existing kernel, which test_gpu_population.py
    pins to the oracle"""
    c = ("fl8", "one_step", "tabular", "eps_greedy", "qlearning")
    kw = dict(pc.base_kw(c, pmc.G), slippery=slippery)
    members = pc.seed_members(3)
    copy = rl.register_map(rl.map_info(1), wide=wide)
    ids = [copy] * 3 if wide else [copy, 1, copy]       # the built-in id itself, as a narrow map
    a = rl.Population(rl.default_params(**kw), members, maps=ids)
    b = rl.Population(rl.default_params(**kw), members)
    try:
        assert a.q_repr() == b.q_repr() == ("f64" if slippery else "fixed40")
        assert list(b.maps()) == [1, 1, 1] and list(a.maps()) == ids
        for _ in range(pmc.LAUNCHES):
            a.run(1)
            b.run(1)
            assert np.array_equal(a.q_raw(), b.q_raw())
        assert int((a.q_raw()[0] != b.q_raw()[1]).sum()) > 0     # the members differ
        for x, y in zip(a.ucb(), b.ucb()):
            assert np.array_equal(x, y)
        assert np.array_equal(a.epsilon().view(np.uint64), b.epsilon().view(np.uint64))
        for x, y in zip(a.lane_state(), b.lane_state()):
            assert np.array_equal(x, y)
        sa, sb = a.member_stats(), b.member_stats()
        assert all(sa[m][k] == sb[m][k] for m in range(3) for k in STAT_KEYS)
        assert a.stats()["train_steps"] == b.stats()["train_steps"] > 0
    finally:
        a.close()
        b.close()


# ---------------------------------------------------------------- 6. train / run / evaluate, reset
def test_train_run_evaluate(rl):
    kw = pmc.base_kw("frozen_lake", "tabular", "eps_greedy", "qlearning", 0)
    ids = pmc.map_ids(rl, "Q4")
    pr = Pair(rl, kw, pmc.seed_members(len(ids)), ids)
    try:
        pr.both(lambda h: h.train(*mc.SHARED_TRAIN))
        pr.assert_state_equal()
        pr.both(lambda h: h.run(2))
        pr.assert_state_equal()
        pr.both(lambda h: h.evaluate(3))
        pr.assert_state_equal()
        st = pr.pop.member_stats()
        assert all(s["train_episodes"] > 0 and s["eval_episodes"] > 0 for s in st)
    finally:
        pr.close()


def test_run_reset_run(rl):
    kw = pmc.base_kw("frozen_lake_edited", "tabular", "ucb", "sarsa", 1)
    ids = pmc.map_ids(rl, "Q4")
    pr = Pair(rl, kw, pmc.seed_members(len(ids)), ids)
    try:
        pr.both(lambda h: h.run(3))
        pr.assert_state_equal()
        pr.both(lambda h: h.reset())
        assert np.all(pr.pop.q() == mc.Q_DEFAULT)
        cnt, t = pr.pop.ucb()
        assert not cnt.any() and np.all(t == 1)
        pr.assert_state_equal()
        pr.both(lambda h: h.run(3))
        pr.assert_state_equal()
    finally:
        pr.close()


def test_set_q_mode_follows_the_lone_agents(rl):
    kw = pmc.base_kw("frozen_lake", "tabular", "eps_greedy", "sarsa", 0)
    ids = pmc.map_ids(rl, "Q4")
    pr = Pair(rl, kw, pmc.seed_members(len(ids)), ids)
    try:
        assert pr.want == "fixed40"
        pr.both(lambda h: h.run(1))
        pr.both(lambda h: h.set_q_mode("f64"))
        pr.want = "f64"
        pr.assert_state_equal()
        pr.both(lambda h: h.run(1))
        pr.assert_state_equal()
    finally:
        pr.close()


# ---------------------------------------------------------------- 7. member order
def _words(rl, kw, members, ids, launches=3):
    pop = rl.Population(rl.default_params(**kw), members, maps=ids)
    try:
        pop.run(launches)
        return pop.q_raw(), pop.ucb(), pop.lane_state(), pop.member_stats()
    finally:
        pop.close()


def test_members_do_not_depend_on_their_neighbours(rl):
    kw = pmc.base_kw("frozen_lake", "tabular", "ucb", "sarsa", 1)
    ids = pmc.map_ids(rl, "Q4")
    A, B, Cm = (dict(seed=31, lr=0.05), dict(seed=32, lr=0.1, lane_offset=7), dict(seed=33, lr=0.02, ucb_c=1.5))
    ia, ib, ic = ids[1], ids[2], ids[4]     # two starts, one start, three starts
    q1, u1, l1, s1 = _words(rl, kw, [A, B, Cm], [ia, ib, ic])
    q2, u2, l2, s2 = _words(rl, kw, [Cm, A], [ic, ia])
    for i1, i2 in ((0, 1), (2, 0)):     # A, then C
        assert np.array_equal(q1[i1], q2[i2])
        assert np.array_equal(u1[0][i1], u2[0][i2]) and u1[1][i1] == u2[1][i2]
        assert np.array_equal(l1[0][i1], l2[0][i2]) and np.array_equal(l1[1][i1], l2[1][i2])
        assert all(s1[i1][k] == s2[i2][k] for k in STAT_KEYS)
    assert not np.array_equal(q1[0], q1[1])


# ---------------------------------------------------------------- 8. rl_population_maps
def test_population_maps_windows_and_state_errors(rl):
    L = rl.lib()
    kw = pmc.base_kw("frozen_lake", "tabular", "eps_greedy", "qlearning", 0)
    ids = pmc.map_ids(rl, "Q4")
    out = (C.c_int32 * 8)(*([-7] * 8))
    pop = rl.Population(rl.default_params(**kw), pmc.seed_members(len(ids)), maps=ids)
    try:
        assert list(pop.maps()) == ids and list(pop.maps(1, 3)) == ids[1:4] and list(pop.maps(4)) == ids[4:]
        assert L.rl_population_maps(pop.h, 3, 3, out, 3) == RL_E_ARG and b"m0" in L.rl_last_error()
        assert L.rl_population_maps(pop.h, 0, 2, out, 3) == RL_E_ARG and b"n_out" in L.rl_last_error()
        assert L.rl_population_maps(pop.h, 0, 2, None, 2) == RL_E_ARG
        assert list(out) == [-7] * 8
        # the calls a population takes work on this one; the rest say RL_E_STATE
        pop.run(1)
        assert pop.occupancy()["block_threads"] == 128
        buf = np.zeros(pop.P * pop.S * pop.A, np.float64)
        assert L.rl_agent_get_q(pop.h, buf.ctypes.data, buf.size) == RL_E_STATE
        assert b"rl_population_get_q" in L.rl_last_error()
        assert L.rl_agent_set_recording(pop.h, 1) == RL_E_STATE
    finally:
        pop.close()
    # a built-in-map population: the shared id for every member
    c = ("fl4-slip", "one_step", "tabular", "eps_greedy", "qlearning")
    pop = rl.Population(rl.default_params(**pc.base_kw(c, pmc.G)), pc.seed_members(3))
    try:
        assert list(pop.maps()) == [0, 0, 0]
    finally:
        pop.close()
    # a population on another env, and a lone agent
    c = ("cw", "one_step", "tabular", "eps_greedy", "qlearning")
    pop = rl.Population(rl.default_params(**pc.base_kw(c, pmc.G)), pc.seed_members(2))
    try:
        assert L.rl_population_maps(pop.h, 0, 2, out, 2) == RL_E_STATE
    finally:
        pop.close()
    dev = rl.Agent(rl.default_params(**dict(kw, map8x8=ids[1])))
    try:
        assert L.rl_population_maps(dev.h, 0, 1, out, 1) == RL_E_STATE
        assert b"not a population" in L.rl_last_error()
    finally:
        dev.close()

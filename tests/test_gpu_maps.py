"""Caller-supplied FrozenLake maps (rl_map_register) on the device: every kernel family
that runs FrozenLake / FrozenLakeEdited, on maps that are not square, start away
from cell 0, have several start cells or none.

Custom maps are checked against tests/maps_model.py (the rectangular restatement
tests/test_maps.py ties to tests/golden/faithful_py.py); the shared-Q arithmetic
against tests/step_model.py, which is env-independent.  A registered copy of a
built-in map runs the new instantiations on the built-in tables, so it must equal the
built-in run bit for bit: that carries the oracle parity of the built-in maps over to
the agents faithful_py does not model (UCB's ln, traces, Dyna, networks).
"""
import numpy as np
import pytest

import maps_model as mm
from golden import faithful_py as fp
from test_step_model import replay_and_check

pytestmark = pytest.mark.gpu
SEED = 0x5EED
KINDS = ("frozen_lake", "frozen_lake_edited")


# ------------------------------------------------------------------ a. Env API streams
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name, slip", [("A", 1), ("B2", 0), ("C", 1), ("N", 0)])
def test_env_streams_equal_the_restatement(rl, name, slip, kind):
    rows, n, steps = mm.MAPS[name], 64, 200
    p = rl.default_params(env=kind, map=rows, slippery=slip, max_steps=24)
    env = rl.Env(p, n, seed=SEED)
    try:
        actions = np.random.RandomState(11).randint(0, 4, size=(steps, n)).astype(np.uint32)
        models = [mm.make_env(kind, rows, slip, 24) for _ in range(n)]
        rngs = [fp.Xoshiro128p(SEED, lane) for lane in range(n)]
        assert env.reset().tolist() == [m.reset(r) for m, r in zip(models, rngs)]
        for k in range(steps):
            obs, rew, term = env.step(actions[k])
            want = [m.step(int(a), r) for m, r, a in zip(models, rngs, actions[k])]
            assert obs.tolist() == [w[0] for w in want], f"step {k}: obs"
            assert rew.tolist() == [w[1] for w in want], f"step {k}: reward"
            assert term.tolist() == [w[2] for w in want], f"step {k}: terminated"
            for lane in np.flatnonzero(term):
                assert env.reset_lane(int(lane)) == models[lane].reset(rngs[lane]), f"step {k}: reset of lane {lane}"
        starts, tot = mm.coverage(models)
        assert set(starts) == ({i for i, ch in enumerate("".join(rows)) if ch == "S"} or {0})
        assert tot["trunc"] > 0 and tot["hole"] > 0
    finally:
        env.close()


# ------------------------------------------------------------------ b. registered copy == built-in
def _snapshot(dev):
    core, aux = dev.lane_state()
    out = dict(core=core, aux=aux, stats=dev.stats())
    out["q"] = dev.q().view(np.uint64) if dev.private else dev.q_raw()
    n, t = dev.ucb()
    out["ucb_n"], out["ucb_t"] = np.asarray(n), np.asarray(t)
    if dev.p["policy"] == "neural":
        out["weights"] = dev.weights().view(np.uint64)
    return out


SHARED = dict(n_lanes=1024, group_size=256, sync_every=16, n_episodes_for_decay=40)
PRIVATE = dict(n_lanes=64, group_size=1, sync_every=32, n_episodes_for_decay=20)
COPY_CASES = {
    # name: (params, map id m, what to run)
    "shared-fixed-det": (dict(SHARED, slippery=0), 1, "run"),
    "shared-slippery": (dict(SHARED, slippery=1), 1, "run"),
    "shared-fixed-det-4x4-train": (dict(SHARED, slippery=0), 0, "train"),
    "shared-ucb-expected-sarsa": (dict(SHARED, slippery=1, selector="ucb", algo="expected_sarsa"), 1, "run"),
    "shared-traces-sarsa-reset-step": (dict(SHARED, slippery=1, agent="traces", algo="sarsa"), 1, "run-rs"),
    "shared-double": (dict(SHARED, slippery=1, policy="double", algo="sarsa"), 0, "run"),
    "shared-edited": (dict(SHARED, env="frozen_lake_edited", slippery=1), 1, "run"),
    "private-one-step": (dict(PRIVATE, slippery=1, algo="expected_sarsa"), 1, "train"),
    "private-double-ucb": (dict(PRIVATE, slippery=1, policy="double", selector="ucb"), 1, "train"),
    "private-traces": (dict(PRIVATE, slippery=1, agent="traces", algo="sarsa"), 0, "train"),
    "private-planning": (dict(PRIVATE, slippery=0), 0, "train-plan"),
    "private-edited-traces": (dict(PRIVATE, env="frozen_lake_edited", agent="traces", slippery=1), 0, "train"),
    "neural-scalar-4x4": (dict(PRIVATE, policy="neural", net_input="scalar", decay_kind=1, eps_decay=0.5), 0, "train"),
    "neural-fl-obs-edited": (dict(PRIVATE, n_lanes=16, env="frozen_lake_edited", policy="neural", net_input="fl_obs",
                                  decay_kind=1, eps_decay=0.5, slippery=1), 0, "train"),
}


@pytest.mark.parametrize("name", list(COPY_CASES))
def test_registered_copy_equals_built_in_bit_for_bit(rl, name):
    kw, m, what = COPY_CASES[name]
    mid = rl.register_map(fp.MAP8 if m else fp.MAP4)
    assert mid >= 2
    snaps = []
    for map_id in (m, mid):
        dev = rl.Agent(rl.default_params(**dict(kw, map8x8=map_id)))
        try:
            if what == "run-rs":
                dev.set_reset_step(True)
            if what == "train-plan":
                dev.set_planning(3)
            if what.startswith("run"):
                dev.run(4)
                dev.synchronize()
            else:
                dev.train(20, 10)
            snaps.append(_snapshot(dev))
        finally:
            dev.close()
    a, b = snaps
    assert a["stats"]["train_steps"] > 0 and a["stats"] == b["stats"], (a["stats"], b["stats"])
    for k in a:
        if k != "stats":
            assert np.array_equal(a[k], b[k]), f"{k} differs between map8x8 = {m} and its registered copy"


# ------------------------------------------------------------------ c. private agents == the Python loop
def _python_lane(kind, rows, slip, algo, lane, n, eval_at, max_steps):
    rng = fp.Xoshiro128p(SEED, lane)
    env = mm.make_env(kind, rows, slip, max_steps)
    ag = fp.Agent(rng, "eps_greedy", algo, n_episodes=n)
    rh, el, te = fp.train(ag, env, n, eval_at)
    q = [ag.values(s) for s in range(len(env.start))]
    return q, rh, el, te, env


@pytest.mark.parametrize("algo", ("qlearning", "sarsa", "expected_sarsa"))
@pytest.mark.parametrize("slip", (0, 1))
@pytest.mark.parametrize("name", ("A", "B2"))
def test_private_agents_equal_the_python_loop(rl, name, slip, algo):
    rows, L, n, eval_at = mm.MAPS[name], 4, 300, 100
    p = rl.default_params(map=rows, slippery=slip, algo=algo, n_lanes=L, group_size=1, max_steps=24,
                          n_episodes_for_decay=n, seed=SEED)
    dev = rl.Agent(p)
    try:
        dev.set_episode_log(1024)
        st = dev.train(n, eval_at)
        q = dev.q()
        eps, lost = dev.episodes()
    finally:
        dev.close()
    assert lost == 0
    updates, envs, learned = 0, [], 0
    for lane in range(L):
        wq, rh, el, te, env = _python_lane("frozen_lake", rows, slip, algo, lane, n, eval_at, 24)
        envs.append(env)
        updates += len(te)
        assert np.array_equal(q[lane, 0].view(np.uint64), np.array(wq, np.float64).view(np.uint64)), f"lane {lane}: Q"
        mine = eps[(eps["lane"] == lane) & (eps["mode"] == 0)]
        assert np.array_equal(mine["reward"], np.array(rh, np.float64)), f"lane {lane}: episode rewards"
        assert np.array_equal(mine["length"], np.array(el, np.uint32)), f"lane {lane}: episode lengths"
        learned += bool(np.count_nonzero(np.array(wq)))
    assert st["train_steps"] == updates
    # the case is on its edges, judged from the Python side
    starts, tot = mm.coverage(envs)
    assert set(starts) == {i for i, ch in enumerate("".join(rows)) if ch == "S"}
    assert tot["goal"] > 0 and tot["hole"] > 0 and tot["trunc"] > 0 and learned > 0


# ------------------------------------------------------------------ d. one lane of a learner group
def test_one_lane_in_a_learner_group_is_the_reference_loop(rl):
    """the custom-map twin of test_gpu_f64.py::test_one_lane_f64_is_the_reference_loop; lane 1,
    because lane 0 learns nothing on map A"""
    n = 300
    p = rl.default_params(map=mm.MAP_A, slippery=1, n_lanes=1, group_size=2, sync_every=37, lane_offset=1,
                          max_steps=24, n_episodes_for_decay=n, seed=SEED)
    dev = rl.Agent(p)
    try:
        dev.set_q_mode("f64")
        dev.train(n, 75)
        q = dev.q()
    finally:
        dev.close()
    wq, _, _, _, env = _python_lane("frozen_lake", mm.MAP_A, 1, "qlearning", 1, n, 75, 24)
    assert np.count_nonzero(np.array(wq)) > 0 and set(env.seen["starts"]) == {3, 8}
    assert np.array_equal(q[0].view(np.uint64), np.array(wq, np.float64).view(np.uint64))


# ------------------------------------------------------------------ e. shared mode, trajectories predicted
class _Tap:
    """the agent, keeping a copy of every records() the replay helper takes"""

    def __init__(self, dev):
        self._dev, self.taken = dev, []

    def __getattr__(self, k):
        return getattr(self._dev, k)

    def records(self):
        r = self._dev.records()
        self.taken.append(r.copy())
        return r


TRAJ = dict(n_lanes=128, group_size=64, sync_every=64, eps0=1.0, eps_decay=0.0, seed=SEED)
TRAJ_CASES = {
    # name: (map, params, expected representation (None: not replayed), reset-and-step)
    "A-det-fixed40": ("A", dict(slippery=0, max_steps=24, algo="qlearning"), "fixed40", False),
    "A-slippery-f64": ("A", dict(slippery=1, max_steps=24, algo="qlearning"), "f64", False),
    "C-slippery": ("C", dict(slippery=1, max_steps=40, algo="qlearning"), "f64", False),
    "A-det-reset-step": ("A", dict(slippery=0, max_steps=24, algo="qlearning"), "fixed40", True),
    "A-traces-sarsa": ("A", dict(slippery=1, max_steps=24, agent="traces", algo="sarsa"), None, False),
}


@pytest.mark.parametrize("name", list(TRAJ_CASES))
def test_shared_trajectories_are_predicted(rl, name):
    """epsilon pinned at 1: every selection explores, so each lane's records follow from
    its stream and the restated env; Q is replayed by the exact step model"""
    mname, kw, repr_, rs = TRAJ_CASES[name]
    rows, launches = mm.MAPS[mname], 2
    p = rl.default_params(map=rows, **TRAJ, **kw)
    dev = rl.Agent(p)
    try:
        if rs:
            dev.set_reset_step(True)
        dev.set_recording(True)
        tap = _Tap(dev)
        if repr_ is None:
            for _ in range(launches):
                dev.run(1)
                dev.synchronize()
                tap.records()
        else:
            assert dev.q_repr() == repr_
            replay_and_check(tap, p, lambda: (dev.run(1), dev.synchronize()), launches=launches)
    finally:
        dev.close()
    got = np.concatenate(tap.taken)
    K = p["sync_every"] * launches
    assert got.shape == (K, p["n_lanes"])
    want, envs = mm.predict_records(lambda: mm.make_env("frozen_lake", rows, kw["slippery"], kw["max_steps"]),
                                    SEED, p["n_lanes"], K, reset_step=rs)
    for k in range(K):
        for lane in range(p["n_lanes"]):
            g = got[k, lane]
            have = (int(g["kind"]), int(g["s"]), int(g["a"]), int(g["s2"]), int(g["a2"]), float(g["r"]), int(g["term"]))
            assert have == want[k][lane] and int(g["mode"]) == 0, f"step {k} lane {lane}: {have} != {want[k][lane]}"
    starts, tot = mm.coverage(envs)
    assert set(starts) == {i for i, ch in enumerate("".join(rows)) if ch == "S"} and min(starts.values()) > 0
    assert tot["goal"] > 0 and tot["hole"] > 0 and tot["trunc"] > 0
    assert bool((got["kind"] == 3).any()) == rs

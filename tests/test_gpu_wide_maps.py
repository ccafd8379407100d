"""FrozenLake maps of up to 1024 cells (rl_map_register_wide) on the device: the wide
transition table (one u16 per (state, direction)) in every kernel family that runs
FrozenLake / FrozenLakeEdited.

The maps are tests/wide_maps.py's, the env model tests/maps_model.py and the shared-Q
arithmetic tests/step_model.py, none of which depends on the map's size.  A wide
copy of a built-in map runs the wide kernels on the built-in tables and must equal
the built-in run bit for bit, which carries the built-in maps' oracle parity over
to UCB's ln, traces (the per-lane pair lists against the pair pool), Dyna and the
networks; the moat pair does the same for state ids >= 256.
"""
import ctypes as C

import numpy as np
import pytest

import maps_model as mm
import wide_maps as wm
from golden import faithful_py as fp
from test_gpu_maps import COPY_CASES, TRAJ, _python_lane, _snapshot, _Tap
from test_step_model import replay_and_check

pytestmark = pytest.mark.gpu
SEED = 0x5EED
KINDS = ("frozen_lake", "frozen_lake_edited")
RL_E_ARG = 2


# ------------------------------------------------------------------ a. Env API streams
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("slip", (0, 1))
@pytest.mark.parametrize("name", ("L65", "L300", "L1024"))
def test_env_streams_equal_the_restatement(rl, name, slip, kind):
    rows, n, steps = wm.LMAPS[name], 64, 200
    p = rl.default_params(env=kind, map=rows, wide=True, slippery=slip, max_steps=24)
    assert rl.map_is_wide(p["map8x8"])
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
        assert set(starts) == {i for i, ch in enumerate("".join(rows)) if ch == "S"}
        assert tot["trunc"] > 0 and tot["hole"] > 0 and tot["goal"] > 0
    finally:
        env.close()


# ------------------------------------------------------------------ b. wide copy == built-in
def _run_case(rl, kw, what, map_id):
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
        return _snapshot(dev)
    finally:
        dev.close()


@pytest.mark.parametrize("name", list(COPY_CASES))
def test_wide_copy_equals_built_in_bit_for_bit(rl, name):
    kw, m, what = COPY_CASES[name]
    mid = rl.register_map(fp.MAP8 if m else fp.MAP4, wide=True)
    assert mid >= 2 and rl.map_is_wide(mid)
    a, b = _run_case(rl, kw, what, m), _run_case(rl, kw, what, mid)
    assert a["stats"]["train_steps"] > 0 and a["stats"] == b["stats"], (a["stats"], b["stats"])
    for k in a:
        if k != "stats":
            assert np.array_equal(a[k], b[k]), f"{k} differs between map8x8 = {m} and its wide copy"


# ------------------------------------------------------------------ c. the moat isomorphism
MOAT_CASES = [n for n in COPY_CASES if not n.startswith("neural")]   # the networks' inputs differ


def _f(s):
    """M1 state -> M2 state; 0 <-> 0 (plain FrozenLake's truncation observation, the
    literal state 0 in both; M1's cell 0 is an unreachable corner)"""
    return np.where(np.asarray(s) == 0, 0, wm.rel(np.asarray(s)))


@pytest.mark.parametrize("name", MOAT_CASES)
def test_moat_copy_at_state_ids_past_255_is_isomorphic(rl, name):
    kw, _, what = COPY_CASES[name]
    assert rl.default_params(**kw)["q_default"] == 0.0
    a = _run_case(rl, kw, what, rl.register_map(wm.M1))
    b = _run_case(rl, kw, what, rl.register_map(wm.M2, wide=True))
    assert a["stats"]["train_steps"] > 0 and a["stats"] == b["stats"], (a["stats"], b["stats"])
    # lane state: s relabelled, everything else equal
    assert np.array_equal(_f(a["core"][:, 0]), b["core"][:, 0]), "lane states"
    assert np.array_equal(a["core"][:, 1:], b["core"][:, 1:]) and np.array_equal(a["aux"], b["aux"])
    assert np.array_equal(a["ucb_t"], b["ucb_t"])
    idx = _f(np.arange(64))
    assert idx.max() >= 256 and len(set(idx.tolist())) == 64
    rest = np.setdiff1d(np.arange(400), idx)
    for k in ("q", "ucb_n"):                       # [..., S, A]
        assert np.array_equal(b[k][..., idx, :], a[k]), f"{k}: M2[rel(s)] != M1[s]"
        assert not b[k][..., rest, :].any(), f"{k}: an M2 entry outside the copy moved"
    assert a["q"].any()


# ------------------------------------------------------------------ d. private agents == the Python loop
@pytest.mark.parametrize("algo", ("qlearning", "sarsa", "expected_sarsa"))
@pytest.mark.parametrize("slip", (0, 1))
@pytest.mark.parametrize("name", ("L65", "L300"))
def test_private_agents_equal_the_python_loop(rl, name, slip, algo):
    rows, L, n, eval_at = wm.LMAPS[name], 4, 300, 100
    p = rl.default_params(map=rows, wide=True, slippery=slip, algo=algo, n_lanes=L, group_size=1, max_steps=24,
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
    starts, tot = mm.coverage(envs)
    assert set(starts) == {i for i, ch in enumerate("".join(rows)) if ch == "S"}
    assert tot["goal"] > 0 and tot["hole"] > 0 and tot["trunc"] > 0 and learned == L   # all four lanes learn


# ------------------------------------------------------------------ e. one lane of a learner group
def test_one_lane_in_a_learner_group_is_the_reference_loop(rl):
    n = 300
    p = rl.default_params(map=wm.L65, wide=True, slippery=1, n_lanes=1, group_size=2, sync_every=37, lane_offset=1,
                          max_steps=24, n_episodes_for_decay=n, seed=SEED)
    dev = rl.Agent(p)
    try:
        dev.set_q_mode("f64")
        dev.train(n, 100)
        q = dev.q()
    finally:
        dev.close()
    wq, _, _, _, env = _python_lane("frozen_lake", wm.L65, 1, "qlearning", 1, n, 100, 24)
    assert np.count_nonzero(np.array(wq)) > 0 and set(env.seen["starts"]) == {30, 64}
    assert np.array_equal(q[0].view(np.uint64), np.array(wq, np.float64).view(np.uint64))


# ------------------------------------------------------------------ f. shared mode, trajectories predicted
TRAJ_CASES = {
    # name: (map, params, expected representation (None: records only), reset-and-step, groups per CU asserted)
    "L65-det-fixed40": ("L65", dict(slippery=0, algo="qlearning"), "fixed40", False, False),
    "L65-slippery-f64": ("L65", dict(slippery=1, algo="qlearning"), "f64", False, False),
    "L256-slippery": ("L256", dict(slippery=1, algo="qlearning"), "f64", False, False),
    "L300-det-reset-step": ("L300", dict(slippery=0, algo="qlearning"), "fixed40", True, False),
    "L1024-det-fixed40-at-the-lds-cap": ("L1024", dict(slippery=0, algo="qlearning"), "fixed40", False, True),
    "L1024-slippery-f64": ("L1024", dict(slippery=1, algo="qlearning"), "f64", False, False),
    "L256-traces-sarsa": ("L256", dict(slippery=1, agent="traces", algo="sarsa"), None, False, False),
}


@pytest.mark.parametrize("name", list(TRAJ_CASES))
def test_shared_trajectories_are_predicted(rl, name):
    """epsilon pinned at 1: every selection explores, so each lane's records follow from
    its stream and the restated env; Q is replayed by the exact step model"""
    mname, kw, repr_, rs, occ = TRAJ_CASES[name]
    rows, launches = wm.LMAPS[mname], 2
    p = rl.default_params(map=rows, wide=True, max_steps=24, **TRAJ, **kw)
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
        if occ:
            o = dev.occupancy()
            print("occupancy", o)
            assert o["groups_per_cu"] >= 1 and o["lds_bytes"] <= 160 * 1024
    finally:
        dev.close()
    got = np.concatenate(tap.taken)
    K = p["sync_every"] * launches
    assert got.shape == (K, p["n_lanes"])
    want, envs = mm.predict_records(lambda: mm.make_env("frozen_lake", rows, kw["slippery"], 24),
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


# ------------------------------------------------------------------ g. the LDS guard
GUARD = dict(n_lanes=128, group_size=64, sync_every=16, slippery=1, policy="double", algo="sarsa")


def test_tables_past_the_lds_are_rejected_at_create_with_the_bytes_needed(rl):
    """the double policy in f64 at 1024 cells: q + sum + cnt alone are 160 KiB"""
    cfg = rl.agent_config(rl.default_params(map=wm.L1024, wide=True, **GUARD))
    h = C.c_void_p()
    assert rl.lib().rl_agent_create(C.byref(cfg), C.byref(h)) == RL_E_ARG
    msg = rl.lib().rl_last_error().decode()
    assert "160 KiB LDS" in msg and "bytes needed" in msg, msg
    need = int(msg.split("(")[1].split(" bytes needed")[0])
    assert need > 160 * 1024 and need >= 2 * 1024 * 4 * (8 + 8 + 4), msg


def test_the_same_agent_at_256_cells_creates_and_runs(rl):
    dev = rl.Agent(rl.default_params(map=wm.L256, wide=True, **GUARD))
    try:
        assert dev.q_repr() == "f64"
        dev.run(1)
        dev.synchronize()
        assert dev.stats()["train_steps"] > 0
    finally:
        dev.close()

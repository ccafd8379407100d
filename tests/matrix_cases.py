"""The parity matrix: every agent / policy / selector / algorithm combination of
every translation unit of the training kernels, shared and private.

tests/test_matrix_coverage.py (CPU) asserts on the oracle's records that every
case is live (tests/coverage.py); tests/test_gpu_matrix.py compares the device
with the oracle on the same cases.

Measured on the oracle at the shapes below (minimum over the 240 cases, and the
case that gives it):
  shared, run (a): 32 steps of 130 lanes in groups of 64, 64 and 2
    share of training STEP records with a finite non-zero td   100 %   (every case)
    Q entries changed                                          20      cw-one_step-tabular-ucb-sarsa
    (step, group, s, a) entries with >= 2 contributions        58      taxi-traces-tabular-eps_greedy-sarsa
    largest contribution count of one entry                    3       taxi-one_step-tabular-eps_greedy-sarsa
    (launch, s, a) entries moved by >= 2 groups                27      cw-traces-tabular-ucb-sarsa
    RESET records                                              134     cw-one_step-tabular-ucb-expected_sarsa
    terminal or truncated training steps                       90      fl8-one_step-tabular-eps_greedy-expected_sarsa
    training STEP records                                      2500    bj-traces-double-ucb-sarsa
  Every case ends episodes inside the window, the UCB ones on fl8 included (with
  q_default 0.25 their lanes reach holes within 32 steps), so no case is excepted
  from the terminal-step condition.  Taxi truncates at max_steps 6.
  private, train(12, 4) (Blackjack train(60, 20)) on 37 agents:
    share of training STEP records with a finite non-zero td   100 %   (every case)
    training STEP records                                      3221    fl4-slip-one_step-tabular-eps_greedy-sarsa
    terminal or truncated training steps                       444     fl8-one_step-tabular-eps_greedy-sarsa
    Q entries changed (all agents)                             574     fl4-slip-one_step-tabular-ucb-expected_sarsa
  the proven bound's edge: max |lr td| / delta_bound between 0.963 (expected SARSA on
  fl8 and CliffWalking) and 1.0 (Blackjack, CliffWalking SARSA); >= 93 (step, entry)
  pairs with >= 2 contributions except Taxi's Q-learning and SARSA (10)
"""
import itertools

import numpy as np

from golden.faithful_py import MAP8

# name -> (env params, registration of the built-in 8x8 map on the device: None,
# "map" (rl_map_register) or "wide" (rl_map_register_wide)).  A registered copy runs
# the *_map / *_wide translation units on the built-in tables; the oracle runs the
# built-in map (tests/test_gpu_maps.py and test_gpu_wide_maps.py establish that a
# copy equals the built-in bit for bit).
ENV_VARIANTS = {
    "fl8": (dict(env="frozen_lake", map8x8=1, slippery=0), None),
    "fl4-slip": (dict(env="frozen_lake", map8x8=0, slippery=1), None),
    "fle8-slip": (dict(env="frozen_lake_edited", map8x8=1, slippery=1), None),
    "cw": (dict(env="cliff_walking"), None),
    "taxi": (dict(env="taxi"), None),
    "bj": (dict(env="blackjack"), None),
    "fl8-map": (dict(env="frozen_lake", map8x8=1, slippery=0), "map"),
    "fle8-slip-map": (dict(env="frozen_lake_edited", map8x8=1, slippery=1), "map"),
    "fl8-slip-wide": (dict(env="frozen_lake", map8x8=1, slippery=1), "wide"),
    "fle8-wide": (dict(env="frozen_lake_edited", map8x8=1, slippery=0), "wide"),
}
AGENTS = ("one_step", "traces")
POLICIES = ("tabular", "double")
SELECTORS = ("eps_greedy", "ucb")
ALGOS = ("sarsa", "qlearning", "expected_sarsa")

Q_DEFAULT = 0.25      # exact in the 2^-40 fixed point; FrozenLake pays nothing before the goal
SHARED = dict(n_lanes=130, group_size=64, sync_every=8, n_episodes_for_decay=40, q_default=Q_DEFAULT)
SHARED_LAUNCHES = 4
SHARED_TRAIN = (6, 3)     # train(n_episodes, eval_at), eval_episodes 3
PRIVATE = dict(n_lanes=37, group_size=1, sync_every=25, max_steps=30, q_default=Q_DEFAULT, eval_episodes=3)
TAXI_SHARED_MAX_STEPS = 6   # truncation inside the 32-step window
FAITHFUL_LANE = 5

# minima every shared case meets on the oracle's records of run (a)
SHARED_NEED = dict(live_share=0.9, entries_changed=6, multi_contrib=50, resets=SHARED["n_lanes"])


def combos():
    return list(itertools.product(ENV_VARIANTS, AGENTS, POLICIES, SELECTORS, ALGOS))


def case_id(c):
    return "-".join(c)


def _kw(c):
    var, agent, policy, selector, algo = c
    return dict(ENV_VARIANTS[var][0], agent=agent, policy=policy, selector=selector, algo=algo)


def shared_kw(c):
    kw = dict(SHARED, eval_episodes=SHARED_TRAIN[1], **_kw(c))
    if kw["env"] == "taxi":
        kw["max_steps"] = TAXI_SHARED_MAX_STEPS
    return kw


def private_kw(c):
    n = private_episodes(c)
    return dict(PRIVATE, n_episodes_for_decay=n, **_kw(c))


def private_episodes(c):
    return 60 if ENV_VARIANTS[c[0]][0]["env"] == "blackjack" else 12


def shared_rejected(c):
    """Blackjack under UCB keeps all 2048 rows in LDS (the compact 484 rows are
    eps-greedy's); with the double policy's two tables that is 8192 entries, and q +
    sum + cnt + the counters need 177 to 200 KiB of the CU's 160: rl_agent_create
    rejects the six combinations with RL_E_ARG (the LDS guard).  The oracle runs
    them, and so do private agents; the device test asserts the rejection.  Whoever
    lifts the limit removes this function: the six cases then run the comparison."""
    return ENV_VARIANTS[c[0]][0]["env"] == "blackjack" and c[2] == "double" and c[3] == "ucb"


def presets_ucb(c):
    """UCB + expected SARSA goes NaN on the first update from fresh counters (SURVEY
    F7: a zero count gives an infinite bonus, inf / inf weights); preset counters
    keep the probability-weighted bootstrap on finite numbers"""
    return c[3] == "ucb" and c[4] == "expected_sarsa"


def ucb_preset(S, A, lanes=None, seed=20):
    """counts in [1, 50) from a fixed stream, t = 5000; lanes: private agents"""
    rs = np.random.RandomState(seed)
    shape = (S, A) if lanes is None else (lanes, S, A)
    counts = rs.randint(1, 50, size=shape).astype(np.uint64)
    t = np.uint64(5000) if lanes is None else np.full(lanes, 5000, np.uint64)
    return counts, t


def device_params(rl, kw, c):
    """the device's parameters of a case: a registered copy's map id in place of 1"""
    reg = ENV_VARIANTS[c[0]][1]
    p = rl.default_params(**kw)
    if reg:
        p["map8x8"] = rl.register_map(MAP8, wide=(reg == "wide"))
    return p


def shared_oracle(oracle, c, q_mode=None):
    """the oracle of a shared case, prepared as the device is in test_gpu_matrix.py"""
    p = oracle.default_params(**shared_kw(c))
    ref = oracle.Batch(p)
    if q_mode:
        ref.set_q_mode(q_mode)
    if presets_ucb(c):
        ref.set_ucb(*ucb_preset(ref.S, ref.A))
    return p, ref


def private_oracle(oracle, c, preset=True):
    p = oracle.default_params(**private_kw(c))
    ref = oracle.Batch(p)
    if preset and presets_ucb(c):
        ref.set_ucb(*ucb_preset(ref.S, ref.A, lanes=p["n_lanes"]))
    return p, ref

# ---------------------------------------------------------------- the proven bound's edge
# rl_host.cpp delta_bound = lr (R + (1 + gamma) max(|Q0|, R / (1 - gamma))): the fixed
# point needs delta_bound < 2000 (fix_proven), the packed step sums of the 8-wave
# kernels G * delta_bound < 2000 (pack_proven).  The table is preset to +-M at random
# signs, M = R / (1 - gamma) rounded down to the 2^-40 grid (the unrounded value is
# not exact in the fixed point and would move the agent to f64), so the first
# updates come close to the bound: name -> (params, R, packed).
# In f64, as the host computes it, 1 - 0.95 = 0.05 + 4.4e-17 and CliffWalking's
# delta_bound is 200 - 1.7e-13: G 10 gives 1999.9999999999983 < 2000, the last packed
# group size (by 1.7e-12), and G 11 is the first unpacked one.
BOUND_GAMMA = 0.95
BOUND_ENVS = {
    "fl8-lr1-G49": (dict(env="frozen_lake", map8x8=1, lr=1.0, group_size=49), 1.0, True),        # 1960
    "fl8-lr0.5-G128": (dict(env="frozen_lake", map8x8=1, lr=0.5, group_size=128), 1.0, False),   # 2560
    "bj-lr1-G49": (dict(env="blackjack", lr=1.0, group_size=49), 1.0, True),                     # 1960
    "taxi-lr0.05-G9": (dict(env="taxi", lr=0.05, group_size=9), 20.0, True),                     # 360
    "cw-lr0.05-G9": (dict(env="cliff_walking", lr=0.05, group_size=9), 100.0, True),             # 1800
    "cw-lr0.05-G10": (dict(env="cliff_walking", lr=0.05, group_size=10), 100.0, True),           # 2000 - 1.7e-12
    "cw-lr0.05-G11": (dict(env="cliff_walking", lr=0.05, group_size=11), 100.0, False),          # 2200
}
BOUND_CASES = [(e, a) for e in BOUND_ENVS for a in ("qlearning", "sarsa", "expected_sarsa")]
BOUND_LAUNCHES = 4
BOUND_TRAIN = (6, 3)


def bound_kw(case):
    env, algo = case
    kw = dict(BOUND_ENVS[env][0])
    if algo == "expected_sarsa":
        # eps-greedy weighs the greedy action 1 - eps and the others eps / A each (sum 1 -
        # eps / A, uniform_epsilon_greed.rs:72-76): at eps 1 the bootstrap stays below
        # 0.75 M with four actions, so these cases start at eps 0.1
        kw["eps0"] = 0.1
    return dict(kw, algo=algo, gamma=BOUND_GAMMA, n_lanes=3 * kw["group_size"] + 5, sync_every=8,
                n_episodes_for_decay=40, eval_episodes=3)


def bound_delta(case):
    """delta_bound of the case, as the host computes it"""
    kw, R, _ = BOUND_ENVS[case[0]]
    return kw["lr"] * (R + (1.0 + BOUND_GAMMA) * (R / (1.0 - BOUND_GAMMA)))


def bound_packed(case):
    """rl_host.cpp pack_proven, in the host's own arithmetic"""
    packed = float(BOUND_ENVS[case[0]][0]["group_size"]) * bound_delta(case) < 2000.0
    assert packed == BOUND_ENVS[case[0]][2], "the case is on the other side of the packed form than its table says"
    return packed


def bound_table(case, P, S, A):
    R = BOUND_ENVS[case[0]][1]
    M = np.floor(R / (1.0 - BOUND_GAMMA) * 2.0 ** 40) * 2.0 ** -40
    rs = np.random.RandomState(4)
    sign = rs.choice([-1.0, 1.0], size=(P, S, A))
    # half the states carry one sign in the whole row: expected SARSA's bootstrap (a
    # probability-weighted sum over the row) reaches +-M only there
    row = rs.rand(S) < 0.5
    sign[:, row, :] = rs.choice([-1.0, 1.0], size=(P, S, 1))[:, row, :]
    return M * sign

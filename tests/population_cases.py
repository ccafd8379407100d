"""Cases of the population tests (rl.h rl_population_create): member m of a population
is the lone shared agent of n_lanes = group_size = G with the member's own fields, so
its reference is the CPU oracle's one-group Batch.

tests/test_population_liveness.py asserts on the oracle alone (CPU) that every case
moves every member's table and that members differ; tests/test_gpu_population.py
compares the device with the same oracles.
"""
import itertools

import matrix_cases as mc

MEMBER_KEYS = ("lr", "gamma", "eps0", "eps_decay", "eps_final", "ucb_c", "seed", "lane_offset")

# the supported slice: one-step agents on the built-in envs, no UCB + expected SARSA
ENVS = ("fl8", "fl4-slip", "cw", "taxi", "bj")
MATRIX = [(e, "one_step", po, se, al)
          for e, po, se, al in itertools.product(ENVS, mc.POLICIES, mc.SELECTORS, mc.ALGOS)
          if not (se == "ucb" and al == "expected_sarsa")]
MATRIX_M, MATRIX_G = 3, 80          # one full wave plus a 16-lane partial one
MATRIX_LAUNCHES = mc.SHARED_LAUNCHES   # 4 launches of K = 8
NEED_CHANGED = mc.SHARED_NEED["entries_changed"]


def rejected(c):
    """Blackjack + double + UCB: the learner group's tables exceed the LDS (matrix_cases.shared_rejected)"""
    return mc.shared_rejected(c)


def expected_repr(c):
    """slippery FrozenLake and the double policy run in f64; the tabular policy on the
    other envs is proven for the fixed point (lr 0.05, gamma 0.95, q_default 0.25)"""
    return "f64" if c[0] == "fl4-slip" or c[2] == "double" else "fixed40"


def seed_members(n, seed0=0x5EED):
    """members that differ in seed and lane_offset only"""
    return [dict(seed=seed0 + 977 * m, lane_offset=1000 * m) for m in range(n)]


def deterministic(c):
    """UCB on a map with one start and no slip draws nothing: selection, env and update
    are functions of the table and the counters alone, so members that differ in seed
    and lane_offset only would all learn the same table"""
    return c[3] == "ucb" and c[0] in ("fl8", "cw")


def matrix_members(c):
    """the matrix's members: they differ in seed and lane_offset only — and, where no
    draw enters the case at all (deterministic), in lr too (0.05, 0.06, 0.07: the same
    representation), so that the condition "no two members learn the same table" can
    hold there as well.  (ucb_c alone does not part them inside the window: untried
    actions carry an infinite bonus whatever c is.)"""
    members = seed_members(MATRIX_M)
    if deterministic(c):
        members = [dict(m, lr=0.05 + 0.01 * i) for i, m in enumerate(members)]
    return members


# train(6, 3) with eval_episodes 3: seeds at which the three members need different
# numbers of launches (fl8: 58 / 61 / 55, Blackjack: 5 / 6 / 5 at K = 8), so that
# members idle while others still run
TRAIN_SEED0 = {"fl8": 0x5EED, "bj": 10}


def train_members(env):
    return seed_members(3, seed0=TRAIN_SEED0[env])


# members with their own lr / gamma / epsilon schedule (and, under UCB, ucb_c); all
# proven for the fixed point on fl8 (delta_bound = lr (1 + (1 + gamma) / (1 - gamma)) <= 10)
HETERO = [dict(lr=0.05, gamma=0.95, eps0=1.0, eps_decay=0.05, eps_final=0.0, seed=11),
          dict(lr=0.1, gamma=0.9, eps0=0.8, eps_decay=0.02, eps_final=0.1, seed=12),
          dict(lr=0.5, gamma=0.5, eps0=0.5, eps_decay=0.1, eps_final=0.3, seed=13),
          dict(lr=0.01, gamma=0.99, eps0=0.3, eps_decay=0.3, eps_final=0.05, seed=14),
          dict(lr=1.0, gamma=0.0, eps0=0.0, eps_decay=0.0, eps_final=0.0, seed=15)]
# (ucb_c 0 would be a greedy walk that never leaves the first row: not live)
HETERO_UCB = [dict(m, ucb_c=c) for m, c in zip(HETERO, (0.5, 0.25, 2.0, 0.1, 10.0))]


def base_kw(c, G, **over):
    """the live parameters of a matrix case for members of G lanes (q_default 0.25,
    n_episodes_for_decay 40, Taxi max_steps 6)"""
    return dict(mc.shared_kw(c), n_lanes=G, group_size=G, **over)


def member_params(mod, base, member):
    """parameters of one member as a lone agent, for `mod`.default_params' consumers
    (mod: rlamd or oracle_ffi): the base with the member's overrides and the eps_decay
    default rule"""
    p = dict(base)
    p.update(member)
    if "eps_decay" not in member and "eps0" in member:
        p["eps_decay"] = p["eps0"] / (p["exploration_time"] * p["n_episodes_for_decay"])
    return p


def member_oracles(oracle, base, members, q_mode=None):
    """one oracle Batch per member (n_lanes = group_size = G), in the population's representation"""
    refs = []
    for m in members:
        ref = oracle.Batch(member_params(oracle, base, m))
        if q_mode:
            ref.set_q_mode(q_mode)
        refs.append(ref)
    return refs


def population_q_mode(refs):
    """a population is fixed point iff every member's lone agent is; else all f64"""
    return None if all(r.q_repr() == "fixed40" for r in refs) else "f64"

"""Cases of the map-population tests (rl.h rl_population_create_maps): member m of such
a population is the lone shared agent of n_lanes = group_size = G on map_ids[m] with
the member's own fields, so its reference is that lone device agent (rl.Agent on the
registered map — tests/test_gpu_maps.py and test_gpu_wide_maps.py pin those kernels to
tests/maps_model.py and, on copies of the built-in maps, to the oracle).

tests/test_population_maps_liveness.py asserts on maps_model alone (CPU) that every
map set is live: every start cell drawn, holes and truncations seen, goals reached
where the set says so, and members of one set on different envs parting;
tests/test_gpu_population_maps.py runs the device.
"""
import maps_model as mm
import matrix_cases as mc

G, K, LAUNCHES, MAX_STEPS = 80, 8, mc.SHARED_LAUNCHES, 12   # one full wave plus a 16-lane partial one
SEED = 0x5EED

MAP_4X4 = ["SFFF", "FHFH", "FFFH", "HFFG"]                  # the built-in id 0
Q4_MID = ["FFFG", "FHFF", "FFSF", "HFFF"]                   # one start, cell 10
Q4_NO_S = ["FFFF", "FHFH", "FFFH", "HFFG"]                  # no 'S': cell 0, the same env as id 0
Q4_THREE = ["SFFS", "FHFF", "FFFH", "SHFG"]                 # three starts, cells 0, 3 and 12
R25_TWO = ["SFHFS", "FFFFG"]                                # two starts, cells 0 and 4
W10_ONE = ["FFFFFFFFFF", "FHFFFFFHFF", "FFFFHFFFFF", "FFFFFFHFFF", "FFFHFHFFFF",
           "FFFFFSFHFF", "FFHFHFFFFF", "FFFFFFHFFF", "FHFFFFFFHF", "FFFFFFFFFG"]   # one start, cell 55
W10_TWO = ["FFFFFFFHFS", "FFHFFFFFHF", "FFFFHFFFFF", "FFFHFFFFFF", "FFFFSHFFFF",
           "FFFFHFFFFF", "FHFFFFFHFF", "FFFFFFFFFF", "FFFHFFHFFF", "GFFFFFFFFF"]   # two starts, cells 9 and 44

# name -> [(member name, rows, the id to pass: 0 for the built-in, None to register the rows)]
SETS = {
    "Q4": [("id0", MAP_4X4, 0), ("A", mm.MAP_A, None), ("mid", Q4_MID, None), ("noS", Q4_NO_S, None),
           ("three", Q4_THREE, None)],
    "R25": [("B2", mm.MAP_B2, None), ("two", R25_TWO, None)],
    "W10": [("one", W10_ONE, None), ("two", W10_TWO, None)],   # 100 cells: the wide format only
}
# members of one set that are the same env (no 'S' starts at cell 0 undrawn, as id 0 does)
SAME_ENV = {"Q4": [("id0", "noS")]}
# members whose random walk reaches the goal inside the liveness window
REACH_GOAL = {"Q4": ("A", "mid", "three"), "R25": ("B2", "two"), "W10": ()}
# minima of the liveness window (eps pinned at 1, 80 lanes, 32 steps, max_steps 12)
NEED = dict(start_draws=100, holes=70, truncations=18, pairs=31)


def start_cells(rows):
    cells = [i for i, ch in enumerate("".join(rows)) if ch == "S"]
    return cells or [0]


def map_ids(rl, set_name, wide=False):
    """the set's map ids on the device (the built-in id as it is, narrow only)"""
    out = []
    for _, rows, mid in SETS[set_name]:
        out.append(mid if mid is not None and not wide else rl.register_map(rows, wide=wide))
    return out


def base_kw(env, policy, selector, algo, slippery, **over):
    """matrix_cases.shared_kw's live values (q_default 0.25, K = 8, n_episodes_for_decay
    40, eval_episodes 3) for members of G lanes on a lake with max_steps 12"""
    c = ("fl4-slip", "one_step", policy, selector, algo)
    kw = dict(mc.shared_kw(c), env=env, slippery=int(slippery), max_steps=MAX_STEPS, n_lanes=G, group_size=G)
    kw.pop("map8x8", None)
    kw.update(over)
    return kw


def same_members(n, **fields):
    """n members with one seed and the same hyper-parameters: only their maps part them"""
    return [dict(seed=SEED, lane_offset=0, **fields) for _ in range(n)]


def seed_members(n, seed0=SEED):
    return [dict(seed=seed0 + 977 * m, lane_offset=1000 * m) for m in range(n)]


# (policy, selector, algo): the population's ten variants, and the three the other envs run
TEN = [(po, se, al) for po in mc.POLICIES for se in mc.SELECTORS for al in mc.ALGOS
       if not (se == "ucb" and al == "expected_sarsa")]
THREE = [("tabular", "eps_greedy", "qlearning"), ("double", "eps_greedy", "sarsa"), ("tabular", "ucb", "qlearning")]

"""Plain-Python restatement of FrozenLakeEnv / FrozenLakeEditedEnv on any rectangular
map (TEST INFRASTRUCTURE ONLY), for the caller-supplied maps of rl_map_register.

oracle/ knows the two built-in maps only, so custom maps are checked against this
file.  It subclasses tests/golden/faithful_py.FrozenLake — the model that
tests/test_oracle_cross.py pins to the oracle — and replaces the constructor with
the reference's own for nrow != ncol (src/env/frozen_lake.rs:48-102,
src/env/frozen_lake_edited.rs:168-224, src/utils.rs:45-76); tests/test_maps.py
first asserts that on both built-in maps it gives faithful_py's `probs` and `start`.

Draw rule (DESIGN.md section 2 "draws"): reset draws one uniform01 only when the map
has two or more 'S' cells; one 'S' is a fixed start, no 'S' the all-false argmax's
cell 0 (src/utils.rs:33-43), neither drawn.
"""
from golden import faithful_py as fp

MAP_A = ["FFFS", "FHFH", "SFFH", "HFFG"]                  # two starts, cells 3 and 8
MAP_B2 = ["FFHFF", "SFFFG"]                                # 2 x 5, start 5
MAP_B3 = ["FSF", "FFF", "HFF", "FFH", "FFG"]               # 5 x 3, start 1
MAP_C = ["SFFFFFFS", "FFFFFFFF", "FFFHFFFF", "FFFFFHFF", "FFFHFFFF", "FHHFFFHF", "FHFFHFHF", "SFFHFFFG"]
MAP_N = ["FFF", "FHG"]                                     # no 'S'
MAPS = {"A": MAP_A, "B2": MAP_B2, "B3": MAP_B3, "C": MAP_C, "N": MAP_N}

WALL, VALUE = "W", {"H": -1.0, "W": -0.5, "S": 0.0, "F": 0.5, "G": 1.0}   # frozen_lake_edited.rs:18-28


def inc(nrow, ncol, r, c, a):                              # src/utils.rs:53-76
    if a == 0:
        c = max(c - 1, 0)
    elif a == 1:
        r = min(r + 1, nrow - 1)
    elif a == 2:
        c = min(c + 1, ncol - 1)
    elif a == 3:
        r = max(r - 1, 0)
    return r, c


def get_obs(rows, r, c):
    """FrozenLakeObs (left, down, right, up, x, y) of a cell: frozen_lake_edited.rs:118-149;
    a neighbour off the grid is WALL, x is the row and y the column"""
    nrow, ncol = len(rows), len(rows[0])
    return (WALL if c == 0 else rows[r][c - 1], WALL if r == nrow - 1 else rows[r + 1][c],
            WALL if c == ncol - 1 else rows[r][c + 1], WALL if r == 0 else rows[r - 1][c], r, c)


def fl_obs_features(rows):
    """[left, down, right, up terrain values, x, y] of every cell (frozen_lake_neural.rs:136-145)"""
    out = []
    for r in range(len(rows)):
        for c in range(len(rows[0])):
            o = get_obs(rows, r, c)
            out.append([VALUE[t] for t in o[:4]] + [float(o[4]), float(o[5])])
    return out


class RectLake(fp.FrozenLake):
    """FrozenLakeEnv::new(map, is_slippery, max_steps) for any rows; reset and step are
    faithful_py's, the reset under the draw rule above"""
    edited = False

    def __init__(self, rows, slippery=False, max_steps=100):
        self.rows, self.slippery = list(rows), slippery
        self.nrow, self.ncol = len(rows), len(rows[0])
        flat = "".join(rows)
        starts = [i for i, ch in enumerate(flat) if ch == "S"]
        self.start = [0.0] * len(flat)
        for i in starts:
            self.start[i] = 1.0 / len(starts)
        self.n_starts = len(starts)
        self.probs = []
        for r in range(self.nrow):
            for c in range(self.ncol):
                s = r * self.ncol + c
                row = []
                for a in range(4):
                    li = [(0.0, 0, 0.0, False)] * 3
                    if rows[r][c] in "GH":
                        li[0] = (1.0, s, 0.0, True)
                    elif slippery:
                        li = [(1.0 / 3.0,) + self.outcome(r, c, b) for b in ((a - 1) % 4, a, (a + 1) % 4)]
                    else:
                        li[0] = (1.0,) + self.outcome(r, c, a)
                    row.append(li)
                self.probs.append(row)
        self.max_steps = max_steps
        self.ready = False
        self.pos = 0
        self.curr_step = 0
        self.seen = {"starts": {}, "goal": 0, "hole": 0, "trunc": 0}   # coverage, from the Python side

    def outcome(self, r, c, a):                            # frozen_lake.rs:32-46
        nr, nc = inc(self.nrow, self.ncol, r, c, a)
        letter = self.rows[nr][nc]
        return nr * self.ncol + nc, 1.0 if letter == "G" else 0.0, letter in "GH"

    def reset(self, rng):
        u = rng.uniform01() if self.n_starts >= 2 else 0.0
        self.pos = fp.categorical_sample(self.start, u)
        self.ready = True
        self.curr_step = 0
        self.seen["starts"][self.pos] = self.seen["starts"].get(self.pos, 0) + 1
        return self.pos

    def truncated(self):                                   # frozen_lake.rs:119-122
        return 0, 0.0, True

    def step(self, a, rng):
        if self.ready and self.curr_step >= self.max_steps:
            self.ready = False
            self.seen["trunc"] += 1
            return self.truncated()
        s, r, t = super().step(a, rng)
        if t:                                              # a terminating move lands on G or H in both envs
            letter = "".join(self.rows)[s]
            assert letter in "GH"
            self.seen["goal" if letter == "G" else "hole"] += 1
        return s, r, t


class RectLakeEdited(RectLake):
    """FrozenLakeEditedEnv::new: reward 10 onto the goal and -1 otherwise, termination
    judged by the terrain in the moved direction (frozen_lake_edited.rs:97-116), so a
    move into a wall stays in place and does not terminate; truncation returns the
    current cell with -1.0 (:242-246).  Observations are dense cell indices."""
    edited = True

    def outcome(self, r, c, a):
        terrain = get_obs(self.rows, r, c)[a]
        nr, nc = inc(self.nrow, self.ncol, r, c, a)
        win = terrain == "G"
        return nr * self.ncol + nc, 10.0 if win else -1.0, win or terrain == "H"

    def truncated(self):
        return self.pos, -1.0, True


def make_env(kind, rows, slippery, max_steps):
    return (RectLakeEdited if kind == "frozen_lake_edited" else RectLake)(rows, bool(slippery), max_steps)


def table_of(env):
    """probs / start in rl_env_table's layout: prob, next, reward, term [S][4][3], start [S]"""
    prob = [[[t[0] for t in li] for li in row] for row in env.probs]
    nxt = [[[t[1] for t in li] for li in row] for row in env.probs]
    rew = [[[t[2] for t in li] for li in row] for row in env.probs]
    term = [[[int(t[3]) for t in li] for li in row] for row in env.probs]
    return dict(prob=prob, next=nxt, reward=rew, term=term, start=list(env.start))


def predict_records(make, seed, n_lanes, n_steps, reset_step=False):
    """Every lane's (kind, s, a, s2, a2, r, term) per synchronous step of a shared-mode
    agent whose epsilon is pinned at 1: every selection explores (one u32 for the eps
    test, one for the action), so a lane's trajectory depends on its stream alone.
    Returns (records[step][lane] as tuples, the lanes' envs for their coverage)."""
    recs = [[None] * n_lanes for _ in range(n_steps)]
    envs = []
    for lane in range(n_lanes):
        rng, env = fp.Xoshiro128p(seed, lane), make()
        envs.append(env)

        def act():
            assert rng.eps_test(1.0)
            return rng.uniform_usize(4)

        need_reset, s, a = True, 0, 0
        for k in range(n_steps):
            kind = 2
            if need_reset:
                s = env.reset(rng)
                a = act()
                need_reset = False
                if not reset_step:
                    recs[k][lane] = (1, s, a, 0, 0, 0.0, 0)
                    continue
                kind = 3
            s2, r, term = env.step(a, rng)
            a2 = act()
            recs[k][lane] = (kind, s, a, s2, a2, r, int(term))
            s, a, need_reset = s2, a2, term
    return recs, envs


def coverage(envs):
    starts, tot = {}, {"goal": 0, "hole": 0, "trunc": 0}
    for e in envs:
        for c, n in e.seen["starts"].items():
            starts[c] = starts.get(c, 0) + n
        for k in tot:
            tot[k] += e.seen[k]
    return starts, tot

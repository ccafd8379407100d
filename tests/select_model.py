"""The closed loop of a shared-mode launch: every record from the seed.

TEST INFRASTRUCTURE ONLY.  tests/step_model.py replays a launch FROM its
rl_step_record entries and so takes (kind, s, a, s2, a2, r, term) on trust.  This
file predicts them.  From the agent's configuration, the seed and lane offset,
the raw words of Q_base and the UCB counters N / t before the launch, and the
per-lane state it carries itself (stream, env, current (s, a), whether a reset is
due; epsilon, the double flag and the traces through step_model), it produces
every field of every lane's record of every synchronous step; step_model's
combine and merge then run on the PREDICTED records.  Records, td, Q words, N, t
and epsilon of the side under test must equal the prediction bit for bit.  ln(t)
stays the one checked scalar input (step_model "ln").

It is written from DESIGN.md section 2 ("Lanes", "Draws", "Cards", "One
synchronous step per lane", "Reset-and-step schedule", "Shared mode", "UCB",
"Blackjack observations") and the reference sources cited there; not from
oracle/rlref.c and not from the kernels.  No oracle, library or ctypes call:
Python ints and floats only.

What it restates
----------------
Stream: golden/faithful_py.Xoshiro128p (the splitmix64 key of seed + global_lane *
0x632BE59BD9B4E019, xoshiro128+, uniform01, the eps test with its high word first
— the low word is drawn only when the high word does not decide `u < eps` —,
UniformInt with the power-of-two shortcut and the widening multiply with its
reject zone for Taxi's 6), plus the card rule here (CardSource): card
1 + (h * 10 >> 16) of a 16-bit half h, rejected when (h * 10) & 0xffff > 65529, one
u32 giving two halves, high half first; an env operation takes its cards from its
own words, skips a rejected half and discards a half left at its end.

Envs, draws at the documented sites only:
  FrozenLake / FrozenLakeEdited   maps_model.RectLake / RectLakeEdited on the built-in
                                  4x4 / 8x8 rows (a registered or wide copy of a
                                  built-in map is the same env); reset draws nothing
                                  with one 'S', a slippery step draws one uniform01
  CliffWalking                    src/env/cliff_walking.rs:22-89; no draw
  Taxi                            src/env/taxi.rs:57-159; reset = categorical_sample of
                                  the 1/300 start distribution at one uniform01
  Blackjack                       src/env/blackjack.rs:60-163; deal player 2 cards then
                                  dealer 2, a hit 1 card, a stick the dealer's cards
                                  while below 17; dense index (p * 32 + d) * 2 + ace;
                                  BlackJackEnv::new (:45-58) deals a hand nobody
                                  looks at: the lane's stream gives it at creation
A step asked of an env whose curr_step has reached max_steps is the truncation
(frozen_lake.rs:119-122 (0, 0.0), frozen_lake_edited.rs:242-246 (pos, -1.0),
cliff_walking.rs:78-81 (0, -100.0), taxi.rs:148-151 (0, 0.0); term true, no draw,
Blackjack has none).

Selection (one_step_agent.rs:48-51: the selector on policy.predict(obs)), on the
group's step-start snapshot:
  values    single table: the table; double policy: (alpha[i] + beta[i]) / 2.0
            (double_tabular_policy.rs:31-39); the fixed point: the raw words
  eps-greedy  uniform_epsilon_greed.rs:51-66 with the lane's epsilon: no draw at
            epsilon == 0; else the eps test, then uniform_usize(A) when exploring,
            else the first maximum under a strict `>` from element 0 (utils.rs:1-11)
  UCB       upper_confidence_bound.rs:29-42: argmax of values[i] + c * sqrt(ln(t) /
            (n[i] + 2^-1022)) with IEEE division and square root; n and t are the
            GROUP's counters at the start of the step (every lane of the group reads
            the same ones; step_model increments them after the step's selections);
            a NaN at action 0 wins

Schedule (src/agent.rs:80-106 cut at its get_action calls): a lane that needs a
reset does env.reset() + get_action (kind 1: s, a; the rest 0), otherwise env.step(a)
+ get_action(s2) + update (kind 2).  With the reset-and-step option (eps-greedy
only; ignored with UCB) the reset and the first step share one kind-3 record and
both selections read the same snapshot.  `term` asks for a reset at the lane's
next step.  Draw order within a step is the reference's call order: reset draws,
selection draws, step draws, selection draws.  Epsilon decay, the double flag and
the traces are step_model's, fed by the predicted records.  All lane state is
carried across launches by the Predictor.

Outside the model
-----------------
ln(t) (a checked input), the train() evaluate interleave (plain run() launches in
RL_MODE_TRAIN only: every record has mode 0) and populations.  Private mode, Dyna-Q
planning and the neural policy are outside this file too, but no longer unpinned:
tests/private_model.py reuses the stream, the card rule, the envs and the selection
helpers here and predicts a private lane's records, values, counters and epsilon.

Mutations
---------
Predictor(mutation=...) switches one rule to a plausible wrong one; the tests use
them as negative controls (a live case must report a mismatch):
  "tie_last"        the last maximum instead of the first
  "end_snapshot"    the step's second selection (a2) reads the values after the
                    step's updates (eps-greedy's greedy branch; draws unchanged)
  "alpha_only"      the double policy selects on table 0 alone
  "counters_incremented"  a UCB selection reads the counters as incremented by the
                    lanes before it in the same step
  "eps_post_decay"  the selection after a terminal step tests against the epsilon
                    the step's update decays to
"""
from golden import faithful_py as fp
import maps_model as mm
import step_model as sm

MUTATIONS = ("tie_last", "end_snapshot", "alpha_only", "counters_incremented", "eps_post_decay")
FIELDS = ("kind", "mode", "s", "a", "s2", "a2", "r", "term", "td")


# ---------------------------------------------------------------- stream
class Stream(fp.Xoshiro128p):
    def __init__(self, seed, lane):
        super().__init__(seed, lane)
        self.rejected_halves = 0


def card_of_half(h):
    """(card, rejected) of a 16-bit half: DESIGN section 2 "Cards\""""
    m = h * 10
    return 1 + (m >> 16), (m & 0xFFFF) > 65535 - 6


class CardSource:
    """the cards of ONE env operation: words drawn as needed, high half first"""

    def __init__(self, rng):
        self.rng, self.low = rng, None

    def card(self):
        while True:
            if self.low is None:
                w = self.rng.u32()
                h, self.low = w >> 16, w & 0xFFFF
            else:
                h, self.low = self.low, None
            c, rejected = card_of_half(h)
            if rejected:
                self.rng.rejected_halves += 1
                continue
            return c


# ---------------------------------------------------------------- envs
class TableEnv:
    """an env of deterministic (next, reward, term) entries with max_steps"""
    TRUNCATED = (0, 0.0, True)

    def __init__(self, max_steps):
        self.max_steps, self.ready, self.pos, self.curr_step = max_steps, False, 0, 0
        self.n_trunc = 0

    def step(self, a, rng):
        if not self.ready:
            raise RuntimeError("EnvNotReady")
        if self.curr_step >= self.max_steps:
            self.ready = False
            self.n_trunc += 1
            return self.TRUNCATED
        self.curr_step += 1
        s, r, t = self.obs[self.pos][a]
        self.pos = s
        if t:
            self.ready = False
        return s, r, t


class CliffWalking(TableEnv):
    """src/env/cliff_walking.rs: 4 x 12, start 36, cliff 37..46, goal 47"""
    TRUNCATED = (0, -100.0, True)

    def __init__(self, max_steps):
        super().__init__(max_steps)
        self.obs = []
        for row in range(4):
            for col in range(12):
                li = []
                for a in range(4):
                    nr, nc = mm.inc(4, 12, row, col, a)
                    ns = nr * 12 + nc
                    lose = 37 <= ns <= 46
                    li.append((ns, -100.0 if lose else -1.0, lose or ns == 47))
                self.obs.append(li)

    def reset(self, rng):
        self.pos, self.ready, self.curr_step = 36, True, 0
        return self.pos


TAXI_MAP = ["+---------+", "|R: | : :G|", "| : | : : |", "| : : : : |", "| | : | : |", "|Y| : |B: |", "+---------+"]
TAXI_LOCS = [(0, 0), (0, 4), (4, 0), (4, 3)]


def taxi_tables():
    """(obs[500][6], start[500]) as TaxiEnv::new builds them (taxi.rs:57-121)"""
    start, obs, total = [0.0] * 500, [None] * 500, 0.0
    for row in range(5):
        for col in range(5):
            for pas in range(5):
                for dest in range(4):
                    state = ((row * 5 + col) * 5 + pas) * 4 + dest
                    if pas < 4 and pas != dest:
                        start[state] += 1.0
                        total += 1.0
                    li = []
                    for a in range(6):
                        nr, nc, npas, reward, term = row, col, pas, -1.0, False
                        if a == 0:
                            nr = min(row + 1, 4)
                        elif a == 1:
                            nr = max(row - 1, 0)
                        if a == 2 and TAXI_MAP[1 + row][2 * col + 2] == ":":
                            nc = min(col + 1, 4)
                        elif a == 3 and TAXI_MAP[1 + row][2 * col] == ":":
                            nc = max(col - 1, 0)
                        elif a == 4:
                            if pas < 4 and (row, col) == TAXI_LOCS[pas]:
                                npas = 4
                            else:
                                reward = -10.0
                        elif a == 5:
                            if (row, col) == TAXI_LOCS[dest] and pas == 4:
                                npas, term, reward = dest, True, 20.0
                            else:
                                reward = -10.0
                        li.append((((nr * 5 + nc) * 5 + npas) * 4 + dest, reward, term))
                    obs[state] = li
    return obs, [v / total for v in start]


class Taxi(TableEnv):
    _tables = None

    def __init__(self, max_steps):
        super().__init__(max_steps)
        if Taxi._tables is None:
            Taxi._tables = taxi_tables()
        self.obs, self.start = Taxi._tables

    def reset(self, rng):
        self.pos = fp.categorical_sample(self.start, rng.uniform01())
        self.ready, self.curr_step = True, 0
        return self.pos


def bj_index(p, d, ace):
    return (p * 32 + d) * 2 + int(ace)


class Blackjack:
    """src/env/blackjack.rs.  The hands are kept as card sums (the reference sums its
    16-slot arrays); a score counts an ace as 11 while that stays within 21."""

    def __init__(self, rng):
        self.n_trunc = 0
        self.reset(rng)                 # BlackJackEnv::new deals a hand (:45-58); nobody looks at it
        self.ready = False

    @staticmethod
    def score(total, ace):
        return total + 10 if ace and total + 10 <= 21 else total

    def reset(self, rng):
        src = CardSource(rng)
        p0, p1, d0, d1 = src.card(), src.card(), src.card(), src.card()
        self.player, self.dealer, self.dealer0 = p0 + p1, d0 + d1, d0
        self.p_ace, self.d_ace = p0 == 1 or p1 == 1, d0 == 1 or d1 == 1
        self.ready = True
        return bj_index(self.score(self.player, self.p_ace), self.dealer0, self.p_ace)

    def step(self, a, rng):
        if not self.ready:
            raise RuntimeError("EnvNotReady")
        src = CardSource(rng)
        if a == 0:
            self.player += src.card()
            p = self.score(self.player, self.p_ace)
            if p > 21:
                self.ready = False
                return bj_index(p, self.score(self.dealer, self.d_ace), self.p_ace), -1.0, True
            return bj_index(p, self.dealer0, self.p_ace), 0.0, False
        self.ready = False
        d = self.score(self.dealer, self.d_ace)
        while d < 17:
            self.dealer += src.card()
            d = self.score(self.dealer, self.d_ace)
        p = self.score(self.player, self.p_ace)
        s = bj_index(p, d, self.p_ace)
        if d > 21:
            return s, 1.0, True
        return s, (1.0 if p > d else (-1.0 if p < d else 0.0)), True


class _Lake:
    """maps_model's env with the truncation count under the common name"""

    def __init__(self, env):
        self.env = env

    def reset(self, rng):
        return self.env.reset(rng)

    def step(self, a, rng):
        return self.env.step(a, rng)

    @property
    def n_trunc(self):
        return self.env.seen["trunc"]


def make_env(env, map8x8=0, slippery=0, max_steps=100):
    """env: the configuration's name.  (S, A, a constructor of one lane's env from the
    lane's stream: Blackjack's draws from it)"""
    if env in ("frozen_lake", "frozen_lake_edited"):
        rows = fp.MAP8 if map8x8 else fp.MAP4
        return len(rows) ** 2, 4, lambda rng: _Lake(mm.make_env(env, rows, slippery, max_steps))
    if env == "cliff_walking":
        return 48, 4, lambda rng: CliffWalking(max_steps)
    if env == "taxi":
        return 500, 6, lambda rng: Taxi(max_steps)
    if env == "blackjack":
        return 2048, 2, Blackjack
    raise ValueError(env)


# ---------------------------------------------------------------- selection
def argmax_first(row):
    """(index of the first maximum, strict `>` from element 0; whether an element
    after it equals it: a tie the rule broke)"""
    m, at = row[0], 0
    for i, v in enumerate(row):
        if v > m:
            m, at = v, i
    return at, any(v == m for v in row[at + 1:])


def argmax_last(row):
    """the mutation: `>=` takes the last of equal maxima"""
    m, at = row[0], 0
    for i, v in enumerate(row):
        if v >= m:
            m, at = v, i
    return at


def policy_values(view, s, alpha_only=False):
    """policy.predict(s): what the selector sees.  The fixed point gives its raw words
    (single table; comparing them is comparing the values)."""
    if view.P == 2:
        if alpha_only:
            return view.row(0, s)
        return [(x + y) / 2.0 for x, y in zip(view.row(0, s), view.row(1, s))]
    return view.row(0, s) if view.f64 else view.raw_row(0, s)


def ucb_scores(values, counts, lnt, c):
    return [v + c * sm.ieee_sqrt(sm.ieee_div(lnt, float(n) + sm.MIN_POSITIVE)) for v, n in zip(values, counts)]


class _Lane:
    __slots__ = ("rng", "env", "need_reset", "s", "a", "greedy_a2")


class Predictor:
    """the lanes of one agent; step_model.replay_launch(predictor=...) calls fill()
    once per group and step, in step order within a group.  stats is the model's own
    bookkeeping for the liveness conditions."""

    def __init__(self, *, env, n_lanes, seed, lane_offset=0, map8x8=0, slippery=0, max_steps=100, ucb=False,
                 ucb_c=0.5, reset_step=False, eps_decay=0.0, eps_final=0.0, decay_kind=0, mutation=None):
        if mutation is not None and mutation not in MUTATIONS:
            raise ValueError(mutation)
        self.S, self.A, make = make_env(env, map8x8, slippery, max_steps)
        self.ucb, self.ucb_c = bool(ucb), float(ucb_c)
        self.reset_step = bool(reset_step) and not self.ucb
        self.eps_decay, self.eps_final, self.decay_kind = float(eps_decay), float(eps_final), decay_kind
        self.mutation = mutation
        self.lanes = []
        for j in range(n_lanes):
            ln = _Lane()
            ln.rng = Stream(seed, lane_offset + j)
            ln.env = make(ln.rng)
            ln.need_reset, ln.s, ln.a, ln.greedy_a2 = True, 0, 0, False
            self.lanes.append(ln)
        self.stats = dict.fromkeys(("explore", "greedy", "eps_zero", "value_reads", "winner_ge_1", "ties_broken",
                                    "after_row_moved", "resets", "terminal", "truncated", "nan_at_0"), 0)

    # -- bookkeeping that needs every lane
    def totals(self):
        out = dict(self.stats)
        out["rejected_halves"] = sum(ln.rng.rejected_halves for ln in self.lanes)
        return out

    def _read(self, view, s, row):
        """a value-reading selection of row s took `row`'s first maximum"""
        at, tie = argmax_first(row)
        st = self.stats
        st["value_reads"] += 1
        st["winner_ge_1"] += at >= 1
        st["ties_broken"] += tie
        st["after_row_moved"] += view.moved(s)
        st["nan_at_0"] += row[0] != row[0]
        return argmax_last(row) if self.mutation == "tie_last" else at

    def select(self, ln, view, s, eps, step_inc):
        if self.ucb:
            counts = view.counts(s)
            if self.mutation == "counters_incremented":
                counts = [n + step_inc.get(s * self.A + i, 0) for i, n in enumerate(counts)]
            vals = policy_values(view, s, self.mutation == "alpha_only")
            if not view.f64:
                vals = [float(w) * 2.0 ** -sm.FIX_SHIFT for w in vals]
            a = self._read(view, s, ucb_scores(vals, counts, view.ln_t(), self.ucb_c))
            step_inc[s * self.A + a] = step_inc.get(s * self.A + a, 0) + 1
            return a, False
        if eps == 0.0:                          # no draw; counted apart from the tested greedy ones
            self.stats["eps_zero"] += 1
        elif ln.rng.eps_test(eps):
            self.stats["explore"] += 1
            return ln.rng.uniform_usize(self.A), False
        else:
            self.stats["greedy"] += 1
        return self._read(view, s, policy_values(view, s, self.mutation == "alpha_only")), True

    def _decayed(self, eps):
        nw = eps * self.eps_decay if self.decay_kind == 1 else eps - self.eps_decay
        return eps if self.eps_final > nw else nw

    def fill(self, recs, k, lane0, lane1, view):
        step_inc = {}                          # the mutation's view of this step's earlier selections
        for j in range(lane0, lane1):
            ln, eps = self.lanes[j], view.eps[j]
            ln.greedy_a2 = False
            kind = sm.KIND_STEP
            if ln.need_reset:
                ln.s = ln.env.reset(ln.rng)
                ln.a, _ = self.select(ln, view, ln.s, eps, step_inc)
                ln.need_reset = False
                self.stats["resets"] += 1
                if not self.reset_step:
                    recs[j] = dict(kind=sm.KIND_RESET, mode=sm.MODE_TRAIN, s=ln.s, a=ln.a, s2=0, a2=0, r=0.0,
                                   term=0, td=0.0)
                    continue
                kind = sm.KIND_RESET_STEP
            before = ln.env.n_trunc
            s2, r, term = ln.env.step(ln.a, ln.rng)
            if ln.env.n_trunc != before:
                self.stats["truncated"] += 1
            elif term:
                self.stats["terminal"] += 1
            if term and self.mutation == "eps_post_decay":
                eps = self._decayed(eps)
            a2, ln.greedy_a2 = self.select(ln, view, s2, eps, step_inc)
            recs[j] = dict(kind=kind, mode=sm.MODE_TRAIN, s=ln.s, a=ln.a, s2=s2, a2=a2, r=r, term=int(term),
                           td=0.0)
            ln.s, ln.a, ln.need_reset = s2, a2, bool(term)

    def after_step(self, recs, k, lane0, lane1, view):
        if self.mutation != "end_snapshot":
            return
        for j in range(lane0, lane1):
            ln = self.lanes[j]
            if ln.greedy_a2:
                at, _ = argmax_first(policy_values(view, recs[j]["s2"]))
                recs[j]["a2"] = ln.a = at


# ---------------------------------------------------------------- the launch
def _same(field, a, b):
    if field in ("r", "td"):
        a, b = float(a), float(b)
        return (a != a and b != b) or sm.f64_bits(a) == sm.f64_bits(b)
    return int(a) == int(b)


def compare_records(predicted, recorded):
    """[(step, lane, field, predicted, recorded)]: every lane's FIRST differing
    record only (all its differing fields); what follows a difference is noise"""
    out = []
    K = len(predicted)
    for j in range(len(predicted[0]) if K else 0):
        for k in range(K):
            bad = [(k, j, f, predicted[k][j][f], recorded[k][j][f]) for f in FIELDS
                   if not _same(f, predicted[k][j][f], recorded[k][j][f])]
            if bad:
                out += bad
                break
    return out


def predict_launch(predictor, q_base, n_base, t_base, K, recorded=None, **kw):
    """One launch of K steps predicted from the state before it.  kw: step_model.
    replay_launch's (G, P, S, A, lr, gamma, algo, repr, eps, flags, traces, ...).
    Returns (the Replay on the predicted records, the predicted records
    [K][n_lanes] as dicts, the mismatches against `recorded` (None: [])).
    A lane that has differed once is NOT re-synchronised: later launches of a
    Predictor continue the predicted trajectory."""
    L = len(predictor.lanes)
    grid = [[None] * L for _ in range(K)]
    rep = sm.replay_launch(q_base, n_base, t_base, grid, predictor=predictor, ucb=predictor.ucb,
                           ucb_c=predictor.ucb_c, eps_decay=predictor.eps_decay, eps_final=predictor.eps_final,
                           decay_kind=predictor.decay_kind, **kw)
    if recorded is None:
        return rep, grid, []
    if len(recorded) != K or any(len(step) != L for step in recorded):
        raise ValueError("recorded must be [K][n_lanes]")
    return rep, grid, compare_records(grid, recorded)

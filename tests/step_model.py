"""An exact replay model of one shared-mode launch (group_size >= 2).

TEST INFRASTRUCTURE ONLY.  This is a third statement of the shared-Q contract,
written from DESIGN.md section 2 ("Step combine", "Traces", "Merge", "Fixed
point", "UCB"), the include/rl.h comment on rl_q_repr and the reference's
sources it cites.  It uses neither the CPU oracle nor the library: no ctypes, no
RNG, no env.  Everything it needs is in the data both sides already expose:

  - the raw words of Q_base and the UCB counters N / t before the launch;
  - the launch's rl_step_record entries as records[K][n_lanes]
    (fields s, a, r, s2, a2, term, mode, kind, td);
  - the per-lane epsilon before the first launch (epsilon()), carried by the
    model from then on;
  - ln(t) of the side under test as a callable (see "ln" below).

From those it predicts the raw words of Q_base, N / t and every lane's epsilon
after the launch, bit for bit.  Arithmetic is Python int and fractions.Fraction
where the contract says "exact", and CPython floats (IEEE binary64, correctly
rounded float(int), a * b, a + b, a / b, sqrt, no fused multiply-add) where the
contract names a rounded operation.

What the model restates
-----------------------
Per learner group g (lanes [g*G, (g+1)*G), the last group possibly ragged),
starting from Q_base, for each of the K synchronous steps:

  * every record with mode == TRAIN and kind in {2 STEP, 3 RESET+STEP} is one
    update.  Its TD error is recomputed from the group's step-start snapshot in
    the reference's operation order (src/agent.rs:19-45,
    src/agent/one_step_agent.rs:62-72):
        td = (r + gamma * next) - V[s][a]
    with next = V[s2][a2] (SARSA), the first maximum of V[s2][:] found with a
    strict `>` from element 0 (Q-learning, src/utils.rs:13-21), or expected
    SARSA's f = 0.0; f += p[i] * V[s2][i] in index order with
      - eps-greedy (uniform_epsilon_greed.rs:72-76): p[i] = eps / A, then
        p[argmax V[s2]] = 1 - eps, eps the LANE's epsilon at this update, before
        the decay the update may trigger (:42-49, on `term`);
      - UCB (upper_confidence_bound.rs:48-63): u_i = V[s2][i] + c * sqrt(ln(t) /
        (n_i + 2^-1022)), sum accumulated from 0.0 in order, p_i = u_i / sum,
        with n and t the GROUP's counters: N_base / t_base plus the group's own
        increments up to and including this step's selections.
    Division and square root are IEEE (x / 0, inf / inf, sqrt(nan) give inf /
    NaN, not an exception), so the NaN regime from fresh counters is
    replayed, not refused.  V is the value table; for the double policy V and
    the updated table alternate per update (double_tabular_policy.rs:41-67:
    flag true reads alpha = table 0 and writes beta = table 1).  The recomputed
    td must equal the recorded one bit for bit (NaN as NaN); differences are
    returned in Replay.td_mismatches.  td_source="record" takes the recorded td
    as the input instead (the hand-worked combine tests inject tds this way).
  * one-step agent: the contribution is d = lr * td to entry (update table, s, a).
  * f64: the n contributions an entry received in the step move it by their
    mean, summed exactly on the grid of the largest: with `code` the largest
    biased exponent among them, e = max(code, 1) - 1075, every d is rounded
    half-to-even to an integer number of 2^e, the integers are added, and the
    entry moves by ldexp(fl(float(sum) * fl(1.0 / n)), e).  A NaN / +inf / -inf
    contribution switches the move to the IEEE sum of the kinds present (NaN
    for +inf with -inf).  NaN is stored canonical (0x7FF8000000000000).
  * fixed40: every d becomes rint(d * 2^40) (an exact int here) and the entry
    moves by trunc(float(sum) * (1.0 / n)).  The fixed point exists only where
    the host proved |Q| <= 2048 and every contribution finite; a non-finite or
    out-of-range value is outside the written contract and the model raises.

Eligibility traces (f64 only; elegibility_traces_agent.rs:61-104)
------------------------------------------------------------------
Each lane keeps a sparse E[s][a] over the states it visited this episode (the
reference's FxHashMap of rows), carried across launches like the flags, empty at
creation, after reset() and after a `term` update.  An update computes td as
above, adds 1.0 to E[s][a], and then EVERY action b of EVERY visited state o
contributes d = lr * (td * E[o][b]) to entry (update table, o, b), also where
E is 0 (d = +-0, or NaN for a non-finite td); E[o][b] *= fl(gamma * lambda).
Per group step there is ONE grid: code = the largest biased exponent over the
FINITE tds of the group's updates (0 if none), e = max(code, 1) - 1075 +
trace_k.  Every finite d is rounded half-to-even onto 2^e; the model raises if
a rounded value reaches 2^51 (the one-add conversion's premise).  An entry's n
is the number of (lane, visited state) pairs that covered its row, whatever
their values, and the entry moves by ldexp(fl(float(sum) * fl(1.0 / n)), e).
trace_k is trace_grid_k() below, DESIGN section 2 restated.

Merge: an entry takes the mean over the groups whose final word differs
BITWISE from Q_base's (so -0.0 against +0.0 is a change, and a group that moves
an entry and brings it back to the same bits did not change it).  f64: the mean
of those groups' VALUES on the grid e = max(code, 1) - 1075 + h of the largest
changed finite value, h = max(0, ceil(log2(merge_groups)) - 10) headroom bits
(also when one group changed the entry); non-finite values give the IEEE sum of
their kinds.  fixed40: Q_base += trunc(float(sum of differences) * (1.0 / n)).
UCB: N[s][a] += 1 for every selection (kind 1: the (s, a) of the reset; kind 2:
(s2, a2)), t += 1 per selection; every group starts from the base and the
launch's totals are the sums over all groups.

Per-lane state the caller carries
---------------------------------
rl_agent_lane_state documents `flags|a|mode` without naming the bits, so the
double-policy flag is NOT read from there.  Every lane starts with the flag
true at rl_agent_create (DoubleTabularPolicy::new) and it flips once per
update.  `replay_launch` takes flags, eps and traces before the launch and
returns them after it (Replay.flags / .eps / .traces, and .last_eps for one
coverage condition); the caller passes them to the next launch.

ln
--
ln(t) is the one value the model cannot form: the project's log is an fdlibm
sequence, not libm's.  `ln` is a callable int -> float supplied by the caller
from the side under test; the tests check every value used against a 50-digit
decimal logarithm (within 1 ulp), which makes it a checked scalar input.

Records as the input, or predicted
----------------------------------
By itself this file takes (kind, s, a, s2, a2, r, term) from the records.
tests/select_model.py closes the loop: its Predictor (replay_launch's
`predictor`) produces every record of a group's step from the seed, the lanes'
envs and the group's step-start snapshot (SnapshotView below), and the combine,
the merge and the counters here then run on the predicted records.  What is
pinned then: the stream and its mappings, the envs, the selections, the
schedule, td, Q words, N, t and epsilon.  Record-driven replay and
td_source="record" stay as they were.

Outside the model
-----------------
ln(t) (a checked input); the train() evaluate interleave (plain run() launches
in RL_MODE_TRAIN only); populations.  Private mode (group_size 1), Dyna-Q
planning and the neural policy are outside THIS model and have one of their own:
tests/private_model.py predicts a private lane from the seed the same way.
Without a predictor also the RNG, the envs and the selections themselves
(records are the input).
"""
import math
import struct
from fractions import Fraction

MODE_TRAIN = 0
KIND_IDLE, KIND_RESET, KIND_STEP, KIND_RESET_STEP = 0, 1, 2, 3
QNAN_BITS = 0x7FF8000000000000
NF_NAN, NF_PINF, NF_NINF = 1, 2, 4
FIX_SHIFT = 40
FIX_LIMIT = 1 << 51          # |Q| <= 2048 in units of 2^-40
TRACE_RAW_LIMIT = 1 << 51    # the one-add conversion (y + 1.5 * 2^52) is exact below this
MIN_POSITIVE = 2.0 ** -1022
_M64 = (1 << 64) - 1
_INF = float("inf")
_NAN = float("nan")


# ---------------------------------------------------------------- bit patterns
def f64_bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def f64_from_bits(u):
    return struct.unpack("<d", struct.pack("<Q", u & _M64))[0]


def canonical(x):
    return f64_from_bits(QNAN_BITS) if x != x else x


def f64_word(x):
    """the int64 raw word of an f64 entry (NaN canonical)"""
    u = f64_bits(canonical(x))
    return u - (1 << 64) if u >> 63 else u


def biased_exponent(x):
    """0 for zero / subnormal, 2047 for inf / NaN"""
    return (f64_bits(x) >> 52) & 0x7FF


def nf_kind(x):
    return NF_NAN if x != x else (NF_PINF if x > 0.0 else NF_NINF)


def nf_value(kinds):
    """the IEEE sum of values of these non-finite kinds"""
    if kinds & NF_NAN or (kinds & NF_PINF and kinds & NF_NINF):
        return f64_from_bits(QNAN_BITS)
    return _INF if kinds & NF_PINF else -_INF


def _finite(x):
    return x == x and x not in (_INF, -_INF)


def grid_exponent(code):
    return max(code, 1) - 1075


def headroom(merge_groups):
    """ceil(log2(groups)) - 10 bits, never negative"""
    return max(0, (max(int(merge_groups), 1) - 1).bit_length() - 10)


def _pow2(e):
    return Fraction(1 << e) if e >= 0 else Fraction(1, 1 << -e)


def on_grid_exact(x, e):
    """(x / 2^e rounded half-to-even as an exact int, whether x was a multiple of
    2^e).  Integers only: x = m * 2^q with m the 53-bit integer mantissa."""
    fr, ex = math.frexp(x)
    m = int(fr * 9007199254740992.0)          # fr * 2^53 is an integer, exactly
    sh = ex - 53 - e
    if sh >= 0:
        return m << sh, True
    s = -sh
    q = m >> s                                # floor, also for negative m
    rem = m - (q << s)                        # 0 <= rem < 2^s
    half = 1 << (s - 1)
    if rem > half or (rem == half and q & 1):
        q += 1
    return q, rem == 0


def on_grid(x, e):
    """x / 2^e rounded half-to-even, as an exact int"""
    return on_grid_exact(x, e)[0]


def _ldexp(m, e):
    try:
        return math.ldexp(m, e)
    except OverflowError:
        return math.copysign(_INF, m)


def grid_mean(total, n, e):
    return _ldexp(float(total) * (1.0 / n), e)


# ---------------------------------------------------------------- IEEE helpers
def ieee_div(a, b):
    """a / b as IEEE 754 defines it where Python raises"""
    if b == 0.0:
        if a != a or a == 0.0:
            return _NAN
        return math.copysign(_INF, a) * math.copysign(1.0, b)
    return a / b


def ieee_sqrt(x):
    if x != x or x < 0.0:
        return _NAN
    if x == _INF:
        return _INF
    return math.sqrt(x)               # sqrt(-0.0) is -0.0


def trace_grid_k(lr, gamma, lam, max_steps, blackjack):
    """DESIGN section 2 "Traces": the exponent k with 2^k > 4 * |lr| * Ebound * margin"""
    a = abs(float(gamma) * float(lam))
    if a < 1.0:
        eb = 1.0 / (1.0 - a)
    else:
        n = 33 if blackjack else int(max_steps) + 2        # terms of the geometric sum
        if a == 1.0:
            eb = float(n)
        else:
            try:
                eb = math.expm1(float(n) * math.log1p(a - 1.0)) / (a - 1.0)
            except OverflowError:
                eb = _INF
    x = abs(float(lr)) * eb * (1.0 + 2.0 ** -50) * 1.0001
    if not x > 0.0:
        return 0
    if not x < _INF:
        return 1100
    return max(-1100, min(1100, math.frexp(x)[1] + 2))


# ---------------------------------------------------------------- events
class StepEvent:
    """one entry in one group step: its contributions and the move taken.
    f64: ds / move in value units, e the grid exponent (None if a contribution
    was non-finite).  fixed40: ds in value units, move an int of 2^-40.
    traces: Es the trace value behind every d, td_big the largest finite |td| of
    the group step, inexact whether some d was no multiple of the grid."""
    __slots__ = ("group", "step", "entry", "ds", "kinds", "e", "move", "before", "after", "Es", "td_big",
                 "inexact")

    def __init__(self, group, step, entry, ds, kinds, e, move, before, after, Es=None, td_big=None,
                 inexact=False):
        self.group, self.step, self.entry = group, step, entry
        self.ds, self.kinds, self.e, self.move = ds, kinds, e, move
        self.before, self.after = before, after          # the entry's value / fixed-point word
        self.Es, self.td_big, self.inexact = Es, td_big, inexact


class MergeEvent:
    """one entry at the merge: base word, the final word of every group that
    received a contribution to it (touched), those that differ bitwise from the
    base (changed), and the merged word"""
    __slots__ = ("entry", "base", "touched", "changed", "e", "merged")

    def __init__(self, entry, base, touched, changed, e, merged):
        self.entry, self.base, self.touched = entry, base, touched
        self.changed, self.e, self.merged = changed, e, merged


class Replay:
    __slots__ = ("words", "n", "t", "flags", "eps", "traces", "td_mismatches", "steps", "merges", "repr",
                 "merge_groups", "n_groups", "agent", "trace_k", "max_raw_bits", "seen", "ln_used", "last_eps")


class LaneTrace:
    """a lane's eligibility trace: rows[s] = [E[s][0..A)] for the states visited
    this episode, in first-visit order; last = the pairs taken in the episode
    that the latest `term` cleared (coverage only)"""
    __slots__ = ("rows", "last", "taken")

    def __init__(self):
        self.rows, self.last, self.taken = {}, set(), set()


class SnapshotView:
    """what a selection may read of its group at the start of a step: the group's
    current values and raw words (Q_base where the group has not moved an entry),
    the group's counters N / t as incremented by its earlier steps, ln(t) and the
    lanes' epsilon.  The dicts are replay_launch's own: they move when the step's
    updates are applied, after every selection of the step."""

    def __init__(self, P, S, A, f64, base, base_val, raw, val, n_base, n_inc, eps, ln_used, ln):
        self.P, self.S, self.A, self.f64 = P, S, A, f64
        self._base, self._base_val, self._raw, self._val = base, base_val, raw, val
        self._n_base, self._n_inc, self.eps, self._ln_used, self._ln = n_base, n_inc, eps, ln_used, ln
        self.t = 0

    def row(self, tbl, s):
        i0 = (tbl * self.S + s) * self.A
        return [self._val[i] if i in self._val else self._base_val[i] for i in range(i0, i0 + self.A)]

    def raw_row(self, tbl, s):
        i0 = (tbl * self.S + s) * self.A
        return [self._raw[i] if i in self._raw else self._base[i] for i in range(i0, i0 + self.A)]

    def counts(self, s):
        return [self._n_base[s * self.A + i] + self._n_inc.get(s * self.A + i, 0) for i in range(self.A)]

    def ln_t(self):
        if self.t not in self._ln_used:
            self._ln_used[self.t] = float(self._ln(self.t))
        return self._ln_used[self.t]

    def moved(self, s):
        """whether the group holds an entry of row s (either table) that differs from Q_base's"""
        for tbl in range(self.P):
            i0 = (tbl * self.S + s) * self.A
            for i in range(i0, i0 + self.A):
                if i in self._raw and self._raw[i] != self._base[i]:
                    return True
        return False


# ---------------------------------------------------------------- the model
def _first_max(row):
    m = row[0]
    for v in row:
        if v > m:
            m = v
    return m


def _argmax(row):
    """utils.rs:1-11: a NaN at element 0 stays the maximum, a NaN elsewhere never wins"""
    m, at = row[0], 0
    for i, v in enumerate(row):
        if v > m:
            m, at = v, i
    return at


def _same_f64(a, b):
    return (a != a and b != b) or f64_bits(a) == f64_bits(b)


def expected_eps_greedy(row2, eps):
    A = len(row2)
    p = [eps / float(A)] * A
    p[_argmax(row2)] = 1.0 - eps
    f = 0.0
    for i in range(A):
        f += p[i] * row2[i]
    return f


def expected_ucb(row2, counts, lnt, c):
    u, total = [], 0.0
    for q, n in zip(row2, counts):
        ui = q + c * ieee_sqrt(ieee_div(lnt, float(n) + MIN_POSITIVE))
        u.append(ui)
        total += ui
    f = 0.0
    for ui, q in zip(u, row2):
        f += ieee_div(ui, total) * q
    return f


def replay_launch(q_base, n_base, t_base, records, *, G, P, S, A, lr, gamma, algo, repr,
                  merge_groups=0, ucb=False, flags=None, agent="one_step", td_source="model",
                  eps=None, eps_decay=0.0, eps_final=0.0, decay_kind=0, ucb_c=0.5, ln=None,
                  lam=0.0, max_steps=0, blackjack=False, traces=None, last_eps=None, predictor=None):
    """Predict Q_base's raw words, N / t and the lanes' epsilon after one launch.

    q_base: P*S*A int64 raw words ([P][S][A] order); n_base: S*A counts; t_base: int;
    records: [K][n_lanes] of rl_step_record (anything indexable by field name);
    algo: "sarsa" | "qlearning" | "expected_sarsa"; repr: "f64" | "fixed40";
    agent: "one_step" | "traces"; td_source: "model" (recompute, report
    td_mismatches) | "record" (the recorded td is the input);
    merge_groups: learner groups over every rank (0: this launch's own);
    ucb: the selector is UCB (N / t move, ucb_c, ln(t) from the callable `ln`);
    eps / eps_decay / eps_final / decay_kind: the eps-greedy selector's per-lane
    epsilon before the launch and its decay (None: 0.0, for records without `term`);
    lam / max_steps / blackjack: what the traces grid needs;
    flags / traces: per-lane double-policy flag and LaneTrace before the launch
    (None: the state at creation); last_eps: the epsilon of every lane's latest
    expected-SARSA update (None where it made none; coverage only).
    predictor: None (records are the input), or tests/select_model.py's Predictor.
    Then `records` is a [K][n_lanes] grid of None that the predictor fills group by
    group and step by step from the group's step-start snapshot (a SnapshotView),
    and every STEP record receives the td computed here.
    """
    if agent not in ("one_step", "traces"):
        raise ValueError(f"unknown agent {agent!r}")
    if algo not in ("sarsa", "qlearning", "expected_sarsa"):
        raise ValueError(f"unknown algo {algo!r}")
    if repr not in ("f64", "fixed40"):
        raise ValueError(f"unknown representation {repr!r}")
    if td_source not in ("model", "record"):
        raise ValueError(f"unknown td_source {td_source!r}")
    if predictor is not None and td_source != "model":
        raise ValueError("predicted records carry no td: a predictor needs td_source=\"model\"")
    if P not in (1, 2) or G < 2 or G > 1024:
        raise ValueError("shared mode: P in {1, 2}, 2 <= group_size <= 1024")
    if repr == "fixed40" and (P != 1 or agent != "one_step"):
        raise ValueError("the fixed point holds single tables of the one-step agent only")
    lr, gamma, lam, ucb_c = float(lr), float(gamma), float(lam), float(ucb_c)
    f64 = repr == "f64"
    tr = agent == "traces"
    es = algo == "expected_sarsa" and td_source == "model"
    nq = P * S * A
    base = [int(w) for w in q_base]
    if len(base) != nq:
        raise ValueError("q_base must hold P*S*A words")
    K = len(records)
    L = len(records[0]) if K else 0
    n_groups = (L + G - 1) // G
    total_groups = int(merge_groups) if merge_groups else n_groups
    h = headroom(total_groups)
    flags = [True] * L if flags is None else [bool(f) for f in flags]
    eps = [0.0] * L if eps is None else [float(x) for x in eps]
    traces = [LaneTrace() for _ in range(L)] if traces is None else list(traces)
    if len(flags) != L or len(eps) != L or len(traces) != L:
        raise ValueError("flags / eps / traces hold one value per lane")
    gl = gamma * lam
    trace_k = trace_grid_k(lr, gamma, lam, max_steps, blackjack) if tr else 0

    if f64:
        base_val = [f64_from_bits(w) for w in base]
    else:
        for w in base:
            if abs(w) > FIX_LIMIT:
                raise ValueError("fixed-point word outside |Q| <= 2048")
        base_val = [float(w) * 2.0 ** -FIX_SHIFT for w in base]

    out = Replay()
    out.repr, out.merge_groups, out.n_groups = repr, total_groups, n_groups
    out.agent, out.trace_k, out.max_raw_bits = agent, trace_k, 0
    out.td_mismatches, out.steps, out.merges = [], [], []
    out.seen, out.ln_used = set(), {}
    n_base = [int(v) for v in n_base]
    n_after = list(n_base)
    t_after = int(t_base)
    finals = []                      # per group: {entry: final word}
    last_eps = [None] * L if last_eps is None else list(last_eps)

    for g in range(n_groups):
        lane0, lane1 = g * G, min(L, (g + 1) * G)
        raw = {}                     # entry -> current word of this group (touched entries)
        val = {}                     # entry -> current value
        n_inc, t_inc = {}, 0         # this group's own counter increments so far

        def V(tbl, s, a):
            i = (tbl * S + s) * A + a
            return val[i] if i in val else base_val[i]

        view = None
        if predictor is not None:
            view = SnapshotView(P, S, A, f64, base, base_val, raw, val, n_base, n_inc, eps, out.ln_used, ln)
        for k in range(K):
            if predictor is not None:
                view.t = int(t_base) + t_inc
                predictor.fill(records[k], k, lane0, lane1, view)
            # every selection of the step moves the counters before any update reads them
            step_inc = set()
            if ucb:
                for j in range(lane0, lane1):
                    rec = records[k][j]
                    kind = int(rec["kind"])
                    if kind == KIND_IDLE:
                        continue
                    if kind == KIND_RESET_STEP:
                        raise ValueError("the reset-and-step schedule does not exist with UCB")
                    sel = (int(rec["s"]), int(rec["a"])) if kind == KIND_RESET else \
                          (int(rec["s2"]), int(rec["a2"]))
                    i = sel[0] * A + sel[1]
                    n_inc[i] = n_inc.get(i, 0) + 1
                    t_inc += 1
                    step_inc.add(sel[0])
            contrib = {}             # entry -> [d]
            contrib_E = {}           # entry -> [E] (traces)
            rows = {}                # (table, state) -> lanes that covered the row (traces)
            td_code, td_big = 0, 0.0
            for j in range(lane0, lane1):
                rec = records[k][j]
                kind = int(rec["kind"])
                if int(rec["mode"]) != MODE_TRAIN or kind not in (KIND_STEP, KIND_RESET_STEP):
                    continue
                s, a, s2, a2 = int(rec["s"]), int(rec["a"]), int(rec["s2"]), int(rec["a2"])
                r = float(rec["r"])
                td_rec = float(rec["td"]) if predictor is None else None
                vt, ut = ((0, 1) if flags[j] else (1, 0)) if P == 2 else (0, 0)
                if td_source == "record":
                    td = td_rec
                else:
                    row2 = [V(vt, s2, i) for i in range(A)]
                    if algo == "sarsa":
                        nxt = row2[a2]
                    elif algo == "qlearning":
                        nxt = _first_max(row2)
                    elif ucb:
                        t_now = int(t_base) + t_inc
                        if t_now not in out.ln_used:
                            out.ln_used[t_now] = float(ln(t_now))
                        counts = [n_base[s2 * A + i] + n_inc.get(s2 * A + i, 0) for i in range(A)]
                        nxt = expected_ucb(row2, counts, out.ln_used[t_now], ucb_c)
                        if s2 in step_inc:
                            out.seen.add("es_counts_moved_in_step")
                    else:
                        nxt = expected_eps_greedy(row2, eps[j])
                        if last_eps[j] is not None and last_eps[j] != eps[j]:
                            out.seen.add("es_eps_decayed_between_updates")
                        last_eps[j] = eps[j]
                    if es and not all(_finite(v) for v in row2):
                        out.seen.add("es_nan_shortcut")
                    td = r + gamma * nxt - V(vt, s, a)
                    if predictor is not None:
                        rec["td"] = td
                    elif not _same_f64(td, td_rec):
                        out.td_mismatches.append((g, k, j, td, td_rec))
                if not tr:
                    contrib.setdefault((ut * S + s) * A + a, []).append(lr * td)
                else:
                    if _finite(td):
                        td_code = max(td_code, biased_exponent(td))
                        td_big = max(td_big, abs(td))
                    lt = traces[j]
                    row = lt.rows.setdefault(s, [0.0] * A)
                    if row[a] != 0.0:
                        out.seen.add("E_ge_2")
                    if (s, a) in lt.last:
                        out.seen.add("cleared_then_revisited")
                    lt.taken.add((s, a))
                    row[a] += 1.0
                    for o, ev in lt.rows.items():
                        rows[(ut, o)] = rows.get((ut, o), 0) + 1
                        for b in range(A):
                            i = (ut * S + o) * A + b
                            contrib.setdefault(i, []).append(lr * (td * ev[b]))
                            contrib_E.setdefault(i, []).append(ev[b])
                            ev[b] *= gl
                    if int(rec["term"]):
                        lt.rows, lt.last, lt.taken = {}, lt.taken, set()
                if P == 2:
                    flags[j] = not flags[j]
                if not ucb and int(rec["term"]):
                    nw = eps[j] * eps_decay if decay_kind == 1 else eps[j] - eps_decay
                    if not eps_final > nw:
                        eps[j] = nw
            # every lane read the step-start snapshot; now the entries move
            e_tr = grid_exponent(td_code) + trace_k
            for i, ds in contrib.items():
                n = len(ds)
                inexact = False
                if tr and n != rows[(i // A // S, i // A % S)]:
                    raise AssertionError("an entry's contributions are not one per covering (lane, state)")
                if f64:
                    kinds = 0
                    code = 0
                    for d in ds:
                        if not _finite(d):
                            kinds |= nf_kind(d)
                        else:
                            code = max(code, biased_exponent(d))
                    if kinds:
                        e, move = None, nf_value(kinds)
                    elif tr:
                        e, total = e_tr, 0
                        for d in ds:
                            x, exact = on_grid_exact(d, e)
                            if abs(x) >= TRACE_RAW_LIMIT:
                                raise ValueError(f"traces: a contribution is {abs(x).bit_length()} bits on the "
                                                 "step grid, the one-add conversion needs |raw| < 2^51")
                            out.max_raw_bits = max(out.max_raw_bits, abs(x).bit_length())
                            inexact = inexact or not exact
                            total += x
                        move = grid_mean(total, n, e)
                    else:
                        e = grid_exponent(code)
                        move = grid_mean(sum(on_grid(d, e) for d in ds), n, e)
                    old = val[i] if i in val else base_val[i]
                    new = canonical(old + move)
                    val[i] = new
                    raw[i] = f64_word(new)
                else:
                    total = 0
                    for d in ds:
                        if not _finite(d):
                            raise ValueError("non-finite contribution in the fixed point: outside "
                                             "the proven range, the contract does not define it")
                        x = on_grid(d, -FIX_SHIFT)
                        if abs(x) > FIX_LIMIT:
                            raise ValueError("fixed-point delta outside the proven range")
                        total += x
                    kinds, e = 0, -FIX_SHIFT
                    move = int(float(total) * (1.0 / n))          # int() truncates
                    old = raw[i] if i in raw else base[i]
                    new = old + move
                    if abs(new) > FIX_LIMIT:
                        raise ValueError("fixed-point entry outside the proven range")
                    raw[i] = new
                    val[i] = float(new) * 2.0 ** -FIX_SHIFT
                out.steps.append(StepEvent(g, k, i, ds, kinds, e, move, old, new, contrib_E.get(i),
                                           td_big if tr else None, inexact))
            if predictor is not None:
                predictor.after_step(records[k], k, lane0, lane1, view)
        finals.append(raw)
        for i, c in n_inc.items():
            n_after[i] += c
        t_after += t_inc

    # ---- merge
    words = list(base)
    touched = {}
    for g, raw in enumerate(finals):
        for i, w in raw.items():
            touched.setdefault(i, []).append(w)
    for i in sorted(touched):
        ws = touched[i]
        changed = [w for w in ws if w != base[i]]          # bitwise
        e = None
        if changed:
            n = len(changed)
            if f64:
                kinds, code, fin = 0, 0, []
                for w in changed:
                    v = f64_from_bits(w)
                    if not _finite(v):
                        kinds |= nf_kind(v)
                    else:
                        code = max(code, biased_exponent(v))
                        fin.append(v)
                if kinds:
                    merged = nf_value(kinds)
                else:
                    e = grid_exponent(code) + h
                    merged = grid_mean(sum(on_grid(v, e) for v in fin), n, e)
                words[i] = f64_word(merged)
            else:
                e = -FIX_SHIFT
                words[i] = base[i] + int(float(sum(w - base[i] for w in changed)) * (1.0 / n))
                if abs(words[i]) > FIX_LIMIT:
                    raise ValueError("fixed-point entry outside the proven range")
        out.merges.append(MergeEvent(i, base[i], ws, changed, e, words[i]))

    out.words, out.n, out.t, out.flags, out.eps, out.traces = words, n_after, t_after, flags, eps, traces
    out.last_eps = last_eps
    return out


# ---------------------------------------------------------------- accuracy
# Independent of the combine above: what "exact on the grid" promises, stated
# against the exact rational mean.  The grid is taken from the largest
# magnitude with frexp, not from the model's own e.
#
# f64 step: each d_i is rounded once onto the grid 2^e (at most half a unit), so
# the mean of the rounded values is within 2^(e-1) of the exact mean; int ->
# double, 1/n and the product are three roundings (at most 3 * 2^-53 relative
# < 2^-51); ldexp may round once more to a subnormal (at most 2^-1075):
#     |move - mean| <= 2^(e-1) + 2^-51 * |mean| + 2^-1075
# traces step: the same bound with e the grid of the step's largest finite |td|
# (frexp) plus trace_k.
# f64 merge: the same with the values v_g and e + headroom.
# fixed40 step (units of 2^-40): rint of each d_i is at most half a unit and
# trunc loses less than one whole unit more, so the bound is 3/2 units + the
# relative term.  One whole unit alone does NOT hold for a correct
# implementation: d = (0.49, 0.49, 0.49, 3.49) units sums to 3 after rint,
# trunc(3/4) = 0, and the exact mean is 1.24.
# fixed40 merge: the differences are exact ints, only trunc and the three
# roundings remain: one unit + the relative term.
_REL = Fraction(1, 1 << 51)
_TINY = Fraction(1, 1 << 1075)
_OVERFLOW = Fraction((1 << 1024) - (1 << 970))     # the least magnitude that rounds to inf


def _natural_grid(values):
    """exponent of the ulp of the largest magnitude: its own grid"""
    big = max(abs(v) for v in values)
    if big == 0.0:
        return -1074
    return max(math.frexp(big)[1] - 53, -1074)


def _check_row(mean, got, bound):
    """(mean, got, bound, ok); an infinite result is right when the exact mean is
    within the bound of the overflow threshold"""
    if got in (_INF, -_INF):
        ok = (mean > 0) == (got > 0) and abs(mean) + bound >= _OVERFLOW
        return (mean, got, bound, ok)
    return (mean, got, bound, abs(Fraction(got) - mean) <= bound)


def step_accuracy(replay):
    """[(exact mean of the d_i, move taken, bound, ok)] for every entry-step whose
    contributions are all finite, in value units"""
    rows = []
    for ev in replay.steps:
        if ev.kinds:
            continue
        n = len(ev.ds)
        mean = sum(Fraction(d) for d in ev.ds) / n
        if replay.repr == "f64":
            if replay.agent == "traces":
                e = _natural_grid([ev.td_big]) + replay.trace_k
            else:
                e = _natural_grid(ev.ds)
            rows.append(_check_row(mean, ev.move, _pow2(e - 1) + _REL * abs(mean) + _TINY))
        else:
            unit = _pow2(-FIX_SHIFT)
            move = Fraction(ev.move) * unit
            rows.append((mean, move, Fraction(3, 2) * unit + _REL * abs(mean),
                         abs(move - mean) <= Fraction(3, 2) * unit + _REL * abs(mean)))
    return rows


def merge_accuracy(replay):
    """[(exact mean over the changed groups, merged value or move, bound, ok)] for
    every merged entry whose changed values are all finite"""
    h = headroom(replay.merge_groups)
    rows = []
    for ev in replay.merges:
        if not ev.changed:
            continue
        n = len(ev.changed)
        if replay.repr == "f64":
            vs = [f64_from_bits(w) for w in ev.changed]
            if any(not _finite(v) for v in vs):
                continue
            mean = sum(Fraction(v) for v in vs) / n
            e = _natural_grid(vs) + h
            rows.append(_check_row(mean, f64_from_bits(ev.merged), _pow2(e - 1) + _REL * abs(mean) + _TINY))
        else:
            unit = _pow2(-FIX_SHIFT)
            mean = Fraction(sum(w - ev.base for w in ev.changed), n) * unit
            move = Fraction(ev.merged - ev.base) * unit
            bound = unit + _REL * abs(mean)
            rows.append((mean, move, bound, abs(move - mean) <= bound))
    return rows


# ---------------------------------------------------------------- coverage
TRACE_CONDITIONS = ("row_count_exceeds_nonzero", "decayed_E", "E_ge_2", "cleared_then_revisited", "grid_rounded",
                    "nonfinite_zero_E")
ES_CONDITIONS = ("es_eps_decayed_between_updates", "es_counts_moved_in_step", "es_nan_shortcut")


def coverage(replay):
    """which edges this launch exercised (conditions, computed from the events and
    from what the replay saw on its way)"""
    c = dict.fromkeys(("codes_54_apart", "subnormal_grid", "pinf_with_ninf", "finite_with_nonfinite",
                       "n_ge_64", "changed_by_2_groups", "changed_and_unchanged", "touched_back_to_base",
                       "sign_of_zero_change", "step_overflow", "merge_nonfinite") + TRACE_CONDITIONS
                      + ES_CONDITIONS, False)
    for name in replay.seen:
        c[name] = True
    for ev in replay.steps:
        n = len(ev.ds)
        if n >= 64:
            c["n_ge_64"] = True
        if replay.repr != "f64":
            continue
        fin = [d for d in ev.ds if _finite(d)]
        if ev.kinds & NF_PINF and ev.kinds & NF_NINF:
            c["pinf_with_ninf"] = True
        if ev.kinds and fin:
            c["finite_with_nonfinite"] = True
        if ev.Es is not None:
            nonzero = sum(1 for d in ev.ds if d != 0.0)
            if 0 < nonzero < n:
                c["row_count_exceeds_nonzero"] = True
            if any(E != math.floor(E) for E in ev.Es):
                c["decayed_E"] = True
            if ev.inexact:
                c["grid_rounded"] = True
            if any(E == 0.0 and d != d for E, d in zip(ev.Es, ev.ds)):
                c["nonfinite_zero_E"] = True
        if not ev.kinds:
            codes = [biased_exponent(d) for d in fin]
            if n >= 2 and max(codes) - min(codes) >= 54:
                c["codes_54_apart"] = True
            if n >= 2 and max(codes) <= 1 and any(d != 0.0 for d in fin):
                c["subnormal_grid"] = True
            if ev.before not in (_INF, -_INF) and ev.after in (_INF, -_INF):
                c["step_overflow"] = True       # finite entry + finite contributions = inf
    for ev in replay.merges:
        if len(ev.changed) >= 2:
            c["changed_by_2_groups"] = True
        if ev.changed and len(ev.changed) < replay.n_groups:
            c["changed_and_unchanged"] = True
        if len(ev.changed) < len(ev.touched):
            c["touched_back_to_base"] = True
        if replay.repr == "f64":
            b = f64_from_bits(ev.base)
            for w in ev.changed:
                v = f64_from_bits(w)
                if v == b:                       # equal as numbers, different bits: -0.0 / +0.0
                    c["sign_of_zero_change"] = True
                if not _finite(v):
                    c["merge_nonfinite"] = True
    return c

"""An exact replay model of one shared-mode launch (group_size >= 2).

TEST INFRASTRUCTURE ONLY.  This is a third statement of the shared-Q contract,
written from DESIGN.md section 2 ("Step combine", "Merge", "Fixed point", "UCB")
and the include/rl.h comment on rl_q_repr.  It uses neither the CPU oracle nor
the library: no ctypes, no RNG, no env.  Everything it needs is in the data
both sides already expose:

  - the raw words of Q_base and the UCB counters N / t before the launch;
  - the launch's rl_step_record entries as records[K][n_lanes]
    (fields s, a, r, s2, a2, term, mode, kind, td).

From those it predicts the raw words of Q_base and N / t after the launch, bit
for bit.  Arithmetic is Python int and fractions.Fraction where the contract
says "exact", and CPython floats (IEEE binary64, correctly rounded float(int),
a * b, a + b, no fused multiply-add) where the contract names a rounded
operation.

What the model restates
-----------------------
Per learner group g (lanes [g*G, (g+1)*G), the last group possibly ragged),
starting from Q_base, for each of the K synchronous steps:

  * every record with mode == TRAIN and kind in {2 STEP, 3 RESET+STEP} is one
    update.  Its TD error is recomputed from the group's step-start snapshot in
    the reference's operation order (src/agent.rs:19-45,
    src/agent/one_step_agent.rs:62-72):
        td = (r + gamma * next) - V[s][a]
    with next = V[s2][a2] (SARSA) or the first maximum of V[s2][:] found with a
    strict `>` from element 0 (Q-learning, src/utils.rs:13-21).  V is the value
    table; for the double policy V and the updated table alternate per update
    (double_tabular_policy.rs:41-67: flag true reads alpha = table 0 and writes
    beta = table 1).  The recomputed td must equal the recorded one bit for bit
    (NaN as NaN); differences are returned in Replay.td_mismatches.
    For expected SARSA the recorded td is the INPUT: its probabilities need the
    per-lane epsilon and the group's UCB state, which the oracle parity tests
    cover and this model does not.
  * the contribution is d = lr * td to entry (update table, s, a).
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

Merge: an entry takes the mean over the groups whose final word differs
BITWISE from Q_base's (so -0.0 against +0.0 is a change, and a group that moves
an entry and brings it back to the same bits did not change it).  f64: the mean
of those groups' VALUES on the grid e = max(code, 1) - 1075 + h of the largest
changed finite value, h = max(0, ceil(log2(merge_groups)) - 10) headroom bits
(also when one group changed the entry); non-finite values give the IEEE sum of
their kinds.  fixed40: Q_base += trunc(float(sum of differences) * (1.0 / n)).
UCB: N[s][a] += 1 for every selection (kind 1: the (s, a) of the reset; kind 2:
(s2, a2)), t += 1 per selection, summed over all groups.

The double-policy flag
----------------------
rl_agent_lane_state documents `flags|a|mode` without naming the bits, so the
flag is NOT read from there.  The caller counts: every lane starts with the
flag true at rl_agent_create (DoubleTabularPolicy::new) and it flips once per
update; `replay_launch` takes the flags before the launch and returns them
after it, and the caller carries them from launch to launch.

Out of scope
------------
Eligibility traces (one grid per group step from trace_k; E is not recorded):
`replay_launch(agent="traces")` raises, it does not approximate.
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
_M64 = (1 << 64) - 1
_INF = float("inf")


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


def grid_exponent(code):
    return max(code, 1) - 1075


def headroom(merge_groups):
    """ceil(log2(groups)) - 10 bits, never negative"""
    return max(0, (max(int(merge_groups), 1) - 1).bit_length() - 10)


def _pow2(e):
    return Fraction(1 << e) if e >= 0 else Fraction(1, 1 << -e)


def on_grid(x, e):
    """x / 2^e rounded half-to-even, as an exact int"""
    return round(Fraction(x) / _pow2(e))


def _ldexp(m, e):
    try:
        return math.ldexp(m, e)
    except OverflowError:
        return math.copysign(_INF, m)


def grid_mean(total, n, e):
    return _ldexp(float(total) * (1.0 / n), e)


# ---------------------------------------------------------------- events
class StepEvent:
    """one entry in one group step: its contributions and the move taken.
    f64: ds / move in value units, e the grid exponent (None if a contribution
    was non-finite).  fixed40: ds in value units, move an int of 2^-40."""
    __slots__ = ("group", "step", "entry", "ds", "kinds", "e", "move", "before", "after")

    def __init__(self, group, step, entry, ds, kinds, e, move, before, after):
        self.group, self.step, self.entry = group, step, entry
        self.ds, self.kinds, self.e, self.move = ds, kinds, e, move
        self.before, self.after = before, after          # the entry's value / fixed-point word


class MergeEvent:
    """one entry at the merge: base word, the final word of every group that
    received a contribution to it (touched), those that differ bitwise from the
    base (changed), and the merged word"""
    __slots__ = ("entry", "base", "touched", "changed", "e", "merged")

    def __init__(self, entry, base, touched, changed, e, merged):
        self.entry, self.base, self.touched = entry, base, touched
        self.changed, self.e, self.merged = changed, e, merged


class Replay:
    __slots__ = ("words", "n", "t", "flags", "td_mismatches", "steps", "merges", "repr", "merge_groups",
                 "n_groups")


# ---------------------------------------------------------------- the model
def _first_max(row):
    m = row[0]
    for v in row:
        if v > m:
            m = v
    return m


def _same_f64(a, b):
    return (a != a and b != b) or f64_bits(a) == f64_bits(b)


def replay_launch(q_base, n_base, t_base, records, *, G, P, S, A, lr, gamma, algo, repr,
                  merge_groups=0, ucb=False, flags=None, agent="one_step"):
    """Predict Q_base's raw words and N / t after one launch.

    q_base: P*S*A int64 raw words ([P][S][A] order); n_base: S*A counts; t_base: int;
    records: [K][n_lanes] of rl_step_record (anything indexable by field name);
    algo: "sarsa" | "qlearning" | "expected_sarsa"; repr: "f64" | "fixed40";
    merge_groups: learner groups over every rank (0: this launch's own);
    ucb: the selector is UCB (N / t move); flags: per-lane double-policy flag
    before the launch (None: all true, the state at creation).
    """
    if agent != "one_step":
        raise NotImplementedError(
            f"step_model replays the one-step agent only, not agent={agent!r}: eligibility "
            "traces use one grid per group step and E is not recorded")
    if algo not in ("sarsa", "qlearning", "expected_sarsa"):
        raise ValueError(f"unknown algo {algo!r}")
    if repr not in ("f64", "fixed40"):
        raise ValueError(f"unknown representation {repr!r}")
    if P not in (1, 2) or G < 2 or G > 1024:
        raise ValueError("shared mode: P in {1, 2}, 2 <= group_size <= 1024")
    if repr == "fixed40" and P != 1:
        raise ValueError("the fixed point holds single tables only")
    lr, gamma = float(lr), float(gamma)
    f64 = repr == "f64"
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

    if f64:
        base_val = [f64_from_bits(w) for w in base]
    else:
        for w in base:
            if abs(w) > FIX_LIMIT:
                raise ValueError("fixed-point word outside |Q| <= 2048")
        base_val = [float(w) * 2.0 ** -FIX_SHIFT for w in base]

    out = Replay()
    out.repr, out.merge_groups, out.n_groups = repr, total_groups, n_groups
    out.td_mismatches, out.steps, out.merges = [], [], []
    n_after = [int(v) for v in n_base]
    t_after = int(t_base)
    finals = []                      # per group: {entry: final word}

    for g in range(n_groups):
        lane0, lane1 = g * G, min(L, (g + 1) * G)
        raw = {}                     # entry -> current word of this group (touched entries)
        val = {}                     # entry -> current value

        def V(tbl, s, a):
            i = (tbl * S + s) * A + a
            return val[i] if i in val else base_val[i]

        for k in range(K):
            contrib = {}
            for j in range(lane0, lane1):
                rec = records[k][j]
                kind = int(rec["kind"])
                if kind == KIND_IDLE:
                    continue
                if ucb:
                    if kind == KIND_RESET_STEP:
                        raise ValueError("the reset-and-step schedule does not exist with UCB")
                    sel = (int(rec["s"]), int(rec["a"])) if kind == KIND_RESET else \
                          (int(rec["s2"]), int(rec["a2"]))
                    n_after[sel[0] * A + sel[1]] += 1
                    t_after += 1
                if int(rec["mode"]) != MODE_TRAIN or kind not in (KIND_STEP, KIND_RESET_STEP):
                    continue
                s, a, s2, a2 = int(rec["s"]), int(rec["a"]), int(rec["s2"]), int(rec["a2"])
                r, td_rec = float(rec["r"]), float(rec["td"])
                vt, ut = ((0, 1) if flags[j] else (1, 0)) if P == 2 else (0, 0)
                if algo == "expected_sarsa":
                    td = td_rec
                else:
                    row2 = [V(vt, s2, i) for i in range(A)]
                    nxt = row2[a2] if algo == "sarsa" else _first_max(row2)
                    td = r + gamma * nxt - V(vt, s, a)
                    if not _same_f64(td, td_rec):
                        out.td_mismatches.append((g, k, j, td, td_rec))
                contrib.setdefault((ut * S + s) * A + a, []).append(lr * td)
                if P == 2:
                    flags[j] = not flags[j]
            # every lane read the step-start snapshot; now the entries move
            for i, ds in contrib.items():
                n = len(ds)
                if f64:
                    kinds = 0
                    code = 0
                    for d in ds:
                        if d != d or d in (_INF, -_INF):
                            kinds |= nf_kind(d)
                        else:
                            code = max(code, biased_exponent(d))
                    if kinds:
                        e, move = None, nf_value(kinds)
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
                        if d != d or d in (_INF, -_INF):
                            raise ValueError("non-finite contribution in the fixed point: outside "
                                             "the proven range, the contract does not define it")
                        x = round(Fraction(d) * (1 << FIX_SHIFT))
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
                out.steps.append(StepEvent(g, k, i, ds, kinds, e, move, old, new))
        finals.append(raw)

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
                    if v != v or v in (_INF, -_INF):
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

    out.words, out.n, out.t, out.flags = words, n_after, t_after, flags
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
            if any(v != v or v in (_INF, -_INF) for v in vs):
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
def coverage(replay):
    """which edges this launch exercised (conditions, computed from the events)"""
    c = dict.fromkeys(("codes_54_apart", "subnormal_grid", "pinf_with_ninf", "finite_with_nonfinite",
                       "n_ge_64", "changed_by_2_groups", "changed_and_unchanged", "touched_back_to_base",
                       "sign_of_zero_change", "step_overflow", "merge_nonfinite"), False)
    for ev in replay.steps:
        n = len(ev.ds)
        if n >= 64:
            c["n_ge_64"] = True
        if replay.repr != "f64":
            continue
        fin = [d for d in ev.ds if d == d and d not in (_INF, -_INF)]
        if ev.kinds & NF_PINF and ev.kinds & NF_NINF:
            c["pinf_with_ninf"] = True
        if ev.kinds and fin:
            c["finite_with_nonfinite"] = True
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
                if v != v or v in (_INF, -_INF):
                    c["merge_nonfinite"] = True
    return c

"""The shared-Q step combine and launch merge against an exact replay model.

tests/step_model.py restates DESIGN.md section 2 (step combine, merge, fixed
point, UCB counters) with Python ints and Fractions and replays one launch from
its rl_step_record entries.  Here the CPU oracle (oracle/rlref.c rlo_batch_*) is
driven launch by launch and must equal the model in every raw Q word and UCB
counter; tests/test_gpu_step_model.py drives the device through the same
helper.  The accuracy rows state what "summed exactly on the grid" promises
against the exact rational mean, and the coverage conditions keep every case on
the edge it was built for (they are asserted, not reported).

The model recomputes every td (expected SARSA's included: per-lane epsilon,
the group's running UCB counters, ln(t) of the side under test checked against
a 50-digit logarithm) and replays eligibility traces; the hand-worked tests
below pin the model itself word by word, and the live cases run every traces /
expected-SARSA combination of the parity matrix plus the edges it lacks.
Measured on the CPU: the slowest live case (Taxi, traces, double, UCB) takes
0.7 s, almost all of it the model.

The last sections close the loop (tests/select_model.py): the records themselves
are predicted from the seed, on all 240 shared combinations of the matrix, with
liveness conditions asserted per case, five negative controls and seven
hand-worked tests; the slowest of those cases takes 0.5 s.
"""
import decimal
import math

import numpy as np
import pytest

import matrix_cases as mc
import step_model as sm

LAUNCHES = 3
COMMON = dict(sync_every=4, n_episodes_for_decay=40)

# id -> (params, options).  options: q_mode ("f64" forces f64), repr (expected),
# reset_step, table (crafted table kind + seed), need (coverage conditions the
# case must meet), merge_groups (external merge with that many declared groups).
# G follows tests/test_gpu_f64.py F64_CASES where a case names a kernel form.
# FrozenLake pays nothing within 12 steps of the start: q_default 0.25 (exact in the
# fixed point) gives every update a non-zero TD error
FL_SLIP = dict(env="frozen_lake", map8x8=1, slippery=1, algo="qlearning", group_size=256, n_lanes=900,
               q_default=0.25)
FL_DET = dict(env="frozen_lake", map8x8=1, slippery=0, algo="qlearning", group_size=256, n_lanes=900,
              q_default=0.25)
TAXI_SARSA = dict(env="taxi", algo="sarsa", group_size=100, n_lanes=750)
TAXI_UCB = dict(env="taxi", selector="ucb", algo="qlearning", group_size=128, n_lanes=700)
BJ_QL = dict(env="blackjack", algo="qlearning", group_size=512, n_lanes=900)
BJ_DOUBLE_QL = dict(env="blackjack", policy="double", algo="qlearning", group_size=300, q_default=0.25,
                    n_lanes=800)
BJ_DOUBLE_ES = dict(env="blackjack", policy="double", algo="expected_sarsa", group_size=300,
                    q_default=0.25, n_lanes=800)
BASIC = ("n_ge_64", "changed_by_2_groups", "changed_and_unchanged")

CASES = {
    "fl8-slippery-ql-f64": (FL_SLIP, dict(repr="f64", need=BASIC)),
    "fl8-ql-fixed40": (FL_DET, dict(repr="fixed40", need=BASIC)),
    "fl8-ql-forced-f64": (FL_DET, dict(q_mode="f64", repr="f64", need=BASIC)),
    "taxi-sarsa-fixed40": (TAXI_SARSA, dict(repr="fixed40", need=BASIC[1:])),
    "taxi-sarsa-forced-f64": (TAXI_SARSA, dict(q_mode="f64", repr="f64", need=BASIC[1:])),
    "taxi-ucb-ql": (TAXI_UCB, dict(repr="fixed40", need=BASIC[1:])),
    "bj-ql-fixed40": (BJ_QL, dict(repr="fixed40", need=BASIC[1:])),
    "bj-ql-forced-f64": (BJ_QL, dict(q_mode="f64", repr="f64", need=BASIC[1:])),
    "bj-double-ql-reset-step": (BJ_DOUBLE_QL, dict(repr="f64", reset_step=True, need=BASIC[1:] + ("kind3",))),
    "bj-double-expected-sarsa": (BJ_DOUBLE_ES, dict(repr="f64", need=BASIC[1:])),
    # crafted tables: (a) magnitudes over the whole exponent range, (b) inf / NaN /
    # -0.0, (c) near DBL_MAX (lr 1.5: with lr <= 1 and gamma < 1 a finite move cannot
    # carry a finite entry past DBL_MAX), (d) equal values that every move returns to
    "fl8-slippery-table-a": (FL_SLIP, dict(repr="f64", table=("a", 7),
                                           need=BASIC + ("codes_54_apart", "subnormal_grid"))),
    "fl8-slippery-table-b": (FL_SLIP, dict(repr="f64", table=("b", 1),
                                           need=BASIC + ("pinf_with_ninf", "finite_with_nonfinite",
                                                         "sign_of_zero_change", "merge_nonfinite"))),
    "fl8-slippery-table-c": (dict(FL_SLIP, lr=1.5), dict(repr="f64", table=("c", 1),
                                           need=BASIC + ("step_overflow", "merge_nonfinite"))),
    "fl8-slippery-table-d": (dict(FL_SLIP, lr=1e-30), dict(repr="f64", table=("d", 0),
                                                           need=("n_ge_64", "touched_back_to_base"))),
    "bj-table-a": (BJ_QL, dict(q_mode="f64", repr="f64", table=("a", 1),
                               need=BASIC[1:] + ("codes_54_apart", "subnormal_grid"))),
    "bj-table-b": (BJ_QL, dict(q_mode="f64", repr="f64", table=("b", 1),
                               need=BASIC[1:] + ("pinf_with_ninf", "finite_with_nonfinite",
                                                 "sign_of_zero_change", "merge_nonfinite"))),
    "bj-table-c": (dict(BJ_QL, lr=1.5), dict(q_mode="f64", repr="f64", table=("c", 1),
                               need=BASIC[1:] + ("step_overflow", "merge_nonfinite"))),
    "bj-table-d": (dict(BJ_QL, lr=1e-30), dict(q_mode="f64", repr="f64", table=("d", 0),
                                               need=("touched_back_to_base",))),
}
HEADROOM_CASE = (FL_SLIP, dict(repr="f64", table=("a", 7), merge_groups=4096,
                               need=BASIC + ("codes_54_apart", "headroom_moves_result")))


def crafted_table(kind, seed, P, S, A):
    """the tables of the issue's list; numpy's legacy RandomState keeps its streams"""
    rs = np.random.RandomState(seed)
    shape = (P, S, A)
    sign = rs.choice([-1.0, 1.0], size=shape)
    if kind == "a":
        # magnitudes log-uniform over 2^-1074 .. 2^1000; two states in five hold only
        # subnormal-range values, so that whole steps run on a subnormal grid
        ex = rs.uniform(-1074, 1000, size=shape)
        tiny = rs.rand(S) < 0.4
        ex[:, tiny, :] = rs.uniform(-1074, -1030, size=shape)[:, tiny, :]
        return sign * np.ldexp(rs.uniform(1.0, 2.0, size=shape), np.floor(ex).astype(np.int64))
    if kind == "b":
        # zeros and unit-scale values with whole rows of -inf and single +inf, NaN, -0.0
        q = np.where(rs.rand(*shape) < 0.5, 0.0, rs.uniform(-1.0, 1.0, size=shape))
        u = rs.rand(*shape)
        q[u < 0.20] = -0.0
        q[(u >= 0.20) & (u < 0.28)] = np.inf
        q[(u >= 0.28) & (u < 0.32)] = np.nan
        q[(u >= 0.32) & (u < 0.36)] = -np.inf
        q[:, rs.rand(S) < 0.15, :] = -np.inf
        return q
    if kind == "c":
        return sign * np.finfo(np.float64).max * rs.uniform(0.5, 1.0, size=shape)
    if kind == "d":
        return np.full(shape, 3.0e9)
    raise ValueError(kind)


def _records_as_dicts(recs):
    names = recs.dtype.names
    return [[dict(zip(names, (row[n] for n in names))) for row in step] for step in recs]


def _first_diffs(got, want, limit=5):
    bad = [(i, hex(g & (2 ** 64 - 1)), hex(w & (2 ** 64 - 1))) for i, (g, w) in enumerate(zip(got, want)) if g != w]
    return len(bad), bad[:limit]


_LN_CHECKED = {}


def assert_ln_within_1ulp(used):
    """every ln(t) the model was given against a 50-digit decimal logarithm: the
    side under test's log is an input of the model, and this makes it a checked one"""
    ctx = decimal.Context(prec=50)
    for t, v in used.items():
        if _LN_CHECKED.get(t) == v:
            continue
        if t == 1:
            assert v == 0.0
        else:
            exact = ctx.ln(decimal.Decimal(t))
            err = abs(ctx.subtract(decimal.Decimal(v), exact))
            assert err <= decimal.Decimal(math.ulp(v)), f"ln({t}) = {v!r} is more than 1 ulp from {exact}"
        _LN_CHECKED[t] = v


def model_kw(obj, p):
    """what replay_launch needs of the parameters"""
    return dict(G=p["group_size"], P=obj.P, S=obj.S, A=obj.A, lr=p["lr"], gamma=p["gamma"], algo=p["algo"],
                ucb=p["selector"] == "ucb", agent=p["agent"], eps_decay=p["eps_decay"], eps_final=p["eps_final"],
                decay_kind=p["decay_kind"], ucb_c=p["ucb_c"], lam=p["lambda_"], max_steps=p["max_steps"],
                blackjack=p["env"] in ("blackjack", 3))


def replay_and_check(obj, p, launch, *, launches=LAUNCHES, merge_groups=0, ln=None, info=None):
    """Run `launches` launches on obj (an oracle Batch or a device Agent, recording
    on), replay each from its records and assert the model's words, counters and
    per-lane epsilon equal obj's, the recomputed td equal the recorded ones and the
    accuracy rows hold.  ln: the log of obj's side, a list of ints -> list of floats
    (called once per launch; needed for UCB + expected SARSA only).  Returns the
    coverage conditions met over all launches; info (a dict) receives max_raw_bits."""
    kw = model_kw(obj, p)
    needs_ln = kw["ucb"] and p["algo"] == "expected_sarsa"
    flags = traces = last_eps = None   # the state at creation
    eps = np.asarray(obj.epsilon(), np.float64).tolist()
    met = {}
    for li in range(launches):
        q0 = obj.q_raw().reshape(-1).tolist()
        n0, t0 = obj.ucb()
        n0 = np.asarray(n0).reshape(-1).tolist()
        launch()
        recs = obj.records()
        assert recs.shape == (p["sync_every"], p["n_lanes"])
        table = {}
        if needs_ln:
            # a group's t runs from t0 to t0 + one increment per lane and step
            ts = list(range(int(t0), int(t0) + p["sync_every"] * min(p["group_size"], p["n_lanes"]) + 1))
            table = dict(zip(ts, (float(v) for v in ln(ts))))
        rep = sm.replay_launch(q0, n0, int(t0), _records_as_dicts(recs), repr=obj.q_repr(), merge_groups=merge_groups,
                               flags=flags, eps=eps, traces=traces, last_eps=last_eps, ln=table.__getitem__, **kw)
        flags, eps, traces, last_eps = rep.flags, rep.eps, rep.traces, rep.last_eps
        assert_ln_within_1ulp(rep.ln_used)
        assert not rep.td_mismatches, f"launch {li}: td recomputed != recorded: {rep.td_mismatches[:5]}"
        nbad, bad = _first_diffs(obj.q_raw().reshape(-1).tolist(), rep.words)
        assert nbad == 0, f"launch {li}: {nbad} Q words differ (entry, got, model): {bad}"
        n1, t1 = obj.ucb()
        assert np.asarray(n1).reshape(-1).tolist() == rep.n and int(t1) == rep.t, f"launch {li}: UCB counters"
        got_eps = np.asarray(obj.epsilon(), np.float64)
        assert got_eps.view(np.uint64).tolist() == [sm.f64_bits(x) for x in rep.eps], f"launch {li}: epsilon"
        for name, rows in (("step", sm.step_accuracy(rep)), ("merge", sm.merge_accuracy(rep))):
            worst = [r for r in rows if not r[3]]
            assert not worst, f"launch {li}: {name} accuracy bound missed (mean, got, bound): " \
                              f"{[(float(m), float(g), float(b)) for m, g, b, _ in worst[:3]]}"
        for k, v in sm.coverage(rep).items():
            met[k] = met.get(k, False) or v
        met["kind3"] = met.get("kind3", False) or bool((recs["kind"] == 3).any())
        if info is not None:
            info["max_raw_bits"] = max(info.get("max_raw_bits", 0), rep.max_raw_bits)
        if merge_groups and sm.headroom(merge_groups):
            # the same launch merged without headroom must differ somewhere, or the
            # headroom bits were never visible in this case
            plain = sm.replay_launch(q0, n0, int(t0), _records_as_dicts(recs), repr=obj.q_repr(), merge_groups=0,
                                     **kw) if obj.P == 1 and p["agent"] == "one_step" else None
            if plain is not None and plain.words != rep.words:
                met["headroom_moves_result"] = True
    return met


def setup_pair(obj, p, opt, shape):
    """the same preparation on either side (names differ only for recording)"""
    if opt.get("q_mode"):
        obj.set_q_mode(opt["q_mode"])
    if opt.get("table"):
        obj.set_q(crafted_table(*opt["table"], *shape))
        if opt.get("q_mode"):
            obj.set_q_mode(opt["q_mode"])
    if opt.get("reset_step"):
        obj.set_reset_step(True)
    (obj.set_record if hasattr(obj, "set_record") else obj.set_recording)(True)
    assert obj.q_repr() == opt["repr"]


def assert_coverage(met, need):
    missing = [k for k in need if not met.get(k)]
    assert not missing, f"the case no longer exercises: {missing}"


@pytest.mark.parametrize("name", list(CASES))
def test_oracle_equals_replay_model(oracle, name):
    kw, opt = CASES[name]
    p = oracle.default_params(**COMMON, **kw)
    ref = oracle.Batch(p)
    setup_pair(ref, p, opt, (ref.P, ref.S, ref.A))
    met = replay_and_check(ref, p, lambda: ref.run(1))
    assert_coverage(met, opt["need"])
    if opt.get("table", ("", 0))[0] == "d":
        want = crafted_table(*opt["table"], ref.P, ref.S, ref.A)
        assert np.array_equal(ref.q(), want), "a move too small to change an entry changed the merged table"


def test_oracle_headroom_equals_replay_model(oracle):
    """4096 declared learner groups: the merge grid gives up 2 low bits, through
    the external-collective path (launch_groups / fold / apply_delta)"""
    kw, opt = HEADROOM_CASE
    p = oracle.default_params(**COMMON, **kw)
    ref = oracle.Batch(p)
    setup_pair(ref, p, opt, (ref.P, ref.S, ref.A))
    ref.set_merge_groups(opt["merge_groups"])

    def launch():
        delta = np.zeros(ref.delta_words(), np.int64)
        ref.launch_groups(delta)
        ref.fold(delta)
        ref.apply_delta(delta)

    met = replay_and_check(ref, p, launch, merge_groups=opt["merge_groups"])
    assert_coverage(met, opt["need"])


ONE_LANE = {"taxi-sarsa": dict(env="taxi", algo="sarsa"),
            "bj-double-ql": dict(env="blackjack", policy="double", algo="qlearning", q_default=0.25)}


def obj_run(obj):
    obj.run(1)
    if hasattr(obj, "synchronize"):
        obj.synchronize()


@pytest.mark.parametrize("name", list(ONE_LANE))
def test_one_lane_is_plain_update(oracle, name):
    p = oracle.default_params(n_lanes=1, group_size=2, **COMMON, **ONE_LANE[name])
    ref = oracle.Batch(p)
    ref.set_q_mode("f64")
    ref.set_record(True)
    one_lane_plain_update(ref, p)


def one_lane_plain_update(obj, p, launches=8):
    P, S, A = obj.P, obj.S, obj.A
    q = [sm.f64_from_bits(w) for w in obj.q_raw().reshape(-1).tolist()]
    flag, updates = True, 0
    for _ in range(launches):
        q0 = obj.q_raw().reshape(-1).tolist()
        obj_run(obj)
        recs = obj.records()
        rep = sm.replay_launch(q0, [0] * (S * A), 1, _records_as_dicts(recs), G=2, P=P, S=S, A=A, lr=p["lr"],
                               gamma=p["gamma"], algo=p["algo"], repr="f64", flags=[flag])
        for rec in recs[:, 0]:
            if rec["mode"] == 0 and rec["kind"] in (2, 3):
                ut = (1 if flag else 0) if P == 2 else 0
                i = (ut * S + int(rec["s"])) * A + int(rec["a"])
                q[i] = sm.canonical(q[i] + p["lr"] * float(rec["td"]))
                flag = not flag if P == 2 else flag
                updates += 1
        words = [sm.f64_word(v) for v in q]
        assert not rep.td_mismatches
        assert rep.words == words, "the model with one lane is not Q += lr * td"
        assert obj.q_raw().reshape(-1).tolist() == words
    assert updates >= launches * p["sync_every"] // 4


# ---------------------------------------------------------------- the model itself
def test_model_imports_neither_oracle_nor_library():
    import ast
    tree = ast.parse(open(sm.__file__).read())
    names = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            names |= {a.name.split(".")[0] for a in node.names}
        elif isinstance(node, ast.ImportFrom):
            names.add((node.module or "").split(".")[0])
    assert names == {"math", "struct", "fractions"}, names


def test_ldexp_rounds_subnormals_half_to_even():
    """the one libm call the model relies on"""
    tiny = 2.0 ** -1074
    assert math.ldexp(1.0, -1075) == 0.0 and math.ldexp(3.0, -1075) == 2 * tiny
    assert math.ldexp(5.0, -1076) == tiny and math.ldexp(-0.75, -1074) == -tiny
    assert math.copysign(1.0, math.ldexp(-0.25, -1074)) == -1.0


def _rec(kind=2, s=0, a=0, s2=1, a2=0, r=0.0, td=0.0, mode=0, term=0):
    return dict(kind=kind, s=s, a=a, s2=s2, a2=a2, r=r, td=td, mode=mode, term=term)


def _replay_td(tds, lr=1.0, base=0.0, **kw):
    """G lanes each contributing lr * td to entry (0, 0) in one step (the recorded
    td is the input: td_source="record")"""
    words = [sm.f64_word(base), 0, 0, 0]
    return sm.replay_launch(words, [0] * 4, 1, [[_rec(td=t) for t in tds]], G=max(2, len(tds)), P=1, S=2, A=2,
                            lr=lr, gamma=0.5, algo="sarsa", repr="f64", td_source="record", **kw)


def test_model_hand_worked_edges():
    inf, tiny = float("inf"), 2.0 ** -1074
    # 60 binades apart: the small one is below half a unit of the large one's grid
    rep = _replay_td([1.0, 2.0 ** -60])
    assert sm.f64_from_bits(rep.words[0]) == 0.5
    # exactly representable sum on the grid of the largest: (1 + 2^-52) / 2
    rep = _replay_td([1.0, 2.0 ** -52])
    assert sm.f64_from_bits(rep.words[0]) == 0.5 + 2.0 ** -53
    # subnormal grid: code 0 and code 1 share e = -1074; mean of 3 and 2^-1022 units
    rep = _replay_td([3 * tiny, 2.0 ** -1022])
    assert sm.f64_from_bits(rep.words[0]) == (2 ** 51 + 2) * tiny        # 2^51 + 1.5 units, half to even
    # +inf with -inf is NaN, canonical; finite with +inf is +inf
    assert _replay_td([inf, -inf, 1.0]).words[0] == sm.QNAN_BITS
    assert sm.f64_from_bits(_replay_td([inf, 1.0]).words[0]) == inf
    # -0.0 moved to +0.0 is a change; a move that returns the same bits is none
    rep = _replay_td([0.0], base=-0.0)
    assert rep.words[0] == 0 and len(rep.merges[0].changed) == 1
    rep = _replay_td([2.0 ** -60], base=1.0)
    assert rep.words[0] == sm.f64_word(1.0) and rep.merges[0].changed == []
    # headroom: 4096 groups drop 2 bits even for an entry one group changed
    v = 1.0 + 3 * 2.0 ** -52
    assert sm.f64_from_bits(_replay_td([v]).words[0]) == v
    assert sm.f64_from_bits(_replay_td([v], merge_groups=4096).words[0]) == 1.0 + 4 * 2.0 ** -52
    assert sm.headroom(1024) == 0 and sm.headroom(1025) == 1 and sm.headroom(4096) == 2 and sm.headroom(4097) == 3


def test_accuracy_rows_reject_a_wrong_grid():
    """the bound is not satisfied by a grid taken from the smallest contribution's
    neighbour or by a headroom shift applied twice"""
    rep = _replay_td([1.0, 2.0 ** -30, 2.0 ** -30])
    assert all(r[3] for r in sm.step_accuracy(rep))
    rep.steps[0].move = 0.5                      # as if the grid were 2^-1 instead of 2^-52
    assert not all(r[3] for r in sm.step_accuracy(rep))
    v = 1.0 + 3 * 2.0 ** -52
    rep = _replay_td([v], merge_groups=4096)
    assert all(r[3] for r in sm.merge_accuracy(rep))
    rep.merges[0].merged = sm.f64_word(1.0 + 16 * 2.0 ** -52)     # 4 bits dropped instead of 2
    assert not all(r[3] for r in sm.merge_accuracy(rep))


# ---------------------------------------------------------------- hand-worked: traces
# lr 0.5, gamma 0.5, lambda 0.5: fl(gamma * lambda) = 0.25, Ebound = 1 / 0.75, and
# 0.5 * 1.333 * (1 + 2^-50) * 1.0001 = 0.6667.. = 0.6667 * 2^0, so trace_k = 0 + 2 = 2:
# a step whose largest |td| is 1.0 (code 1023) runs on the grid 2^(1023 - 1075 + 2) = 2^-50.
def _traces(records, S=2, P=1, lr=0.5, gamma=0.5, lam=0.5, max_steps=100, q=None, **kw):
    words = [sm.f64_word(v) for v in (q or [0.0] * (P * S * 2))]
    G = max(2, len(records[0]))
    return sm.replay_launch(words, [0] * (S * 2), 1, records, G=G, P=P, S=S, A=2, lr=lr, gamma=gamma,
                            algo="sarsa", repr="f64", agent="traces", td_source="record", lam=lam,
                            max_steps=max_steps, **kw)


def _values(rep):
    return [sm.f64_from_bits(w) for w in rep.words]


def test_trace_grid_k_by_hand():
    assert sm.trace_grid_k(0.5, 0.5, 0.5, 100, False) == 2
    # gamma * lambda = 1: Ebound is the max_steps + 2 = 4 terms; 0.5 * 4 * 1.0001.. = 0.50005 * 2^2: k = 4
    assert sm.trace_grid_k(0.5, 1.0, 1.0, 2, False) == 4
    # Blackjack has 33 terms whatever max_steps says: 33 * 1.0001 = 0.5157 * 2^6: k = 8
    assert sm.trace_grid_k(1.0, 1.0, 1.0, 2, True) == 8
    # above 1: (1.5^4 - 1) / 0.5 = 8.125, times 0.5 * 1.0001 = 4.06 = 0.508 * 2^3: k = 5
    assert sm.trace_grid_k(0.5, 1.0, 1.5, 2, False) == 5
    assert sm.trace_grid_k(0.0, 0.5, 0.5, 100, False) == 0
    assert sm.trace_grid_k(1e300, 1.0, 10.0, 10 ** 6, False) == 1100        # the sum overflows


def test_traces_row_count_includes_a_zero_E_action():
    """lane 0 takes (0, 0), lane 1 takes (0, 1), both td 1.0: both lanes cover row 0,
    so entry (0, 0) receives 0.5 * (1 * 1) and 0.5 * (1 * 0) and n = 2: it moves by
    0.25.  Counting only the non-zero contribution would move it by 0.5."""
    rep = _traces([[_rec(s=0, a=0, td=1.0), _rec(s=0, a=1, td=1.0)]])
    assert _values(rep) == [0.25, 0.25, 0.0, 0.0]
    assert sm.coverage(rep)["row_count_exceeds_nonzero"]
    assert all(r[3] for r in sm.step_accuracy(rep))


def test_traces_grid_comes_from_the_steps_largest_td():
    """lane 0's td 2^30 (code 1053) puts the whole step on 2^(1053 - 1075 + 2) = 2^-20.
    Lanes 1 and 2 contribute 0.5 + 2^-21 (2^19 + 0.5 units: the tie goes to the even
    2^19) and 0.5 + 3 * 2^-21 (2^19 + 1.5 units: up to 2^19 + 2) to entries of their
    own; on those entries' own grids both would be stored exactly."""
    rep = _traces([[_rec(s=0, a=0, td=2.0 ** 30), _rec(s=1, a=0, td=1.0 + 2.0 ** -20),
                    _rec(s=2, a=0, td=1.0 + 3 * 2.0 ** -20)]], S=3)
    assert _values(rep) == [2.0 ** 29, 0.0, 0.5, 0.0, 0.5 + 2.0 ** -19, 0.0]
    assert sm.coverage(rep)["grid_rounded"] and rep.steps[0].e == -20
    assert all(r[3] for r in sm.step_accuracy(rep))
    assert rep.max_raw_bits == 50                        # 2^29 / 2^-20 = 2^49
    # the accuracy row takes its grid from the td, not from the combine: a move on
    # the entries' own grid is as far from it as a rounding on 2^-18 would be
    rep.steps[2].move = 0.5 + 2.0 ** -18
    assert not all(r[3] for r in sm.step_accuracy(rep))


def test_traces_E_accumulates_and_decays_between_visits():
    """one lane, td 1.0 each step, visits (0,0), (1,0), (0,0):
    step 0: Q00 += 0.5 * 1;                         E00 = 1 -> 0.25
    step 1: Q00 += 0.5 * 0.25, Q10 += 0.5 * 1;      E00 -> 0.0625, E10 = 1 -> 0.25
    step 2: E00 = 1.0625: Q00 += 0.53125, Q10 += 0.5 * 0.25
    Q00 = 1.15625, Q10 = 0.625 (replacing traces: 1.125; no decay: 2.0)."""
    rep = _traces([[_rec(s=0, a=0, td=1.0)], [_rec(s=1, a=0, td=1.0)], [_rec(s=0, a=0, td=1.0)]])
    assert _values(rep) == [1.15625, 0.0, 0.625, 0.0]
    cov = sm.coverage(rep)
    assert cov["decayed_E"] and cov["E_ge_2"]
    # gamma * lambda = 1, max_steps 2 (trace_k 4): E is exactly 2 at the revisit,
    # Q00 = 0.5 * 1 + 0.5 * 2 = 1.5
    rep = _traces([[_rec(s=0, a=0, s2=0, td=1.0)], [_rec(s=0, a=0, td=1.0)]], gamma=1.0, lam=1.0, max_steps=2)
    assert _values(rep) == [1.5, 0.0, 0.0, 0.0] and rep.steps[2].Es == [2.0] and rep.steps[0].e == -48


def test_traces_E_is_cleared_at_term():
    """(0,0) with term, a reset, (0,0) again: the second visit starts from E = 0, so
    Q00 = 0.5 + 0.5 = 1.0; a trace kept over the episode's end would give 0.5 + 0.625.
    The state carried to the next launch is the trace after its decay."""
    rep = _traces([[_rec(s=0, a=0, td=1.0, term=1)], [_rec(kind=1, s=0, a=0)], [_rec(s=0, a=0, td=1.0)]])
    assert _values(rep) == [1.0, 0.0, 0.0, 0.0]
    assert sm.coverage(rep)["cleared_then_revisited"]
    assert rep.traces[0].rows == {0: [0.25, 0.0]}
    nxt = _traces([[_rec(s=1, a=1, td=1.0)]], traces=rep.traces)
    assert _values(nxt) == [0.125, 0.0, 0.0, 0.5]        # 0.5 * (1 * 0.25) for the carried pair


def test_traces_nonfinite_td_makes_the_untaken_action_nan():
    """td = +inf at (0, 0): 0.5 * (inf * 1) = +inf for the taken action and
    0.5 * (inf * 0) = NaN for action 1 of the same state, which the lane never took"""
    rep = _traces([[_rec(s=0, a=0, td=float("inf"))]])
    assert rep.words == [sm.f64_word(float("inf")), sm.QNAN_BITS, 0, 0]
    assert sm.coverage(rep)["nonfinite_zero_E"]


def test_traces_double_update_goes_to_the_flagged_table():
    """the flag starts true: the first update writes table 1, the second table 0,
    with one trace for both.  T1[0][0] = 0.5; then T0[0][0] = 0.5 * 0.25, T0[1][0] = 0.5."""
    rep = _traces([[_rec(s=0, a=0, td=1.0)], [_rec(s=1, a=0, td=1.0)]], P=2)
    assert _values(rep) == [0.125, 0.0, 0.5, 0.0, 0.5, 0.0, 0.0, 0.0]
    assert rep.flags == [True]


def test_traces_breach_of_the_one_add_premise_is_an_error():
    """a contribution of 2^51 grid units: the model raises, it does not round on"""
    lt = sm.LaneTrace()
    lt.rows = {0: [8.0, 0.0]}                 # E = 9 at the update: 0.5 * 9 / 2^-50 = 2^51 * 1.125
    with pytest.raises(ValueError, match="2\\^51"):
        _traces([[_rec(s=0, a=0, td=1.0)]], traces=[lt])


# ---------------------------------------------------------------- hand-worked: expected SARSA
def _es(records, q, **kw):
    kw = dict(dict(lr=1.0, gamma=1.0), **kw)
    return sm.replay_launch([sm.f64_word(v) for v in q], kw.pop("n0", [0] * 4), kw.pop("t0", 1), records,
                            G=max(2, len(records[0])), P=1, S=2, A=2, algo="expected_sarsa", repr="f64", **kw)


def test_expected_sarsa_reads_epsilon_before_its_decay():
    """row 1 = [1, 3], eps 0.5 with a linear decay of 0.25.  The terminal update of
    (0, 0) reads eps 0.5: p = [0.25, 0.5], f = 0.25 + 1.5 = 1.75 = td.  With the
    decayed 0.25 it would be p = [0.125, 0.75], f = 2.375 — which is what the lane's
    next update, of (0, 1) after the reset, gets."""
    recs = [[_rec(s=0, a=0, s2=1, td=1.75, term=1)], [_rec(kind=1, s=0, a=1)], [_rec(s=0, a=1, s2=1, td=2.375)]]
    rep = _es(recs, [0.0, 0.0, 1.0, 3.0], eps=[0.5], eps_decay=0.25)
    assert not rep.td_mismatches
    assert _values(rep) == [1.75, 2.375, 1.0, 3.0] and rep.eps == [0.25]
    assert sm.coverage(rep)["es_eps_decayed_between_updates"]
    # eps_final above the decayed value keeps epsilon; decay_kind 1 multiplies
    assert _es(recs, [0.0, 0.0, 1.0, 3.0], eps=[0.5], eps_decay=0.25, eps_final=0.3).eps == [0.5]
    assert _es(recs, [0.0, 0.0, 1.0, 3.0], eps=[0.5], eps_decay=0.25, decay_kind=1).eps == [0.125]


def test_expected_sarsa_ucb_reads_the_counters_after_the_steps_selections():
    """two lanes select (1, 0) in the same step: the group's N[1] goes from [2, 1] to
    [4, 1] and t from 1 to 3 before either update reads them.  With ln(3) given as 4.0
    (ln is an input; any function shows which t and n are read) and c = 1:
    u = [0 + sqrt(4 / 4), 1 + sqrt(4 / 1)] = [1, 3], sum 4, p = [0.25, 0.75],
    f = 0.75 = td for both lanes.  The step-start counters (t = 1, n = [2, 1]) or the
    lane's own increment alone (t = 2, n = [3, 1]) give other numbers."""
    recs = [[_rec(s=0, a=0, s2=1, a2=0, td=0.75), _rec(s=0, a=1, s2=1, a2=0, td=0.75)]]
    rep = _es(recs, [0.0, 0.0, 0.0, 1.0], ucb=True, ucb_c=1.0, n0=[0, 0, 2, 1], t0=1,
              ln={1: 1.0, 2: 2.0, 3: 4.0}.__getitem__)
    assert not rep.td_mismatches
    assert _values(rep) == [0.75, 0.75, 0.0, 1.0]
    assert rep.n == [0, 0, 4, 1] and rep.t == 3 and rep.ln_used == {3: 4.0}
    assert sm.coverage(rep)["es_counts_moved_in_step"]


def test_nan_at_action_0_is_the_argmax():
    nan = float("nan")
    assert sm._argmax([nan, 5.0]) == 0 and sm._argmax([1.0, nan, 0.5]) == 0 and sm._argmax([1.0, nan, 2.0]) == 2
    assert sm._argmax([3.0, 3.0]) == 0
    # eps 0.5, row [NaN, 5]: p[0] = 0.5 is the greedy weight, f = 0.5 * NaN + 0.25 * 5 = NaN
    rep = _es([[_rec(s=0, a=0, s2=1, td=nan)]], [0.0, 0.0, nan, 5.0], eps=[0.5])
    assert not rep.td_mismatches and rep.words[0] == sm.QNAN_BITS
    assert sm.coverage(rep)["es_nan_shortcut"]
    # p[argmax] = 1 - eps and the others eps / A: row [1, 3], eps 0.5 -> 0.25 * 1 + 0.5 * 3
    assert sm.expected_eps_greedy([1.0, 3.0], 0.5) == 1.75 and sm.expected_eps_greedy([3.0, 1.0], 0.5) == 1.75


def test_zero_ucb_sum_is_nan_by_ieee_division():
    """c = 0 and a zero row: u = [0, 0], sum 0, p = 0 / 0 = NaN where Python's own
    division raises; the td and the entry are NaN"""
    rep = _es([[_rec(s=0, a=0, s2=1, td=float("nan"))]], [0.0, 0.0, 0.0, 0.0], ucb=True, ucb_c=0.0,
              n0=[0, 0, 1, 1], ln=math.log)
    assert not rep.td_mismatches and rep.words[0] == sm.QNAN_BITS
    inf = float("inf")
    assert sm.ieee_div(1.0, 0.0) == inf and sm.ieee_div(-1.0, 0.0) == -inf and sm.ieee_div(1.0, -0.0) == -inf
    assert sm.ieee_div(0.0, 0.0) != sm.ieee_div(0.0, 0.0) and sm.ieee_div(inf, inf) != sm.ieee_div(inf, inf)
    assert sm.ieee_sqrt(-1.0) != sm.ieee_sqrt(-1.0) and sm.ieee_sqrt(inf) == inf
    # fresh counters: ln(55) / 2^-1022 overflows to +inf, an unvisited action's bonus
    assert sm.ieee_div(math.log(55.0), sm.MIN_POSITIVE) == inf and sm.ieee_div(math.log(54.0), sm.MIN_POSITIVE) < inf


def test_on_grid_is_the_rational_rounding():
    """the integer-only rounding against Fraction division, ties and signs included"""
    from fractions import Fraction
    rs = np.random.RandomState(3)
    xs = [0.0, -0.0, 0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 2.0 ** -1074, -3 * 2.0 ** -1074, 1.7976931348623157e308]
    xs += list(np.ldexp(rs.uniform(-1, 1, 200), rs.randint(-60, 60, 200)))
    for x in xs:
        for e in (-1074, -60, -3, -1, 0, 1, 5, 40):
            want = round(Fraction(float(x)) / (Fraction(2) ** e))
            got, exact = sm.on_grid_exact(float(x), e)
            assert got == want and exact == (Fraction(float(x)) == want * Fraction(2) ** e), (x, e)


def test_trace_grid_k_equals_the_oracles(oracle):
    """the documented formula in CPython floats against rlo_trace_grid_k"""
    L = oracle.lib()
    one_up = 1.0 + 2.0 ** -52
    n = 0
    for lr in (0.0, 1e-300, 1e-30, 0.05, 0.5, 1.0, 3.0, 1e30, 1e300, -0.05):
        for gamma, lam in ((0.95, 0.5), (0.5, 0.5), (0.99, 0.999), (1.0, 1.0 - 2.0 ** -53), (1.0, 1.0), (1.0, one_up),
                           (1.0, 1.5), (1.0, 10.0), (0.9, 0.0), (-1.0, 1.0), (1.0, -1.5), (2.0, 0.5)):
            for max_steps in (1, 6, 20, 100, 10 ** 6, 2 ** 32 - 1):
                for env in ("cliff_walking", "blackjack"):
                    want = L.rlo_trace_grid_k(lr, gamma, lam, max_steps, oracle.ENV[env])
                    got = sm.trace_grid_k(lr, gamma, lam, max_steps, env == "blackjack")
                    assert got == want, (lr, gamma, lam, max_steps, env, got, want)
                    n += 1
    assert n == 1440


# ---------------------------------------------------------------- live: traces and expected SARSA
# every shared combination of the parity matrix (tests/matrix_cases.py) whose agent
# is the traces one or whose algorithm is expected SARSA: 160 of the 240, at the
# matrix's geometry (130 lanes in groups of 64, 64 and 2, K 8, q_default 0.25, preset
# counters for UCB + expected SARSA), 2 launches from creation.
MATRIX = [c for c in mc.combos() if c[1] == "traces" or c[4] == "expected_sarsa"]
# AUTO holds these in the fixed point; they run once more forced to f64
MATRIX_FIXED = [c for c in MATRIX if c[0] in ("fl8", "cw", "taxi", "bj", "fl8-map", "fle8-wide")
                and c[1:4] == ("one_step", "tabular", "eps_greedy")]
MATRIX_LAUNCHES = 2
assert len(MATRIX) == 160 and len(MATRIX_FIXED) == 6


def matrix_need(c):
    """the conditions every matrix case of its kind meets (measured on the oracle).
    Under UCB the lanes of CliffWalking and FrozenLake 8x8 start in one cell and pick
    the same actions, so rows are covered by equal traces and episodes outlast the
    window: those conditions are asserted for eps-greedy."""
    need = ()
    if c[1] == "traces":
        need += ("decayed_E", "grid_rounded")
        if c[3] == "eps_greedy":
            need += ("row_count_exceeds_nonzero", "E_ge_2", "cleared_then_revisited")
    if c[4] == "expected_sarsa":
        need += ("es_counts_moved_in_step",) if c[3] == "ucb" else ("es_eps_decayed_between_updates",)
    return need


def check_matrix_case(obj, p, c, ln, q_mode=None, info=None):
    """the same on either side: obj is the oracle's Batch or the device's Agent of case c"""
    auto = obj.q_repr()
    assert (auto == "fixed40") == (c in MATRIX_FIXED)
    if q_mode:
        obj.set_q_mode(q_mode)
        assert obj.q_repr() == q_mode
    if mc.presets_ucb(c):
        obj.set_ucb(*mc.ucb_preset(obj.S, obj.A))
    (obj.set_record if hasattr(obj, "set_record") else obj.set_recording)(True)
    met = replay_and_check(obj, p, lambda: obj_run(obj), launches=MATRIX_LAUNCHES, ln=ln, info=info)
    assert_coverage(met, matrix_need(c))


def oracle_ln(oracle):
    log = oracle.lib().rlo_log
    return lambda ts: [log(float(t)) for t in ts]


@pytest.mark.parametrize("c", MATRIX, ids=mc.case_id)
def test_oracle_matrix_case_equals_replay_model(oracle, c):
    p = oracle.default_params(**mc.shared_kw(c))
    check_matrix_case(oracle.Batch(p), p, c, oracle_ln(oracle))


@pytest.mark.parametrize("c", MATRIX_FIXED, ids=mc.case_id)
def test_oracle_matrix_case_forced_f64_equals_replay_model(oracle, c):
    p = oracle.default_params(**mc.shared_kw(c))
    check_matrix_case(oracle.Batch(p), p, c, oracle_ln(oracle), q_mode="f64")


# edges the matrix lacks: id -> (params, conditions the case must meet)
EDGE_COMMON = dict(sync_every=8, n_episodes_for_decay=40)
CW_TRACES = dict(env="cliff_walking", agent="traces", algo="sarsa", group_size=64, n_lanes=200)
EDGE_CASES = {
    # gamma * lambda at and above 1: Ebound is the geometric sum over the longest episode
    "cw-traces-gl-1": (dict(CW_TRACES, gamma=1.0, lambda_=1.0), ("E_ge_2", "grid_rounded")),
    "cw-traces-gl-1.5": (dict(CW_TRACES, gamma=1.0, lambda_=1.5, max_steps=20), ("E_ge_2", "decayed_E")),
    # lr 1e300 reaches +-inf and NaN within a few steps (tests/test_gpu_f64.py runs the
    # same three pair-storage forms against the oracle)
    "cw-traces-lr1e300": (dict(CW_TRACES, lr=1e300), ("nonfinite_zero_E", "merge_nonfinite")),
    "taxi-traces-lr1e300": (dict(env="taxi", agent="traces", algo="qlearning", group_size=128, n_lanes=200, lr=1e300),
                            ("nonfinite_zero_E", "merge_nonfinite")),
    "bj-traces-double-lr1e300": (dict(env="blackjack", agent="traces", policy="double", algo="sarsa", group_size=256,
                                      n_lanes=300, lr=1e300), ("nonfinite_zero_E", "merge_nonfinite")),
    # fresh counters: the NaN regime of SURVEY F7 and the kernel's IEEE shortcuts
    "taxi-ucb-es-fresh": (dict(env="taxi", selector="ucb", algo="expected_sarsa", group_size=128, n_lanes=200),
                          ("es_nan_shortcut", "es_counts_moved_in_step", "merge_nonfinite")),
    # one group of 512: more than 64 (lane, state) pairs on a row
    "cw-traces-G512": (dict(CW_TRACES, algo="qlearning", group_size=512, n_lanes=600),
                       ("n_ge_64", "row_count_exceeds_nonzero", "decayed_E")),
    "one-lane-traces": (dict(CW_TRACES, group_size=2, n_lanes=1), ("decayed_E",)),
}


def check_edge_case(obj, p, name, ln, info=None):
    (obj.set_record if hasattr(obj, "set_record") else obj.set_recording)(True)
    assert obj.q_repr() == "f64"
    met = replay_and_check(obj, p, lambda: obj_run(obj), launches=MATRIX_LAUNCHES, ln=ln, info=info)
    assert_coverage(met, EDGE_CASES[name][1])


@pytest.mark.parametrize("name", list(EDGE_CASES))
def test_oracle_edge_case_equals_replay_model(oracle, name):
    p = oracle.default_params(**EDGE_COMMON, **EDGE_CASES[name][0])
    check_edge_case(oracle.Batch(p), p, name, oracle_ln(oracle))


# ---------------------------------------------------------------- the closed loop: records from the seed
# tests/select_model.py predicts every record of a launch from the seed and the state
# before it; the replay above then runs on the predicted records.  All 240 shared
# combinations of the parity matrix at its geometry (130 lanes in groups of 64, 64 and
# 2, K 8), 2 launches from creation, with inputs chosen so that the selection
# arithmetic is live (asserted per case by assert_selection_live, on the model's own
# bookkeeping):
#   - eps0 0.5 and a linear decay of 0.5 / (0.5 * 16) = 0.0625 per terminated episode:
#     both branches of the eps test occur from the first step, the lanes' epsilons
#     differ after their first episodes and Blackjack's reach the eps == 0 shortcut;
#   - max_steps 5: every lane that survives truncates at its 7th synchronous step, inside
#     the 16.  Two kinds of variant cannot end an episode in the env itself under that:
#     on the deterministic 8x8 map the nearest hole (cell 19) is exactly 5 moves from the
#     start, and a Taxi delivery takes a pickup, at least 4 moves and the drop-off.  They
#     get inputs of their own, so that every case has both a terminal step of its env
#     and a truncation:
#       deterministic 8x8 (fl8, fl8-map, fle8-wide): max_steps 7 (truncation at the 9th
#         step), the start table holds 1/2 in both tables at LAKE_STEER, the five
#         (cell, action) pairs of the path 0 -> 8 -> 16 -> 17 -> 18 -> hole 19, and the UCB
#         counters of those five rows are 1 in every action.  Greedy selections follow
#         the path (1/2 > 3/8); under UCB, where a group's lanes move in lockstep, the
#         first episode falls into the hole at its 5th move, the 64 increments then take
#         the steered action's bonus from 1.46 to 0.18 and the second episode leaves the
#         path and is truncated;
#       Taxi: max_steps 13 (truncation at the 15th step) and a start table of twice the
#         undiscounted optimal action values (integers; taxi_optimal_table) plus the
#         {0, 1/8, 1/4, 3/8} draw: the optimal actions stay ahead by more than the draw and
#         the UCB bonuses can reorder, equal optimal actions tie where their draws do, and
#         lanes that start within reach deliver (+20) while the others are truncated;
SEL_LAUNCHES = 2
SEL_VALUES = (0.0, 0.125, 0.25, 0.375)
SEL_COUNTS = (1, 4, 9)
SEL_MATRIX = mc.combos()
SEL_EPS_GREEDY = [c for c in SEL_MATRIX if c[3] == "eps_greedy"]
# AUTO holds these in the fixed point (one-step agent, single table: the range proof
# covers SARSA, Q-learning and expected SARSA over eps-greedy, and SARSA / Q-learning
# whatever selected the actions); they run once more forced to f64
SEL_FIXED = [c for c in SEL_MATRIX if c[0] in ("fl8", "cw", "taxi", "bj", "fl8-map", "fle8-wide")
             and c[1:3] == ("one_step", "tabular") and (c[3] == "eps_greedy" or c[4] != "expected_sarsa")]
assert len(SEL_MATRIX) == 240 and len(SEL_EPS_GREEDY) == 120
# combinations that cannot meet a liveness condition: name -> reason (cap: 5 % of 240)
SEL_LEFT_OUT = {}
assert len(SEL_LEFT_OUT) <= 12


LAKE_STEER = ((0, 1), (8, 1), (16, 2), (17, 2), (18, 2))      # down, down, right, right, right: into cell 19


def lake_det8(kw):
    return kw["env"].startswith("frozen_lake") and bool(kw["map8x8"]) and not kw["slippery"]


def sel_kw(c, **over):
    kw = dict(mc.shared_kw(c), eps0=0.5, n_episodes_for_decay=16)
    kw["max_steps"] = 13 if kw["env"] == "taxi" else (7 if lake_det8(kw) else 5)
    kw.update(over)
    return kw


def sel_table(P, S, A, kw, seed=11):
    q = np.random.RandomState(seed).choice(SEL_VALUES, size=(P, S, A))
    if kw["env"] == "taxi":
        q += 2.0 * taxi_optimal_table()
    elif lake_det8(kw):
        for s, a in LAKE_STEER:
            q[:, s, a] = 0.5
    return q


def sel_counters(S, A, kw, seed=20):
    """half the rows hold one count in every action (the scores tie where the values
    do), the others a count per entry"""
    rs = np.random.RandomState(seed)
    counts = rs.choice(SEL_COUNTS, size=(S, A))
    flat = rs.rand(S) < 0.5
    counts[flat, :] = rs.choice(SEL_COUNTS, size=(S, 1))[flat, :]
    if lake_det8(kw):
        for s, _ in LAKE_STEER:
            counts[s, :] = 1
    return counts.astype(np.uint64), np.uint64(5000)


def sel_prepare(obj, kw, q_mode=None, reset_step=False):
    obj.set_q(sel_table(obj.P, obj.S, obj.A, kw))
    if q_mode:
        obj.set_q_mode(q_mode)
    if kw["selector"] == "ucb":
        obj.set_ucb(*sel_counters(obj.S, obj.A, kw))
    if reset_step:
        obj.set_reset_step(True)
    (obj.set_record if hasattr(obj, "set_record") else obj.set_recording)(True)


def sel_predictor(p, kw, reset_step=False, mutation=None):
    """kw: the case's own parameters (a device case's p carries a registered map's id
    in map8x8; the model runs the built-in rows the copy was made of)"""
    import select_model as selm
    return selm.Predictor(env=kw["env"], n_lanes=p["n_lanes"], seed=p["seed"], lane_offset=p["lane_offset"],
                          map8x8=kw.get("map8x8", 0), slippery=kw.get("slippery", 0), max_steps=p["max_steps"],
                          ucb=kw["selector"] == "ucb", ucb_c=p["ucb_c"], reset_step=reset_step,
                          eps_decay=p["eps_decay"], eps_final=p["eps_final"], decay_kind=p["decay_kind"],
                          mutation=mutation)


def sel_launch_kw(obj, p):
    kw = model_kw(obj, p)
    for k in ("ucb", "ucb_c", "eps_decay", "eps_final", "decay_kind"):       # the predictor's
        del kw[k]
    return kw


def sel_ln_table(p, t0, ln):
    ts = list(range(int(t0), int(t0) + p["sync_every"] * min(p["group_size"], p["n_lanes"]) + 1))
    return dict(zip(ts, (float(v) for v in ln(ts))))


def predict_and_check(obj, p, kw, ln, *, launches=SEL_LAUNCHES, reset_step=False, keep=None):
    """obj (an oracle Batch or a device Agent, prepared and recording) against the
    closed loop: every record field, td, Q word, N, t and epsilon of every launch.
    Returns the model's bookkeeping; keep (a list) receives every launch's inputs and
    records for the negative controls."""
    import select_model as selm
    pr = sel_predictor(p, kw, reset_step)
    assert (pr.S, pr.A) == (obj.S, obj.A)
    lkw = sel_launch_kw(obj, p)
    flags = traces = last_eps = None
    eps = np.asarray(obj.epsilon(), np.float64).tolist()
    for li in range(launches):
        q0 = obj.q_raw().reshape(-1).tolist()
        n0, t0 = obj.ucb()
        n0 = np.asarray(n0).reshape(-1).tolist()
        obj_run(obj)
        recs = _records_as_dicts(obj.records())
        assert len(recs) == p["sync_every"] and len(recs[0]) == p["n_lanes"]
        table = sel_ln_table(p, t0, ln) if pr.ucb else {}
        if keep is not None:
            keep.append((q0, n0, int(t0), recs, table, obj.q_repr()))
        rep, _, bad = selm.predict_launch(pr, q0, n0, int(t0), p["sync_every"], recorded=recs, repr=obj.q_repr(),
                                          flags=flags, eps=eps, traces=traces, last_eps=last_eps,
                                          ln=table.__getitem__, **lkw)
        flags, eps, traces, last_eps = rep.flags, rep.eps, rep.traces, rep.last_eps
        assert_ln_within_1ulp(rep.ln_used)
        assert not bad, f"launch {li}: {len(bad)} record fields differ (step, lane, field, model, got): {bad[:6]}"
        nbad, diffs = _first_diffs(obj.q_raw().reshape(-1).tolist(), rep.words)
        assert nbad == 0, f"launch {li}: {nbad} Q words differ (entry, got, model): {diffs}"
        n1, t1 = obj.ucb()
        assert np.asarray(n1).reshape(-1).tolist() == rep.n and int(t1) == rep.t, f"launch {li}: UCB counters"
        got_eps = np.asarray(obj.epsilon(), np.float64)
        assert got_eps.view(np.uint64).tolist() == [sm.f64_bits(x) for x in rep.eps], f"launch {li}: epsilon"
    return pr.totals()


def assert_selection_live(st, kw, name=""):
    """the issue's per-case conditions on the model's bookkeeping"""
    if name in SEL_LEFT_OUT:
        return
    if kw["selector"] == "eps_greedy":
        n = st["explore"] + st["greedy"] + st["eps_zero"]          # every selection is one of the three
        assert st["explore"] >= 0.1 * n and st["greedy"] + st["eps_zero"] >= 0.1 * n, st
    assert st["winner_ge_1"] >= 20 and st["ties_broken"] >= 5 and st["after_row_moved"] >= 1, st
    assert st["resets"] >= 1 and st["terminal"] >= 1, st           # the env's own terminal steps
    if kw["env"] != "blackjack":                                    # Blackjack has no max_steps
        assert st["truncated"] >= 1, st


def check_selection_case(obj, p, c, ln, q_mode=None, reset_step=False):
    kw = sel_kw(c)
    sel_prepare(obj, kw, q_mode, reset_step)
    if q_mode:
        assert obj.q_repr() == q_mode
    else:
        assert (obj.q_repr() == "fixed40") == (c in SEL_FIXED), obj.q_repr()
    st = predict_and_check(obj, p, kw, ln, reset_step=reset_step)
    assert_selection_live(st, kw, mc.case_id(c))
    return st


@pytest.mark.parametrize("c", SEL_MATRIX, ids=mc.case_id)
def test_oracle_records_equal_the_closed_loop(oracle, c):
    """Blackjack double-UCB runs here too (the device rejects it)"""
    p = oracle.default_params(**sel_kw(c))
    check_selection_case(oracle.Batch(p), p, c, oracle_ln(oracle))


@pytest.mark.parametrize("c", SEL_FIXED, ids=mc.case_id)
def test_oracle_records_equal_the_closed_loop_forced_f64(oracle, c):
    p = oracle.default_params(**sel_kw(c))
    check_selection_case(oracle.Batch(p), p, c, oracle_ln(oracle), q_mode="f64")


@pytest.mark.parametrize("c", SEL_EPS_GREEDY, ids=mc.case_id)
def test_oracle_records_equal_the_closed_loop_reset_step(oracle, c):
    p = oracle.default_params(**sel_kw(c))
    st = check_selection_case(oracle.Batch(p), p, c, oracle_ln(oracle), reset_step=True)
    assert st["resets"] >= p["n_lanes"]


# units beside the matrix: name -> (combination, parameters over sel_kw's, options,
# minima of the model's bookkeeping the unit is there for).
#   taxi-delivers-*: the start table is Taxi's undiscounted optimal action values
#     (integers, exact in both representations; value iteration over the model's own
#     table), max_steps 100 and eps0 0.125: greedy lanes deliver within the 16 steps
#     (the env's own terminal step, +20), under either selector (UCB from a flat count
#     of 9: the bonuses differ by less than the values' unit gaps);
#   bj-G512-rejects: one group of 512 and a ragged one of 388; 6 of 65536 halves are
#     rejected, about 3 over a 130-lane case and about 20 over this one;
#   one-lane: a single lane in a group of its own;
#   lane-offset: another seed and a lane offset.
SEL_UNITS = {
    "taxi-delivers-eps": (("taxi", "one_step", "tabular", "eps_greedy", "qlearning"),
                          dict(max_steps=100, eps0=0.125), dict(table="taxi_optimal"), dict(terminal=20)),
    "taxi-delivers-ucb": (("taxi", "one_step", "tabular", "ucb", "sarsa"),
                          dict(max_steps=100), dict(table="taxi_optimal", counts=9), dict(terminal=20)),
    "bj-G512-rejects": (("bj", "one_step", "tabular", "eps_greedy", "qlearning"),
                        dict(n_lanes=900, group_size=512), {}, dict(rejected_halves=1, terminal=900)),
    "one-lane": (("fl4-slip", "traces", "double", "eps_greedy", "expected_sarsa"),
                 dict(n_lanes=1, group_size=2), {}, dict(resets=2)),
    # the streams are keyed by the global lane id: lane_offset + lane
    "lane-offset": (("fle8-slip", "one_step", "tabular", "eps_greedy", "sarsa"),
                    dict(lane_offset=123457, seed=99), {}, dict(explore=200, terminal=1)),
}


def taxi_optimal_table():
    import select_model as selm
    obs, _ = selm.taxi_tables()
    v = [0.0] * 500
    for _ in range(40):                       # no state is more than 17 steps from its delivery
        q = [[r + (0.0 if term else v[s2]) for s2, r, term in row] for row in obs]
        v = [max(row) for row in q]
    return np.asarray(q, np.float64).reshape(1, 500, 6)


def check_selection_unit(obj, p, name, ln):
    c, over, opt, need = SEL_UNITS[name]
    kw = sel_kw(c, **over)
    sel_prepare(obj, kw)
    if opt.get("table") == "taxi_optimal":
        obj.set_q(taxi_optimal_table())
    if opt.get("counts"):
        obj.set_ucb(np.full((obj.S, obj.A), opt["counts"], np.uint64), np.uint64(5000))
    st = predict_and_check(obj, p, kw, ln)
    short = {k: (st[k], m) for k, m in need.items() if st[k] < m}
    assert not short, f"the unit no longer meets (got, needed): {short}"


@pytest.mark.parametrize("name", list(SEL_UNITS))
def test_oracle_unit_equals_the_closed_loop(oracle, name):
    c, over, _, _ = SEL_UNITS[name]
    p = oracle.default_params(**sel_kw(c, **over))
    check_selection_unit(oracle.Batch(p), p, name, oracle_ln(oracle))


# negative controls: a model with one rule switched must disagree with the oracle's
# records on a live case (mutation -> the cases it is tried on; every one must report)
SEL_MUTANTS = {
    "tie_last": [("cw", "one_step", "tabular", "eps_greedy", "qlearning"),
                 ("taxi", "traces", "double", "ucb", "sarsa")],
    "end_snapshot": [("fl8-slip-wide", "one_step", "tabular", "eps_greedy", "qlearning"),
                     ("taxi", "one_step", "double", "eps_greedy", "expected_sarsa")],
    "alpha_only": [("bj", "one_step", "double", "eps_greedy", "sarsa"),
                   ("fl4-slip", "traces", "double", "ucb", "qlearning")],
    "counters_incremented": [("taxi", "one_step", "tabular", "ucb", "sarsa"),
                             ("bj", "one_step", "double", "ucb", "expected_sarsa")],
    "eps_post_decay": [("bj", "one_step", "tabular", "eps_greedy", "qlearning"),
                       ("cw", "traces", "tabular", "eps_greedy", "sarsa")],
}


@pytest.mark.parametrize("mutation", list(SEL_MUTANTS))
def test_closed_loop_mutation_is_detected(oracle, mutation):
    import select_model as selm
    assert mutation in selm.MUTATIONS and set(SEL_MUTANTS) == set(selm.MUTATIONS)
    for c in SEL_MUTANTS[mutation]:
        kw = sel_kw(c)
        p = oracle.default_params(**kw)
        ref = oracle.Batch(p)
        sel_prepare(ref, kw)
        keep = []
        st = predict_and_check(ref, p, kw, oracle_ln(oracle), keep=keep)       # the true model agrees
        assert_selection_live(st, kw, mc.case_id(c))
        pr = sel_predictor(p, kw, mutation=mutation)
        lkw = sel_launch_kw(ref, p)
        flags = traces = last_eps = None
        eps = [p["eps0"]] * p["n_lanes"]
        found = []
        for q0, n0, t0, recs, table, rp in keep:
            rep, _, bad = selm.predict_launch(pr, q0, n0, t0, p["sync_every"], recorded=recs, repr=rp, flags=flags,
                                              eps=eps, traces=traces, last_eps=last_eps,
                                              ln=table.__getitem__, **lkw)
            flags, eps, traces, last_eps = rep.flags, rep.eps, rep.traces, rep.last_eps
            found += bad
        assert found, f"{mutation} goes unnoticed on {mc.case_id(c)}: the case is too weak"


# ---------------------------------------------------------------- hand-worked: the closed loop
# no oracle, no library: CliffWalking (no draws; 0 LEFT, 1 DOWN, 2 RIGHT, 3 UP; start 36
# in the bottom-left corner, where LEFT and DOWN stay in place), two identical lanes in
# one group, epsilon 0 (greedy, no draw) unless said otherwise, lr 0.5, gamma 0.5
class _Words:
    """a stream that hands out the given u32 words"""

    def __init__(self, *words):
        self.words, self.rejected_halves = list(words), 0

    def u32(self):
        return self.words.pop(0)

    def u64(self):
        lo = self.u32()
        return lo | (self.u32() << 32)

    def uniform01(self):
        return sm.f64_from_bits((self.u64() >> 12) | 0x3FF0000000000000) - 1.0


def _cliff(rows, K, *, P=1, lanes=2, max_steps=100, ucb=False, n_rows=None, ln=None, mutation=None):
    """rows: {(table, state): [4 values]} over a zero table; n_rows: {state: [4 counts]}"""
    import select_model as selm
    pr = selm.Predictor(env="cliff_walking", n_lanes=lanes, seed=1, max_steps=max_steps, ucb=ucb, ucb_c=1.0,
                        mutation=mutation)
    q = [0.0] * (P * 48 * 4)
    for (tbl, s), vals in rows.items():
        q[(tbl * 48 + s) * 4:(tbl * 48 + s) * 4 + 4] = vals
    n0 = [0] * (48 * 4)
    for s, vals in (n_rows or {}).items():
        n0[s * 4:s * 4 + 4] = vals
    rep, recs, _ = selm.predict_launch(pr, [sm.f64_word(v) for v in q], n0, 1, K, G=2, P=P, S=48, A=4, lr=0.5,
                                       gamma=0.5, algo="qlearning", repr="f64", eps=[0.0] * lanes, ln=ln)
    assert all(_fields(recs[k][0]) == _fields(recs[k][-1]) for k in range(K))      # identical lanes
    return rep, [r[0] for r in recs], pr


def _fields(rec, names=("kind", "s", "a", "s2", "a2", "r", "term")):
    return tuple(rec[n] for n in names)


def test_closed_loop_tie_at_1_and_3_takes_1_until_the_entry_moves():
    """row 36 = [1/8, 3/8, 1/4, 3/8]: the maximum is at 1 and 3, the first wins.
    k0 RESET: a = 1.  k1 DOWN stays at 36 (r -1); a2 reads the same snapshot: 1;
    td = -1 + 0.5 * 3/8 - 3/8 = -1.1875 and Q[36][1] = 3/8 - 0.59375 = -0.21875 (two equal
    contributions, their mean).  k2: the row is now [1/8, -0.21875, 1/4, 3/8], a2 = 3;
    td = -1 + 0.1875 + 0.21875 = -0.59375.  k3 UP moves to 24 (zero row): a2 = 0."""
    rep, recs, pr = _cliff({(0, 36): [0.125, 0.375, 0.25, 0.375]}, 4)
    assert [_fields(r) for r in recs] == [(1, 36, 1, 0, 0, 0.0, 0), (2, 36, 1, 36, 1, -1.0, 0),
                                          (2, 36, 1, 36, 3, -1.0, 0), (2, 36, 3, 24, 0, -1.0, 0)]
    assert [r["td"] for r in recs] == [0.0, -1.1875, -0.59375, -1.0 + 0.5 * 0.0 - 0.375]
    st = pr.totals()
    # ties: k0, k1 and k3's zero row 24, for each lane; k2 reads row 36 after it moved
    assert st["ties_broken"] == 2 * 3 and st["after_row_moved"] == 2 * 1
    # the last maximum instead: a = 3 at the reset already
    _, recs, _ = _cliff({(0, 36): [0.125, 0.375, 0.25, 0.375]}, 1, mutation="tie_last")
    assert _fields(recs[0])[:3] == (1, 36, 3)
    # reading the values after the step's updates: k1's a2 is 3 a step early
    _, recs, _ = _cliff({(0, 36): [0.125, 0.375, 0.25, 0.375]}, 2, mutation="end_snapshot")
    assert _fields(recs[1]) == (2, 36, 1, 36, 3, -1.0, 0)


def test_closed_loop_nan_at_0_wins_and_nan_at_2_never_does():
    import select_model as selm
    nan = float("nan")
    assert selm.argmax_first([nan, 5.0, 1.0, 7.0]) == (0, False)
    assert selm.argmax_first([0.25, 0.125, nan, 0.375]) == (3, False)
    assert selm.argmax_first([0.5, 0.125, nan, 0.375]) == (0, False)
    # through a launch: NaN at LEFT keeps the lane in the corner, td and the entry go NaN
    rep, recs, pr = _cliff({(0, 36): [nan, 5.0, 1.0, 7.0]}, 2)
    assert _fields(recs[0]) == (1, 36, 0, 0, 0, 0.0, 0) and _fields(recs[1])[:5] == (2, 36, 0, 36, 0)
    assert recs[1]["td"] != recs[1]["td"] and rep.words[36 * 4] == sm.QNAN_BITS
    # NaN at RIGHT: UP (7.0) wins; a UCB score of NaN at 0 wins the same way
    _, recs, _ = _cliff({(0, 36): [0.25, 5.0, nan, 7.0]}, 1)
    assert _fields(recs[0])[:3] == (1, 36, 3)
    assert selm.argmax_first(selm.ucb_scores([nan, 9.0], [1, 1], 4.0, 1.0)) == (0, False)


def test_closed_loop_double_policy_selects_on_the_average():
    """alpha[36] = [0, 0, 0, 3/8], beta[36] = [1/2, 0, 0, 0]: (alpha + beta) / 2 =
    [1/4, 0, 0, 3/16] picks LEFT; alpha alone picks UP"""
    rows = {(0, 36): [0.0, 0.0, 0.0, 0.375], (1, 36): [0.5, 0.0, 0.0, 0.0]}
    _, recs, _ = _cliff(rows, 2, P=2)
    assert _fields(recs[0]) == (1, 36, 0, 0, 0, 0.0, 0) and _fields(recs[1]) == (2, 36, 0, 36, 0, -1.0, 0)
    # the update reads alpha (flag true): td = -1 + 0.5 * 3/8 - 0 = -0.8125
    assert recs[1]["td"] == -0.8125
    _, recs, _ = _cliff(rows, 1, P=2, mutation="alpha_only")
    assert _fields(recs[0])[:3] == (1, 36, 3)


def test_closed_loop_ucb_reads_the_step_start_counters():
    """zero values, c = 1, ln(t) given as 4: N[36] = [1, 1, 4, 4] scores [2, 2, 1, 1]: both
    lanes of the group take LEFT (the first maximum) at the reset.  Had lane 1 read
    lane 0's increment, N = [2, 1, 4, 4] would score [1.41, 2, 1, 1]: DOWN.  After the
    step N[36][0] = 3 and t = 3; at k1 both read [3, 1, 4, 4] -> [1.15, 2, 1, 1]: DOWN."""
    import select_model as selm
    rep, recs, pr = _cliff({}, 2, ucb=True, n_rows={36: [1, 1, 4, 4]}, ln=lambda t: 4.0)
    assert _fields(recs[0]) == (1, 36, 0, 0, 0, 0.0, 0) and _fields(recs[1]) == (2, 36, 0, 36, 1, -1.0, 0)
    assert rep.n[36 * 4:36 * 4 + 4] == [3, 3, 4, 4] and rep.t == 5 and sorted(rep.ln_used) == [1, 3]
    pr = selm.Predictor(env="cliff_walking", n_lanes=2, seed=1, ucb=True, ucb_c=1.0, mutation="counters_incremented")
    n0 = [0] * 192
    n0[144:148] = [1, 1, 4, 4]
    _, recs, _ = selm.predict_launch(pr, [0] * 192, n0, 1, 1, G=2, P=1, S=48, A=4, lr=0.5, gamma=0.5,
                                     algo="qlearning", repr="f64", eps=[0.0, 0.0], ln=lambda t: 4.0)
    assert (recs[0][0]["a"], recs[0][1]["a"]) == (0, 1)


def test_card_word_with_a_rejected_high_half():
    """h = 6553: 6553 * 10 = 65530 > 65529 is rejected; the low half 0x8000 gives
    1 + (327680 >> 16) = 6, from the same word.  h = 6552: 65520, card 1; 0xffff: card 10."""
    import select_model as selm
    assert selm.card_of_half(6553) == (1, True) and selm.card_of_half(6552) == (1, False)
    assert selm.card_of_half(0x8000) == (6, False) and selm.card_of_half(0xFFFF) == (10, False)
    assert sum(selm.card_of_half(h)[1] for h in range(1 << 16)) == 6
    rng = _Words((6553 << 16) | 0x8000, 0xDEAD0000)
    src = selm.CardSource(rng)
    assert src.card() == 6 and rng.rejected_halves == 1 and rng.words == [0xDEAD0000]    # one word for the hit
    # a deal whose first word's high half is rejected needs a third word: cards 6 | 1, 10 | 4, a half left over
    rng = _Words((6553 << 16) | 0x8000, (0 << 16) | 0xFFFF, (0x6666 << 16) | 0x1234, 7)
    env = selm.Blackjack.__new__(selm.Blackjack)
    env.n_trunc = 0
    assert env.reset(rng) == selm.bj_index(17, 10, True) and rng.words == [7]      # 6 + ace = 17, dealer shows 10
    # a hit takes its own word: the half left over by the deal is gone
    rng.words = [(0x4000 << 16) | 0, 8]
    assert env.step(0, rng) == (selm.bj_index(20, 10, True), 0.0, False) and rng.words == [8]   # 0x4000: card 3, soft 20


def test_taxi_reset_above_the_last_running_sum_is_cell_0():
    """300 start probabilities of 1/300 sum to 0.9999999999999961 in order; uniform01's
    largest value 1 - 2^-52 is above it, no running sum exceeds it and the all-false
    argmax gives cell 0, which is no start state (passenger at its destination)"""
    import select_model as selm
    env = selm.Taxi(6)
    acc = 0.0
    for v in env.start:
        acc += v
    assert acc == 0.9999999999999961 and env.start[0] == 0.0 and sum(1 for v in env.start if v) == 300
    assert env.reset(_Words(0xFFFFFFFF, 0xFFFFFFFF)) == 0
    below = _Words(0, 0xFFFFFFFF - (1 << 12))             # u = 1 - 2^-20 - ..: below the last sum
    assert below.uniform01() < acc
    # the last start state: taxi (4, 4), passenger at 3, destination 2
    assert env.reset(_Words(0, 0xFFFFFFFF - (1 << 12))) == ((4 * 5 + 4) * 5 + 3) * 4 + 2 == 494


def test_closed_loop_truncates_on_the_step_after_max_steps():
    """max_steps 2, UP preferred at 36 and 24: k0 RESET, k1 36 -> 24, k2 24 -> 12 (the
    last allowed step), k3 is asked of an env at curr_step 2 = max_steps: (0, -100.0,
    term) without moving, and the selection reads row 0; k4 RESET"""
    rows = {(0, 36): [0.0, 0.0, 0.0, 1.0], (0, 24): [0.0, 0.0, 0.0, 1.0], (0, 0): [0.0, 0.0, 2.0, 0.0]}
    rep, recs, pr = _cliff(rows, 5, max_steps=2)
    assert [_fields(r) for r in recs] == [(1, 36, 3, 0, 0, 0.0, 0), (2, 36, 3, 24, 3, -1.0, 0),
                                          (2, 24, 3, 12, 0, -1.0, 0), (2, 12, 0, 0, 2, -100.0, 1),
                                          (1, 36, 3, 0, 0, 0.0, 0)]
    assert recs[3]["td"] == -100.0 + 0.5 * 2.0 - 0.0
    st = pr.totals()
    assert st["truncated"] == 2 and st["terminal"] == 0 and st["resets"] == 4


def test_closed_loop_model_imports_neither_oracle_nor_library():
    import ast
    import select_model as selm
    names = set()
    for node in ast.walk(ast.parse(open(selm.__file__).read())):
        if isinstance(node, ast.Import):
            names |= {a.name.split(".")[0] for a in node.names}
        elif isinstance(node, ast.ImportFrom):
            names.add((node.module or "").split(".")[0])
    assert names == {"golden", "maps_model", "step_model"}, names


def test_closed_loop_tables_equal_the_fixture():
    """the Taxi and CliffWalking tables restated in select_model against
    tests/golden/tables.json (an independent restatement of its own)"""
    import json
    import os
    import select_model as selm
    tables = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "tables.json")))
    obs, start = selm.taxi_tables()
    for name, obs, start in (("taxi", obs, start),
                             ("cliff_walking", selm.CliffWalking(100).obs, [float(i == 36) for i in range(48)])):
        t = tables[name]
        assert start == t["start"]
        for s, row in enumerate(obs):
            for a, (s2, r, term) in enumerate(row):
                assert (t["prob"][s][a][0], t["next"][s][a][0], t["reward"][s][a][0], bool(t["term"][s][a][0])) == \
                       (1.0, s2, r, term), (name, s, a)

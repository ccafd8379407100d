"""The shared-Q step combine and launch merge against an exact replay model.

tests/step_model.py restates DESIGN.md section 2 (step combine, merge, fixed
point, UCB counters) with Python ints and Fractions and replays one launch from
its rl_step_record entries.  Here the CPU oracle (oracle/rlref.c rlo_batch_*) is
driven launch by launch and must equal the model in every raw Q word and UCB
counter; tests/test_gpu_step_model.py drives the device through the same
helper.  The accuracy rows state what "summed exactly on the grid" promises
against the exact rational mean, and the coverage conditions keep every case on
the edge it was built for (they are asserted, not reported).
"""
import math

import numpy as np
import pytest

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


def replay_and_check(obj, p, launch, *, launches=LAUNCHES, merge_groups=0):
    """Run `launches` launches on obj (an oracle Batch or a device Agent, recording
    on), replay each from its records and assert the model's words and counters
    equal obj's, the recomputed td equal the recorded ones and the accuracy rows
    hold.  Returns the coverage conditions met over all launches."""
    S, A, P = obj.S, obj.A, obj.P
    ucb = p["selector"] == "ucb"
    flags = None                       # every lane's double-policy flag starts true
    met = {}
    for li in range(launches):
        q0 = obj.q_raw().reshape(-1).tolist()
        n0, t0 = obj.ucb()
        n0 = np.asarray(n0).reshape(-1).tolist()
        launch()
        recs = obj.records()
        assert recs.shape == (p["sync_every"], p["n_lanes"])
        rep = sm.replay_launch(q0, n0, int(t0), _records_as_dicts(recs), G=p["group_size"], P=P, S=S, A=A,
                               lr=p["lr"], gamma=p["gamma"], algo=p["algo"], repr=obj.q_repr(),
                               merge_groups=merge_groups, ucb=ucb, flags=flags, agent=p["agent"])
        flags = rep.flags
        assert not rep.td_mismatches, f"launch {li}: td recomputed != recorded: {rep.td_mismatches[:5]}"
        nbad, bad = _first_diffs(obj.q_raw().reshape(-1).tolist(), rep.words)
        assert nbad == 0, f"launch {li}: {nbad} Q words differ (entry, got, model): {bad}"
        n1, t1 = obj.ucb()
        assert np.asarray(n1).reshape(-1).tolist() == rep.n and int(t1) == rep.t, f"launch {li}: UCB counters"
        for name, rows in (("step", sm.step_accuracy(rep)), ("merge", sm.merge_accuracy(rep))):
            worst = [r for r in rows if not r[3]]
            assert not worst, f"launch {li}: {name} accuracy bound missed (mean, got, bound): " \
                              f"{[(float(m), float(g), float(b)) for m, g, b, _ in worst[:3]]}"
        for k, v in sm.coverage(rep).items():
            met[k] = met.get(k, False) or v
        met["kind3"] = met.get("kind3", False) or bool((recs["kind"] == 3).any())
        if merge_groups and sm.headroom(merge_groups):
            # the same launch merged without headroom must differ somewhere, or the
            # headroom bits were never visible in this case
            plain = sm.replay_launch(q0, n0, int(t0), _records_as_dicts(recs), G=p["group_size"], P=P, S=S,
                                     A=A, lr=p["lr"], gamma=p["gamma"], algo=p["algo"], repr=obj.q_repr(),
                                     merge_groups=0, ucb=ucb, flags=None, agent=p["agent"]) if P == 1 else None
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
def test_model_refuses_traces():
    with pytest.raises(NotImplementedError, match="traces"):
        sm.replay_launch([0] * 4, [0] * 4, 1, [], G=2, P=1, S=2, A=2, lr=0.1, gamma=0.9, algo="sarsa",
                         repr="f64", agent="traces")


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


def _rec(kind=2, s=0, a=0, s2=1, a2=0, r=0.0, td=0.0, mode=0):
    return dict(kind=kind, s=s, a=a, s2=s2, a2=a2, r=r, td=td, mode=mode, term=0)


def _replay_td(tds, lr=1.0, base=0.0, **kw):
    """G lanes each contributing lr * td to entry (0, 0) in one step (expected
    SARSA takes the recorded td as its input)"""
    words = [sm.f64_word(base), 0, 0, 0]
    return sm.replay_launch(words, [0] * 4, 1, [[_rec(td=t) for t in tds]], G=max(2, len(tds)), P=1, S=2, A=2,
                            lr=lr, gamma=0.5, algo="expected_sarsa", repr="f64", **kw)


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

"""CPU: the map sets of tests/population_map_cases.py are live, so that the device
cases of tests/test_gpu_population_maps.py cannot pass on dead inputs.

Asserted through maps_model.predict_records (epsilon pinned at 1, one seed for all
members, 80 lanes, 32 synchronous steps — 4 launches of K = 8 — max_steps 12), for
every set and both slippery settings: every start cell of every map is drawn at least
100 times, every member falls into holes (>= 70) and is truncated (>= 18), the goal is
reached where the set says so, every member visits >= 31 distinct (s, a) pairs, and
the members' records differ pairwise — except the pair that is one env (id 0 and the
map without an 'S'), whose records are equal.
"""
import pytest

import maps_model as mm
import population_map_cases as pmc

STEPS = pmc.LAUNCHES * pmc.K


@pytest.fixture(scope="module")
def predicted():
    """(set, slippery) -> {member name: (records, (start counts, totals))}, computed once"""
    out = {}
    for name, members in pmc.SETS.items():
        for slip in (0, 1):
            d = {}
            for mname, rows, _ in members:
                recs, envs = mm.predict_records(lambda: mm.make_env("frozen_lake", rows, slip, pmc.MAX_STEPS),
                                                pmc.SEED, pmc.G, STEPS)
                d[mname] = (recs, mm.coverage(envs))
            out[name, slip] = d
    return out


CASES = [(name, slip) for name in pmc.SETS for slip in (0, 1)]


@pytest.mark.parametrize("name,slip", CASES, ids=[f"{n}-{'slippery' if s else 'det'}" for n, s in CASES])
def test_every_member_of_the_set_is_live(predicted, name, slip):
    d = predicted[name, slip]
    for mname, rows, _ in pmc.SETS[name]:
        recs, (starts, tot) = d[mname]
        for cell in pmc.start_cells(rows):
            assert starts.get(cell, 0) >= pmc.NEED["start_draws"], (mname, cell, starts)
        assert set(starts) == set(pmc.start_cells(rows)), (mname, starts)
        assert tot["hole"] >= pmc.NEED["holes"], (mname, tot)
        assert tot["trunc"] >= pmc.NEED["truncations"], (mname, tot)
        if mname in pmc.REACH_GOAL[name]:
            assert tot["goal"] >= 1, (mname, tot)
        pairs = {(r[1], r[2]) for step in recs for r in step if r[0] == 2}
        assert len(pairs) >= pmc.NEED["pairs"], (mname, len(pairs))


@pytest.mark.parametrize("name,slip", CASES, ids=[f"{n}-{'slippery' if s else 'det'}" for n, s in CASES])
def test_members_part_on_their_maps_alone(predicted, name, slip):
    d = predicted[name, slip]
    names = [m[0] for m in pmc.SETS[name]]
    same = {frozenset(p) for p in pmc.SAME_ENV.get(name, [])}
    for i, a in enumerate(names):
        for b in names[:i]:
            if frozenset((a, b)) in same:
                assert d[a][0] == d[b][0], f"{a} and {b} are one env"
            else:
                assert d[a][0] != d[b][0], f"{a} and {b} see the same records"


def test_the_set_shapes_are_what_the_device_cases_assume():
    for name, (nrow, ncol) in (("Q4", (4, 4)), ("R25", (2, 5)), ("W10", (10, 10))):
        for _, rows, _ in pmc.SETS[name]:
            assert len(rows) == nrow and all(len(r) == ncol for r in rows)
            assert "".join(rows).count("G") == 1
    assert pmc.start_cells(pmc.W10_ONE) == [55] and pmc.start_cells(pmc.W10_TWO) == [9, 44]
    assert pmc.start_cells(pmc.Q4_MID) == [10] and pmc.start_cells(pmc.Q4_NO_S) == [0]
    assert len(pmc.start_cells(pmc.Q4_THREE)) == 3 and len(pmc.start_cells(mm.MAP_A)) == 2
    assert len(pmc.TEN) == 10

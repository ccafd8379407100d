#!/usr/bin/env python3
"""What a population buys: a sweep of M shared-Q agents as one launch per K steps
against the same M agents as lone handles.

In one process, alternating per repeat (other work shares the host, so a difference
is only trusted when it holds in every alternated repeat):
  (a) a population of M members x G lanes                 (rl_population_create)
  (b) the same M members as M lone agents of G lanes      (rl_agent_create each), as a
      sweep is run today: b_streams queues every agent's launches on the agent's own
      stream, one agent after another, and waits once at the end (whatever overlap the
      runtime's hardware queues give is (b)'s to keep); b_serial waits for each agent
      before it starts the next
  (c) one shared agent of M * G lanes in groups of G — the default kernel, for
      orientation only: it learns ONE table, so it is not the same work
Before timing, (a)'s member tables are checked equal to (b)'s.

Every window is warmed up, ends in a device synchronise and lasts at least
--seconds of launches; the rate is env steps (rl_stats.train_steps) over the host
clock around it; the library's HIP-event time of the train kernels alone
(rl_agent_set_timing) comes from one more window of the same length per form.
Prints one JSON document; --out writes it to a file as well.  Needs a GPU: there is
no fallback.

--maps times what a map of the member's own costs (rl_population_create_maps), the
same way:
  (a) the map population with every member on a registered copy of the built-in 8x8
  (b) the built-in population of the same members (rl_population_create, map8x8 = 1):
      the same work, so a / b is the cost of the map path
  (c) the same members as lone map agents on their own streams
and adds (d), one window series of a map population over M distinct random 8x8 lakes
(--random-seed; one 'S' and one 'G' each, a fifth of the other cells holes).  Before
timing, (a)'s member tables are checked equal to (b)'s and (c)'s.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rl-rust_amd"))

import numpy as np  # noqa: E402

import rlamd  # noqa: E402


def _steps(h):
    return h.stats()["train_steps"]


class PopulationRun:
    name = "a_population"

    def __init__(self, base, members, maps=None, name=None):
        self.pop = rlamd.Population(base, members, maps=maps)
        if name:
            self.name = name

    def round(self, n):
        self.pop.run(n)
        self.pop.synchronize()

    def steps(self):
        return _steps(self.pop)

    def set_timing(self, on):
        self.pop.set_timing(on)

    def event_ms(self):
        return self.pop.timing()


class LoneRun:
    """M lone agents; serial: wait for each agent before the next starts"""

    def __init__(self, agents, serial, name=None):
        self.agents = agents
        self.serial = serial
        self.name = name or ("b_serial" if serial else "b_streams")

    def round(self, n):
        for a in self.agents:
            a.run(n)
            if self.serial:
                a.synchronize()
        if not self.serial:
            for a in self.agents:
                a.synchronize()

    def steps(self):
        return sum(_steps(a) for a in self.agents)

    def set_timing(self, on):
        for a in self.agents:
            a.set_timing(on)

    def event_ms(self):
        ms = cnt = 0
        for a in self.agents:
            m, c = a.timing()
            ms += m
            cnt += c
        return ms, cnt


class SharedRun:
    name = "c_one_shared_agent"

    def __init__(self, p):
        self.a = rlamd.Agent(p)

    def round(self, n):
        self.a.run(n)
        self.a.synchronize()

    def steps(self):
        return _steps(self.a)

    def set_timing(self, on):
        self.a.set_timing(on)

    def event_ms(self):
        return self.a.timing()


def window(run, n):
    """n launches per handle, ended by a synchronise, under the host clock (events off:
    two event records per launch would weigh on the lone agents' many launches)"""
    s0 = run.steps()
    t0 = time.perf_counter()
    run.round(n)
    dt = time.perf_counter() - t0
    return dict(launches_per_handle=n, seconds=dt, env_steps=run.steps() - s0,
                env_steps_per_s=(run.steps() - s0) / dt)


def event_window(run, n):
    """the same window with the library's HIP events around every train kernel: their
    summed time (kernels only: neither the lone agents' merge launches nor the gaps)"""
    run.set_timing(True)
    run.round(n)
    ms, cnt = run.event_ms()
    run.set_timing(False)
    return dict(train_kernel_event_ms=ms, train_kernels=cnt, ms_per_train_kernel=ms / max(cnt, 1))


def random_lake(rng, n=8, holes=0.2):
    """n x n rows: 'S' and 'G' on two distinct random cells, `holes` of the rest 'H'"""
    cells = np.where(rng.random(n * n) < holes, "H", "F")
    s, g = rng.choice(n * n, size=2, replace=False)
    cells[s], cells[g] = "S", "G"
    return ["".join(cells[r * n:(r + 1) * n]) for r in range(n)]


def measure(runs, args):
    """warm-up, window lengths for at least --seconds, then the alternated repeats"""
    n = {}
    for r in runs:
        r.round(2)
        w = window(r, 4)
        n[r.name] = max(4, int(np.ceil(4 * args.seconds / w["seconds"] * 1.1)))
    reps = []
    for i in range(args.repeats):
        reps.append({r.name: window(r, n[r.name]) for r in runs})
    rates = {k: [rep[k]["env_steps_per_s"] for rep in reps] for k in reps[0]}
    return reps, rates


def spread(v):
    return dict(median=float(np.median(v)), min=min(v), max=max(v))


def main_maps(args):
    M, G = args.members, args.group
    base = rlamd.default_params(env="frozen_lake", map8x8=1, algo="qlearning", group_size=G, n_lanes=G,
                                sync_every=args.sync)
    members = [dict(seed=0x5EED + m, lane_offset=m * G) for m in range(M)]
    copy = rlamd.register_map(rlamd.map_info(1))
    a = PopulationRun(base, members, maps=[copy] * M, name="a_map_population")
    b = PopulationRun(base, members, name="b_builtin_population")
    agents = [rlamd.Agent(dict(a.pop.members[m], n_lanes=G, group_size=G, map8x8=copy)) for m in range(M)]
    a.round(2)
    b.round(2)
    raw = a.pop.q_raw()
    if not np.array_equal(raw, b.pop.q_raw()):
        raise SystemExit("the map population's tables differ from the built-in population's")
    for m, ag in enumerate(agents):
        ag.run(2)
        if not np.array_equal(raw[m], ag.q_raw()):
            raise SystemExit(f"member {m}: the map population's table differs from the lone map agent's")
    runs = [a, b, LoneRun(agents, serial=False, name="c_lone_map_agents")]
    reps, rates = measure(runs, args)
    rng = np.random.default_rng(args.random_seed)
    lakes = [random_lake(rng) for _ in range(M)]
    d = PopulationRun(base, members, maps=lakes, name="d_distinct_random_maps")
    d_reps, d_rates = measure([d], args)
    out = dict(
        mode="maps", build_id=rlamd.build_id(), members=M, lanes_per_member=G, sync_every=args.sync,
        q_repr=a.pop.q_repr(), occupancy=dict(a=a.pop.occupancy(), b=b.pop.occupancy(), d=d.pop.occupancy()),
        tables_equal_before_timing=True, repeats=reps,
        env_steps_per_s={k: spread(v) for k, v in rates.items()},
        a_over_b=[x / y for x, y in zip(rates["a_map_population"], rates["b_builtin_population"])],
        a_over_c=[x / y for x, y in zip(rates["a_map_population"], rates["c_lone_map_agents"])],
        distinct_random_maps=dict(n_distinct=len(set(d.pop.maps().tolist())), random_seed=args.random_seed,
                                  repeats=d_reps, env_steps_per_s=spread(d_rates[d.name])),
    )
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--members", type=int, default=256)
    ap.add_argument("--group", type=int, default=512)
    ap.add_argument("--sync", type=int, default=64, help="K: synchronous steps per launch")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=1.0, help="least length of a timed window")
    ap.add_argument("--out", default=None)
    ap.add_argument("--maps", action="store_true", help="time the map population (rl_population_create_maps)")
    ap.add_argument("--random-seed", type=int, default=2026, help="--maps: seed of the distinct random lakes")
    args = ap.parse_args()
    if args.maps:
        return main_maps(args)
    M, G = args.members, args.group

    base = rlamd.default_params(env="frozen_lake", map8x8=1, algo="qlearning", group_size=G, n_lanes=G,
                                sync_every=args.sync)
    members = [dict(seed=0x5EED + m, lane_offset=m * G) for m in range(M)]
    a = PopulationRun(base, members)
    agents = [rlamd.Agent(dict(a.pop.members[m], n_lanes=G, group_size=G)) for m in range(M)]
    # (a) == (b) before anything is timed: same words after the same launches
    a.round(2)
    raw = a.pop.q_raw()
    for m, ag in enumerate(agents):
        ag.run(2)
        if not np.array_equal(raw[m], ag.q_raw()):
            raise SystemExit(f"member {m}: the population's table differs from the lone agent's")
    runs = [a, LoneRun(agents, serial=False), LoneRun(agents, serial=True),
            SharedRun(dict(base, n_lanes=M * G))]
    # warm-up and window length: launches per handle for at least --seconds
    n = {}
    for r in runs:
        r.round(2)
        w = window(r, 4)
        n[r.name] = max(4, int(np.ceil(4 * args.seconds / w["seconds"] * 1.1)))
    reps = []
    for i in range(args.repeats):
        rep = {}
        for r in runs:                 # alternating a, b, b, c within every repeat
            rep[r.name] = window(r, n[r.name])
        reps.append(rep)
    events = {r.name: event_window(r, n[r.name]) for r in runs}
    rates = {k: [rep[k]["env_steps_per_s"] for rep in reps] for k in reps[0]}
    out = dict(
        build_id=rlamd.build_id(), members=M, lanes_per_member=G, sync_every=args.sync,
        q_repr=a.pop.q_repr(), occupancy=a.pop.occupancy(), member_tables_equal_lone_agents=True,
        repeats=reps, train_kernel_events=events,
        env_steps_per_s={k: dict(median=float(np.median(v)), min=min(v), max=max(v)) for k, v in rates.items()},
        a_over_b_streams=[x / y for x, y in zip(rates["a_population"], rates["b_streams"])],
        a_over_b_serial=[x / y for x, y in zip(rates["a_population"], rates["b_serial"])],
        a_over_c=[x / y for x, y in zip(rates["a_population"], rates["c_one_shared_agent"])],
    )
    out["a_faster_than_b_in_every_repeat"] = bool(min(out["a_over_b_streams"]) > 1.0 and
                                                  min(out["a_over_b_serial"]) > 1.0)
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0 if out["a_faster_than_b_in_every_repeat"] else 1


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""A parent commit's librlamd.so against this checkout's (profiles/host_refactor.md):
bench.py --config 2..7, the two libraries alternating (and the order inside a pair
alternating: the second run follows a warmer GPU), three repeats each, every run a
fresh process under its own time limit, the library chosen with RLAMD_LIB.  The first
repeat of each runs --full (q_check / the private-row checks).  Stops at the first
failing run.  The bar: per configuration the new median is no lower than the parent's
lowest repeat, q_check and the launch shape are equal.
  python scripts/ab_libs.py PARENT_LIB [2,3,4,5,6,7]      (writes out/ab_*.json*)"""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, os.environ.get("OUT", "out"))
os.makedirs(OUT, exist_ok=True)
LIBS = {"parent": os.path.abspath(sys.argv[1]),
        "new": os.path.join(ROOT, "rl-rust_amd", "lib", "librlamd.so")}
CONFIGS = [int(c) for c in (sys.argv[2] if len(sys.argv) > 2 else "2,3,4,5,6,7").split(",")]
REPS = 3
res = {}
log = open(os.path.join(OUT, "ab_runs.jsonl"), "a")
for cfg in CONFIGS:
    for rep in range(REPS):
        for which in (("parent", "new") if rep % 2 == 0 else ("new", "parent")):
            cmd = ["timeout", "-k", "10", "400" if rep == 0 else "200", sys.executable, "-u", "bench.py",
                   "--gpus", "1", "--config", str(cfg)]
            if rep == 0:
                cmd += ["--full", "--no-cpu-baseline"]
            env = dict(os.environ, RLAMD_LIB=LIBS[which])
            r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True)
            lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
            if r.returncode != 0 or not lines or "illegal memory access" in r.stderr:
                print(f"cfg{cfg} rep{rep} {which}: rc={r.returncode}\n{r.stdout[-1500:]}\n{r.stderr[-3000:]}", flush=True)
                sys.exit(1)   # nothing more on the GPU after a failed run
            d = json.loads(lines[-1])
            rec = {"cfg": cfg, "rep": rep, "lib": which, "value": d["value"], "ms_per_step": d["ms_per_step"],
                   "q_check": d.get("q_check"), "build_id": d.get("build_id"),
                   "groups_per_cu": d["config"]["groups_per_cu"], "lds": d["config"]["lds_bytes_per_group"],
                   "q_repr": d["config"]["q_repr"]}
            log.write(json.dumps(rec) + "\n")
            log.flush()
            res.setdefault((cfg, which), []).append(rec)
            qc = rec["q_check"]
            print(f"cfg{cfg} rep{rep} {which:6s} {d['value']:.5g} env-steps/s  q_check "
                  f"{json.dumps(qc)[:200] if qc else None}", flush=True)
ok = True
summary = []
for cfg in CONFIGS:
    p = [x["value"] for x in res[(cfg, "parent")]]
    n = [x["value"] for x in res[(cfg, "new")]]
    row = {"cfg": cfg, "parent_median": statistics.median(p), "parent_min": min(p), "parent_max": max(p),
           "new_median": statistics.median(n), "new_min": min(n), "new_max": max(n),
           "pass": statistics.median(n) >= min(p),
           "q_check_parent": res[(cfg, "parent")][0]["q_check"], "q_check_new": res[(cfg, "new")][0]["q_check"],
           "same_q_check": res[(cfg, "parent")][0]["q_check"] == res[(cfg, "new")][0]["q_check"],
           "same_launch_shape": all(res[(cfg, "parent")][0][k] == res[(cfg, "new")][0][k]
                                    for k in ("groups_per_cu", "lds", "q_repr"))}
    ok = ok and row["pass"] and row["same_q_check"] and row["same_launch_shape"]
    summary.append(row)
    print(json.dumps(row), flush=True)
json.dump(summary, open(os.path.join(OUT, "ab_summary.json"), "w"), indent=1)
print("AB", "PASS" if ok else "FAIL", flush=True)
sys.exit(0 if ok else 2)

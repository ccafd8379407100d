"""GPU: a plain bench.py run prints the headline line without the --full extras, and
--dump-outputs writes what its last timed step left: the same Q, lane states and
counters as the same launches made here through rlamd (lanes are seeded by their
global id, so a run's inputs are a function of its arguments)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LANES, STEPS, WARMUP = 3 * 512, 3, 1      # three learner groups of cfg 2's 512 lanes


def _bench(*extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS),
                        "--warmup", str(WARMUP), "--lanes", str(LANES), *extra],
                       cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return lines[0]


def test_plain_run_dumps_the_last_steps_outputs(rl, tmp_path):
    d = _bench("--dump-outputs", str(tmp_path / "o"))
    assert d["steps"] == STEPS and d["ms_per_step"] > 0 and d["value"] > 0 and d["unit"] == "env-steps/s"
    assert abs(d["ms_per_step"] * STEPS / 1e3 - d["timing"]["wall_s"]) < 1e-9
    assert d["q_check"] is None and "cpu_baseline" not in d
    got = {f[:-4]: np.load(tmp_path / "o" / f) for f in sorted(os.listdir(tmp_path / "o"))}
    assert sorted(got) == ["lane_ids", "lane_state", "q", "stats"]
    assert all(a.dtype == np.float64 for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 << 20

    p = rl.default_params(env="frozen_lake", map8x8=1, n_lanes=LANES, group_size=512, sync_every=64)
    a = rl.Agent(p)
    a.run(WARMUP + STEPS)
    a.synchronize()
    core, aux = a.lane_state()
    st = a.stats()
    assert np.array_equal(got["q"], a.q()) and np.any(got["q"] != 0)
    assert np.array_equal(got["lane_ids"], np.arange(LANES))
    assert np.array_equal(got["lane_state"], np.concatenate([core, aux], axis=1).astype(np.float64))
    assert np.array_equal(got["stats"], np.array([st[k] for k, _ in rl.Stats._fields_], np.float64))
    assert st["train_steps"] > 0
    a.close()


def test_full_run_adds_the_q_check():
    d = _bench("--full", "--no-cpu-baseline")
    assert d["q_check"]["ranks_agree"] is True and len(d["q_check"]["q_sha256"]) == 64
    assert "cpu_baseline" not in d

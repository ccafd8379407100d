"""The device's shared-Q step combine and launch merge against the exact replay
model (tests/step_model.py): the cases, tables and helper of
tests/test_step_model.py, driven on rl.Agent instead of the CPU oracle.

Every launch is replayed from the device's own rl_step_record entries: the
model's raw Q words, UCB counters and per-lane epsilon must equal the device's,
every td recomputed from the group's step-start snapshot must equal the recorded
one (expected SARSA's with the device's own log, rl_kat_log, checked against a
50-digit logarithm), and the coverage conditions must hold on the device's
records.  The traces and expected-SARSA combinations of the parity matrix and the
edge cases run here as they do on the oracle.  No oracle call is made here, so a
mistake shared by the oracle and the kernels cannot hide.

The closed loop (tests/select_model.py) takes the records off the input side as
well: every record field of every lane and step is predicted from the seed and
the state before the launch, and the device's records, td, Q words, N, t and
epsilon must equal the prediction.  All shared combinations of the parity matrix
the device accepts run it (234 of 240; the registered-map and wide variants put
fl_advance and fl_advance_wide on the path), the fixed-point ones once more in
f64, the eps-greedy ones once more with the reset-and-step schedule, plus the
units: Taxi deliveries, a group of 512 with rejected card halves, a single lane.
"""
import ctypes as C

import numpy as np
import pytest

import matrix_cases as mc
from test_step_model import (CASES, COMMON, EDGE_CASES, EDGE_COMMON, HEADROOM_CASE, MATRIX, MATRIX_FIXED, ONE_LANE,
                             SEL_EPS_GREEDY, SEL_FIXED, SEL_MATRIX, SEL_UNITS, assert_coverage, check_edge_case,
                             check_matrix_case, check_selection_case, check_selection_unit, crafted_table,
                             one_lane_plain_update, replay_and_check, sel_kw, setup_pair)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(CASES))
def test_device_equals_replay_model(rl, name):
    kw, opt = CASES[name]
    p = rl.default_params(**COMMON, **kw)
    dev = rl.Agent(p)
    try:
        setup_pair(dev, p, opt, (dev.P, dev.S, dev.A))
        met = replay_and_check(dev, p, lambda: dev.run(1))
        assert_coverage(met, opt["need"])
        if opt.get("table", ("", 0))[0] == "d":
            want = crafted_table(*opt["table"], dev.P, dev.S, dev.A)
            assert np.array_equal(dev.q(), want), "a move too small to change an entry changed the merged table"
    finally:
        dev.close()


def test_device_headroom_equals_replay_model(rl):
    """4096 declared learner groups (2 headroom bits) through the external-collective
    path: caller-owned merge buffer, launch_train / launch_fold / launch_apply; one
    rank, so the collectives are the identity"""
    kw, opt = HEADROOM_CASE
    p = rl.default_params(**COMMON, **kw)
    # device memory from the HIP runtime librlamd itself is linked to
    hip = C.CDLL("libamdhip64.so")
    dev = rl.Agent(p)
    buf = C.c_void_p()
    try:
        setup_pair(dev, p, opt, (dev.P, dev.S, dev.A))
        cap = dev.delta_cap_words()
        assert cap >= dev.delta_words()
        assert hip.hipMalloc(C.byref(buf), C.c_size_t(cap * 8)) == 0
        assert hip.hipMemset(buf, 0, C.c_size_t(cap * 8)) == 0
        dev.set_delta_buffer(buf.value, cap)
        dev.set_merge_groups(opt["merge_groups"])

        def launch():
            dev.launch_train()
            dev.launch_fold()
            dev.launch_apply()
            dev.synchronize()

        met = replay_and_check(dev, p, launch, merge_groups=opt["merge_groups"])
        assert_coverage(met, opt["need"])
    finally:
        dev.close()
        if buf.value:
            hip.hipFree(buf)


@pytest.mark.parametrize("name", list(ONE_LANE))
def test_device_one_lane_is_plain_update(rl, name):
    p = rl.default_params(n_lanes=1, group_size=2, **COMMON, **ONE_LANE[name])
    dev = rl.Agent(p)
    try:
        dev.set_q_mode("f64")
        dev.set_recording(True)
        one_lane_plain_update(dev, p)
    finally:
        dev.close()


# ---------------------------------------------------------------- traces and expected SARSA
# Blackjack's double policy under UCB does not fit a learner group's LDS
# (matrix_cases.shared_rejected; tests/test_gpu_matrix.py asserts the rejection)
DEVICE_MATRIX = [c for c in MATRIX if not mc.shared_rejected(c)]
assert len(DEVICE_MATRIX) == 156         # four of the six rejected combinations are among the 160


def device_ln(rl):
    return lambda ts: rl.kat_log(np.asarray(ts, np.float64)).tolist()


@pytest.mark.parametrize("c", DEVICE_MATRIX, ids=mc.case_id)
def test_device_matrix_case_equals_replay_model(rl, c):
    p = mc.device_params(rl, mc.shared_kw(c), c)
    dev = rl.Agent(p)
    try:
        check_matrix_case(dev, p, c, device_ln(rl))
    finally:
        dev.close()


@pytest.mark.parametrize("c", MATRIX_FIXED, ids=mc.case_id)
def test_device_matrix_case_forced_f64_equals_replay_model(rl, c):
    p = mc.device_params(rl, mc.shared_kw(c), c)
    dev = rl.Agent(p)
    try:
        check_matrix_case(dev, p, c, device_ln(rl), q_mode="f64")
    finally:
        dev.close()


@pytest.mark.parametrize("name", list(EDGE_CASES))
def test_device_edge_case_equals_replay_model(rl, name):
    p = rl.default_params(**EDGE_COMMON, **EDGE_CASES[name][0])
    dev = rl.Agent(p)
    try:
        check_edge_case(dev, p, name, device_ln(rl))
    finally:
        dev.close()


# ---------------------------------------------------------------- the closed loop: records from the seed
DEVICE_SEL = [c for c in SEL_MATRIX if not mc.shared_rejected(c)]
assert len(DEVICE_SEL) == 234 and not any(mc.shared_rejected(c) for c in SEL_EPS_GREEDY + SEL_FIXED)


@pytest.mark.parametrize("c", DEVICE_SEL, ids=mc.case_id)
def test_device_records_equal_the_closed_loop(rl, c):
    p = mc.device_params(rl, sel_kw(c), c)
    dev = rl.Agent(p)
    try:
        check_selection_case(dev, p, c, device_ln(rl))
    finally:
        dev.close()


@pytest.mark.parametrize("c", SEL_FIXED, ids=mc.case_id)
def test_device_records_equal_the_closed_loop_forced_f64(rl, c):
    p = mc.device_params(rl, sel_kw(c), c)
    dev = rl.Agent(p)
    try:
        check_selection_case(dev, p, c, device_ln(rl), q_mode="f64")
    finally:
        dev.close()


@pytest.mark.parametrize("c", SEL_EPS_GREEDY, ids=mc.case_id)
def test_device_records_equal_the_closed_loop_reset_step(rl, c):
    p = mc.device_params(rl, sel_kw(c), c)
    dev = rl.Agent(p)
    try:
        st = check_selection_case(dev, p, c, device_ln(rl), reset_step=True)
        assert st["resets"] >= p["n_lanes"]
    finally:
        dev.close()


@pytest.mark.parametrize("name", list(SEL_UNITS))
def test_device_unit_equals_the_closed_loop(rl, name):
    c, over, _, _ = SEL_UNITS[name]
    p = mc.device_params(rl, sel_kw(c, **over), c)
    dev = rl.Agent(p)
    try:
        check_selection_unit(dev, p, name, device_ln(rl))
    finally:
        dev.close()

"""The table checks shared by latte_sample_plan_loop and latte_t2v_guided_linear_loop (csrc/plan.h: plan_check) through the host-only
latte_debug_plan_check: a valid plan passes, every single-rule violation returns LATTE_ERR_INVALID with the words callers rely on.
No engine, no GPU."""
import ctypes

import numpy as np
import pytest

from latte_amd.schedulers import P_C1, P_C2, P_CN, P_IN, P_PUSH, P_RSV, P_T, PLAN_COLS, EulerDiscreteScheduler

INVALID = 1          # LATTE_ERR_INVALID
MAX_EVALS = 4096     # LATTE_PLAN_MAX_EVALS
T_LIMIT = 1000


@pytest.fixture(scope="module")
def valid_plan():
    sch = EulerDiscreteScheduler()
    sch.set_timesteps(6)
    plan = np.ascontiguousarray(sch.engine_plan(), dtype=np.float64)
    assert plan.shape == (6, PLAN_COLS)
    return plan


def run(lib, plan, max_evals=MAX_EVALS, t_limit=T_LIMIT, noise_given=0, may_draw_noise=0):
    plan = np.ascontiguousarray(plan, dtype=np.float64)
    rc = lib.latte_debug_plan_check(plan.ctypes.data_as(ctypes.c_void_p), plan.shape[0], max_evals, t_limit, noise_given, may_draw_noise)
    return rc, (lib.latte_last_error() or b"").decode()


def edited(plan, row, col, value):
    p = plan.copy()
    p[row, col] = value
    return p


def test_valid_plan_passes(lib, valid_plan):
    for t_limit in (T_LIMIT, 0):
        for flags in ((0, 0), (0, 1), (1, 0)):
            assert run(lib, valid_plan, t_limit=t_limit, noise_given=flags[0], may_draw_noise=flags[1])[0] == 0


@pytest.mark.parametrize("name,row,col,value,word", [
    ("nan", 2, P_IN, float("nan"), "non-finite"),
    ("fractional_t", 1, P_T, 3.5, "integer"),
    ("negative_t", 1, P_T, -1.0, "integer"),
    ("push_2", 3, P_PUSH, 2.0, "push must be 0 or 1"),
    ("reserved", 4, P_RSV, 1.0, "push must be 0 or 1"),
    ("c1_in_row_0", 0, P_C1, 0.5, "history"),
])
def test_single_rule_violations(lib, valid_plan, name, row, col, value, word):
    rc, msg = run(lib, edited(valid_plan, row, col, value), noise_given=1)
    assert rc == INVALID and word in msg and msg.startswith("plan_check: "), (name, rc, msg)
    assert f"row {row}" in msg


def test_trained_range_bound_only_with_a_limit(lib, valid_plan):
    for t in (float(T_LIMIT), float(T_LIMIT + 7)):
        p = edited(valid_plan, 0, P_T, t)
        rc, msg = run(lib, p)
        assert rc == INVALID and "trained range" in msg and f"[0, {T_LIMIT})" in msg, (rc, msg)
        assert run(lib, p, t_limit=0)[0] == 0           # text-to-video: no bound
    assert run(lib, edited(valid_plan, 0, P_T, float(T_LIMIT - 1)))[0] == 0


def test_history_slot_needs_that_many_pushes(lib, valid_plan):
    p = valid_plan.copy()
    p[:, P_PUSH] = 0.0
    p[0, P_PUSH] = 1.0                                   # one push before row 1
    assert run(lib, edited(p, 1, P_C1, 0.5))[0] == 0
    rc, msg = run(lib, edited(p, 1, P_C2, 0.5))
    assert rc == INVALID and "history" in msg and "slot 2" in msg, (rc, msg)


def test_c_noise_needs_given_or_drawn_noise(lib, valid_plan):
    p = edited(valid_plan, 2, P_CN, 0.25)
    rc, msg = run(lib, p, noise_given=0, may_draw_noise=0)
    assert rc == INVALID and "c_noise" in msg, (rc, msg)
    assert run(lib, p, noise_given=0, may_draw_noise=1)[0] == 0
    assert run(lib, p, noise_given=1, may_draw_noise=0)[0] == 0


def test_more_rows_than_max_evals(lib, valid_plan):
    n = valid_plan.shape[0]
    assert run(lib, valid_plan, max_evals=n)[0] == 0
    rc, msg = run(lib, valid_plan, max_evals=n - 1)      # n_evals = max_evals + 1
    assert rc == INVALID and f"more than {n - 1} evaluations" in msg, (rc, msg)


def test_whole_table_is_checked(lib, valid_plan):
    """The last row's violation is found: nothing is accepted on the strength of the first rows."""
    rc, msg = run(lib, edited(valid_plan, valid_plan.shape[0] - 1, P_T, 3.5))
    assert rc == INVALID and "integer" in msg and "row 5" in msg, (rc, msg)

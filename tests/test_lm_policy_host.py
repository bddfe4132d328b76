"""csrc/lm_policy.hpp - the trust-region rules pp_ba_solve takes every decision from - without a device: the header compiles with plain g++ and, driving
a dense Levenberg-Marquardt (tests/lm_policy_host_driver.cpp), reproduces the two iteration tables Ceres publishes; scripted verdict sequences check
the rules whose answer follows from their own statement (Ceres documentation, TrustRegionMinimizer / LevenbergMarquardtStrategy)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CONVERGENCE, NO_CONVERGENCE, FAILURE = 0, 1, 2      # PP_TERM_*


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("lm_policy") / "lm_policy_host_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-o", exe, os.path.join(ROOT, "tests", "lm_policy_host_driver.cpp")])
    return exe


def _table(exe, problem):
    out = subprocess.run([exe, problem], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    rows = {"policy": [], "oracle": []}
    x = term = None
    for line in out.stdout.splitlines():
        tok = line.split()
        if tok[0] in rows:
            rows[tok[0]].append([float(t) for t in tok[1:]])
        elif tok[0] == "x":
            x = [float(t) for t in tok[1:]]
        elif tok[0] == "termination":
            term = int(tok[1])
    return rows["policy"], rows["oracle"], x, term


def _same_radius_and_verdicts_as_the_oracle(trace, oracle_rows):
    assert len(trace) == len(oracle_rows)
    for got, want in zip(trace, oracle_rows):
        assert got[5] == want[5] and got[6] == want[6], (want, got)


def test_policy_reproduces_the_powell_trace_ceres_publishes(driver):
    """what test_trust_region_rules_reproduce_the_powell_trace_ceres_publishes asserts of the oracle's rules, of the product's"""
    rows, final = [], None
    for line in open(os.path.join(GOLDEN, "ceres_powell_trace.txt")):
        if line.startswith("# Final"):
            final = [float(t.split("=")[1]) for t in line[len("# Final"):].split(",")]
        if not line.startswith("#") and line.strip():
            rows.append(line.split())
    trace, oracle_rows, x, term = _table(driver, "powell")
    assert len(trace) == len(rows) == 15
    for want, got in zip(rows, trace):
        assert "%.6e" % got[0] == want[1], (want, got)
        for col, k in ((2, 1), (3, 2), (4, 3), (5, 4), (6, 5)):
            assert "%.2e" % got[k] == want[col], (want, got)
        assert got[6] == 1.0
    assert trace[-1][2] <= 1e-10 < trace[-2][2]                      # Gradient tolerance reached
    assert "%.6e" % trace[-1][2] == "3.642190e-11"
    assert ["%.6g" % v for v in x] == ["%.6g" % v for v in final]
    assert term == CONVERGENCE
    _same_radius_and_verdicts_as_the_oracle(trace, oracle_rows)


def test_policy_reproduces_the_helloworld_trace_ceres_publishes(driver):
    """the second published table: three rows, then the parameter tolerance ends the solve at x = 10"""
    rows = [l.split() for l in open(os.path.join(GOLDEN, "ceres_helloworld_trace.txt")) if l.strip() and not l.startswith("#")]
    trace, oracle_rows, x, term = _table(driver, "helloworld")
    assert len(trace) == len(rows) == 3
    for want, got in zip(rows, trace):
        assert "%.6e" % got[0] == want[1] and ["%.2e" % got[k] for k in (1, 2, 3, 4, 5)] == want[2:7], (want, got)
    assert "%.6g" % x[0] == "10"
    assert term == CONVERGENCE
    _same_radius_and_verdicts_as_the_oracle(trace, oracle_rows)


def _script(exe, lines):
    """-> (one dict per command that is not `opt`: answer + state, the trace rows at the end)"""
    out = subprocess.run([exe, "script"], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    states, rows = [], []
    for line in out.stdout.splitlines():
        tok = line.split()
        if tok[0] == "row":
            rows.append([float(t) for t in tok[1:]])
        else:
            st = {k: float(v) for k, v in (t.split("=") for t in tok[1:])}
            st["answer"] = tok[0]
            states.append(st)
    assert len(states) == sum(1 for l in lines if not l.startswith("opt"))
    return states, rows


INVALID = "judge -1 0 1 1 0 0"            # a step without model decrease
PIVOT = "judge 1 0.5 1 1 1 0"             # the linear solve raised the failed-pivot bit
TIMEOUT = "judge 1 0.5 1 1 4 1"           # bit 4, and the caller can repeat the step


def test_ten_consecutive_invalid_steps_fail_on_the_tenth(driver):
    st, rows = _script(driver, ["opt max_num_consecutive_invalid_steps 10", "opt initial_trust_region_radius 1024", "start 1 1"] + [INVALID, PIVOT] * 5)
    assert [s["answer"] for s in st] == ["started"] + ["invalid"] * 9 + ["invalid_failed"]
    radius, factor = 1024.0, 2.0
    for k, s in enumerate(st[1:10], 1):       # radius / 2, then / 4, / 8, ...: the factor doubles with every unsuccessful step
        radius /= factor; factor *= 2.0
        assert s["radius"] == radius and s["factor"] == factor and s["invalid"] == k and s["bad"] == k and s["rows"] == 1 + k and s["last_ok"] == 0
        assert rows[k] == [1.0, 0.0, 1.0, 0.0, 0.0, radius, 0.0]
    last = st[10]
    assert last["term"] == FAILURE and last["radius"] == radius and last["rows"] == 10 and last["bad"] == 9 and len(rows) == 10


def test_a_valid_step_ends_the_run_of_invalid_ones(driver):
    st, _ = _script(driver, ["opt max_num_consecutive_invalid_steps 2", "start 1 1", INVALID, "judge 1 2 1 1 0 0", INVALID, INVALID])
    assert [s["answer"] for s in st] == ["started", "invalid", "rejected", "invalid", "invalid_failed"]


def test_accept_after_rejects_resets_factor_and_diagonal(driver):
    # cost 8 -> candidate 9 twice (rho = -1), then 8 -> 4 with a model change of 4: rho = 1, radius / max(1/3, 1 - 1) = 3 radius
    st, rows = _script(driver, ["opt initial_trust_region_radius 64", "start 8 1", "judge 1 9 4 1 0 0", "judge 1 9 4 1 0 0", "judge 4 4 4 1 0 0"])
    assert [s["answer"] for s in st] == ["started", "rejected", "rejected", "accepted"]
    assert st[0]["reuse"] == 0 and st[0]["factor"] == 2.0
    assert (st[1]["radius"], st[1]["factor"], st[1]["reuse"], st[1]["last_ok"]) == (32.0, 4.0, 1, 0)
    assert (st[2]["radius"], st[2]["factor"], st[2]["reuse"], st[2]["bad"]) == (8.0, 8.0, 1, 2)
    assert (st[3]["radius"], st[3]["factor"], st[3]["reuse"], st[3]["last_ok"], st[3]["ok"], st[3]["cost"]) == (24.0, 2.0, 0, 1, 1, 4.0)
    assert rows[1] == [8.0, -1.0, 1.0, 2.0, -1.0, 32.0, 0.0] and rows[3] == [4.0, 4.0, 1.0, 2.0, 1.0, 24.0, 1.0]


def test_a_timeout_retry_changes_nothing(driver):
    st, rows = _script(driver, ["start 8 1", "judge 1 9 4 1 0 0", TIMEOUT, TIMEOUT, "before 0"])
    before, after = st[1], st[3]
    assert [s["answer"] for s in st] == ["started", "rejected", "retry", "retry", "step"]
    assert {k: v for k, v in after.items() if k != "answer"} == {k: v for k, v in before.items() if k != "answer"}
    assert len(rows) == 2
    # bit 4 without a way to repeat the step is an invalid step like any other
    st, _ = _script(driver, ["start 8 1", "judge 1 9 4 1 4 0"])
    assert st[1]["answer"] == "invalid"


def test_gradient_tolerance_waits_for_the_evaluation_and_for_a_successful_step(driver):
    head = ["opt gradient_tolerance 10", "start 8 100"]
    # the gradient norm in hand (100) is the previous point's while the evaluation at the accepted one is pending
    st, rows = _script(driver, head + ["judge 4 4 4 1 0 0", "before 1", "resolve 3.5 5", "before 0"])
    assert [s["answer"] for s in st] == ["started", "accepted", "step", "ok", "stop"]
    assert st[4]["term"] == CONVERGENCE and rows[1][0] == 3.5 and rows[1][2] == 5.0 and st[4]["cost"] == 3.5
    # below the tolerance from the start: no step is made
    st, _ = _script(driver, ["opt gradient_tolerance 10", "start 8 5", "before 0"])
    assert st[1]["answer"] == "stop" and st[1]["term"] == CONVERGENCE and st[1]["rows"] == 1
    # after an unsuccessful step the test does not fire, whatever the gradient norm; after the next successful one it does
    st, _ = _script(driver, head + ["judge 1 9 4 1 0 0", "resolve 8 5", "before 0", "judge 4 4 4 1 0 0", "resolve 4 5", "before 0"])
    assert [s["answer"] for s in st] == ["started", "rejected", "ok", "step", "accepted", "ok", "stop"]
    # a limit reached while the evaluation is pending: the caller brings the evaluation first, then the tests run in their order
    st, _ = _script(driver, ["opt max_num_iterations 1"] + head + ["judge 4 4 4 1 0 0", "before 1", "resolve 3.5 5", "before 0"])
    assert [s["answer"] for s in st][2:] == ["resolve_first", "ok", "stop"] and st[4]["term"] == CONVERGENCE


def test_zero_iterations_terminate_with_one_row(driver):
    st, rows = _script(driver, ["opt max_num_iterations 0", "start 8 1", "before 0"])
    assert st[1]["answer"] == "stop" and st[1]["term"] == NO_CONVERGENCE and len(rows) == 1
    assert rows[0] == [8.0, 0.0, 1.0, 0.0, 0.0, 1e4, 1.0]


def test_iteration_cap_and_minimum_radius(driver):
    st, _ = _script(driver, ["opt max_num_iterations 2", "start 8 1", "before 0", "judge 1 9 4 1 0 0", "before 0", "judge 1 9 4 1 0 0", "before 0"])
    assert [s["answer"] for s in st] == ["started", "step", "rejected", "step", "rejected", "stop"] and st[5]["term"] == NO_CONVERGENCE
    st, _ = _script(driver, ["opt initial_trust_region_radius 4", "opt min_trust_region_radius 1", "start 8 1", "judge 1 9 4 1 0 0", "before 0", "judge 1 9 4 1 0 0",
                             "before 0"])
    assert [(s["answer"], s["radius"]) for s in st[1:]] == [("rejected", 2.0), ("step", 2.0), ("rejected", 0.5), ("stop", 0.5)] and st[4]["term"] == CONVERGENCE


def test_radius_is_capped(driver):
    st, rows = _script(driver, ["opt initial_trust_region_radius 64", "opt max_trust_region_radius 100", "start 8 1", "judge 4 4 4 1 0 0"])
    assert st[1]["answer"] == "accepted" and st[1]["radius"] == 100.0 and rows[1][5] == 100.0      # (3 x 64 without the cap)


def test_rho_equal_to_min_relative_decrease_is_a_reject(driver):
    head = ["opt min_relative_decrease 0.5", "start 8 1"]
    st, _ = _script(driver, head + ["judge 8 4 4 1 0 0"])          # rho = (8 - 4) / 8 = 0.5 exactly
    assert st[1]["answer"] == "rejected" and st[1]["cost"] == 8.0
    st, _ = _script(driver, head + ["judge 7.5 4 4 1 0 0"])        # rho = 4 / 7.5 > 0.5
    assert st[1]["answer"] == "accepted" and st[1]["cost"] == 4.0


def test_tolerance_stops_record_nothing_and_stay(driver):
    """parameter and function tolerance end the solve AT the current point: no row, no counter, cost unchanged (the one deliberate difference to
    oracle::lm::DenseLevenbergMarquardt, which records the function-tolerance iteration as Ceres does - see oracle/bundle_adjustment.h)"""
    st, rows = _script(driver, ["opt parameter_tolerance 1e-3", "start 8 1", "judge 1 7 1e-8 1 0 0"])
    assert st[1]["answer"] == "parameter_tolerance" and st[1]["term"] == CONVERGENCE and len(rows) == 1 and st[1]["cost"] == 8.0
    st, rows = _script(driver, ["opt function_tolerance 1e-3", "opt parameter_tolerance 0", "start 8 1", "judge 1 7.999 4 1 0 0"])
    assert st[1]["answer"] == "function_tolerance" and st[1]["term"] == CONVERGENCE and len(rows) == 1 and st[1]["cost"] == 8.0 and st[1]["ok"] == 0

"""csrc/host_ticket.hpp - the host's wait for a ticket a kernel releases into pinned memory (the LM loop's scalars, the conjugate-gradient state, a
four-view model's errors) - without a device and under the sanitizers: the header is std only, tests/host_ticket_host_driver.cpp compiles with
g++ -fsanitize=address,undefined -pthread, a writer thread stands in for the kernel.  No upper time bounds are asserted (a loaded host may be slow):
only what was called, how often, and what must not have happened earlier than asked.  A sanitizer report ends the driver with a non-zero status."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TYPES = ("i32", "u64")      # the PCG ticket / the LM and four-view tickets


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("host_ticket") / "host_ticket_host_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-pthread",
                           "-o", exe, os.path.join(ROOT, "tests", "host_ticket_host_driver.cpp")])
    return exe


def _run(exe, ticket_type, case):
    out = subprocess.run([exe, ticket_type, case], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    got = dict(t.split("=") for t in out.stdout.split())
    return got["result"], int(got["syncs"]), int(got["naps"]), int(got["elapsed_us"]), int(got["payload"])


@pytest.mark.parametrize("ticket_type", TYPES)
def test_a_ticket_that_is_there_returns_at_once(driver, ticket_type):
    result, syncs, naps, _, payload = _run(driver, ticket_type, "present")
    assert (result, syncs, naps, payload) == ("arrived", 0, 0, 42)


@pytest.mark.parametrize("ticket_type", TYPES)
def test_a_ticket_written_during_the_spin_arrives_without_a_synchronisation(driver, ticket_type):
    result, syncs, _, _, payload = _run(driver, ticket_type, "writer_in_the_spin")      # writer after ~200 us, spin 1500 us
    assert (result, syncs, payload) == ("arrived", 0, 42)


@pytest.mark.parametrize("ticket_type", TYPES)
def test_a_late_ticket_arrives_through_the_naps(driver, ticket_type):
    result, syncs, naps, elapsed, payload = _run(driver, ticket_type, "writer_in_the_naps")      # writer after ~20 ms, spin 100 us
    assert (result, syncs, payload) == ("arrived", 0, 42) and naps > 0 and elapsed >= 20000


@pytest.mark.parametrize("ticket_type", TYPES)
def test_a_negative_spin_never_naps(driver, ticket_type):
    result, syncs, naps, elapsed, payload = _run(driver, ticket_type, "writer_never_nap")      # the same writer, spin_us = -1 (the four-view wait)
    assert (result, syncs, naps, payload) == ("arrived", 0, 0, 42) and elapsed >= 20000


@pytest.mark.parametrize("ticket_type", TYPES)
def test_giving_up_synchronises_exactly_once_and_not_early(driver, ticket_type):
    result, syncs, naps, elapsed, _ = _run(driver, ticket_type, "give_up")      # give_up = 50 ms, nobody writes
    assert (result, syncs) == ("never_arrived", 1) and elapsed >= 50000 and naps > 0


@pytest.mark.parametrize("ticket_type", TYPES)
def test_a_ticket_the_synchronisation_brings_counts_as_arrived(driver, ticket_type):
    result, syncs, _, elapsed, payload = _run(driver, ticket_type, "give_up_sync_ships")
    assert (result, syncs, payload) == ("arrived", 1, 42) and elapsed >= 50000


@pytest.mark.parametrize("ticket_type", TYPES)
def test_a_failed_synchronisation_is_reported_as_such(driver, ticket_type):
    result, syncs, _, elapsed, _ = _run(driver, ticket_type, "give_up_sync_fails")
    assert (result, syncs) == ("sync_failed", 1) and elapsed >= 50000


@pytest.mark.parametrize("ticket_type", TYPES)
def test_sync_first_synchronises_before_the_first_poll_and_only_then(driver, ticket_type):
    """spin_us = 0: a poll that found no ticket would nap at its first look at the clock; the synchronisation brings the ticket, so no nap, one call"""
    result, syncs, naps, _, payload = _run(driver, ticket_type, "sync_first")
    assert (result, syncs, naps, payload) == ("arrived", 1, 0, 42)
    result, syncs, naps, _, _ = _run(driver, ticket_type, "sync_first_fails")
    assert (result, syncs, naps) == ("sync_failed", 1, 0)

"""GPU tests of put_signal, the signal operations and wait_until / test: 1, 2 and 3 PEs as separate
processes on the test box's one GPU (tests/signal_worker.py).  The target of a put_signal learns of
the payload through the signal word alone; both put_signal paths run in every test that moves a
payload (ISHMEM_PUT_SIGNAL_FUSED_MAX_BYTES is pinned to 64 KiB here whatever the default becomes)."""
import multiprocessing as mp
import queue
import sys
import time
import uuid

import pytest

from tests import signal_worker

pytestmark = pytest.mark.gpu

# HSA_ENABLE_IPC_MODE_LEGACY is removed from every PE's environment: the library sets it itself.
ENV = {"ISHMEM_TIMEOUT_MS": 20000, "ISHMEM_SYMMETRIC_SIZE": "256M", "ISHMEM_PUT_SIGNAL_FUSED_MAX_BYTES": "64K",
       "HSA_ENABLE_IPC_MODE_LEGACY": None}


def run_pes(npes: int, scenarios: list[str], timeout: float = 240.0, env: dict | None = None):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    key = f"s{uuid.uuid4().hex[:12]}"
    procs = [ctx.Process(target=signal_worker.run, args=(pe, npes, key, scenarios, q, {**ENV, **(env or {})}))
             for pe in range(npes)]
    for p in procs:
        p.start()
    results = {}
    t0 = time.monotonic()
    try:
        while len(results) < npes:
            try:
                pe, fails = q.get(timeout=min(30.0, max(1.0, timeout - (time.monotonic() - t0))))
            except queue.Empty:
                if time.monotonic() - t0 >= timeout:
                    break
                print(f"[run_pes {npes} PEs {scenarios}] {time.monotonic() - t0:.0f} s, "
                      f"{len(results)} reported", file=sys.stderr, flush=True)
                continue
            results[pe] = fails
    finally:
        for p in procs:
            p.join(timeout=30)
            if p.is_alive():
                p.kill()
                p.join()
    assert len(results) == npes, f"only {len(results)} of {npes} PEs reported"
    allfails = [f for pe in sorted(results) for f in results[pe]]
    assert not allfails, "\n".join(allfails[:20])


NPES = [1, 2, 3]


@pytest.mark.parametrize("npes", NPES)
def test_put_signal_sizes_paths_and_names(npes):
    run_pes(npes, ["sizes"])


@pytest.mark.parametrize("npes", NPES)
def test_put_signal_source_and_dest_phases(npes):
    run_pes(npes, ["offsets"])


@pytest.mark.parametrize("npes", NPES)
def test_signal_is_not_seen_before_the_payload(npes):
    run_pes(npes, ["ordering"])


@pytest.mark.parametrize("npes", NPES)
def test_fan_in_with_signal_add(npes):
    run_pes(npes, ["fanin"])


@pytest.mark.parametrize("npes", NPES)
def test_wait_until_and_test_every_typename_and_comparison(npes):
    run_pes(npes, ["waittest"])


@pytest.mark.parametrize("npes", NPES)
def test_signal_set_add_and_fetch(npes):
    run_pes(npes, ["sigops"])


@pytest.mark.parametrize("npes", NPES)
def test_on_stream_handshake_eager(npes):
    run_pes(npes, ["chain"])


@pytest.mark.parametrize("npes", NPES)
def test_on_stream_handshake_captured_into_a_graph(npes):
    run_pes(npes, ["graph"])


@pytest.mark.parametrize("npes", NPES)
def test_host_wait_does_not_hold_the_lock_against_a_second_thread(npes):
    run_pes(npes, ["thread"])


@pytest.mark.parametrize("npes", NPES)
def test_argument_failures_launch_nothing(npes):
    run_pes(npes, ["argfail"])


@pytest.mark.parametrize("npes", NPES)
def test_waits_are_bounded_and_the_library_works_afterwards(npes):
    run_pes(npes, ["bounded"], env={"ISHMEM_TIMEOUT_MS": 300})

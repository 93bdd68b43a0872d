"""GPU tests of the atomic memory operations through the C ABI's Python mirror: 1, 2 and 3 PEs as
separate processes on the test box's one GPU (tests/amo_worker.py).  Expected values come from
amo_worker.amo_model; DESIGN.md §3d names the test that pins each clause of the contract."""
import multiprocessing as mp
import queue
import sys
import time
import uuid

import pytest

from tests import amo_worker

pytestmark = pytest.mark.gpu

# HSA_ENABLE_IPC_MODE_LEGACY is removed from every PE's environment: the library sets it itself.
ENV = {"ISHMEM_TIMEOUT_MS": 20000, "ISHMEM_SYMMETRIC_SIZE": "256M", "HSA_ENABLE_IPC_MODE_LEGACY": None}


def run_pes(npes: int, scenarios: list[str], timeout: float = 240.0):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    key = f"a{uuid.uuid4().hex[:12]}"
    procs = [ctx.Process(target=amo_worker.run, args=(pe, npes, key, scenarios, q, ENV)) for pe in range(npes)]
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
def test_every_op_and_dtype_matches_the_model_and_spares_the_guards(npes):
    run_pes(npes, ["matrix"])


@pytest.mark.parametrize("npes", NPES)
def test_contended_fetch_add_inc_and_compare_swap_lose_no_update(npes):
    run_pes(npes, ["contended"])


@pytest.mark.parametrize("npes", NPES)
def test_nbi_fetch_words_are_defined_after_quiet(npes):
    run_pes(npes, ["nbi"])


@pytest.mark.parametrize("npes", NPES)
def test_amo_after_fence_is_not_seen_before_the_put(npes):
    run_pes(npes, ["ordering"])


@pytest.mark.parametrize("npes", NPES)
def test_fan_in_with_atomic_inc_and_wait_until(npes):
    run_pes(npes, ["fanin"])


@pytest.mark.parametrize("npes", NPES)
def test_two_host_threads_lose_no_update(npes):
    run_pes(npes, ["threads"])


@pytest.mark.parametrize("npes", NPES)
def test_argument_failures_launch_nothing(npes):
    run_pes(npes, ["argfail"])

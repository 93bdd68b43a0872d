"""GPU tests of the vector waits and tests (wait_until_all / any / some, test_all / any / some and their
_vector forms): 1, 2 and 3 PEs as separate processes on the test box's one GPU
(tests/syncvec_worker.py), with tests/test_gpu_signal.py's launcher.  Expectations come from the model
in tests/syncvec_cases.py."""
import multiprocessing as mp
import queue
import sys
import time
import uuid

import pytest

from tests import syncvec_worker

pytestmark = pytest.mark.gpu

# HSA_ENABLE_IPC_MODE_LEGACY is removed from every PE's environment: the library sets it itself.
ENV = {"ISHMEM_TIMEOUT_MS": 20000, "ISHMEM_SYMMETRIC_SIZE": "256M", "HSA_ENABLE_IPC_MODE_LEGACY": None}


def run_pes(npes: int, scenarios: list[str], timeout: float = 240.0, env: dict | None = None):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    key = f"v{uuid.uuid4().hex[:12]}"
    hb = ctx.Barrier(npes)  # a host-side meeting point for the steps that must not touch the GPU
    procs = [ctx.Process(target=syncvec_worker.run, args=(pe, npes, key, scenarios, q, {**ENV, **(env or {})}, hb))
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
def test_every_typename_and_comparison_against_the_model(npes):
    run_pes(npes, ["types"])


@pytest.mark.parametrize("npes", NPES)
def test_sizes_status_kinds_and_array_placement_against_the_model(npes):
    run_pes(npes, ["sizes"])


@pytest.mark.parametrize("npes", NPES)
def test_wait_until_all_does_not_return_early(npes):
    run_pes(npes, ["all"])


@pytest.mark.parametrize("npes", NPES)
def test_wait_until_any_and_some_find_the_written_element_and_rotate(npes):
    run_pes(npes, ["anysome"])


@pytest.mark.parametrize("npes", NPES)
def test_wait_until_some_on_stream_captured_into_a_graph(npes):
    run_pes(npes, ["graph"])


@pytest.mark.parametrize("npes", NPES)
def test_payloads_are_visible_after_the_vector_wait(npes):
    run_pes(npes, ["payload"])


@pytest.mark.parametrize("npes", NPES)
def test_argument_failures_launch_nothing(npes):
    run_pes(npes, ["argfail"])


@pytest.mark.parametrize("npes", NPES)
def test_waits_are_bounded_and_the_library_works_afterwards(npes):
    run_pes(npes, ["bounded"], env={"ISHMEM_TIMEOUT_MS": 300})

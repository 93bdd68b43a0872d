"""GPU tests of put / get: 1, 2 and 3 PEs as separate processes on the test box's one GPU
(tests/rma_worker.py).  Every PE puts to (me + 1) % p, or gets from it; the reference tester's
pattern and seeded random bytes; guards around dest; bit-exact."""
import multiprocessing as mp
import queue
import sys
import time
import uuid

import pytest

from tests import rma_worker

pytestmark = pytest.mark.gpu

# HSA_ENABLE_IPC_MODE_LEGACY is removed from every PE's environment: the library sets it itself.
ENV = {"ISHMEM_MAX_BLOCKS": rma_worker.MAX_BLOCKS, "ISHMEM_TIMEOUT_MS": 20000, "ISHMEM_SYMMETRIC_SIZE": "256M",
       "HSA_ENABLE_IPC_MODE_LEGACY": None}


def run_pes(npes: int, scenarios: list[str], timeout: float = 240.0, env: dict | None = None):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    key = f"r{uuid.uuid4().hex[:12]}"
    procs = [ctx.Process(target=rma_worker.run, args=(pe, npes, key, scenarios, q, {**ENV, **(env or {})}))
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
def test_put_sizes_and_names(npes):
    run_pes(npes, ["put_sizes", "typed"])


@pytest.mark.parametrize("npes", NPES)
def test_get_sizes(npes):
    run_pes(npes, ["get_sizes"])


@pytest.mark.parametrize("npes", NPES)
def test_put_source_and_dest_offsets(npes):
    run_pes(npes, ["put_offsets"])


@pytest.mark.parametrize("npes", NPES)
def test_get_source_and_dest_offsets(npes):
    run_pes(npes, ["get_offsets"])


@pytest.mark.parametrize("npes", NPES)
def test_nbi_then_quiet_and_quiet_on_stream(npes):
    run_pes(npes, ["nbi"])


@pytest.mark.parametrize("npes", NPES)
def test_barrier_all_completes_a_pending_nbi_put(npes):
    run_pes(npes, ["pending"])


@pytest.mark.parametrize("npes", NPES)
def test_on_stream_chain_eager_and_with_deps(npes):
    run_pes(npes, ["chain"])


@pytest.mark.parametrize("npes", NPES)
def test_on_stream_chain_captured_into_a_graph(npes):
    run_pes(npes, ["graph"])


@pytest.mark.parametrize("npes", NPES)
def test_local_buffer_kinds(npes):
    run_pes(npes, ["kinds"])


@pytest.mark.parametrize("npes", NPES)
def test_put_into_a_target_with_warm_caches(npes):
    run_pes(npes, ["warm"])


@pytest.mark.parametrize("npes", NPES)
def test_argument_failures_do_not_hang(npes):
    run_pes(npes, ["argfail"])

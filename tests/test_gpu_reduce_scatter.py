"""GPU tests of the reduce-scatter extension (ishmemx_<TN>_<op>_reduce_scatter): 2, 3, 4 and 8 PEs as
separate processes on the test box's one GPU (tests/reduce_scatter_worker.py), both paths (granule
and barrier), every comparison on raw bits against the sliced fold of the existing oracle, guard
bytes on both sides of dest, the source read back unchanged."""
import multiprocessing as mp
import queue
import sys
import time
import uuid

import pytest

from tests import reduce_scatter_worker

pytestmark = pytest.mark.gpu

# HSA_ENABLE_IPC_MODE_LEGACY is removed from every PE's environment: the library sets it itself.
ENV = {"ISHMEM_MAX_BLOCKS": 32, "ISHMEM_TIMEOUT_MS": 20000, "ISHMEM_SYMMETRIC_SIZE": "1G",
       "HSA_ENABLE_IPC_MODE_LEGACY": None}

PATHS = {
    "default": {},  # the granule path at these sizes
    "barrier": {"ISHMEM_LL_MAX_BYTES": 0},
}


def run_pes(npes: int, scenarios: list[str], timeout: float = 240.0, env: dict | None = None):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    key = f"r{uuid.uuid4().hex[:12]}"
    procs = [ctx.Process(target=reduce_scatter_worker.run, args=(pe, npes, key, scenarios, q, {**ENV, **(env or {})}))
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


@pytest.mark.parametrize("path", ["default", "barrier"])
@pytest.mark.parametrize("npes", [2, 3, 4])
def test_sizes_and_offsets(npes, path):
    run_pes(npes, ["sizes"], env=PATHS[path])


@pytest.mark.parametrize("path", ["default", "barrier"])
def test_8_pes(path):
    run_pes(8, ["wide"], env=PATHS[path])


@pytest.mark.parametrize("path", ["default", "barrier"])
@pytest.mark.parametrize("npes", [2, 3])
def test_half_and_bfloat16(npes, path):
    run_pes(npes, ["half"], env=PATHS[path])


@pytest.mark.parametrize("path", ["default", "barrier"])
@pytest.mark.parametrize("npes", [2, 3])
def test_special_values(npes, path):
    run_pes(npes, ["special"], env=PATHS[path])


def test_realign_kernel_and_grid_stride():
    run_pes(3, ["realigncap"], env=PATHS["barrier"])


@pytest.mark.parametrize("path", ["default", "barrier"])
def test_teams(path):
    run_pes(4, ["teams"], env=PATHS[path])


@pytest.mark.parametrize("npes", [2, 4])
def test_on_stream_chain_and_deps(npes):
    run_pes(npes, ["chain"])


@pytest.mark.parametrize("path", ["default", "barrier"])
def test_captured_into_a_graph(path):
    run_pes(2, ["graph"], env=PATHS[path])


def test_argument_failures_do_not_hang():
    run_pes(3, ["argfail"])

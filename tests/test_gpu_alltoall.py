"""GPU tests of alltoall over teams: 2, 3, 4 and 8 PEs as separate processes on the test box's one
GPU (tests/alltoall_worker.py), every path (granule, handshake, phased), the reference tester's
pattern and seeded random bytes, guards around dest, bit-exact."""
import multiprocessing as mp
import queue
import sys
import time
import uuid

import pytest

from tests import alltoall_worker

pytestmark = pytest.mark.gpu

# HSA_ENABLE_IPC_MODE_LEGACY is removed from every PE's environment: the library sets it itself.
ENV = {"ISHMEM_MAX_BLOCKS": 32, "ISHMEM_TIMEOUT_MS": 20000, "ISHMEM_SYMMETRIC_SIZE": "1G",
       "HSA_ENABLE_IPC_MODE_LEGACY": None}

PATHS = {
    "default": {},
    "handshake": {"ISHMEM_LL_MAX_BYTES": 0},
    "phased": {"ISHMEM_LL_MAX_BYTES": 0, "ISHMEM_PHASED_MIN_BYTES": 0},
}


def run_pes(npes: int, scenarios: list[str], timeout: float = 240.0, env: dict | None = None):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    key = f"a{uuid.uuid4().hex[:12]}"
    procs = [ctx.Process(target=alltoall_worker.run, args=(pe, npes, key, scenarios, q, {**ENV, **(env or {})}))
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


@pytest.mark.parametrize("path", ["default", "handshake", "phased"])
@pytest.mark.parametrize("npes", [2, 3, 4])
def test_alltoall_sizes_and_shifted_arrays(npes, path):
    run_pes(npes, ["sizes", "shifted"], env=PATHS[path])


@pytest.mark.parametrize("path", ["default", "phased"])
def test_alltoall_8_pes(path):
    run_pes(8, ["sizes", "shifted"], env=PATHS[path])


def test_alltoall_teams_single_member_and_zero_elements():
    run_pes(4, ["teams"])


@pytest.mark.parametrize("npes", [2, 4])
def test_alltoall_on_stream_chain_and_deps(npes):
    run_pes(npes, ["chain"])


def test_alltoall_captured_into_a_graph():
    run_pes(2, ["graph"])


def test_alltoall_argument_failures_do_not_hang():
    run_pes(3, ["argfail"])

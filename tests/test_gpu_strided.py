"""GPU tests of strided / blocked put / get (ishmem_iput / iget, ishmemx_ibput / ibget): 1, 2 and 3 PEs
as separate processes on the test box's one GPU (tests/strided_worker.py).  Every PE targets
(me + 1) % p; the dest arena is prefilled with a sentinel and compared whole, so the gaps between
strided elements and the guards must come back unchanged; bit-exact."""
import multiprocessing as mp
import queue
import time
import uuid

import pytest

from tests import strided_cases, strided_worker

pytestmark = pytest.mark.gpu

# HSA_ENABLE_IPC_MODE_LEGACY is removed from every PE's environment: the library sets it itself.
ENV = {"ISHMEM_MAX_BLOCKS": strided_cases.MAX_BLOCKS, "ISHMEM_TIMEOUT_MS": 20000, "ISHMEM_SYMMETRIC_SIZE": "256M",
       "HSA_ENABLE_IPC_MODE_LEGACY": None}
NPES = [1, 2, 3]


def run_pes(npes, scenarios):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    key = f"s{uuid.uuid4().hex[:12]}"
    procs = [ctx.Process(target=strided_worker.run, args=(pe, npes, key, scenarios, q, dict(ENV))) for pe in range(npes)]
    for p in procs:
        p.start()
    results = {}
    t0 = time.monotonic()
    try:
        while len(results) < npes and time.monotonic() - t0 < 240.0:
            try:
                pe, fails = q.get(timeout=5.0)
            except queue.Empty:
                if not any(p.is_alive() for p in procs) and q.empty():
                    break
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


@pytest.mark.parametrize("npes", NPES)
def test_iput_widths_strides_and_counts(npes):
    run_pes(npes, ["iput"])


@pytest.mark.parametrize("npes", NPES)
def test_iget_widths_strides_and_counts(npes):
    run_pes(npes, ["iget"])


@pytest.mark.parametrize("npes", NPES)
def test_ibput_shapes(npes):
    run_pes(npes, ["ibput"])


@pytest.mark.parametrize("npes", NPES)
def test_ibget_shapes(npes):
    run_pes(npes, ["ibget"])


@pytest.mark.parametrize("npes", NPES)
def test_ibput_byte_offsets_cover_every_item_width(npes):
    run_pes(npes, ["put_offsets"])


@pytest.mark.parametrize("npes", NPES)
def test_ibget_byte_offsets_cover_every_item_width(npes):
    run_pes(npes, ["get_offsets"])


@pytest.mark.parametrize("npes", NPES)
def test_reference_tester_shapes_and_typed_names(npes):
    run_pes(npes, ["tester", "typed"])


@pytest.mark.parametrize("npes", NPES)
def test_local_buffer_kinds(npes):
    run_pes(npes, ["kinds"])


@pytest.mark.parametrize("npes", NPES)
def test_on_stream_eager_deps_and_graph(npes):
    run_pes(npes, ["stream", "graph"])


@pytest.mark.parametrize("npes", NPES)
def test_strided_put_into_a_target_with_warm_caches(npes):
    run_pes(npes, ["warm"])


@pytest.mark.parametrize("npes", NPES)
def test_argument_failures_do_not_hang(npes):
    run_pes(npes, ["argfail"])

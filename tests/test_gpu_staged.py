"""GPU tests of the host-buffer reduce: a source or dest outside the symmetric heap (pageable host,
pinned host, plain device memory) goes through reduce_staged / reduce_staged_pipeline, chunk by
chunk over the slots of the staging region.  Worker: tests/staged_worker.py; case tables and the
chunk-plan model: tests/staged_cases.py (pinned on the CPU by tests/test_staged_cases.py).

The staging region is 1 MiB, so a 2.5 MiB payload is six chunks over two slots and every case takes
milliseconds; the worker fails a case whose live plan is not the one its table promises.  Every
result is bit-exact against oracle.reduce_fold, every dest has guard bytes before and after.

Which test pins which property of the pipeline (DESIGN.md §6b lists them too):
  slot rotation, chunk offsets, ragged tail     test_chunk_counts_and_ragged_tail, test_every_op_and_type
  the wait before a slot is refilled             the `full` / `ragged` sizes of the same tests (each slot
                                                 filled two and three times) and test_copy_kernel
  paths mixed inside one call                    test_collective_path_inside_the_chunk
  the final join                                 every blocking case with a pinned dest (read at return, the
                                                 last bytes first), test_on_stream_and_back_to_back (d),
                                                 test_captured_five_chunks_replayed_twice
  page-lock and unlock                           test_buffer_kinds_and_page_lock
  staging hand-over between calls                test_on_stream_and_back_to_back (b), (c)
"""
import pytest

from tests import staged_cases as sc
from tests import staged_worker
from tests.test_gpu_multi import run_pes

pytestmark = pytest.mark.gpu


def run_staged(npes, scenarios, slots=2, staging=sc.STAGING, env=None, timeout=120.0):
    full = {"ISHMEM_STAGING_SIZE": staging, "ISHMEM_STAGING_SLOTS": slots, "STAGED_WANT_BYTES": staging,
            "STAGED_WANT_SLOTS": slots, "ISHMEM_STAGED_COPY_KERNEL": None, **(env or {})}
    run_pes(npes, scenarios, timeout=timeout, env=full, worker=staged_worker.run)


@pytest.mark.parametrize("slots", sc.SLOT_COUNTS)
@pytest.mark.parametrize("npes", [2, 3])
def test_chunk_counts_and_ragged_tail(npes, slots):
    # int32 sum, pageable buffers: c - 1, c, c + 1, 2c, 2 * slots * c, (2 * slots + 1) c + 17, 3c + 1.
    run_staged(npes, ["chunks"], slots=slots)


def test_every_op_and_type():
    # The 64 valid (op, type) pairs at 2c + 3 of each type's chunk: element sizes 1, 2, 4 and 8.
    run_staged(2, ["matrix"])


@pytest.mark.parametrize("npes,slots,envs", sc.PATH_RUNS, ids=lambda v: "-".join(v) if isinstance(v, tuple) else str(v))
def test_collective_path_inside_the_chunk(npes, slots, envs):
    # The in-place slot reduce forced onto the granule path, the in-place fold through the team
    # scratch, the persistent kernel and the phased path; `mixed` / `default`: the 17-element tail
    # chunk takes the granule path inside a call whose full chunks do not.
    run_staged(npes, ["paths=" + ",".join(envs)], slots=slots, env=sc.PATH_ENVS[envs[0]][0])


@pytest.mark.parametrize("npes", [2, 3])
def test_buffer_kinds_and_page_lock(npes):
    # Pageable (page-locked for the call), pinned and plain device buffers, the mixed pairs, in and
    # out of place, aligned and one element off; then the page-lock corner cases, a heap reduce
    # after each.
    run_staged(npes, ["kinds", "pagelock"])


@pytest.mark.parametrize("npes", [2, 3])
def test_pageable_buffers_below_the_page_lock_threshold(npes):
    # The same six chunks with a 256 KiB region: 640 KiB payloads stay on HIP's pageable copies.
    run_staged(npes, ["kinds"], staging=sc.SMALL_STAGING)


@pytest.mark.parametrize("npes", [2, 3])
def test_copy_kernel(npes):
    # staged_copy_kernel 1, 2, 3 with pinned buffers; 3 with pageable buffers (DMA fallback).
    run_staged(npes, ["copykernel"])


def test_strided_team_and_team_of_one():
    # The even PEs of four reduce host buffers over six chunks while the odd PEs reduce in the heap;
    # then every PE alone: copy-in and copy-out only.
    run_staged(4, ["teams"])


@pytest.mark.parametrize("npes", [2, 3])
def test_on_stream_and_back_to_back(npes):
    # On-stream calls with *ret; two staged reduces on two streams and a staged reduce followed by a
    # host-source fcollect with no host synchronisation between; a blocking call read at return;
    # large pageable buffers on a stream complete before the call returns.
    run_staged(npes, ["stream"])


def test_captured_five_chunks_replayed_twice():
    # One on-stream reduce of five chunks, pinned buffers, captured and replayed with new sources.
    run_staged(2, ["graph"])

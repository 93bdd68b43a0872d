"""GPU tests of the path choice at its thresholds on cross-GPU and mixed-topology teams
(tests/topology_worker.py, tables in tests/topology_cases.py).

Every PE runs on the one GPU of the test box and reports the PCI bus its topology gives it
(ISHMEM_TEST_PCI_BUS, test-hooks library): one PE per GPU at 2, 3, 4 and 8 PEs, two PEs per GPU at
4 and 6, and three PEs on one GPU with one alone.  On every team of a topology (WORLD, a
co-located split team, a cross-device one) every form runs at a payload of exactly each threshold
and one element more, bit-exact against the oracle with guard bytes, and get_param("last_path")
must name the path the model gives.  The same tables run once on co-located worlds without hooks.
The shifted reduce-scatter runs at grids of 63, 64, 65 and 145 workgroups in both block orders
where the PE has its (emulated) GPU to itself.  This is emulation: path choice and kernels under
the node's launch shapes on one GPU, not behaviour across real links.
"""
import multiprocessing as mp
import queue
import sys
import time
import uuid
from pathlib import Path

import pytest

from tests import alltoall_worker, coll_cases, coll_worker, reduce_scatter_worker
from tests import topology_cases as tc
from tests import topology_worker

ROOT = Path(__file__).resolve().parents[1]

pytestmark = pytest.mark.gpu

TESTHOOKS = {"ISHMEM_AMD_LIB": str(ROOT / "ishmem_amd" / "libishmem_amd_testhooks.so")}
# The grid cap lifted, as for the other emulated one-PE-per-GPU runs; HSA_ENABLE_IPC_MODE_LEGACY is
# removed from every PE's environment: the library sets it itself.
ENV = {"ISHMEM_MAX_BLOCKS": 1024, "ISHMEM_TIMEOUT_MS": 20000, "ISHMEM_SYMMETRIC_SIZE": "1G",
       "HSA_ENABLE_IPC_MODE_LEGACY": None}
# Thresholds at their defaults apart from the phased one, whatever the outer environment holds.
BOUNDARY_ENV = {"ISHMEM_PHASED_MIN_BYTES": tc.PHASED_MIN, "ISHMEM_LL_MAX_BYTES": None,
                "ISHMEM_ONESHOT_P2_MAX_BYTES": None, "ISHMEM_XGMI_LL_MAX_BYTES": None,
                "ISHMEM_XGMI_FOLD_MAX_BYTES": None}


def run_pes(npes: int, worker, args: tuple, env: dict, timeout: float = 240.0):
    """worker(pe, npes, key, *args[:1], q, env, *args[1:]) on npes processes; collects their failures."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    key = f"y{uuid.uuid4().hex[:12]}"
    procs = [ctx.Process(target=worker, args=(pe, npes, key, args[0], q, env, *args[1:])) for pe in range(npes)]
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
                print(f"[run_pes {npes} PEs {args}] {time.monotonic() - t0:.0f} s, {len(results)} reported",
                      file=sys.stderr, flush=True)
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


def emulated(topo: tc.Topology) -> dict:
    return {**TESTHOOKS, "ISHMEM_TEST_PCI_BUS": list(topo.buses)} if topo.buses else {}


@pytest.mark.parametrize("topology", [t.name for t in tc.EMULATED])
def test_thresholds_stood_on_by_every_team_of_an_emulated_topology(topology):
    topo = tc.TOPOLOGIES[topology]
    run_pes(tc.npes(topo), topology_worker.run, (["boundary"], topology), {**ENV, **BOUNDARY_ENV, **emulated(topo)})


@pytest.mark.parametrize("topology", [t.name for t in tc.CONTROL])
def test_thresholds_stood_on_by_a_colocated_world(topology):
    # The control: no hooks, every PE on the real GPU, the measured crossovers.
    topo = tc.TOPOLOGIES[topology]
    run_pes(tc.npes(topo), topology_worker.run, (["boundary"], topology), {**ENV, **BOUNDARY_ENV})


@pytest.mark.parametrize("topology", ["one_per_gpu2", "one_per_gpu3", "one_per_gpu4", "one_per_gpu8", "uneven"])
def test_xcd_grouped_reduce_scatter_with_shifted_sources(topology):
    # device_share == 1: rs_phase_kernel with a.shift && a.xcd_group — the whole-array fold at 2 PEs,
    # the phased path at 3, 4 and 8 (P = 0, 4, 8), reduce-scatter blocks on the barrier path.  On the
    # uneven layout PE 3 alone is grouped.
    topo = tc.TOPOLOGIES[topology]
    n = tc.npes(topo)
    run_pes(n, topology_worker.run, (["shifted"], topology), {**ENV, **tc.shifted_env(n), **emulated(topo)})


def one_per_gpu(n: int) -> dict:
    return emulated(tc.TOPOLOGIES[f"one_per_gpu{n}"])


def test_scans_and_copies_one_pe_per_gpu_emulated():
    # tests/coll_worker.py's scan and copy tables at 3 PEs under the link-byte model's limits.
    env = {**ENV, "ISHMEM_STAGING_SIZE": "4M", **coll_cases.ENVS["granule"], **one_per_gpu(3)}
    run_pes(3, coll_worker.run, (["scan", "coll"], "granule"), env)


def test_alltoall_one_pe_per_gpu_emulated():
    run_pes(4, alltoall_worker.run, (["sizes", "shifted"],), {**ENV, **one_per_gpu(4)})


def test_reduce_scatter_barrier_path_one_pe_per_gpu_emulated():
    run_pes(3, reduce_scatter_worker.run, (["sizes"],), {**ENV, "ISHMEM_LL_MAX_BYTES": 0, **one_per_gpu(3)})

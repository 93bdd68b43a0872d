"""GPU tests of the host and on-stream scans, fcollect, collect and broadcast at their edges
(tests/coll_worker.py, case tables in tests/coll_cases.py): in place and at every byte-offset pair,
sizes round the vector width and the chunk unit, teams of 2, 3, 4 and 8 PEs and strided, offset,
reversed and one-member teams of six, on every path (granule, handshake / persistent, phased, the
direct fold and both with the fold bound at 0), guard bytes round every dest, bit-exact."""
import multiprocessing as mp
import queue
import sys
import time
import uuid

import pytest

from tests import coll_cases, coll_worker

pytestmark = pytest.mark.gpu

# HSA_ENABLE_IPC_MODE_LEGACY is removed from every PE's environment: the library sets it itself.
# The staging region is 4 MiB so the multi-segment scan stays small.
ENV = {"ISHMEM_MAX_BLOCKS": 32, "ISHMEM_TIMEOUT_MS": 20000, "ISHMEM_SYMMETRIC_SIZE": "1G",
       "ISHMEM_STAGING_SIZE": "4M", "HSA_ENABLE_IPC_MODE_LEGACY": None}
WIDE = {"ISHMEM_MAX_BLOCKS": 8}  # 8 PEs on one GPU, as the other 8-PE tests


def run_pes(npes: int, envname: str, scenarios: list[str], timeout: float = 240.0, env: dict | None = None):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    key = f"c{uuid.uuid4().hex[:12]}"
    full = {**ENV, **coll_cases.ENVS[envname], **(env or {})}
    procs = [ctx.Process(target=coll_worker.run, args=(pe, npes, key, scenarios, q, full, envname))
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
                print(f"[run_pes {npes} PEs {envname} {scenarios}] {time.monotonic() - t0:.0f} s, "
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


def scan_scenarios(envname: str, npes: int) -> list[str]:
    # A second pass with the fold bound at 0 where the first one folds disjoint scans directly.
    return ["scan", "multiseg"] + (["nodirect"] if envname != "granule" and npes in (3, 4) else [])


@pytest.mark.parametrize("envname", ["granule", "handshake", "phased"])
@pytest.mark.parametrize("npes", [2, 3, 4])
def test_scans_in_place_and_at_offsets(npes, envname):
    run_pes(npes, envname, scan_scenarios(envname, npes))


@pytest.mark.parametrize("envname", ["granule", "handshake", "phased"])
def test_scans_in_place_and_at_offsets_8_pes(envname):
    # handshake / phased: float and uint8 only (scan_kernel<T, VEC, 8>: two items a thread).
    run_pes(8, envname, scan_scenarios(envname, 8), env=WIDE)


@pytest.mark.parametrize("envname", ["granule", "handshake", "phased"])
@pytest.mark.parametrize("npes", [2, 3, 4])
def test_fcollect_collect_broadcast_at_offsets(npes, envname):
    # phased: a second pass with the narrow-item kernels in place of the realigned movers.
    run_pes(npes, envname, ["coll"] + (["norealign"] if envname == "phased" else []))


@pytest.mark.parametrize("envname", ["granule", "phased"])
def test_fcollect_collect_broadcast_at_offsets_8_pes(envname):
    run_pes(8, envname, ["coll"] + (["norealign"] if envname == "phased" else []), env=WIDE)


@pytest.mark.parametrize("envname", ["granule", "handshake", "phased"])
def test_scans_and_copies_on_six_pe_teams(envname):
    # Two concurrent strided teams, an offset team, a reversed team (its member 0 is PE 5) and a
    # one-member team.  Scans in granule and handshake (they are order-sensitive: a.src[j], me and
    # exscan's member 0), the copies in every environment.
    run_pes(6, envname, (["scan_teams"] if envname != "phased" else []) + ["coll_teams"], env=WIDE)


@pytest.mark.parametrize("npes", [2, 4])
def test_on_stream_forms_chained_without_sync(npes):
    # scan / fcollect / collect (collect_dyn_kernel) / broadcast on stream: 12 cases each on one
    # stream, own arenas, one synchronisation, *ret preset to 0x7F7F7F7F.
    run_pes(npes, "granule", ["stream"])

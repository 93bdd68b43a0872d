"""Worker body of the multi-PE tests of the 16-bit floating-point reductions (tests/test_gpu_half.py):
one process = one PE, all PEs on one GPU, run with run_pes(..., worker=half_worker.run).

Scenario "half": both types x max / min / sum / prod at n = 1, 7, 8, 9, 1027 and 4099 elements (8
fill one 16-B item, 2 one granule word), inputs = the 16-bit special table and seeded random values
of tests/half_model.py, through every form of the host reduce on whichever path the environment and
the set_param scenarios force.  Every result is held to the model's team-order fold under its
comparison rule (NaN where the model has NaN, either zero for a max / min over zeros of both signs,
the model's bits everywhere else).
Scenario "staged": the host-buffer pipeline over 2 c + 3 elements of the type's chunk.
Scenario "refuse": a sum scan of the ids is refused on every PE before anything is launched.
"""
from __future__ import annotations

import os
import traceback

import numpy as np

SIZES = (1, 7, 8, 9, 1027, 4099)
OFFSETS = (0, 2, 14)
GB = 0xA5
NBIG = 262_147


def run(pe: int, npes: int, key: str, scenarios: list[str], q, env: dict | None = None) -> None:
    fails: list[str] = []
    try:
        for k, v in (env or {}).items():  # a list gives each PE its own value, None removes it
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v[pe] if isinstance(v, list) else v)
        import ishmem_amd as ish
        from ishmem_amd import hip
        from tests import half_model as hm

        ish.init(pe, npes, 0, key)
        # The same switches as tests/mp_worker.py (alike on every PE).
        if "arshift0" in scenarios:
            ish.set_param("ar_shifted", 0)
        if "nodirect" in scenarios:
            ish.set_param("direct_p2", 0)
        if "realigncap" in scenarios:
            ish.set_param("realign_grid_cap", 3)
            ish.set_param("phase_unaligned", 0)
        W, INV = ish.ISHMEM_TEAM_WORLD, ish.ISHMEM_TEAM_INVALID

        def fail(msg):
            fails.append(f"pe{pe} {msg}")

        if "half" in scenarios:
            PADB, nmax = 32, max(SIZES)
            arena = nmax * 2 + 2 * PADB + 16
            base_s, base_d = ish.ishmem_malloc(arena), ish.ishmem_malloc(arena)
            big = ish.ishmem_malloc(NBIG * 2)
            ret = ish.ishmem_malloc(4)
            st = hip.stream_create()
            r, even = ish.ishmem_team_split_strided(W, 0, 2, (npes + 1) // 2)
            r1, solo = ish.ishmem_team_split_strided(W, pe, 1, 1)
            if r or r1 or solo == INV or (even != INV) != (pe % 2 == 0):
                fail(f"team splits rc={r}/{r1} even={even} solo={solo} {ish.last_error()}")
            evens = list(range(0, npes, 2))
            pin = hip.host_malloc(2 * nmax * 2)
            ran = 0

            def reduce(tag, op, kind, dst, src, n, team=W, stream=False, fresh=True):
                """0 if the call succeeded (on a stream: with *ret clean).  fresh: the source was
                written since the last call, so every PE's upload has to be in place first (a blocking
                reduce returns only when no member reads this PE's buffers any more)."""
                nonlocal ran
                ran += 1
                if fresh:
                    ish.ishmem_barrier_all()
                if stream:
                    hip.memset(ret, 0xFF, 4)
                    rc = getattr(ish, f"ishmemx_{kind}_{op}_reduce_on_stream")(team, dst, src, n, ret, st)
                    hip.stream_synchronize(st)
                    rc = rc or int(hip.download(ret, 1, np.int32)[0])
                else:
                    rc = ish.reduce(op, kind, dst, src, n, team)
                if rc:
                    fail(f"{tag}: rc={rc} {ish.last_error()}")
                return rc

            for kind in hm.KINDS:
                for op in hm.OPS:
                    for n in SIZES:
                        tag = f"{op} {kind} n={n}"
                        srcs = hm.sources(kind, op, npes, n)
                        ref = hm.fold(kind, op, srcs)  # once per case, shared by every form

                        def check(t, got, srcs=srcs, ref=ref, op=op, kind=kind):
                            fails.extend(f"pe{pe} {t}: {m}" for m in hm.compare_ref(kind, op, srcs, ref, got)[:2])

                        s0, d0 = base_s + PADB, base_d + PADB
                        hip.upload(s0, srcs[pe])
                        if not reduce(tag, op, kind, d0, s0, n):
                            check(tag, hip.download(d0, n, np.uint16))
                        if not reduce(tag + " on stream", op, kind, d0, s0, n, stream=True):
                            check(tag + " on stream", hip.download(d0, n, np.uint16))
                        if not reduce(tag + " in place", op, kind, s0, s0, n):
                            check(tag + " in place", hip.download(s0, n, np.uint16))
                        # dest and source at every pair of byte offsets, inside guard blocks
                        for so in OFFSETS:
                            hip.memset(base_s, GB, arena)
                            hip.upload(s0 + so, srcs[pe])
                            for do in OFFSETS:
                                t = f"{tag} s+{so} d+{do}"
                                hip.memset(base_d, GB, arena)
                                if reduce(t, op, kind, d0 + do, s0 + so, n, fresh=do == OFFSETS[0]):
                                    continue
                                raw = hip.download(base_d, arena, np.uint8)
                                lo, hi = PADB + do, PADB + do + n * 2
                                check(t, raw[lo:hi].copy().view(np.uint16))
                                if not ((raw[:lo] == GB).all() and (raw[hi:] == GB).all()):
                                    fail(f"{t}: guard bytes around dest written")
                            sraw = hip.download(base_s, arena, np.uint8)
                            if not np.array_equal(sraw[PADB + so:PADB + so + n * 2].view(np.uint16), srcs[pe]) or \
                                    not ((sraw[:PADB + so] == GB).all() and (sraw[PADB + so + n * 2:] == GB).all()):
                                fail(f"{tag} s+{so}: source or its guard bytes written")
                        # the strided team of the even PEs (every PE joins the barriers)
                        tsrcs = hm.sources(kind, op, len(evens), n, seed=1)
                        if even != INV:
                            hip.upload(s0, tsrcs[evens.index(pe)])
                        ish.ishmem_barrier_all()
                        if even != INV:
                            ran += 1
                            if ish.reduce(op, kind, d0, s0, n, even):
                                fail(f"{tag} strided team: {ish.last_error()}")
                            else:
                                got = hip.download(d0, n, np.uint16)
                                fails.extend(f"pe{pe} {tag} strided team: {m}"
                                             for m in hm.compare(kind, op if len(evens) > 1 else "copy", tsrcs, got)[:2])
                        # a team of one: a copy, signalling NaNs and payloads included
                        x = hm.copy_source(kind, n)
                        hip.upload(s0 + 2, x)
                        hip.memset(base_d, GB, arena)
                        if not reduce(tag + " team of one", op, kind, d0, s0 + 2, n, team=solo):
                            raw = hip.download(base_d, arena, np.uint8)
                            if not np.array_equal(raw[PADB:PADB + n * 2].view(np.uint16), x):
                                fail(f"{tag} team of one: dest != source bit for bit")
                            if not ((raw[:PADB] == GB).all() and (raw[PADB + n * 2:] == GB).all()):
                                fail(f"{tag} team of one: guard bytes written")
                # from pageable and from pinned host buffers, through the staging pipeline
                for op, n in (("sum", 4099), ("max", 1027)):
                    srcs = hm.sources(kind, op, npes, n)
                    hsrc, hdst = srcs[pe].copy(), np.zeros(n, np.uint16)
                    t = f"pageable host buffers {op} {kind} n={n}"
                    if not reduce(t, op, kind, hdst.ctypes.data, hsrc.ctypes.data, n):
                        fails.extend(f"pe{pe} {t}: {m}" for m in hm.compare(kind, op, srcs, hdst)[:2])
                    t = f"pinned host buffers {op} {kind} n={n}"
                    hip.memcpy(pin, hsrc.ctypes.data, n * 2)
                    hip.memset(pin + nmax * 2, GB, n * 2)
                    if not reduce(t, op, kind, pin + nmax * 2, pin, n):
                        got = np.zeros(n, np.uint16)
                        hip.memcpy(got.ctypes.data, pin + nmax * 2, n * 2)
                        fails.extend(f"pe{pe} {t}: {m}" for m in hm.compare(kind, op, srcs, got)[:2])
            # in place at 262,147 bfloat16: the size class of the large in-place paths
            srcs = hm.sources("bfloat16", "sum", npes, NBIG)
            hip.upload(big, srcs[pe])
            if not reduce(f"sum bfloat16 n={NBIG} in place", "sum", "bfloat16", big, big, NBIG):
                fails.extend(f"pe{pe} sum bfloat16 n={NBIG} in place: {m}"
                             for m in hm.compare("bfloat16", "sum", srcs, hip.download(big, NBIG, np.uint16))[:2])
            want_calls = 2 * (4 * len(SIZES) * (3 + 9 + 1) + 4) + 1
            if ran < want_calls and not fails:
                fail(f"{ran} of {want_calls} world calls ran")
            ish.ishmem_barrier_all()
            hip.host_free(pin)
            hip.stream_destroy(st)
            ish.ishmem_team_destroy(solo)
            if even != INV:
                ish.ishmem_team_destroy(even)
            for b_ in (ret, big, base_d, base_s):
                ish.ishmem_free(b_)

        if "staged" in scenarios:
            # 2 c + 3 elements of the type's chunk: two full chunks (both slots) and a ragged third.
            from tests import staged_cases as sc
            staging, slots = int(ish.get_param("staging_bytes")), int(ish.get_param("staging_slots"))
            if (staging, slots) != (int(os.environ["STAGED_WANT_BYTES"]), int(os.environ["STAGED_WANT_SLOTS"])):
                fail(f"staging region {staging} B x {slots} slots is not the one the test sets")
            n = 2 * sc.chunk_elems(staging, slots, 2) + 3
            for kind, op in (("bfloat16", "sum"), ("half", "prod")):
                srcs = hm.sources(kind, op, npes, n)
                hsrc, hdst = srcs[pe].copy(), np.full(n + 8, 0xA5A5, np.uint16)
                ish.ishmem_barrier_all()
                if ish.reduce(op, kind, hdst.ctypes.data, hsrc.ctypes.data, n):
                    fail(f"staged {op} {kind} n={n}: {ish.last_error()}")
                    continue
                fails.extend(f"pe{pe} staged {op} {kind} n={n}: {m}" for m in hm.compare(kind, op, srcs, hdst[:n].copy())[:2])
                if not (hdst[n:] == 0xA5A5).all() or not np.array_equal(hsrc, srcs[pe]):
                    fail(f"staged {op} {kind} n={n}: bytes past dest or the source written")

        if "refuse" in scenarios:
            s = ish.ishmem_malloc(64)
            hip.memset(s, GB, 64)
            ish.ishmem_barrier_all()
            for dt in ("half", "bfloat16"):
                for inclusive in (True, False):
                    if ish.scan(dt, inclusive, s + 32, s, 4) == 0 or "invalid dtype" not in ish.last_error():
                        fail(f"sum scan of {dt} was not refused: {ish.last_error()!r}")
                if ish.lib().ishmemi_c_scan_on_stream(W, ish.DTYPES[dt], 1, s + 32, s, 4, None, None) == 0:
                    fail(f"sum scan on a stream of {dt} was not refused")
                for op in ("and", "or", "xor"):
                    if ish.reduce(op, dt, s + 32, s, 4) == 0:
                        fail(f"{op} reduce of {dt} was not refused")
            if not (hip.download(s, 64, np.uint8) == GB).all():
                fail("a refused call wrote its buffers")
            # ... and the team still works: nobody launched anything, nobody waits
            x = hm.sources("bfloat16", "sum", npes, 8)
            hip.upload(s, x[pe])
            if ish.reduce("sum", "bfloat16", s + 32, s, 8):
                fail(f"reduce after the refusals: {ish.last_error()}")
            else:
                fails.extend(f"pe{pe} reduce after the refusals: {m}"
                             for m in hm.compare("bfloat16", "sum", x, hip.download(s + 32, 8, np.uint16)))
            ish.ishmem_barrier_all()
            ish.ishmem_free(s)

        if ish.lib().ishmemi_c_error_count() != 0:
            fail(f"device barrier timeouts: {ish.lib().ishmemi_c_error_count()}")
        ish.ishmem_barrier_all()
        ish.ishmem_finalize()
    except Exception:
        fails.append(f"pe{pe} exception: {traceback.format_exc()}")
    q.put((pe, fails))

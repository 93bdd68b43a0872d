"""Worker body of the team-epoch GPU tests (tests/test_gpu_epochs.py): one process = one PE, all on
one GPU, the test-hooks library loaded (set_param "test_epoch_team" / "test_epoch_advance" /
"test_refresh_every").  Tables and model: tests/epoch_cases.py.

Every call is compared bit for bit with the oracle, dest between two 64-B guards.  Arrival is
skewed so that a wait that lets a launch through early shows as wrong values: before a skewed call
one member (rotating) sleeps SKEW_S on the host and only then uploads its new source and calls; the
others upload and call at once; until then the late member's source holds the previous call's
values, and nothing but the call itself makes the others wait for it (no barrier between calls;
the forms that would first exchange a word over the team run in their stream-ordered form).

Scenarios, on TEAM_WORLD and on a split team of all PEs that ages alone:
  counts  - every row of the table, stream-ordered and blocking, and a host-buffer reduce of two
            staged chunks: the host's launch count rises by at least the epoch's advance.
  past31  - the table at small epochs, 2^31 - 1 launches later the table skewed, with a persistent
            reduce whose Mid rows and claim words nothing touched before.
  wrap    - 32 skewed mixed calls started WRAP_MARGIN launches before 0xFFFFFFFF.
  period  - a granule-path call at its limit and a multi-segment persistent call, run again skewed at
            the very epochs they had one period earlier.
  trigger - the refresh every 7 launches under 100 mixed calls, then resync and the table.
Failures are returned as strings through the queue.
"""
from __future__ import annotations

import os
import time
import traceback

import numpy as np

from tests import epoch_cases as ec

GUARD = 64
GB = 0xA5
MAX_FAILS = 30


def run(pe: int, npes: int, key: str, scenario: str, q, env: dict | None = None, refresh: bool = True) -> None:
    fails: list[str] = []
    try:
        for k, v in (env or {}).items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        import ishmem_amd as ish
        import oracle
        from ishmem_amd import hip

        ish.init(pe, npes, 0, key)
        W = ish.ISHMEM_TEAM_WORLD
        F32 = oracle.DTYPES["float"]
        SUM = oracle.OPS["sum"]
        p = npes
        words = ish.get_param("launch_words")

        def fail(msg):
            if len(fails) < MAX_FAILS:
                fails.append(f"pe{pe} [{scenario} p={npes}] {msg}")

        rc, S = ish.ishmem_team_split_strided(W, 0, 1, npes)
        if rc or S == ish.ISHMEM_TEAM_INVALID:
            raise RuntimeError(f"split: {ish.last_error()}")
        names = {W: "world", S: "split"}
        if not refresh and ish.set_param("test_refresh_every", 0):
            raise RuntimeError(ish.last_error())

        foot = max(ec.footprint(c, p) for c in ec.table())
        sbuf = ish.ishmem_align(256, foot + 2 * GUARD + 256)
        dbuf = ish.ishmem_align(256, foot + 2 * GUARD + 256)
        retbuf = hip.malloc(64)
        if not sbuf or not dbuf:
            raise RuntimeError(f"arenas: {ish.last_error()}")
        src, dst = sbuf + GUARD, dbuf + GUARD

        def epoch(team) -> int:
            return int(hip.download(words + 4 * (team * ec.TEAM_WORDS + ec.EP_EPOCH), 1, np.uint32)[0])

        def launches(team) -> int:
            return ish.get_param(f"team_launches:{team}")

        live = {}

        def configure(name):
            for k, v in ec.CONFIGS[name].items():
                if live.get(k) != v:
                    if ish.set_param(k, v):
                        raise RuntimeError(f"set_param {k}: {ish.last_error()}")
                    live[k] = v

        def advance(team, n):
            e = epoch(team)
            if ish.set_param("test_epoch_team", team) or ish.set_param("test_epoch_advance", n):
                raise RuntimeError(f"test_epoch_advance {n}: {ish.last_error()}")
            if epoch(team) != ec.epoch_after(e, n):
                fail(f"advance {names[team]} by {n}: epoch {e:#x} -> {epoch(team):#x}, the model says {ec.epoch_after(e, n):#x}")

        def check(tag, want):
            want = np.ascontiguousarray(want).view(np.uint8)
            got = hip.download(dst - GUARD, 2 * GUARD + want.size, np.uint8)
            g = np.full(GUARD, GB, np.uint8)
            full = np.concatenate([g, want, g])
            if not np.array_equal(got, full):
                bad = np.nonzero(got != full)[0]
                first = int(bad[0]) - GUARD
                where = "guard before" if first < 0 else "guard after" if first >= want.size else "payload"
                fail(f"{tag}: {len(bad)} of {want.size} bytes differ, first at {first} ({where})")
                return False
            return True

        seq = [0]

        def call(team, c: ec.Case, skew: bool, blocking: bool = False):
            """One call of the table on `team`; True when rc, path and every byte are right."""
            seq[0] += 1
            seed, late = seq[0], seq[0] % p
            me = pe  # both teams hold every PE in world order
            configure(c.config)
            nb = ec.case_bytes(c, p)
            tag = f"#{seed} {names[team]} {c.label}{' skewed' if skew else ''}{' blocking' if blocking else ''}"
            n = nb // 4
            form = c.form
            if form == "team_sync":
                ins, want, out_bytes = [], None, 0
            elif form in ("reduce", "reduce_on_stream"):
                ins = [oracle.fill_random(F32, 1000 * seed + j + 1, n) for j in range(p)]
                want, out_bytes = oracle.reduce_fold(SUM, F32, ins, 0), nb
            elif form == "reduce_scatter":
                ins = [oracle.fill_random(F32, 1000 * seed + j + 1, p * n) for j in range(p)]
                want, out_bytes = oracle.reduce_fold(SUM, F32, ins, 0)[me * n:(me + 1) * n], nb
            elif form == "inscan":
                ins = [oracle.fill_random(F32, 1000 * seed + j + 1, n) for j in range(p)]
                want, out_bytes = oracle.scan_fold(F32, ins, me, True), nb
            elif form == "fcollect":
                ins = [np.random.default_rng([seed, j]).integers(0, 256, nb, dtype=np.uint8) for j in range(p)]
                want, out_bytes = np.concatenate(ins), p * nb
            elif form == "alltoall":
                ins = [np.random.default_rng([seed, j]).integers(0, 256, p * nb, dtype=np.uint8) for j in range(p)]
                want, out_bytes = np.concatenate([ins[j][me * nb:(me + 1) * nb] for j in range(p)]), p * nb
            else:  # broadcast
                ins = [np.random.default_rng([seed, j]).integers(0, 256, nb, dtype=np.uint8) for j in range(p)]
                want, out_bytes = ins[seed % p], nb
            if skew and me == late:
                time.sleep(ec.SKEW_S)
            if ins:
                hip.memset(dst - GUARD, GB, 2 * GUARD + out_bytes)
                hip.upload(src, ins[me])
            st = 0  # the null stream
            if form == "team_sync":
                r = ish.ishmem_team_sync(team)
            elif form == "reduce":
                r = ish.reduce("sum", "float", dst, src, n, team)
            elif form == "reduce_on_stream":
                r = ish.reduce_on_stream("sum", "float", dst, src, n, retbuf, st, team)
            elif form == "reduce_scatter":
                r = (ish.reduce_scatter("sum", "float", dst, src, n, team) if blocking else
                     ish.reduce_scatter_on_stream("sum", "float", dst, src, n, retbuf, st, team))
            elif form == "inscan":
                r = (ish.scan("float", True, dst, src, n, team) if blocking else
                     ish.lib().ishmemi_c_scan_on_stream(team, ish.DTYPES["float"], 1, dst, src, n, retbuf, None))
            elif form == "fcollect":
                r = (ish.ishmem_fcollectmem(team, dst, src, nb) if blocking else
                     ish.fcollect_on_stream(dst, src, nb, retbuf, st, team))
            elif form == "alltoall":
                r = (ish.ishmem_alltoallmem(team, dst, src, nb) if blocking else
                     ish.alltoall_on_stream(dst, src, nb, retbuf, st, team))
            else:
                r = (ish.ishmem_broadcastmem(team, dst, src, nb, seed % p) if blocking else
                     ish.broadcast_on_stream(dst, src, nb, seed % p, retbuf, st, team))
            path = ish.last_path()
            stream_ordered = form == "reduce_on_stream" or (not blocking and form not in ("team_sync", "reduce"))
            if stream_ordered and not r:
                hip.synchronize()
                r = int(hip.download(retbuf, 1, np.int32)[0])
            if r:
                fail(f"{tag}: rc={r} {ish.last_error()}")
                return False
            ok = True
            if form != "team_sync":
                if (c.path is not None and path != c.path) or (c.path is None and path == "granule"):
                    fail(f"{tag}: last_path {path}, meant to take {c.path or 'a barrier path'}")
                    ok = False
                ok = check(tag, want) and ok
            return ok

        def warm_up(team, k=2):
            for _ in range(k):
                if ish.ishmem_team_sync(team):
                    raise RuntimeError(f"team_sync: {ish.last_error()}")

        def budget(skewed):
            if skewed > ec.MAX_SKEWED:
                fail(f"{skewed} skewed calls, the budget is {ec.MAX_SKEWED}")

        if scenario == "counts":
            deepest = {}
            for team in (W, S):
                warm_up(team)
                for blocking in (False, True):
                    for c in ec.table():
                        if blocking and c.form in ("reduce", "reduce_on_stream", "team_sync"):
                            continue
                        e0, n0 = epoch(team), launches(team)
                        if not call(team, c, False, blocking):
                            continue
                        path = "sync" if c.form == "team_sync" else ish.last_path()
                        de, dn = ec.launches_between(e0, epoch(team)), launches(team) - n0
                        if not 1 <= de <= dn:
                            fail(f"{names[team]} {c.label} blocking={blocking}: epoch advanced {de}, host count {dn}")
                        deepest[path] = max(deepest.get(path, 0), de)
                # Host buffers: two staged chunks, each a launch (or several) of its own.
                configure("granule")
                n = ec.STAGED_ELEMS
                ins = [oracle.fill_random(F32, 77_000 + 10 * team + j, n) for j in range(p)]
                hsrc, hdst = ins[pe].copy(), np.zeros(n, np.float32)
                e0, n0 = epoch(team), launches(team)
                if ish.reduce("sum", "float", hdst.ctypes.data, hsrc.ctypes.data, n, team):
                    fail(f"{names[team]} host-buffer reduce: {ish.last_error()}")
                de, dn = ec.launches_between(e0, epoch(team)), launches(team) - n0
                if not 2 <= de <= dn:
                    fail(f"{names[team]} host-buffer reduce over two chunks: epoch advanced {de}, host count {dn}")
                if not np.array_equal(hdst.view(np.uint32), oracle.reduce_fold(SUM, F32, ins, 0).view(np.uint32)):
                    fail(f"{names[team]} host-buffer reduce: wrong values")
            for path in ("granule", "fold", "persistent", "phased"):
                if deepest.get(path, 0) < 2:
                    fail(f"no call on the {path} path advanced the epoch by more than 1 ({deepest})")

        elif scenario == "past31":
            for team in (W, S):
                warm_up(team)
                for c in ec.table(large=False):
                    call(team, c, False)
            e = epoch(S)
            if not 2 <= e < 100 or not 2 <= epoch(W) < 100:
                fail(f"epochs {e} / {epoch(W)} before the advance, meant to be under 100")
            advance(S, ec.MAX_ADVANCE)
            if launches(S) < ec.REFRESH_LAUNCHES:
                fail(f"host count {launches(S)} after the advance")
            skewed = 0
            for c in ec.table(large=True):
                call(S, c, True)
                skewed += 1
            if epoch(S) < 1 << 31:
                fail(f"split epoch {epoch(S):#x} is not past 2^31")
            if refresh and launches(S) >= 100:
                fail(f"host count {launches(S)}: no refresh ran on the aged team")
            for c in ec.table(large=False):
                call(W, c, True)
                skewed += 1
            if not 2 <= epoch(W) < 200 or launches(W) >= 400:
                fail(f"world epoch {epoch(W)} / count {launches(W)}: the split team's age leaked into it")
            budget(skewed)

        elif scenario == "wrap":
            warm_up(S)
            warm_up(W)
            advance(S, ec.MAX_ADVANCE)
            warm_up(S, 1)  # refreshed here: the rows are never more than 2^31 launches old
            n2 = ec.launches_between(epoch(S), ec.MASK - ec.WRAP_MARGIN)
            advance(S, n2)
            if epoch(S) != ec.MASK - ec.WRAP_MARGIN:
                fail(f"start epoch {epoch(S):#x}")
            seen = []  # (epoch before, epoch after, path) per call
            calls = ec.mixed(32)
            for c in calls:
                e0 = epoch(S)
                ok = call(S, c, True)
                seen.append((e0, epoch(S), "sync" if c.form == "team_sync" else ish.last_path(), ok))
            if any(e1 in (0, 1) for _, e1, _, _ in seen):
                fail(f"an epoch read 0 or 1: {[hex(e1) for _, e1, _, _ in seen]}")
            wrapped = [i for i, (e0, e1, _, _) in enumerate(seen) if e1 < e0]
            if len(wrapped) != 1:
                fail(f"the wrap was crossed {len(wrapped)} times: {[hex(e1) for _, e1, _, _ in seen]}")
            else:
                w = wrapped[0]
                # A granule call is one launch: its epoch is the one read back after it.
                before = {e1 & 1 for e0, e1, path, _ in seen[:w] if path == "granule" and ec.launches_between(e0, e1) == 1}
                after = {e1 & 1 for e0, e1, path, _ in seen[w + 1:] if path == "granule" and ec.launches_between(e0, e1) == 1}
                if before != {0, 1} or after != {0, 1}:
                    fail(f"granule-path parities before the wrap {sorted(before)}, after it {sorted(after)}")
            for c in ec.table()[:4]:
                call(W, c, True)
            if not 2 <= epoch(W) < 100:
                fail(f"world epoch {epoch(W)}")
            budget(len(calls) + 4)

        elif scenario == "period":
            warm_up(S, 6)
            warm_up(W)
            A, B = ec.table()[2], ec.LARGE  # the granule path at its limit; several segments
            if A.nbytes != 0 or A.config != "granule":
                raise RuntimeError("table()[2] is not the granule-limit reduce")
            call(S, A, False)
            e1 = epoch(S)
            call(S, B, False)
            e2 = epoch(S)
            if e2 != ec.step(e1):
                fail(f"the persistent call took {ec.launches_between(e1, e2)} launches")
            # The refresh before the replayed call A costs two launches (its barriers), A one: A runs
            # at e1 again when the epoch before them is three launches short of it.  The two
            # team_syncs between the hook's steps cost three each (refresh + barrier).
            between = 3 if refresh else 1
            start = ec.FIRST_AFTER_WRAP + (e1 - ec.FIRST_AFTER_WRAP - between) % ec.PERIOD
            total = ec.launches_between(e2, start) - 2 * between
            steps = ec.advance_steps(total, 3)
            for i, n in enumerate(steps):
                advance(S, n)
                if i < 2:
                    warm_up(S, 1)
            if epoch(S) != start:
                fail(f"epoch {epoch(S):#x} before the replay, meant {start:#x}")
            okA = call(S, A, True)
            if epoch(S) != e1:
                fail(f"the granule call ran at {epoch(S):#x}, one period ago at {e1:#x}")
            okB = call(S, B, True)
            if epoch(S) != e2:
                fail(f"the persistent call ran at {epoch(S):#x}, one period ago at {e2:#x}")
            if not (okA and okB) and not fails:
                fail("a replayed call failed")
            for c in (A, B):
                call(W, c, True)
            budget(4)

        elif scenario == "trigger":
            if ish.set_param("test_refresh_every", ec.REFRESH_EVERY_E):
                raise RuntimeError(ish.last_error())
            warm_up(S)
            skewed = refreshes = 0
            prev = launches(S)
            for i, c in enumerate(ec.mixed(ec.CALLS_E)):
                skew = i % ec.SKEW_EVERY_E == 0
                skewed += skew
                call(S, c, skew)
                now = launches(S)
                refreshes += now < prev
                if now > ec.REFRESH_EVERY_E + 8:
                    fail(f"call {i}: host count {now} with a refresh due every {ec.REFRESH_EVERY_E}")
                prev = now
            if refreshes < 10:
                fail(f"{refreshes} refreshes over {ec.CALLS_E} calls")
            if ish.resync():
                fail(f"resync: {ish.last_error()}")
            if launches(S) != 0 or launches(W) != 0:
                fail(f"host counts {launches(S)} / {launches(W)} after resync")
            for c in ec.table():
                call(S, c, True)
                skewed += 1
            for c in ec.table()[:2]:
                call(W, c, False)
            budget(skewed)
        else:
            raise RuntimeError(f"unknown scenario {scenario}")

        ish.ishmem_barrier_all()
        if ish.lib().ishmemi_c_error_count() != 0:
            fail(f"device error count {ish.lib().ishmemi_c_error_count()}")
        hip.free(retbuf)
        ish.ishmem_free(dbuf)
        ish.ishmem_free(sbuf)
        ish.ishmem_team_destroy(S)
        ish.ishmem_finalize()
    except Exception:
        fails.append(f"pe{pe} exception:\n{traceback.format_exc()}")
    q.put((pe, fails))

"""Worker body of the multi-PE alltoall GPU tests (tests/test_gpu_alltoall.py): one process = one
PE, all PEs on one GPU, symmetric heaps mapped into each other over HIP IPC.

The expected result is computed here in numpy — expected[i][j] = source[j][i], block by block — for
two kinds of input per shape: the reference tester's pattern (test/unit/alltoall.cpp:47-90) and
seeded random bytes (for blocks under 5 bytes the tester's pattern is the same for every pair of
members).  dest sits between two 64-byte guards of 0xA5 which must come back unchanged; the
comparison is bit-exact.  Failures are returned as strings through the queue.
"""
from __future__ import annotations

import os
import time
import traceback

import numpy as np

GUARD = 64
MAXP = 8
MAX_BLOCK = (1 << 20) + 16


def pattern_block(nelems: int, f: int, t: int, nbytes: int) -> np.ndarray:
    """The block member f sends to member t: word k = (nelems<<48) + ((0x80+f)<<40) + ((0x80+t)<<32) + k
    as little-endian int64 (wrapping), truncated to nbytes."""
    base = ((nelems << 48) + ((0x80 + f) << 40) + ((0x80 + t) << 32)) & 0xFFFFFFFFFFFFFFFF
    words = (np.arange((nbytes + 7) // 8, dtype=np.uint64) + np.uint64(base)).astype("<u8")
    return words.view(np.uint8)[:nbytes]


def member_source(kind: str, seed: int, nelems: int, f: int, p: int, nbytes: int) -> np.ndarray:
    """All p blocks of member f's source (p * nbytes bytes)."""
    if kind == "tester":
        return np.concatenate([pattern_block(nelems, f, t, nbytes) for t in range(p)]) if nbytes else np.zeros(0, np.uint8)
    return np.random.default_rng([seed, f]).integers(0, 256, p * nbytes, dtype=np.uint8)


def expected_dest(kind: str, seed: int, nelems: int, me: int, p: int, nbytes: int) -> np.ndarray:
    if kind == "tester":
        return np.concatenate([pattern_block(nelems, j, me, nbytes) for j in range(p)]) if nbytes else np.zeros(0, np.uint8)
    return np.concatenate([member_source(kind, seed, nelems, j, p, nbytes)[me * nbytes:(me + 1) * nbytes]
                           for j in range(p)])


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

        ish.init(pe, npes, 0, key)
        W = ish.ISHMEM_TEAM_WORLD
        # The environment took effect: a path must not go untested in silence.
        if "ISHMEM_LL_MAX_BYTES" in (env or {}) and env["ISHMEM_LL_MAX_BYTES"] is not None:
            if int(ish.get_param("ll_max_bytes")) != int(env["ISHMEM_LL_MAX_BYTES"]):
                fails.append(f"pe{pe}: ll_max_bytes {ish.get_param('ll_max_bytes')} != {env['ISHMEM_LL_MAX_BYTES']}")
            if int(env["ISHMEM_LL_MAX_BYTES"]) == 0 and int(ish.get_param("ll_limit_bytes")) != 0:
                fails.append(f"pe{pe}: granule path still on (ll_limit_bytes {ish.get_param('ll_limit_bytes')})")
        if "ISHMEM_PHASED_MIN_BYTES" in (env or {}) and env["ISHMEM_PHASED_MIN_BYTES"] is not None:
            if int(ish.get_param("phased_min_bytes")) != int(env["ISHMEM_PHASED_MIN_BYTES"]):
                fails.append(f"pe{pe}: phased_min_bytes {ish.get_param('phased_min_bytes')}")
        if env and "ISHMEM_LL_MAX_BYTES" not in env and "ISHMEM_PHASED_MIN_BYTES" not in env:
            if int(ish.get_param("ll_limit_bytes")) <= 0 or int(ish.get_param("phased_min_bytes")) <= 0:
                fails.append(f"pe{pe}: default thresholds expected, got ll_limit {ish.get_param('ll_limit_bytes')} "
                             f"phased_min {ish.get_param('phased_min_bytes')}")

        # One source and one dest arena for every case (256-B aligned bases).
        arena = MAXP * MAX_BLOCK + 2 * GUARD + 256
        sbuf = ish.ishmem_align(256, arena)
        dbuf = ish.ishmem_align(256, arena)
        ret = ish.ishmem_malloc(4)
        case_no = [0]

        def put_inputs(kind, seed, nelems, me, p, B, soff, doff):
            """Uploads this member's source at sbuf + soff and 0xA5 over dest and both guards; returns
            (source address, dest address)."""
            if p * B:
                hip.upload(sbuf + soff, member_source(kind, seed, nelems, me, p, B))
            hip.upload(dbuf + doff, np.full(2 * GUARD + p * B, 0xA5, np.uint8))
            return sbuf + soff, dbuf + doff + GUARD

        def check(tag, kind, seed, nelems, me, p, B, doff, touched=True):
            got = hip.download(dbuf + doff, 2 * GUARD + p * B, np.uint8)
            g = np.full(GUARD, 0xA5, np.uint8)
            body = expected_dest(kind, seed, nelems, me, p, B) if touched else np.full(p * B, 0xA5, np.uint8)
            want = np.concatenate([g, body, g])
            if not np.array_equal(got, want):
                bad = np.nonzero(got != want)[0]
                where = "guard" if (bad[0] < GUARD or bad[0] >= GUARD + p * B) else f"block {(bad[0] - GUARD) // max(B, 1)}"
                fails.append(f"pe{pe} {tag}: {len(bad)} bytes differ, first at {int(bad[0]) - GUARD} ({where})")

        def one(tag, team, me, p, B, nelems, soff=0, doff=0, kinds=("tester", "random"), call=None):
            for kind in kinds:
                case_no[0] += 1
                seed = case_no[0]
                src, dst = put_inputs(kind, seed, nelems, me, p, B, soff, doff)
                rc = call(team, dst, src) if call else ish.ishmem_alltoallmem(team, dst, src, B)
                if rc:
                    fails.append(f"pe{pe} {tag} {kind}: rc={rc} {ish.last_error()}")
                    return False
                check(f"{tag} {kind}", kind, seed, nelems, me, p, B, doff)
            return True

        if "sizes" in scenarios:
            # Both arrays 16-B aligned; every size at which a kernel takes another path.
            # lim: the largest block that takes the granule path for this team (with the path
            # switched off, the size it would be: the same bytes then go through the other kernels).
            lim = min(int(ish.get_param("ll_limit_bytes")) or (512 << 10), int(ish.get_param("ll_capacity_bytes")) // 2)
            sizes = [1, 2, 3, 7, 8, 9, 12, 15, 16, 17, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 4099,
                     280_004, (1 << 20) + 16, lim, lim + 8]
            for B in sizes:
                if not one(f"sizes B={B}", W, pe, npes, B, B):
                    break

        if "shifted" in scenarios:
            ok = True
            for n in (1, 5, 15, 1000):
                for soff in (0, 4, 8, 12):
                    for doff in (0, 4, 8):
                        ok = ok and one(f"shifted float n={n} s+{soff} d+{doff}", W, pe, npes, 4 * n, n, soff, doff,
                                        call=lambda t, d, s, n=n: ish.ishmem_float_alltoall(t, d, s, n))
            for B in (13, 1000, 70_003):
                for soff in (1, 3):
                    for doff in (0, 2):
                        ok = ok and one(f"shifted uint8 B={B} s+{soff} d+{doff}", W, pe, npes, B, B, soff, doff,
                                        call=lambda t, d, s, B=B: ish.ishmem_uint8_alltoall(t, d, s, B))

        if "sizes" in scenarios and "shifted" in scenarios and not fails:
            # Every shape ran, with both kinds of input: 24 sizes, 48 float and 12 uint8 shifts.
            if case_no[0] != 2 * (24 + 48 + 12):
                fails.append(f"pe{pe}: {case_no[0]} cases ran, expected {2 * (24 + 48 + 12)}")

        if "teams" in scenarios:
            # 4 PEs.  Two concurrent strided teams {0,2} and {1,3}: a member's index in the team is
            # not its world PE number.
            assert npes == 4
            r, tx, t2 = ish.ishmem_team_split_2d(W, 2)  # y-axis teams: {0,2} and {1,3}
            if r or t2 == ish.ISHMEM_TEAM_INVALID:
                fails.append(f"pe{pe} teams: strided split failed: {ish.last_error()}")
            else:
                me2 = ish.ishmem_team_my_pe(t2)
                if me2 != pe // 2:
                    fails.append(f"pe{pe} teams: index {me2} in the strided team")
                for B in (4, 24, 4099, 300_000):
                    case_no[0] += 1000 * (pe % 2)  # the two teams run different data
                    one(f"teams strided B={B}", t2, me2, 2, B, B)
                    case_no[0] -= 1000 * (pe % 2)
                ish.ishmem_team_sync(t2)
                ish.ishmem_team_destroy(t2)
                ish.ishmem_team_destroy(tx)
            ish.ishmem_barrier_all()
            # {0,1,2} of 4: PE 3 does not call.
            r, t3 = ish.ishmem_team_split_strided(W, 0, 1, 3)
            if pe < 3:
                if r or t3 == ish.ISHMEM_TEAM_INVALID:
                    fails.append(f"pe{pe} teams: 3-member split failed: {ish.last_error()}")
                else:
                    for B in (8, 1000, 70_003):
                        one(f"teams 3of4 B={B}", t3, pe, 3, B, B)
                    ish.ishmem_team_destroy(t3)
            ish.ishmem_barrier_all()
            # One member: a copy of one block.
            r, t1 = ish.ishmem_team_split_strided(W, pe, 1, 1)
            if r or t1 == ish.ISHMEM_TEAM_INVALID:
                fails.append(f"pe{pe} teams: 1-member split failed: {ish.last_error()}")
            else:
                for B in (5, 4096, 70_003):
                    case_no[0] += 100 * pe
                    one(f"teams single B={B}", t1, 0, 1, B, B)
                    case_no[0] -= 100 * pe
                ish.ishmem_team_destroy(t1)
            ish.ishmem_barrier_all()
            # nelems == 0: returns 0, dest untouched.
            src, dst = put_inputs("random", 1, 0, pe, npes, 16, 0, 0)
            rc = ish.ishmem_int_alltoall(dst, src, 0)
            if rc:
                fails.append(f"pe{pe} teams nelems=0: rc={rc} {ish.last_error()}")
            check("teams nelems=0", "random", 1, 0, pe, npes, 16, 0, touched=False)

        if "chain" in scenarios:
            # 24 calls back to back on one stream, no host synchronisation: alltoall / fcollect /
            # f32 sum reduce in turn, random sizes up to the granule limit, random host delays per PE,
            # every call with its own dest slice checked at the end (the ring's parity alternation
            # across modes).
            K = 24
            rng = np.random.default_rng(20260)
            lim = min(int(ish.get_param("ll_limit_bytes")), int(ish.get_param("ll_capacity_bytes")) // 2)
            plan = []
            for k in range(K):
                kind = ("alltoall", "fcollect", "reduce")[k % 3]
                B = max(1, int(np.exp(rng.uniform(0.0, np.log(lim)))))
                if kind == "reduce":
                    B = max(4, B & ~3)
                plan.append((kind, B))
            bufs = []
            for k, (kind, B) in enumerate(plan):
                if kind == "alltoall":
                    ins = [member_source("random", 7000 + k, 0, j, npes, B) for j in range(npes)]
                    sb, db = ish.ishmem_malloc(npes * B), ish.ishmem_malloc(npes * B)
                elif kind == "fcollect":
                    ins = [np.random.default_rng([7000 + k, j]).integers(0, 256, B, dtype=np.uint8) for j in range(npes)]
                    sb, db = ish.ishmem_malloc(B), ish.ishmem_malloc(npes * B)
                else:
                    ins = [np.random.default_rng([7000 + k, j]).integers(-1000, 1000, B // 4).astype(np.float32)
                           for j in range(npes)]
                    sb, db = ish.ishmem_malloc(B), ish.ishmem_malloc(B)
                hip.upload(sb, ins[pe])
                bufs.append((sb, db, ins))
            st = hip.stream_create()
            hip.memset(ret, 0, 4)
            ish.ishmem_barrier_all()
            delays = np.random.default_rng(77 + pe).uniform(0, 2e-4, K)
            for k, (kind, B) in enumerate(plan):
                time.sleep(float(delays[k]))  # host skew between the PEs, at most 0.2 ms a call
                sb, db, _ = bufs[k]
                if kind == "alltoall":
                    r = ish.alltoall_on_stream(db, sb, B, ret, st)
                elif kind == "fcollect":
                    r = ish.fcollect_on_stream(db, sb, B, ret, st)
                else:
                    r = ish.reduce_on_stream("sum", "float", db, sb, B // 4, ret, st)
                if r:
                    fails.append(f"pe{pe} chain k={k} {kind}: rc={r} {ish.last_error()}")
                    break
            hip.stream_synchronize(st)
            if int(hip.download(ret, 1, np.int32)[0]) != 0:
                fails.append(f"pe{pe} chain: *ret set")
            for k, (kind, B) in enumerate(plan):
                sb, db, ins = bufs[k]
                if kind == "alltoall":
                    want = np.concatenate([ins[j][pe * B:(pe + 1) * B] for j in range(npes)])
                    got = hip.download(db, npes * B, np.uint8)
                elif kind == "fcollect":
                    want, got = np.concatenate(ins), hip.download(db, npes * B, np.uint8)
                else:
                    # Integer-valued floats below 2^24 in total: the sum is exact in any order.
                    want = np.sum(np.stack(ins).astype(np.float64), axis=0).astype(np.float32).view(np.uint8)
                    got = hip.download(db, B // 4, np.float32).view(np.uint8)
                if not np.array_equal(got, want):
                    fails.append(f"pe{pe} chain k={k} {kind} B={B} wrong")
                ish.ishmem_free(db)
                ish.ishmem_free(sb)
            # deps / done: the call waits for `dep`, `done` is recorded after it, *ret == 0.
            dep, done = hip.Event(), hip.Event()
            B = 4099
            src, dst = put_inputs("random", 555, B, pe, npes, B, 0, 0)
            hip.memset(ret, 0xFF, 4)
            ish.ishmem_barrier_all()
            dep.record(st)
            r = ish.alltoall_on_stream(dst, src, B, ret, st, deps=[dep], done=done)
            if r:
                fails.append(f"pe{pe} deps: rc={r} {ish.last_error()}")
            else:
                done.synchronize()  # raises if `done` was never recorded on a stream
                if int(hip.download(ret, 1, np.int32)[0]) != 0:
                    fails.append(f"pe{pe} deps: *ret != 0")
                check("deps", "random", 555, B, pe, npes, B, 0)
            hip.stream_synchronize(st)
            hip.stream_destroy(st)

        if "graph" in scenarios:
            # Three alltoalls (granule, handshake and - with its own threshold - phased size) captured
            # on a single stream into a HIP graph, replayed twice with fresh inputs.
            st = hip.stream_create()
            Bs = (600, 700_000, 2_000_003)
            tot = sum(npes * B for B in Bs)
            gs, gd = ish.ishmem_align(256, tot + 256), ish.ishmem_align(256, tot + 256)
            offs = np.cumsum([0] + [npes * B for B in Bs])
            ish.ishmem_barrier_all()
            with hip.Graph(st) as g:
                for i, B in enumerate(Bs):
                    if ish.alltoall_on_stream(gd + int(offs[i]), gs + int(offs[i]), B, ret, st):
                        fails.append(f"pe{pe} graph capture B={B}: {ish.last_error()}")
            for rep in range(2):
                for i, B in enumerate(Bs):
                    hip.upload(gs + int(offs[i]), member_source("random", 8000 + 10 * rep + i, 0, pe, npes, B))
                hip.memset(gd, 0xA5, tot)
                hip.memset(ret, 0xFF, 4)
                ish.ishmem_barrier_all()  # everyone's inputs are in place
                g.launch()
                hip.stream_synchronize(st)
                if int(hip.download(ret, 1, np.int32)[0]) != 0:
                    fails.append(f"pe{pe} graph replay {rep}: ret != 0")
                for i, B in enumerate(Bs):
                    want = expected_dest("random", 8000 + 10 * rep + i, 0, pe, npes, B)
                    if not np.array_equal(hip.download(gd + int(offs[i]), npes * B, np.uint8), want):
                        fails.append(f"pe{pe} graph replay {rep} B={B} wrong")
                ish.ishmem_barrier_all()  # nobody refills a source a peer's replay still reads
            del g
            hip.stream_destroy(st)
            ish.ishmem_free(gd)
            ish.ishmem_free(gs)

        if "argfail" in scenarios:
            # None of these may hang; each is followed by a correct alltoall on the same team.
            B = 1000
            plain = hip.malloc(npes * B)

            def expect_fail(tag, rc, word):
                if rc == 0:
                    fails.append(f"pe{pe} argfail {tag}: returned 0")
                elif word not in ish.last_error():
                    fails.append(f"pe{pe} argfail {tag}: message '{ish.last_error()}' lacks '{word}'")

            def good(tag):
                ish.ishmem_barrier_all()
                one(f"argfail after {tag}", W, pe, npes, B, B, kinds=("random",))

            # One member alone passes a non-heap source to the blocking call: every member fails.
            src, dst = put_inputs("random", 1, B, pe, npes, B, 0, 0)
            rc = ish.ishmem_alltoallmem(dst, plain if pe == npes - 1 else src, B)
            expect_fail("one non-heap source", rc, "symmetric-heap")
            good("one non-heap source")
            # dest == source, and a partial overlap.
            rc = ish.ishmem_alltoallmem(sbuf, sbuf, B)
            expect_fail("dest == source", rc, "overlap")
            good("dest == source")
            rc = ish.ishmem_alltoallmem(sbuf + npes * B - 8, sbuf, B)
            expect_fail("partial overlap", rc, "overlap")
            good("partial overlap")
            # A caller that is not a member: the others complete the call without it.
            r, sub = ish.ishmem_team_split_strided(W, 0, 1, npes - 1)
            if pe == npes - 1:
                # The split gave this PE no handle; 3 is the slot its members hold (no other user
                # team exists here), which on this PE names no team it belongs to.
                rc = ish.lib().ishmemi_c_alltoall(3, dbuf + 4096, sbuf, B)
                expect_fail("not a member", rc, "member")
                case_no[0] += 1  # the members' case below: the seeds stay in step
            elif r == 0:
                one("argfail sub-team", sub, pe, npes - 1, B, B, kinds=("random",))
                ish.ishmem_team_destroy(sub)
            else:
                fails.append(f"pe{pe} argfail: split failed: {ish.last_error()}")
                case_no[0] += 1
            good("not a member")
            # An invalid team handle.
            rc = ish.ishmem_alltoallmem(57, dst, src, B)
            expect_fail("invalid team", rc, "invalid team")
            rc = ish.ishmem_alltoallmem(ish.ISHMEM_TEAM_INVALID, dst, src, B)
            expect_fail("ISHMEM_TEAM_INVALID", rc, "invalid team")
            good("invalid team")
            # Every member passes a non-heap source to the on-stream call: each fails locally.
            rc = ish.alltoall_on_stream(dst, plain, B, ret, 0)
            expect_fail("on-stream non-heap source", rc, "symmetric-heap")
            good("on-stream non-heap source")
            hip.free(plain)

        ish.ishmem_barrier_all()
        if ish.lib().ishmemi_c_error_count() != 0:
            fails.append(f"pe{pe}: device error count {ish.lib().ishmemi_c_error_count()}")
        ish.ishmem_free(ret)
        ish.ishmem_free(dbuf)
        ish.ishmem_free(sbuf)
        ish.ishmem_finalize()
    except Exception:
        fails.append(f"pe{pe} exception:\n{traceback.format_exc()}")
    q.put((pe, fails))

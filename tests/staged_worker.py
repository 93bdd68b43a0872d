"""Worker body of the host-buffer reduce tests (tests/test_gpu_staged.py): one process = one PE,
all PEs on one GPU.  Case tables and the chunk-plan model are in tests/staged_cases.py.

Every reduce here has a source or dest outside the symmetric heap, so it runs through
reduce_staged / reduce_staged_pipeline (runtime.cpp): copy-in, in-place collective on a staging
slot, copy-out, slot by slot.  The staging region is shrunk to 1 MiB (STAGED_WANT_BYTES /
STAGED_WANT_SLOTS carry what the test set); before a case runs, the plan the live staging_bytes /
staging_slots give is compared with the one the table promises, so no case passes because the region
was silently larger.

Inputs are oracle.fill_random over the full range, seeded per case and per PE.  Every dest sits in
a larger allocation of its kind as [4 KiB of 0x3C | payload | 4 KiB of 0x3C]; payload and guards are
read back after every call (host memory directly, with no HIP call in between) and compared under
the rule of mp_worker's check(): bit-exact against oracle.reduce_fold's canonical fold, FP sum /
prod also within the existing tolerance of the reference's own-PE fold.  Failures are returned as
strings through the queue.
"""
from __future__ import annotations

import ctypes
import os
import traceback

import numpy as np

from tests import staged_cases as sc

PAD = sc.PAD
MAX_FAILS = 40
PRESET = 0xFF  # every byte of *ret before an on-stream call
LAST_FIRST = PAD + 64 + (64 << 10)  # bytes at the end of a host arena that Buf.raw reads first


class Buf:
    """[PAD | payload at +off | PAD (+ slack)] of pageable host, pinned host or plain device memory.
    The arena starts a page (pageable: aligned by hand), so off = 0 puts the payload on a page
    boundary and off = one element puts it off the 16-B phase and off the page."""

    def __init__(self, hip, kind: str, nbytes: int, off: int = 0):
        self.hip, self.kind, self.nbytes, self.off = hip, kind, nbytes, off
        self.total = 2 * PAD + nbytes + 64
        assert 0 <= off <= 64
        if kind == "pageable":
            self.arena = np.empty(self.total + PAD, np.uint8)
            skip = -self.arena.ctypes.data % PAD
            self.view = self.arena[skip:skip + self.total]
            self.base = self.view.ctypes.data
        elif kind == "pinned":
            self.base = hip.host_malloc(self.total)
            self.view = np.ctypeslib.as_array((ctypes.c_uint8 * self.total).from_address(self.base))
        else:
            assert kind == "device"
            self.base = hip.malloc(self.total)
            self.view = None
        assert self.base % PAD == 0
        self.ptr = self.base + PAD + off

    def fill(self) -> None:
        if self.view is not None:
            self.view[:] = sc.GUARD_BYTE
        else:
            self.hip.memset(self.base, sc.GUARD_BYTE, self.total)
            self.hip.synchronize()

    def put(self, arr: np.ndarray) -> None:
        b = np.ascontiguousarray(arr).view(np.uint8)
        assert b.size == self.nbytes
        if self.view is not None:
            self.view[PAD + self.off:PAD + self.off + b.size] = b
        else:
            self.hip.upload(self.ptr, b)
            self.hip.synchronize()

    def raw(self) -> np.ndarray:
        """The whole arena as it is now.  Host memory is read directly, its last 64 KiB first: the
        pipeline writes them last, so a call that returned before its last copy-out shows here."""
        if self.view is not None:
            cut = max(0, self.total - LAST_FIRST)
            tail = self.view[cut:].copy()
            return np.concatenate([self.view[:cut], tail])
        return self.hip.download(self.base, self.total, np.uint8)

    def free(self) -> None:
        if self.kind == "pinned":
            self.view = None
            self.hip.host_free(self.base)
        elif self.kind == "device":
            self.hip.free(self.base)
        self.base = self.ptr = 0


def run(pe: int, npes: int, key: str, scenarios: list[str], q, env: dict | None = None) -> None:
    fails: list[str] = []
    try:
        for k, v in (env or {}).items():  # a list gives each PE its own value, None removes it
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v[pe] if isinstance(v, list) else v)
        import oracle
        import ishmem_amd as ish
        from ishmem_amd import hip

        ish.init(pe, npes, 0, key)
        W, INV = ish.ISHMEM_TEAM_WORLD, ish.ISHMEM_TEAM_INVALID
        OPS, DT = oracle.OPS, oracle.DTYPES
        ran = {"n": 0}

        def fail(msg):
            if len(fails) < MAX_FAILS:
                fails.append(f"pe{pe} {msg}")

        # The staging region is the one the test set.
        want_bytes, want_slots = int(os.environ["STAGED_WANT_BYTES"]), int(os.environ["STAGED_WANT_SLOTS"])
        live_bytes, live_slots = int(ish.get_param("staging_bytes")), int(ish.get_param("staging_slots"))
        if (live_bytes, live_slots) != (want_bytes, want_slots):
            fail(f"staging region {live_bytes} B x {live_slots} slots, the test sets {want_bytes} x {want_slots}")
        if int(ish.get_param("staged_copy_kernel")) != 0:
            fail(f"staged_copy_kernel {ish.get_param('staged_copy_kernel')} at start")

        def plan_ok(tag, staging, slots, es, n):
            """The live plan is the one the table promises for (staging, slots)."""
            live = sc.chunk_plan(live_bytes, live_slots, es, n)
            want = sc.chunk_plan(staging, slots, es, n)
            if live != want:
                fail(f"{tag}: the live plan has {len(live)} chunks (last {live[-1]}), the table promises "
                     f"{len(want)} (last {want[-1]})")
            return live == want

        def inputs(op, dtype, n, seed, members):
            lo, hi = (0.5, 2.0) if op == "prod" else (-1.0, 1.0)  # as the golden inputs
            return [oracle.fill_random(DT[dtype], seed + 1009 * j, n, lo, hi) for j in members]

        def check(tag, op, dtype, srcs, got, me):
            """mp_worker's check(): the canonical team-order fold bit for bit; FP sum / prod within
            twice fp_tolerance of the reference's fold on this member."""
            op_, dt = OPS[op], DT[dtype]
            ref = oracle.reduce_fold(op_, dt, srcs, 0)
            gb, rb = got.view(np.uint8), ref.view(np.uint8)
            if not np.array_equal(gb, rb):
                bad = np.nonzero(gb != rb)[0]
                fail(f"{tag}: {len(bad)} of {rb.size} bytes differ from the oracle, first at byte {int(bad[0])}, "
                     f"last at {int(bad[-1])}")
                return
            if dt >= 8 and op in ("sum", "prod") and len(srcs) > 1:
                own = oracle.reduce_fold(op_, dt, srcs, me)
                tol = 2.0 * oracle.fp_tolerance(dt, op_, srcs, ref)
                if not np.all(np.abs(own.astype(np.float64) - got.astype(np.float64)) <= tol):
                    fail(f"{tag}: outside tolerance of the reference's member-{me} fold")

        def verify(tag, op, dtype, srcs, dbuf, n, me, raw=None):
            raw = dbuf.raw() if raw is None else raw
            lo, hi = PAD + dbuf.off, PAD + dbuf.off + dbuf.nbytes
            if not (raw[:lo] == sc.GUARD_BYTE).all():
                fail(f"{tag}: guard bytes before dest written")
            if not (raw[hi:] == sc.GUARD_BYTE).all():
                fail(f"{tag}: guard bytes after dest written")
            check(tag, op, dtype, srcs, raw[lo:hi].copy().view(oracle.NP[DT[dtype]])[:n], me)

        def stage(op, dtype, n, sbuf, dbuf, seed, members, me):
            """This member's source in place, 0x3C over the rest of dest's arena."""
            ins = inputs(op, dtype, n, seed, members)
            if dbuf is sbuf:
                dbuf.fill()
                dbuf.put(ins[me])
            else:
                sbuf.put(ins[me])
                dbuf.fill()
            return ins

        def reduce_into(tag, op, dtype, n, sbuf, dbuf, seed, team=W, members=None, me=None):
            """One blocking reduce; dest is read the moment the call returns."""
            members = list(range(npes)) if members is None else members
            me = pe if me is None else me
            ins = stage(op, dtype, n, sbuf, dbuf, seed, members, me)
            ran["n"] += 1
            rc = ish.reduce(op, dtype, dbuf.ptr, sbuf.ptr, n, team)
            raw = dbuf.raw()
            if rc:
                fail(f"{tag}: rc={rc} {ish.last_error()}")
                return
            verify(tag, op, dtype, ins, dbuf, n, me, raw)

        def tag_of(c):
            return (f"{c.group} {c.variant + ' ' if c.variant else ''}{c.op} {c.dtype} n={c.n} {c.skind}"
                    f"{' in place' if c.inplace else ' -> ' + c.dkind} +{c.off}")

        def run_case(c, seed):
            tag = tag_of(c)
            es = sc.ES[c.dtype]
            if not plan_ok(tag, c.staging, c.slots, es, c.n):
                return
            dbuf = Buf(hip, c.dkind, c.n * es, c.off)
            sbuf = dbuf if c.inplace else Buf(hip, c.skind, c.n * es, c.off)
            try:
                reduce_into(tag, c.op, c.dtype, c.n, sbuf, dbuf, seed)
            finally:
                if sbuf is not dbuf:
                    sbuf.free()
                dbuf.free()

        def run_table(cases, seed0):
            before = ran["n"]
            for i, c in enumerate(cases):
                run_case(c, seed0 + 100_003 * i)
            if ran["n"] - before != len(cases) and not fails:
                fail(f"{ran['n'] - before} of {len(cases)} {cases[0].group} cases ran")

        # A plain heap reduce: the library works after whatever came before.
        hn = 4099
        h_s, h_d = ish.ishmem_malloc(4 * hn), ish.ishmem_malloc(4 * hn)

        def heap_reduce(tag, seed):
            ins = inputs("sum", "int32", hn, seed, range(npes))
            hip.upload(h_s, ins[pe])
            ish.ishmem_barrier_all()  # nobody still reads the last source
            if ish.ishmem_int32_sum_reduce(h_d, h_s, hn):
                fail(f"heap reduce after {tag}: {ish.last_error()}")
            else:
                check(f"heap reduce after {tag}", "sum", "int32", ins, hip.download(h_d, hn, np.int32), pe)

        # ---- 1. chunk counts and the ragged tail ---------------------------------------------------
        if "chunks" in scenarios:
            run_table(sc.chunk_cases(want_slots), 0x1000_0000)

        # ---- 2. every valid (op, type) -------------------------------------------------------------
        if "matrix" in scenarios:
            run_table(sc.matrix_cases(), 0x2000_0000)

        # ---- 3. the collective path inside the chunk -----------------------------------------------
        for scen in scenarios:
            if not scen.startswith("paths="):
                continue
            for ei, envname in enumerate(scen[len("paths="):].split(",")):
                _, direct, full_path, tail_path = sc.PATH_ENVS[envname]
                ish.ishmem_barrier_all()
                ish.set_param("direct_p2", direct)  # alike on every PE
                ll, fold = int(ish.get_param("ll_limit_bytes")), int(ish.get_param("fold_limit_bytes"))
                phased_min = int(ish.get_param("phased_min_bytes"))
                cases = sc.path_cases(want_slots, envname)
                c_full = sc.chunk_elems(want_bytes, want_slots, 4)
                for c in cases:
                    for _, _, m in sc.chunk_plan(live_bytes, live_slots, 4, c.n):
                        got = sc.chunk_path(npes, 4 * m, ll, fold, phased_min)
                        want = full_path if m == c_full else tail_path
                        if got != want:
                            fail(f"{tag_of(c)}: a chunk of {m} elements takes the {got} path, this environment is "
                                 f"meant to reach {want} (thresholds {ll} / {fold} / {phased_min})")
                if not fails:
                    run_table(cases, 0x3000_0000 + 0x10_0000 * ei)
                ish.ishmem_barrier_all()
                ish.set_param("direct_p2", 1)
                ish.ishmem_barrier_all()

        # ---- 4. buffer kinds -----------------------------------------------------------------------
        if "kinds" in scenarios:
            cases = sc.kind_cases(want_bytes)
            flavour = "large" if want_bytes == sc.STAGING else "small"
            if {sc.pageable_flavour(c) for c in cases} != {flavour}:
                fail(f"kinds: pageable payloads are not all {flavour}")
            run_table(cases, 0x4000_0000)
            heap_reduce("kinds", 0x4F00_0000)

        # ---- 5. page-lock corner cases ---------------------------------------------------------------
        if "pagelock" in scenarios:
            pl = sc.pagelock_sizes()
            # (a) source and dest are two slices of one numpy allocation and share a page: whether
            # HIP accepts or refuses the second registration, the bytes must be right.
            n = pl["shared_page"]
            nb = 4 * n
            if plan_ok("pagelock shared page", sc.STAGING, 2, 4, n):
                arena = np.empty(3 * PAD + 2 * nb + 64, np.uint8)
                skip = -arena.ctypes.data % PAD
                view = arena[skip:skip + 2 * PAD + 2 * nb + 64]
                s_lo, d_lo = PAD, PAD + nb + 64
                if (view.ctypes.data + s_lo + nb - 1) // PAD != (view.ctypes.data + d_lo) // PAD:
                    fail("pagelock shared page: the slices share no page")
                ins = inputs("sum", "int32", n, 0x5000_0000, range(npes))
                view[:] = sc.GUARD_BYTE
                view[s_lo:s_lo + nb] = ins[pe].view(np.uint8)
                ran["n"] += 1
                rc = ish.ishmem_int32_sum_reduce(view.ctypes.data + d_lo, view.ctypes.data + s_lo, n)
                got = view.copy()
                if rc:
                    fail(f"pagelock shared page: rc={rc} {ish.last_error()}")
                else:
                    check("pagelock shared page", "sum", "int32", ins, got[d_lo:d_lo + nb].copy().view(np.int32), pe)
                    if not np.array_equal(got[s_lo:s_lo + nb], ins[pe].view(np.uint8)):
                        fail("pagelock shared page: the source changed")
                    if not ((got[:s_lo] == sc.GUARD_BYTE).all() and (got[s_lo + nb:d_lo] == sc.GUARD_BYTE).all()
                            and (got[d_lo + nb:] == sc.GUARD_BYTE).all()):
                        fail("pagelock shared page: guard bytes written")
                heap_reduce("pagelock shared page", 0x5100_0000)
            # (b) one element below the page-lock threshold and exactly at it, back to back: a buffer
            # kept on HIP's pageable copies, then one locked for the call.
            for i, k in enumerate(("below", "at", "below")):
                run_case(sc.Case("pagelock", "sum", "int32", pl[k], 2, sc.STAGING, variant=k), 0x5200_0000 + 7919 * i)
                heap_reduce(f"pagelock {k}", 0x5300_0000 + i)
            # (c) two consecutive calls on the same buffers: unlock, then a fresh lock; out of place
            # and in place.
            n = pl["twice"]
            if plan_ok("pagelock twice", sc.STAGING, 2, 4, n):
                sbuf, dbuf = Buf(hip, "pageable", 4 * n), Buf(hip, "pageable", 4 * n)
                for rep in range(2):
                    reduce_into(f"pagelock twice, call {rep}", "sum", "int32", n, sbuf, dbuf, 0x5400_0000 + 31 * rep)
                for rep in range(2):
                    reduce_into(f"pagelock twice in place, call {rep}", "max", "int32", n, dbuf, dbuf, 0x5500_0000 + 31 * rep)
                heap_reduce("pagelock twice", 0x5600_0000)
                sbuf.free()
                dbuf.free()

        # ---- 6. the copy kernel in place of the DMA copies ----------------------------------------------
        if "copykernel" in scenarios:
            cases = sc.copykernel_cases()
            for v in (1, 2, 3):
                ish.set_param("staged_copy_kernel", v)  # per PE, nothing is paired
                if int(ish.get_param("staged_copy_kernel")) != v:
                    fail(f"staged_copy_kernel {v} did not take")
                run_table([c for c in cases if c.variant.startswith(str(v))], 0x6000_0000 + 0x100_0000 * v)
            ish.set_param("staged_copy_kernel", 0)
            heap_reduce("copykernel", 0x6F00_0000)

        # ---- 7. teams ------------------------------------------------------------------------------
        if "teams" in scenarios:
            assert npes == 4
            ts = sc.team_sizes()
            r0, even = ish.ishmem_team_split_strided(W, 0, 2, 2)
            r1, odd = ish.ishmem_team_split_strided(W, 1, 2, 2)
            r2, solo = ish.ishmem_team_split_strided(W, pe, 1, 1)
            if r0 or r1 or r2 or solo == INV or (even != INV) != (pe % 2 == 0) or (odd != INV) != (pe % 2 == 1):
                fail(f"teams: splits rc={r0}/{r1}/{r2} even={even} odd={odd} solo={solo} {ish.last_error()}")
            else:
                # heap allocation is collective over the world: the odd PEs' buffers exist on every PE
                o_s, o_d = ish.ishmem_malloc(8 * ts["heap"]), ish.ishmem_malloc(8 * ts["heap"])
                ish.ishmem_barrier_all()
                if pe % 2 == 0:
                    # the even PEs: host buffers, six chunks ...
                    n = ts["strided"]
                    if plan_ok("teams strided", sc.STAGING, 2, 8, n):
                        sbuf, dbuf = Buf(hip, "pageable", 8 * n), Buf(hip, "pageable", 8 * n, 8)
                        reduce_into("teams strided int64 sum, host buffers", "sum", "int64", n, sbuf, dbuf, 0x7000_0000,
                                    even, [0, 2], pe // 2)
                        sbuf.free()
                        dbuf.free()
                else:
                    # ... while the odd PEs reduce in the heap on the complementary team
                    n = ts["heap"]
                    ins = inputs("max", "int64", n, 0x7100_0000, [1, 3])
                    hip.upload(o_s, ins[pe // 2])
                    ish.ishmem_team_sync(odd)
                    ran["n"] += 1
                    if ish.ishmem_int64_max_reduce(odd, o_d, o_s, n):
                        fail(f"teams complementary heap reduce: {ish.last_error()}")
                    else:
                        check("teams complementary heap reduce", "max", "int64", ins, hip.download(o_d, n, np.int64), pe // 2)
                ish.ishmem_barrier_all()
                ish.ishmem_free(o_d)
                ish.ishmem_free(o_s)
                # a team of one: copy-in and copy-out only, dest == source bit for bit
                for i, k in enumerate(("one_c+1", "one_3c+1")):
                    n = ts[k]
                    if not plan_ok(f"teams {k}", sc.STAGING, 2, 8, n):
                        continue
                    x = inputs("sum", "int64", n, 0x7200_0000 + 17 * i, [pe])[0]
                    sbuf, dbuf = Buf(hip, "pageable", 8 * n, 8), Buf(hip, "pageable", 8 * n)
                    sbuf.put(x)
                    dbuf.fill()
                    ran["n"] += 1
                    rc = ish.ishmem_int64_sum_reduce(solo, dbuf.ptr, sbuf.ptr, n)
                    raw = dbuf.raw()
                    if rc:
                        fail(f"teams {k}: rc={rc} {ish.last_error()}")
                    else:
                        if not np.array_equal(raw[PAD:PAD + 8 * n], x.view(np.uint8)):
                            fail(f"teams {k}: team of one, dest != source")
                        if not ((raw[:PAD] == sc.GUARD_BYTE).all() and (raw[PAD + 8 * n:] == sc.GUARD_BYTE).all()):
                            fail(f"teams {k}: team of one, guard bytes written")
                    sbuf.free()
                    dbuf.free()
                ish.ishmem_barrier_all()
                ish.ishmem_team_destroy(solo)
                ish.ishmem_team_destroy(even if pe % 2 == 0 else odd)
                heap_reduce("teams", 0x7F00_0000)

        # ---- 8. on a stream and back to back ---------------------------------------------------------
        if "stream" in scenarios:
            ss = sc.stream_sizes()
            st1, st2 = hip.stream_create(), hip.stream_create()
            rets = ish.ishmem_malloc(16)

            def rets_clean(tag, k):
                got = hip.download(rets, 4, np.uint32)[:k]
                if got.any():
                    fail(f"{tag}: *ret = {[hex(int(x)) for x in got]}, must come back 0")

            def staged(op, n, sbuf, dbuf, seed):
                return stage(op, "int32", n, sbuf, dbuf, seed, list(range(npes)), pe)

            def enqueue(op, n, sbuf, dbuf, slot, st):
                ran["n"] += 1
                return ish.reduce_on_stream(op, "int32", dbuf.ptr, sbuf.ptr, n, rets + 4 * slot, st)

            ok = all(plan_ok(f"stream {k}", sc.STAGING, 2, 4, ss[k]) for k in ("ragged", "full", "tail1", "pageable"))
            if ok:
                n_r, n_f, n_t = ss["ragged"], ss["full"], ss["tail1"]
                pin = [Buf(hip, "pinned", 4 * n_r, o) for o in (0, 4, 0)]
                dev = [Buf(hip, "device", 4 * n_r, o) for o in (0, 4)]
                # (a) one call at a time: pinned -> pinned, device -> device, device in place
                for i, (tag, sb, db) in enumerate((("pinned -> pinned", pin[0], pin[1]), ("device -> device", dev[0], dev[1]),
                                                   ("device in place", dev[1], dev[1]))):
                    hip.memset(rets, PRESET, 16)
                    ins = staged("sum", n_r, sb, db, 0x8000_0000 + 41 * i)
                    ish.ishmem_barrier_all()
                    rc = enqueue("sum", n_r, sb, db, 0, st1)
                    hip.stream_synchronize(st1)
                    if rc:
                        fail(f"stream {tag}: rc={rc} {ish.last_error()}")
                    else:
                        rets_clean(f"stream {tag}", 1)
                        verify(f"stream {tag} n={n_r}", "sum", "int32", ins, db, n_r, pe)
                # (b) two staged reduces on two streams with no host synchronisation between them: the
                # second takes the staging region over from the first
                hip.memset(rets, PRESET, 16)
                pf, df = Buf(hip, "pinned", 4 * n_f), Buf(hip, "device", 4 * n_f)
                ins1 = staged("sum", n_r, pin[0], dev[0], 0x8100_0000)
                ins2 = staged("xor", n_f, df, pf, 0x8200_0000)
                ish.ishmem_barrier_all()
                rc1 = enqueue("sum", n_r, pin[0], dev[0], 0, st1)
                rc2 = enqueue("xor", n_f, df, pf, 1, st2)
                hip.stream_synchronize(st1)
                hip.stream_synchronize(st2)
                if rc1 or rc2:
                    fail(f"stream back to back: rc={rc1}/{rc2} {ish.last_error()}")
                else:
                    rets_clean("stream back to back", 2)
                    verify("stream back to back, first (pinned -> device)", "sum", "int32", ins1, dev[0], n_r, pe)
                    verify("stream back to back, second (device -> pinned)", "xor", "int32", ins2, pf, n_f, pe)
                # (c) a staged reduce, then an fcollect from a host source (two segments through the
                # same staging region) on another stream
                nbf = ss["fcollect_bytes"]
                fsrc = Buf(hip, "pinned", nbf)
                fdst = ish.ishmem_malloc(nbf * npes)
                mine = [np.random.default_rng([0x83, j]).integers(0, 256, nbf, dtype=np.uint8) for j in range(npes)]
                fsrc.put(mine[pe])
                hip.memset(fdst, 0, nbf * npes)
                hip.memset(rets, PRESET, 16)
                sb_t, db_t = Buf(hip, "pinned", 4 * n_t, 4), Buf(hip, "pinned", 4 * n_t)
                ins3 = staged("min", n_t, sb_t, db_t, 0x8400_0000)
                hip.synchronize()
                ish.ishmem_barrier_all()
                rc3 = enqueue("min", n_t, sb_t, db_t, 0, st1)
                rc4 = ish.fcollect_on_stream(fdst, fsrc.ptr, nbf, rets + 4, st2)
                hip.stream_synchronize(st1)
                hip.stream_synchronize(st2)
                if rc3 or rc4:
                    fail(f"stream reduce then fcollect: rc={rc3}/{rc4} {ish.last_error()}")
                else:
                    rets_clean("stream reduce then fcollect", 2)
                    verify("stream reduce before the fcollect", "min", "int32", ins3, db_t, n_t, pe)
                    if not np.array_equal(hip.download(fdst, nbf * npes, np.uint8), np.concatenate(mine)):
                        fail("stream fcollect from a host source after the staged reduce: wrong bytes")
                ish.ishmem_barrier_all()
                # (d) blocking, the last chunk full size, dest pinned and read by the host at once
                # (reduce_into reads it with no HIP call after the return): three rounds
                for rnd in range(3):
                    reduce_into(f"blocking into pinned, round {rnd}", "sum", "int32", n_f, df, pf, 0x8500_0000 + 37 * rnd)
                # (e) large pageable buffers on a stream are page-locked for the call, which therefore
                # completes before it returns: the stream is idle and dest final with no synchronisation
                n_p = ss["pageable"]
                if 4 * n_p < sc.PIN_MIN:
                    fail("stream pageable: payload below the page-lock threshold")
                ps, pd = Buf(hip, "pageable", 4 * n_p), Buf(hip, "pageable", 4 * n_p, 4)
                hip.memset(rets, PRESET, 16)
                ins5 = staged("sum", n_p, ps, pd, 0x8600_0000)
                hip.synchronize()
                ish.ishmem_barrier_all()
                rc5 = enqueue("sum", n_p, ps, pd, 0, st1)
                idle = hip.stream_query(st1)
                raw = pd.raw()
                if rc5:
                    fail(f"stream pageable: rc={rc5} {ish.last_error()}")
                else:
                    if not idle:
                        fail("stream pageable: the stream still had work when the call returned")
                    verify("stream pageable, read at return", "sum", "int32", ins5, pd, n_p, pe, raw)
                    rets_clean("stream pageable", 1)
                ish.ishmem_barrier_all()
                ish.ishmem_free(fdst)
                for b in pin + dev + [pf, df, fsrc, sb_t, db_t, ps, pd]:
                    b.free()
            hip.stream_destroy(st1)
            hip.stream_destroy(st2)
            ish.ishmem_free(rets)
            heap_reduce("stream", 0x8F00_0000)

        # ---- 9. captured into a graph ------------------------------------------------------------------
        if "graph" in scenarios:
            n = sc.graph_size()
            if plan_ok("graph", sc.STAGING, 2, 4, n):
                st = hip.stream_create()
                ret = ish.ishmem_malloc(4)
                sbuf, dbuf = Buf(hip, "pinned", 4 * n), Buf(hip, "pinned", 4 * n)
                ish.ishmem_barrier_all()
                with hip.Graph(st) as g:
                    rc = ish.ishmemx_float_sum_reduce_on_stream(dbuf.ptr, sbuf.ptr, n, ret, st)
                if rc:
                    fail(f"graph: captured call failed: {ish.last_error()}")
                else:
                    for rep in range(2):
                        ins = stage("sum", "float", n, sbuf, dbuf, 0x9000_0000 + 53 * rep, list(range(npes)), pe)
                        hip.memset(ret, PRESET, 4)
                        hip.synchronize()
                        ish.ishmem_barrier_all()  # everyone's inputs are in place
                        ran["n"] += 1
                        g.launch()
                        hip.stream_synchronize(st)
                        if int(hip.download(ret, 1, np.int32)[0]) != 0:
                            fail(f"graph replay {rep}: ret != 0")
                        verify(f"graph replay {rep}", "sum", "float", ins, dbuf, n, pe)
                del g
                ish.ishmem_barrier_all()
                sbuf.free()
                dbuf.free()
                hip.stream_destroy(st)
                ish.ishmem_free(ret)
            heap_reduce("graph", 0x9F00_0000)

        if ran["n"] == 0 and not fails:
            fail(f"no case ran for {scenarios}")
        ish.ishmem_barrier_all()
        if ish.lib().ishmemi_c_error_count() != 0:
            fail(f"device error count {ish.lib().ishmemi_c_error_count()}")
        ish.ishmem_free(h_d)
        ish.ishmem_free(h_s)
        ish.ishmem_finalize()
    except Exception:
        fails.append(f"pe{pe} exception:\n{traceback.format_exc()}")
    q.put((pe, fails))

"""Worker body of the multi-PE strided / blocked put / get GPU tests (tests/test_gpu_strided.py): one
process = one PE, all PEs on one GPU.  Every PE targets (me + 1) % p.

The dest arena (64-B guard, the dest extent, 64-B guard) is prefilled with a sentinel and downloaded
whole: every written element must be bit-exact and every other byte — the gaps between strided
elements as well as the guards — unchanged.  Expected bytes come from numpy index arithmetic
(tests/strided_cases.py) over the tester word pattern (rma_worker.expected_word) or seeded random
bytes.  Failures are returned as strings through the queue.
"""
from __future__ import annotations

import ctypes
import os
import traceback

import numpy as np

from tests import strided_cases as sc
from tests.rma_worker import payload

GUARD, SENT = sc.GUARD, sc.SENTINEL
ARENA = 8 << 20  # the largest extent, (LOOP_TWICE - 1) * 7 * 16 + 16 bytes, plus guards and offsets


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
        L = ish.lib()
        if int(ish.get_param("max_blocks")) != sc.MAX_BLOCKS:
            fails.append(f"pe{pe}: max_blocks {ish.get_param('max_blocks')} != {sc.MAX_BLOCKS}")
        nxt, prv = (pe + 1) % npes, (pe - 1) % npes
        sbuf = ish.ishmem_align(256, ARENA)
        dbuf = ish.ishmem_align(256, ARENA)
        seedc = [0]

        def up(ptr, arr):  # default-kind copies: the local buffer may be pinned host memory
            a = np.ascontiguousarray(arr)
            hip.memcpy(ptr, a.ctypes.data, a.nbytes)

        def down(ptr, n):
            out = np.empty(n, np.uint8)
            hip.memcpy(out.ctypes.data, ptr, n)
            return out

        def default_call(put):
            fn = ish.ibput if put else ish.ibget
            return lambda d, s, case, p: fn(d, s, case[1], case[2], case[3], case[4], case[0], p)

        def one(tag, put, case, soff=0, doff=0, call=None, kinds=("tester", "random"), src=None, dst=None,
                sync=None, expect_rc0=True):
            """put: every PE moves `case` from its source + soff into dest + GUARD + doff on the next
            PE.  get: every PE moves `case` from source + soff on the next PE into its own dest.  src /
            dst: the LOCAL buffer when it is not the heap arena (device address, upload / download by
            hipMemcpy)."""
            es, dstr, sstr, bsize, nblocks = case
            dext, sext = sc.extent(dstr, bsize, nblocks, es), sc.extent(sstr, bsize, nblocks, es)
            assert max(dext, sext) + 2 * GUARD + 16 <= ARENA, case
            for kind in kinds:
                seedc[0] += 1
                seed = seedc[0]
                to = nxt if put else prv  # who reads this PE's source bytes
                sp = (src if src is not None else sbuf) + soff
                dp = (dst if dst is not None else dbuf) + doff
                if sext:
                    up(sp, payload(kind, seed, sext, pe, to))
                up(dp, np.full(2 * GUARD + dext, SENT, np.uint8))
                ish.ishmem_barrier_all()  # every source and every prefilled dest is in place
                rc = (call or default_call(put))(dp + GUARD, sp, case, nxt)
                if sync:
                    sync()
                if (rc == 0) != expect_rc0:
                    fails.append(f"pe{pe} {tag} {kind}: rc={rc} {ish.last_error()}")
                ish.ishmem_barrier_all()  # every PE's transfer is complete
                got = down(dp, 2 * GUARD + dext)
                want = np.full(2 * GUARD + dext, SENT, np.uint8)
                if rc == 0:
                    frm = prv if put else nxt
                    sc.apply(want, payload(kind, seed, sext, frm, pe), case, doff=GUARD)
                if not np.array_equal(got, want):
                    bad = np.nonzero(got != want)[0]
                    where = "guard" if (bad[0] < GUARD or bad[0] >= GUARD + dext) else "extent"
                    fails.append(f"pe{pe} {tag} {kind} case {case} s+{soff} d+{doff}: {len(bad)} bytes differ, first at "
                                 f"{int(bad[0]) - GUARD} ({where}): got {int(got[bad[0]]):#x} want {int(want[bad[0]]):#x}")
                ish.ishmem_barrier_all()  # nobody refills a source a peer still reads

        for put, name in ((True, "iput"), (False, "iget")):
            if name in scenarios:
                for case in sc.iput_cases():
                    one(name, put, case)
        for put, name in ((True, "ibput"), (False, "ibget")):
            if name in scenarios:
                for i, case in enumerate(sc.ib_cases()):
                    one(name, put, case, kinds=(("tester", "random")[i % 2],))
        for put, name in ((True, "put_offsets"), (False, "get_offsets")):
            if name in scenarios:
                for soff, doff, case in sc.offset_cases():
                    one(name, put, case, soff=soff, doff=doff, kinds=("random",))

        if "tester" in scenarios:
            # The reference ibput tester's pair of calls, and its iget mirror, for uint8 .. 16-B elements.
            for es in sc.WIDTHS:
                for nelems in sc.TESTER_NELEMS:
                    for put in (True, False):
                        fn = ish.ibput if put else ish.ibget
                        seedc[0] += 1
                        nbytes = (nelems + 2) * es
                        hip.upload(sbuf, payload("tester", seedc[0], nbytes, pe, nxt if put else prv))
                        hip.upload(dbuf, np.full(2 * GUARD + nbytes, SENT, np.uint8))
                        ish.ishmem_barrier_all()
                        want = np.full(2 * GUARD + nbytes, SENT, np.uint8)
                        srcb = payload("tester", seedc[0], nbytes, prv if put else nxt, pe)
                        for doe, soe, dstr, sstr, bsize, nblocks in sc.tester_calls(nelems):
                            rc = fn(dbuf + GUARD + doe * es, sbuf + soe * es, dstr, sstr, bsize, nblocks, es, nxt)
                            ok = sc.strides_valid(dstr, sstr, bsize)
                            if (rc == 0) != ok:
                                fails.append(f"pe{pe} tester es={es} nelems={nelems}: rc={rc} {ish.last_error()}")
                            if ok:
                                sc.apply(want, srcb, (es, dstr, sstr, bsize, nblocks), doff=GUARD + doe * es, soff=soe * es)
                        ish.ishmem_barrier_all()
                        got = hip.download(dbuf, 2 * GUARD + nbytes, np.uint8)
                        if not np.array_equal(got, want):
                            fails.append(f"pe{pe} tester {'ibput' if put else 'ibget'} es={es} nelems={nelems}: "
                                         f"{int(np.count_nonzero(got != want))} bytes differ")
                        ish.ishmem_barrier_all()
            # int_iput_device's shape: 20 ints, dst = 3, sst = 2, 5 elements.
            d = sc.INT_IPUT_DEVICE
            one("int_iput shape", True, (4, d["dst"], d["sst"], 1, d["nelems"]),
                call=lambda dp, sp, c, p: ish.ishmem_int_iput(dp, sp, c[1], c[2], c[4], p))
            one("int_iget shape", False, (4, d["dst"], d["sst"], 1, d["nelems"]),
                call=lambda dp, sp, c, p: ish.ishmem_int_iget(dp, sp, c[1], c[2], c[4], p))

        if "typed" in scenarios:
            # The typed and sized names count elements and element strides; iput128 with stride 2 moves
            # 16-byte units 32 bytes apart.
            one("float_iput", True, (4, 3, 2, 1, 1000),
                call=lambda d, s, c, p: ish.ishmem_float_iput(d, s, c[1], c[2], c[4], p))
            one("double_iget", False, (8, 2, 5, 1, 333),
                call=lambda d, s, c, p: ish.ishmem_double_iget(d, s, c[1], c[2], c[4], p))
            one("iput128 stride 2", True, (16, 2, 2, 1, 33),
                call=lambda d, s, c, p: ish.ishmem_iput128(d, s, c[1], c[2], c[4], p))
            one("iget128 stride 2", False, (16, 2, 3, 1, 33),
                call=lambda d, s, c, p: ish.ishmem_iget128(d, s, c[1], c[2], c[4], p))
            one("iput16", True, (2, 5, 1, 1, 777),
                call=lambda d, s, c, p: ish.ishmem_iput16(d, s, c[1], c[2], c[4], p))
            one("uint16_ibput", True, (2, 9, 7, 5, 77),
                call=lambda d, s, c, p: ish.ishmemx_uint16_ibput(d, s, c[1], c[2], c[3], c[4], p))
            one("ibget64", False, (8, 4, 6, 3, 129),
                call=lambda d, s, c, p: ish.ishmemx_ibget64(d, s, c[1], c[2], c[3], c[4], p))
            one("ibput128", True, (16, 3, 2, 2, 65),
                call=lambda d, s, c, p: ish.ishmemx_ibput128(d, s, c[1], c[2], c[3], c[4], p))
            one("size_ibget", False, (8, 2, 3, 2, 40),
                call=lambda d, s, c, p: ish.ishmemx_size_ibget(d, s, c[1], c[2], c[3], c[4], p))

        if "kinds" in scenarios:
            # The local buffer: heap (every case above), plain device, pinned host; pageable is refused.
            case = (4, 5, 3, 2, 3001)
            nloc = max(sc.extent(5, 2, 3001, 4), sc.extent(3, 2, 3001, 4)) + 2 * GUARD + 64
            plain = hip.malloc(nloc)
            pinned = hip.host_malloc(nloc)
            for name, loc in (("device", plain), ("pinned", pinned)):
                one(f"kinds put {name}", True, case, soff=4, src=loc, kinds=("random",))
                one(f"kinds get {name}", False, case, doff=4, dst=loc, kinds=("random",))
            page = np.zeros(nloc, np.uint8)
            lp = page.ctypes.data
            st = hip.stream_create()
            for what, call in (("ibput", lambda: ish.ibput(dbuf + GUARD, lp, 5, 3, 2, 3001, 4, nxt)),
                               ("ibget", lambda: ish.ibget(lp, sbuf, 5, 3, 2, 3001, 4, nxt)),
                               ("contiguous ibput", lambda: ish.ibput(dbuf + GUARD, lp, 2, 2, 2, 3001, 4, nxt)),
                               ("contiguous ibget", lambda: ish.ibget(lp, sbuf, 1, 1, 1, 100, 4, nxt)),
                               ("ibput_on_stream", lambda: ish.ibput_on_stream(dbuf + GUARD, lp, 5, 3, 2, 3001, 4, nxt, st)),
                               ("ibget_on_stream", lambda: ish.ibget_on_stream(lp, sbuf, 5, 3, 2, 3001, 4, nxt, st))):
                if call() == 0 or "not device-accessible" not in ish.last_error():
                    fails.append(f"pe{pe} kinds {what} on pageable memory: not refused ('{ish.last_error()}')")
            hip.stream_destroy(st)
            ish.ishmem_barrier_all()
            hip.host_free(pinned)
            hip.free(plain)

        if "stream" in scenarios:
            st = hip.stream_create()
            case = (4, 3, 2, 2, 20_001)
            sync = lambda: hip.stream_synchronize(st)  # noqa: E731
            # eager
            one("ibput_on_stream", True, case, sync=sync, kinds=("random",),
                call=lambda d, s, c, p: ish.ibput_on_stream(d, s, c[1], c[2], c[3], c[4], c[0], p, st))
            one("ibget_on_stream", False, case, sync=sync, kinds=("random",),
                call=lambda d, s, c, p: ish.ibget_on_stream(d, s, c[1], c[2], c[3], c[4], c[0], p, st))
            # contiguous on a stream
            one("contiguous ibput_on_stream", True, (4, 2, 2, 2, 5001), sync=sync, kinds=("random",),
                call=lambda d, s, c, p: ish.ibput_on_stream(d, s, c[1], c[2], c[3], c[4], c[0], p, st))
            # deps / done
            dep, done = hip.Event(), hip.Event()

            def with_deps(d, s, c, p):
                dep.record(st)
                return ish.ibput_on_stream(d, s, c[1], c[2], c[3], c[4], c[0], p, st, deps=[dep], done=done)
            one("ibput_on_stream deps", True, case, sync=done.synchronize, kinds=("random",), call=with_deps)
            hip.stream_destroy(st)

        if "graph" in scenarios:
            # Captured once, replayed twice with the source refilled between the replays.
            st = hip.stream_create()
            case = (8, 3, 2, 1, 30_001)
            es, dstr, sstr, bsize, nblocks = case
            dext, sext = sc.extent(dstr, bsize, nblocks, es), sc.extent(sstr, bsize, nblocks, es)
            ish.ishmem_barrier_all()
            with hip.Graph(st) as g:
                if ish.ibput_on_stream(dbuf + GUARD, sbuf, dstr, sstr, bsize, nblocks, es, nxt, st):
                    fails.append(f"pe{pe} graph capture: {ish.last_error()}")
            for rep in range(2):
                seedc[0] += 1
                hip.upload(sbuf, payload("random", seedc[0], sext, pe, nxt))
                hip.upload(dbuf, np.full(2 * GUARD + dext, SENT, np.uint8))
                ish.ishmem_barrier_all()
                g.launch()
                hip.stream_synchronize(st)
                ish.ishmem_barrier_all()
                got = hip.download(dbuf, 2 * GUARD + dext, np.uint8)
                want = np.full(2 * GUARD + dext, SENT, np.uint8)
                sc.apply(want, payload("random", seedc[0], sext, prv, pe), case, doff=GUARD)
                if not np.array_equal(got, want):
                    fails.append(f"pe{pe} graph replay {rep}: {int(np.count_nonzero(got != want))} bytes differ")
                ish.ishmem_barrier_all()
            del g
            hip.stream_destroy(st)

        if "warm" in scenarios:
            # The target's caches hold dest's OLD lines when the strided put lands: G workgroups each
            # read all of dest with plain loads, barrier, the origin puts, barrier, the same kernel
            # again must see every new element, and the old bytes in the gaps, in every workgroup.
            G = 16
            case = (4, 3, 1, 1, 5000)
            es, dstr, sstr, bsize, nblocks = case
            dext, sext = sc.extent(dstr, bsize, nblocks, es), sc.extent(sstr, bsize, nblocks, es)
            out = hip.malloc(G * dext)
            for rep in range(2):
                seedc[0] += 1
                old = payload("random", seedc[0], dext, 99, pe)
                hip.upload(dbuf + GUARD, old)
                hip.upload(sbuf, payload("random", seedc[0], sext, pe, nxt))
                if L.ishmemi_c_read_all_u32(out, dbuf + GUARD, dext // 4, G, None):
                    fails.append(f"pe{pe} warm: {ish.last_error()}")
                got = hip.download(out, G * dext, np.uint8).reshape(G, dext)
                if not all(np.array_equal(got[b], old) for b in range(G)):
                    fails.append(f"pe{pe} warm: the warming read is wrong")
                ish.ishmem_barrier_all()
                if ish.ibput(dbuf + GUARD, sbuf, dstr, sstr, bsize, nblocks, es, nxt):
                    fails.append(f"pe{pe} warm put: {ish.last_error()}")
                ish.ishmem_barrier_all()
                L.ishmemi_c_read_all_u32(out, dbuf + GUARD, dext // 4, G, None)
                got = hip.download(out, G * dext, np.uint8).reshape(G, dext)
                new = old.copy()
                sc.apply(new, payload("random", seedc[0], sext, prv, pe), case)
                stale = [b for b in range(G) if not np.array_equal(got[b], new)]
                if stale:
                    fails.append(f"pe{pe} warm rep {rep}: workgroups {stale} read stale or wrong bytes")
                ish.ishmem_barrier_all()
            hip.free(out)

        if "argfail" in scenarios:
            errs0 = L.ishmemi_c_error_count()
            base, size, used = ctypes.c_void_p(), ctypes.c_size_t(), ctypes.c_size_t()
            L.ishmemi_c_heap_info(ctypes.byref(base), ctypes.byref(size), ctypes.byref(used))
            heap_end = base.value + size.value
            plain = hip.malloc(4096)
            # (tag, (dst, sst, bsize, nblocks, es, pe), remote address or None for the arena, word)
            n = 100
            cases = [
                ("pe -1", (2, 2, 1, n, 4, -1), None, "outside [0"),
                ("pe npes", (2, 2, 1, n, 4, npes), None, "outside [0"),
                ("stride 0", (0, 2, 1, n, 4, nxt), None, "not positive"),
                ("source stride 0", (2, 0, 1, n, 4, nxt), None, "not positive"),
                ("negative stride", (-3, 2, 1, n, 4, nxt), None, "not positive"),
                ("stride < bsize", (3, 4, 4, n, 4, nxt), None, "less than the block size"),
                ("elem_bytes 3", (2, 2, 1, n, 3, nxt), None, "elem_bytes"),
                ("remote outside heap", (2, 2, 1, n, 4, nxt), plain, "not inside the symmetric heap"),
                # ((n - 1) * 2 + 1) * 4 bytes: the last element ends one byte past the heap's end
                ("extent one byte past the heap", (2, 2, 1, n, 4, nxt), heap_end - ((n - 1) * 2 + 1) * 4 + 1,
                 "not inside the symmetric heap"),
                ("null", (2, 2, 1, n, 4, nxt), 0, "null pointer"),
            ]
            forms = [(True, ish.ibput), (False, ish.ibget),
                     (True, lambda *a: ish.ibput_on_stream(*a, 0)), (False, lambda *a: ish.ibget_on_stream(*a, 0))]
            for tag, (dstr, sstr, bsize, nblocks, es, tpe), remote, word in cases:
                for put, f in forms:
                    r = dbuf if remote is None else remote
                    d, s = (r, sbuf) if put else (dbuf, r if remote is not None else sbuf)
                    rc = f(d, s, dstr, sstr, bsize, nblocks, es, tpe)
                    if rc == 0:
                        fails.append(f"pe{pe} argfail {tag}: returned 0")
                    elif word not in ish.last_error():
                        fails.append(f"pe{pe} argfail {tag}: message '{ish.last_error()}' lacks '{word}'")
            # The extent that ends exactly at the heap's end is inside; empty calls succeed whatever the pointers.
            if ish.ibput(0, 0, 1, 1, 1, 0, 4, nxt) or ish.ibget(0, 0, 5, 5, 0, 7, 4, nxt) or \
                    ish.ibput_on_stream(0, 0, 2, 3, 1, 0, 8, nxt, 0):
                fails.append(f"pe{pe} argfail: an empty call failed: {ish.last_error()}")
            if L.ishmemi_c_error_count() != errs0:
                fails.append(f"pe{pe} argfail: error count moved")
            hip.free(plain)
            ish.ishmem_barrier_all()  # a barrier after the failures completes
            one("after argfail", True, (4, 3, 2, 1, 1025), kinds=("random",))

        ish.ishmem_barrier_all()
        if L.ishmemi_c_error_count() != 0:
            fails.append(f"pe{pe}: device error count {L.ishmemi_c_error_count()}")
        for b in (dbuf, sbuf):
            ish.ishmem_free(b)
        ish.ishmem_finalize()
    except Exception:
        fails.append(f"pe{pe} exception:\n{traceback.format_exc()}")
    q.put((pe, fails))

"""Worker body of the multi-PE put / get GPU tests (tests/test_gpu_rma.py): one process = one PE,
all PEs on one GPU, symmetric heaps mapped into each other over HIP IPC.

Every PE puts to (me + 1) % p, or gets from it.  Inputs are the reference tester's pattern
(ishmem_tester.h:1118-1149: word idx = (nelems<<48) + ((0x80+from)<<40) + ((0x80+to)<<32) + idx) and
seeded random bytes; dest sits between two 64-byte guards of 0xA5 that must come back unchanged;
the comparison is bit-exact.  Failures are returned as strings through the queue.
"""
from __future__ import annotations

import ctypes
import os
import traceback

import numpy as np

GUARD = 64
# The put / get kernel moves tiles of 256 threads x 4 items x 16 B = 16 KiB, one tile per workgroup
# per step; under the suite's ISHMEM_MAX_BLOCKS=32 a payload of 2 x 32 tiles makes every workgroup run
# its grid-stride loop twice (and 4097 bytes more leave a partial third step and a tail).
TILE_BYTES = 256 * 4 * 16
MAX_BLOCKS = 32
LOOP_TWICE = 2 * MAX_BLOCKS * TILE_BYTES + 4097
SIZES = [0, 1, 15, 16, 17, 255, 4097, (64 << 10) + 1, (1 << 20) + 16, LOOP_TWICE]
MAXB = LOOP_TWICE


def expected_word(nelems: int, frm: int, to: int, idx):
    """The tester's word for element idx of a transfer of nelems elements from PE frm to PE to."""
    base = ((nelems << 48) + ((0x80 + frm) << 40) + ((0x80 + to) << 32)) & 0xFFFFFFFFFFFFFFFF
    return (np.asarray(idx, dtype=np.uint64) + np.uint64(base)).astype("<u8")


def payload(kind: str, seed: int, nbytes: int, frm: int, to: int) -> np.ndarray:
    """The bytes PE frm holds for PE to."""
    if kind == "tester":
        return expected_word(nbytes, frm, to, np.arange((nbytes + 7) // 8)).view(np.uint8)[:nbytes]
    return np.random.default_rng([seed, frm, to]).integers(0, 256, nbytes, dtype=np.uint8)


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
        if int(ish.get_param("max_blocks")) != MAX_BLOCKS:
            fails.append(f"pe{pe}: max_blocks {ish.get_param('max_blocks')} != {MAX_BLOCKS}")
        nxt, prv = (pe + 1) % npes, (pe - 1) % npes
        arena = MAXB + 2 * GUARD + 256
        sbuf = ish.ishmem_align(256, arena)
        dbuf = ish.ishmem_align(256, arena)
        tbuf = ish.ishmem_align(256, arena)
        ret = ish.ishmem_malloc(4)
        seedc = [0]

        def fill_dest(buf, doff, B):
            hip.upload(buf + doff, np.full(2 * GUARD + B, 0xA5, np.uint8))

        def check(tag, buf, doff, want_body):
            B = len(want_body)
            got = hip.download(buf + doff, 2 * GUARD + B, np.uint8)
            g = np.full(GUARD, 0xA5, np.uint8)
            want = np.concatenate([g, want_body, g])
            if not np.array_equal(got, want):
                bad = np.nonzero(got != want)[0]
                where = "guard" if (bad[0] < GUARD or bad[0] >= GUARD + B) else "payload"
                fails.append(f"pe{pe} {tag}: {len(bad)} bytes differ, first at {int(bad[0]) - GUARD} ({where})")

        def put_case(tag, B, soff=0, doff=0, call=None, kinds=("tester", "random")):
            """Every PE puts B bytes from sbuf + soff into dbuf + doff + GUARD on the next PE."""
            for kind in kinds:
                seedc[0] += 1
                seed = seedc[0]
                if B:
                    hip.upload(sbuf + soff, payload(kind, seed, B, pe, nxt))
                fill_dest(dbuf, doff, B)
                ish.ishmem_barrier_all()  # every dest is filled before a peer writes into it
                rc = (call or ish.ishmem_putmem)(dbuf + doff + GUARD, sbuf + soff, B, nxt)
                if rc:
                    fails.append(f"pe{pe} {tag} {kind}: rc={rc} {ish.last_error()}")
                ish.ishmem_barrier_all()
                check(f"{tag} {kind}", dbuf, doff, payload(kind, seed, B, prv, pe))

        def get_case(tag, B, soff=0, doff=0, call=None, kinds=("tester", "random")):
            """Every PE gets B bytes from sbuf + soff on the next PE into its dbuf + doff + GUARD."""
            for kind in kinds:
                seedc[0] += 1
                seed = seedc[0]
                if B:
                    hip.upload(sbuf + soff, payload(kind, seed, B, pe, prv))
                fill_dest(dbuf, doff, B)
                ish.ishmem_barrier_all()  # every source is in place
                rc = (call or ish.ishmem_getmem)(dbuf + doff + GUARD, sbuf + soff, B, nxt)
                if rc:
                    fails.append(f"pe{pe} {tag} {kind}: rc={rc} {ish.last_error()}")
                check(f"{tag} {kind}", dbuf, doff, payload(kind, seed, B, nxt, pe))
                ish.ishmem_barrier_all()  # nobody refills a source a peer still reads

        if "put_sizes" in scenarios:
            for B in SIZES:
                put_case(f"put B={B}", B)
        if "get_sizes" in scenarios:
            for B in SIZES:
                get_case(f"get B={B}", B)

        def offsets(case, what):
            # Source and dest byte offsets 0-15, independently: every pair at 4097 bytes and at sizes
            # that walk 1..48 as the pairs go by (each size meets several residue pairs).
            n = 0
            for soff in range(16):
                for doff in range(16):
                    n += 1
                    case(f"{what} off s+{soff} d+{doff}", 1 + (n * 7) % 48, soff, doff, kinds=("random",))
                    case(f"{what} off s+{soff} d+{doff}", 4097, soff, doff, kinds=("random",))
            for B in range(1, 49):  # every size 1..48 on a fully misaligned pair
                case(f"{what} off B={B}", B, 5, 11, kinds=("tester",))

        if "put_offsets" in scenarios:
            offsets(put_case, "put")
        if "get_offsets" in scenarios:
            offsets(get_case, "get")

        if "typed" in scenarios:
            # The typed and sized names count elements.
            put_case("float_put", 4 * 1000, call=lambda d, s, B, p: ish.ishmem_float_put(d, s, B // 4, p))
            put_case("put128", 16 * 33, call=lambda d, s, B, p: ish.ishmem_put128(d, s, B // 16, p))
            get_case("uint16_get", 2 * 777, call=lambda d, s, B, p: ish.ishmem_uint16_get(d, s, B // 2, p))
            get_case("get64", 8 * 129, call=lambda d, s, B, p: ish.ishmem_get64(d, s, B // 8, p))

        if "nbi" in scenarios:
            # Several _nbi puts to different PEs, then quiet, then a barrier, then check: PE me writes
            # slot me of every PE's dest (its own included).
            B = 70_003
            slot = (B + 255) & ~255
            for kind in ("tester", "random"):
                seedc[0] += 1
                seed = seedc[0]
                hip.upload(dbuf, np.full(GUARD + npes * slot + GUARD, 0xA5, np.uint8))
                for t in range(npes):
                    hip.upload(sbuf + t * slot, payload(kind, seed, B, pe, t))
                ish.ishmem_barrier_all()
                for k in range(npes):
                    t = (pe + k) % npes
                    rc = ish.ishmem_putmem_nbi(dbuf + GUARD + pe * slot, sbuf + t * slot, B, t)
                    if rc:
                        fails.append(f"pe{pe} nbi put to {t}: {ish.last_error()}")
                if ish.ishmem_fence() or ish.ishmem_quiet():
                    fails.append(f"pe{pe} nbi fence/quiet: {ish.last_error()}")
                ish.ishmem_sync_all()  # quiet completed them: a sync (no implied quiet) is enough
                got = hip.download(dbuf, GUARD + npes * slot + GUARD, np.uint8)
                want = np.full_like(got, 0xA5)
                for f in range(npes):
                    want[GUARD + f * slot:GUARD + f * slot + B] = payload(kind, seed, B, f, pe)
                if not np.array_equal(got, want):
                    fails.append(f"pe{pe} nbi {kind}: {int(np.count_nonzero(got != want))} bytes differ")
                ish.ishmem_barrier_all()
            # _nbi gets, then quiet.
            seedc[0] += 1
            seed = seedc[0]
            hip.upload(sbuf, payload("random", seed, B, pe, prv))
            fill_dest(dbuf, 0, B)
            ish.ishmem_barrier_all()
            if ish.ishmem_getmem_nbi(dbuf + GUARD, sbuf, B, nxt) or ish.ishmem_quiet():
                fails.append(f"pe{pe} nbi get: {ish.last_error()}")
            check("nbi get", dbuf, 0, payload("random", seed, B, nxt, pe))
            ish.ishmem_barrier_all()
            # quiet_on_stream: a stream waits for the pending _nbi put, then a team sync on it.
            seedc[0] += 1
            seed = seedc[0]
            st = hip.stream_create()
            hip.upload(sbuf, payload("random", seed, B, pe, nxt))
            fill_dest(dbuf, 0, B)
            ish.ishmem_barrier_all()
            if ish.ishmem_putmem_nbi(dbuf + GUARD, sbuf, B, nxt) or ish.quiet_on_stream(st) or \
                    ish.team_sync_on_stream(ish.ISHMEM_TEAM_WORLD, None, st):
                fails.append(f"pe{pe} quiet_on_stream: {ish.last_error()}")
            hip.stream_synchronize(st)
            check("quiet_on_stream", dbuf, 0, payload("random", seed, B, prv, pe))
            hip.stream_destroy(st)
            ish.ishmem_barrier_all()

        if "pending" in scenarios:
            # barrier_all alone, without a quiet, completes a pending _nbi put.
            for B in (4097, (1 << 20) + 16):
                seedc[0] += 1
                seed = seedc[0]
                hip.upload(sbuf, payload("random", seed, B, pe, nxt))
                fill_dest(dbuf, 0, B)
                ish.ishmem_barrier_all()
                if ish.ishmem_putmem_nbi(dbuf + GUARD, sbuf, B, nxt):
                    fails.append(f"pe{pe} pending: {ish.last_error()}")
                ish.ishmem_barrier_all()
                check(f"pending B={B}", dbuf, 0, payload("random", seed, B, prv, pe))

        def chain_enqueue(st, B):
            # put to the next PE's dbuf, team sync, get it back from there into tbuf.
            r = ish.put_on_stream(dbuf + GUARD, sbuf, B, nxt, st)
            r = r or ish.team_sync_on_stream(ish.ISHMEM_TEAM_WORLD, ret, st)
            r = r or ish.get_on_stream(tbuf + GUARD, dbuf + GUARD, B, nxt, st)
            if r:
                fails.append(f"pe{pe} chain enqueue: {ish.last_error()}")

        def chain_check(tag, seed, B):
            if int(hip.download(ret, 1, np.int32)[0]) != 0:
                fails.append(f"pe{pe} {tag}: *ret set")
            check(f"{tag} dest", dbuf, 0, payload("random", seed, B, prv, pe))
            check(f"{tag} back", tbuf, 0, payload("random", seed, B, pe, nxt))

        if "chain" in scenarios:
            st = hip.stream_create()
            B = 300_001
            dep, done = hip.Event(), hip.Event()
            seedc[0] += 1
            hip.upload(sbuf, payload("random", seedc[0], B, pe, nxt))
            fill_dest(dbuf, 0, B)
            fill_dest(tbuf, 0, B)
            hip.memset(ret, 0xFF, 4)
            ish.ishmem_barrier_all()
            chain_enqueue(st, B)
            hip.stream_synchronize(st)
            chain_check("chain eager", seedc[0], B)
            ish.ishmem_barrier_all()
            # deps / done on a put.
            seedc[0] += 1
            hip.upload(sbuf, payload("random", seedc[0], B, pe, nxt))
            fill_dest(dbuf, 0, B)
            ish.ishmem_barrier_all()
            dep.record(st)
            if ish.put_on_stream(dbuf + GUARD, sbuf, B, nxt, st, deps=[dep], done=done):
                fails.append(f"pe{pe} chain deps: {ish.last_error()}")
            done.synchronize()
            ish.ishmem_barrier_all()
            check("chain deps", dbuf, 0, payload("random", seedc[0], B, prv, pe))
            hip.stream_destroy(st)

        if "graph" in scenarios:
            st = hip.stream_create()
            B = 300_001
            ish.ishmem_barrier_all()
            with hip.Graph(st) as g:
                chain_enqueue(st, B)
            for rep in range(2):
                seedc[0] += 1
                hip.upload(sbuf, payload("random", seedc[0], B, pe, nxt))
                fill_dest(dbuf, 0, B)
                fill_dest(tbuf, 0, B)
                hip.memset(ret, 0xFF, 4)
                ish.ishmem_barrier_all()
                g.launch()
                hip.stream_synchronize(st)
                chain_check(f"graph replay {rep}", seedc[0], B)
                ish.ishmem_barrier_all()
            del g
            hip.stream_destroy(st)

        if "kinds" in scenarios:
            # The local buffer: heap (every case above), plain device, pinned host, pageable host.
            B = 70_003
            plain = hip.malloc(B + 32)
            pinned = hip.host_malloc(B + 32)
            for name, loc in (("device", plain + 4), ("pinned", pinned + 4), ("pageable", None)):
                seedc[0] += 1
                seed = seedc[0]
                data = payload("random", seed, B, pe, nxt)
                page = np.zeros(B + 32, np.uint8)
                lp = loc if loc is not None else page.ctypes.data + 4
                if name == "pageable":
                    page[4:4 + B] = data
                else:
                    hip.memcpy(lp, np.ascontiguousarray(data).ctypes.data, B)
                fill_dest(dbuf, 0, B)
                ish.ishmem_barrier_all()
                if ish.ishmem_putmem(dbuf + GUARD, lp, B, nxt):
                    fails.append(f"pe{pe} kinds put {name}: {ish.last_error()}")
                ish.ishmem_barrier_all()
                check(f"kinds put {name}", dbuf, 0, payload("random", seed, B, prv, pe))
                # get dbuf's payload on the next PE back into the local buffer
                if ish.ishmem_getmem(lp, dbuf + GUARD, B, nxt):
                    fails.append(f"pe{pe} kinds get {name}: {ish.last_error()}")
                back = np.empty(B, np.uint8)
                if name == "pageable":
                    back[:] = page[4:4 + B]
                else:
                    hip.memcpy(back.ctypes.data, lp, B)
                if not np.array_equal(back, data):  # the next PE's dest holds what this PE put there
                    fails.append(f"pe{pe} kinds get {name}: wrong bytes")
                ish.ishmem_barrier_all()
                if name == "pageable":
                    for fn, nm in ((ish.ishmem_putmem_nbi, "put_nbi"), (ish.ishmem_getmem_nbi, "get_nbi")):
                        args = (dbuf + GUARD, lp, B, nxt) if nm == "put_nbi" else (lp, dbuf + GUARD, B, nxt)
                        if fn(*args) == 0 or "not device-accessible" not in ish.last_error():
                            fails.append(f"pe{pe} kinds {nm} on pageable memory: not refused ('{ish.last_error()}')")
                    if ish.put_on_stream(dbuf + GUARD, lp, B, nxt, 0) == 0 or "not device-accessible" not in ish.last_error():
                        fails.append(f"pe{pe} kinds put_on_stream on pageable memory: not refused")
            hip.host_free(pinned)
            hip.free(plain)

        if "warm" in scenarios:
            # The target's caches hold dest's OLD lines when the put lands: G workgroups each read all
            # of dest with plain loads (two per XCD), barrier, the origin puts, barrier, the same
            # kernel again must see every new byte in every workgroup.
            G = 16
            for B in (64, 4096, 1 << 20):
                n = B // 4
                out = hip.malloc(G * B)
                for rep in range(2):  # the second round finds lines the first round's read left warm
                    seedc[0] += 1
                    seed = seedc[0]
                    old = payload("random", seed, B, 99, pe)
                    hip.upload(dbuf + GUARD, old)
                    hip.upload(sbuf, payload("random", seed, B, pe, nxt))
                    if L.ishmemi_c_read_all_u32(out, dbuf + GUARD, n, G, None):
                        fails.append(f"pe{pe} warm: {ish.last_error()}")
                    got = hip.download(out, G * B, np.uint8).reshape(G, B)
                    if not all(np.array_equal(got[b], old) for b in range(G)):
                        fails.append(f"pe{pe} warm B={B}: the warming read is wrong")
                    ish.ishmem_barrier_all()
                    if ish.ishmem_putmem(dbuf + GUARD, sbuf, B, nxt):
                        fails.append(f"pe{pe} warm put: {ish.last_error()}")
                    ish.ishmem_barrier_all()
                    L.ishmemi_c_read_all_u32(out, dbuf + GUARD, n, G, None)
                    got = hip.download(out, G * B, np.uint8).reshape(G, B)
                    new = payload("random", seed, B, prv, pe)
                    stale = [b for b in range(G) if not np.array_equal(got[b], new)]
                    if stale:
                        fails.append(f"pe{pe} warm B={B} rep {rep}: workgroups {stale} read stale bytes "
                                     f"({int(np.count_nonzero(got != new[None, :]))} bytes)")
                    ish.ishmem_barrier_all()
                hip.free(out)

        if "argfail" in scenarios:
            B = 1000
            plain = hip.malloc(B)
            errs0 = L.ishmemi_c_error_count()
            base, size, used = ctypes.c_void_p(), ctypes.c_size_t(), ctypes.c_size_t()
            L.ishmemi_c_heap_info(ctypes.byref(base), ctypes.byref(size), ctypes.byref(used))
            heap_end = base.value + size.value
            cases = [
                ("pe -1", lambda f: f(dbuf, sbuf, B, -1), "outside [0"),
                ("pe npes", lambda f: f(dbuf, sbuf, B, npes), "outside [0"),
                ("null", lambda f: f(0, sbuf, B, nxt) if f in puts else f(dbuf, 0, B, nxt), "null pointer"),
                ("remote outside heap", lambda f: f(plain, sbuf, B, nxt) if f in puts else f(dbuf, plain, B, nxt),
                 "not inside the symmetric heap"),
                ("remote runs past the heap", lambda f: f(heap_end - 8, sbuf, B, nxt) if f in puts
                 else f(dbuf, heap_end - 8, B, nxt), "not inside the symmetric heap"),
            ]
            puts = (ish.ishmem_putmem, ish.ishmem_putmem_nbi, lambda d, s, n, p: ish.put_on_stream(d, s, n, p, 0))
            gets = (ish.ishmem_getmem, ish.ishmem_getmem_nbi, lambda d, s, n, p: ish.get_on_stream(d, s, n, p, 0))
            for tag, call, word in cases:
                for f in puts + gets:
                    rc = call(f)
                    if rc == 0:
                        fails.append(f"pe{pe} argfail {tag}: returned 0")
                    elif word not in ish.last_error():
                        fails.append(f"pe{pe} argfail {tag}: message '{ish.last_error()}' lacks '{word}'")
            # nbytes == 0 succeeds whatever the pointers.
            if ish.ishmem_putmem(0, 0, 0, nxt) or ish.ishmem_getmem_nbi(0, 0, 0, nxt):
                fails.append(f"pe{pe} argfail: nbytes == 0 failed: {ish.last_error()}")
            if L.ishmemi_c_error_count() != errs0:
                fails.append(f"pe{pe} argfail: error count moved")
            hip.free(plain)
            put_case("after argfail", 4097, kinds=("random",))

        ish.ishmem_barrier_all()
        if L.ishmemi_c_error_count() != 0:
            fails.append(f"pe{pe}: device error count {L.ishmemi_c_error_count()}")
        for b in (ret, tbuf, dbuf, sbuf):
            ish.ishmem_free(b)
        ish.ishmem_finalize()
    except Exception:
        fails.append(f"pe{pe} exception:\n{traceback.format_exc()}")
    q.put((pe, fails))

"""Worker body of the multi-PE put_signal / wait_until GPU tests (tests/test_gpu_signal.py): one
process = one PE, all PEs on one GPU, symmetric heaps mapped into each other over HIP IPC.

Every PE targets (me + 1) % p unless stated.  A dest sits between two 64-byte guards of 0xA5; the
signal word sits in the 8 bytes directly after dest's end rounded up to 8, so a tail store that
overruns lands in the padding, the signal or the guard and shows.  Nothing but the signal tells the
target that the payload has arrived: there is no barrier between a put_signal and the check.
Failures are returned as strings through the queue.
"""
from __future__ import annotations

import ctypes
import os
import threading
import time
import traceback

import numpy as np

GUARD = 64
FUSED_MAX = 64 << 10  # ISHMEM_PUT_SIGNAL_FUSED_MAX_BYTES of the tests' environment
SIZES = [0, 1, 15, 16, 17, 4099, (1 << 20) + 5, FUSED_MAX - 1, FUSED_MAX, FUSED_MAX + 1]
MAXB = (1 << 20) + 64
EQ, NE, GT, GE, LT, LE = 1, 2, 3, 4, 5, 6
SET, ADD = 0, 1
CMP_NAMES = {EQ: "EQ", NE: "NE", GT: "GT", GE: "GE", LT: "LT", LE: "LE"}
# typename -> (bits, signed): the 12 synchronisation typenames on LP64.
SYNC_TYPES = {"int": (32, True), "long": (64, True), "longlong": (64, True), "uint": (32, False), "ulong": (64, False),
              "ulonglong": (64, False), "int32": (32, True), "int64": (64, True), "uint32": (32, False),
              "uint64": (64, False), "size": (64, False), "ptrdiff": (64, True)}


def as_type(v: int, bits: int, signed: bool) -> int:
    """v's low `bits` bits read as a value of the type."""
    v &= (1 << bits) - 1
    return v - (1 << bits) if signed and v >> (bits - 1) else v


def cmp_holds(v: int, cmp: int, c: int, bits: int, signed: bool) -> bool:
    """ISHMEM_CMP_* of two values in the variable's own type (the expectation of the GPU tests)."""
    a, b = as_type(v, bits, signed), as_type(c, bits, signed)
    return {EQ: a == b, NE: a != b, GT: a > b, GE: a >= b, LT: a < b, LE: a <= b}[cmp]


def flip_case(bits: int, signed: bool, cmp: int) -> tuple[int, int, int]:
    """(before, cmp_value, after): `cmp` against cmp_value is false for before and true for after.
    The values are chosen so that a comparison in the wrong signedness, or of the low 32 bits of a
    64-bit variable only, gives another answer: -1 / 0 / 1 (int32), 0 / 0x7FFFFFFF / 0xFFFFFFFF
    (uint32), and 64-bit values whose low halves are all 7."""
    if bits == 32:
        lo, mid, hi = (-1, 0, 1) if signed else (0, 0x7FFFFFFF, 0xFFFFFFFF)
    else:
        lo, mid, hi = (7 - (1 << 32), 7, 7 + (1 << 32)) if signed else (7, 7 + (1 << 32), 7 + (1 << 63))
    return {EQ: (lo, mid, mid), NE: (mid, mid, hi), GT: (mid, mid, hi), GE: (lo, mid, mid), LT: (mid, mid, lo),
            LE: (hi, mid, mid)}[cmp]


def round_pattern(r: int, frm: int, n: int) -> np.ndarray:
    """n uint32 words that depend on the round, the origin and every word index."""
    i = np.arange(n, dtype=np.uint64)
    return ((i * np.uint64(2654435761) + np.uint64(r * 0x9E3779B1 + frm * 0x85EBCA6B + 1)) & np.uint64(0xFFFFFFFF)).astype("<u4")


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
        from tests.rma_worker import payload

        ish.init(pe, npes, 0, key)
        L = ish.lib()
        if int(ish.get_param("put_signal_fused_max_bytes")) != FUSED_MAX:
            fails.append(f"pe{pe}: put_signal_fused_max_bytes {ish.get_param('put_signal_fused_max_bytes')} != {FUSED_MAX}")
        nxt, prv = (pe + 1) % npes, (pe - 1) % npes
        arena = MAXB + 2 * GUARD + 256
        sbuf = ish.ishmem_align(256, arena)
        dbuf = ish.ishmem_align(256, arena)
        tbuf = ish.ishmem_align(256, arena)
        words = ish.ishmem_align(256, 256)  # small symmetric words: signals, variables, *ret, *value
        sigA, sigB, ivar, retw, valw = words, words + 8, words + 16, words + 24, words + 32
        seedc = [0]
        expected_errors = 0

        def set_u64(addr, v):
            hip.upload(addr, np.array([v & ((1 << 64) - 1)], dtype="<u8"))

        def sig_after(dest, B):
            return (dest + B + 7) & ~7

        def region_len(doff, B):
            """guard, doff + B payload bytes, padding to 8, the signal word, guard."""
            return sig_after(GUARD + doff + B, 0) + 8 + GUARD

        def check_region(tag, buf, doff, want_body, want_sig):
            B = len(want_body)
            n = region_len(doff, B)
            got = hip.download(buf, n, np.uint8)
            want = np.full(n, 0xA5, np.uint8)
            want[GUARD + doff:GUARD + doff + B] = want_body
            so = sig_after(GUARD + doff + B, 0)
            want[so:so + 8] = np.array([want_sig], dtype="<u8").view(np.uint8)
            if not np.array_equal(got, want):
                bad = np.nonzero(got != want)[0]
                first = int(bad[0])
                where = ("payload" if GUARD + doff <= first < GUARD + doff + B else "signal" if so <= first < so + 8
                         else "guard or padding")
                fails.append(f"pe{pe} {tag}: {len(bad)} bytes differ, first at {first - GUARD - doff} ({where})")

        def put_signal_case(tag, B, op, soff=0, doff=0, call=None, after=None, kind="random"):
            """Every PE puts B bytes into dbuf + GUARD + doff on the next PE and updates the signal word
            directly behind it; the target learns of it through signal_wait_until alone."""
            seedc[0] += 1
            seed = seedc[0]
            init, val = (0, seed + 1) if op == SET else (1000 + seed, 3)
            expect = val if op == SET else init + val
            if B:
                hip.upload(sbuf + soff, payload(kind, seed, B, pe, nxt))
            n = region_len(doff, B)
            fill = np.full(n, 0xA5, np.uint8)
            so = sig_after(GUARD + doff + B, 0)
            fill[so:so + 8] = np.array([init], dtype="<u8").view(np.uint8)
            hip.upload(dbuf, fill)
            ish.ishmem_barrier_all()  # every dest and signal word is prepared before a peer writes
            dest = dbuf + GUARD + doff
            rc = (call or ish.ishmem_putmem_signal)(dest, sbuf + soff, B, dbuf + so, val, op, nxt)
            if rc:
                fails.append(f"pe{pe} {tag}: rc={rc} {ish.last_error()}")
            rc, v = ish.wait_until(dbuf + so, "uint64", EQ, expect)
            if rc or v != expect:
                fails.append(f"pe{pe} {tag}: wait rc={rc} value {v} != {expect} {ish.last_error()}")
            check_region(tag, dbuf, doff, payload(kind, seed, B, prv, pe), expect)
            if after:
                after()
            ish.ishmem_barrier_all()

        if "sizes" in scenarios:
            for B in SIZES:
                for op in (SET, ADD):
                    put_signal_case(f"put_signal B={B} op={op}", B, op)
            # typed, sized and mem names (the typed and sized ones count elements), _nbi too
            put_signal_case("float_put_signal", 4 * 1000, SET,
                            call=lambda d, s, B, sg, v, op, p: ish.ishmem_float_put_signal(d, s, B // 4, sg, v, op, p))
            put_signal_case("put128_signal", 16 * 33, ADD,
                            call=lambda d, s, B, sg, v, op, p: ish.ishmem_put128_signal(d, s, B // 16, sg, v, op, p))
            put_signal_case("uint16_put_signal_nbi", 2 * 777, SET, after=ish.ishmem_quiet,
                            call=lambda d, s, B, sg, v, op, p: ish.ishmem_uint16_put_signal_nbi(d, s, B // 2, sg, v, op, p))
            put_signal_case("put64_signal_nbi", 8 * 9001, ADD, after=ish.ishmem_quiet,
                            call=lambda d, s, B, sg, v, op, p: ish.ishmem_put64_signal_nbi(d, s, B // 8, sg, v, op, p))
            put_signal_case("putmem_signal_nbi", FUSED_MAX + 77, SET, after=ish.ishmem_quiet,
                            call=ish.ishmem_putmem_signal_nbi)

        if "offsets" in scenarios:
            for soff in (0, 4, 9):
                for doff in (0, 8, 13):
                    for B in (37, 4099, FUSED_MAX + 4099):
                        put_signal_case(f"put_signal off s+{soff} d+{doff} B={B}", B, SET if (soff + doff) % 2 else ADD,
                                        soff, doff)

        if "ordering" in scenarios:
            # In round r the origin fills its source with a pattern of r and every index and calls
            # put_signal(SET, r).  The target warms its caches with dest's old lines from 16 workgroups,
            # waits for the signal on the host, and 16 workgroups then read dest with plain loads: every
            # one of them must see round r in every word.  No barrier between the put and the check.
            G = 16
            st = hip.stream_create()
            for form in ("blocking", "nbi", "on_stream"):
                for B in (64, 4096, 1 << 20):
                    n = B // 4
                    out = hip.malloc(G * B)
                    sig = dbuf + GUARD + B  # directly after dest
                    fill = np.full(GUARD + B + 8 + GUARD, 0xA5, np.uint8)
                    fill[GUARD + B:GUARD + B + 8] = 0
                    hip.upload(dbuf, fill)
                    ish.ishmem_barrier_all()
                    for r in range(1, 7):
                        hip.upload(sbuf, round_pattern(r, pe, n))
                        if L.ishmemi_c_read_all_u32(out, dbuf + GUARD, n, G, None):
                            fails.append(f"pe{pe} ordering warm: {ish.last_error()}")
                        hip.synchronize()
                        if form == "blocking":
                            rc = ish.ishmem_putmem_signal(dbuf + GUARD, sbuf, B, sig, r, SET, nxt)
                        elif form == "nbi":
                            rc = ish.ishmem_putmem_signal_nbi(dbuf + GUARD, sbuf, B, sig, r, SET, nxt)
                        else:
                            rc = ish.put_signal_on_stream(dbuf + GUARD, sbuf, B, sig, r, SET, nxt, st)
                        if rc:
                            fails.append(f"pe{pe} ordering {form} put_signal: {ish.last_error()}")
                        v = ish.ishmem_signal_wait_until(sig, EQ, r)
                        if v != r:
                            fails.append(f"pe{pe} ordering {form} B={B} round {r}: wait returned {v}: {ish.last_error()}")
                        L.ishmemi_c_read_all_u32(out, dbuf + GUARD, n, G, None)
                        got = hip.download(out, G * n, np.uint32).reshape(G, n)
                        want = round_pattern(r, prv, n)
                        stale = [b for b in range(G) if not np.array_equal(got[b], want)]
                        if stale:
                            fails.append(f"pe{pe} ordering {form} B={B} round {r}: workgroups {stale} read "
                                         f"{int(np.count_nonzero(got != want[None, :]))} words that are not round {r}'s")
                        # This PE's own put is complete before its source is refilled ...
                        if form == "nbi":
                            ish.ishmem_quiet()
                        elif form == "on_stream":
                            hip.stream_synchronize(st)
                        # ... and round r + 1 must not overwrite a dest that is still being checked.
                        ish.ishmem_sync_all()
                    tail = hip.download(dbuf, GUARD + B + 8 + GUARD, np.uint8)
                    if not (np.all(tail[:GUARD] == 0xA5) and np.all(tail[GUARD + B + 8:] == 0xA5)):
                        fails.append(f"pe{pe} ordering {form} B={B}: guard bytes changed")
                    hip.free(out)
                    ish.ishmem_barrier_all()
            hip.stream_destroy(st)

        if "fanin" in scenarios:
            B = 70_003
            slot = (B + 255) & ~255
            for rep in range(2):
                seedc[0] += 1
                seed = seedc[0]
                hip.upload(dbuf, np.full(GUARD + npes * slot + GUARD, 0xA5, np.uint8))
                set_u64(sigA, 0)
                hip.upload(sbuf, payload("random", seed, B, pe, 0))
                ish.ishmem_barrier_all()
                if npes == 1 or pe != 0:
                    if ish.ishmem_putmem_signal(dbuf + GUARD + pe * slot, sbuf, B, sigA, 1, ADD, 0):
                        fails.append(f"pe{pe} fanin put_signal: {ish.last_error()}")
                if pe == 0:
                    want_n = max(1, npes - 1)
                    rc, v = ish.wait_until(sigA, "uint64", EQ, want_n)
                    if rc or v != want_n:
                        fails.append(f"pe0 fanin wait rc={rc} v={v}: {ish.last_error()}")
                    got = hip.download(dbuf, GUARD + npes * slot + GUARD, np.uint8)
                    want = np.full_like(got, 0xA5)
                    for f in range(npes):
                        if npes == 1 or f != 0:
                            want[GUARD + f * slot:GUARD + f * slot + B] = payload("random", seed, B, f, 0)
                    if not np.array_equal(got, want):
                        fails.append(f"pe0 fanin: {int(np.count_nonzero(got != want))} bytes differ")
                    if ish.signal_fetch(sigA) != (0, want_n) or ish.ishmem_signal_fetch(sigA) != want_n:
                        fails.append(f"pe0 fanin: signal_fetch {ish.signal_fetch(sigA)} != (0, {want_n})")
                ish.ishmem_barrier_all()

        def p_value(addr, v, bits, to):
            """ishmem_<TN>_p: one element through a host variable (the blocking put's pageable path)."""
            a = np.array([v & ((1 << bits) - 1)], dtype="<u4" if bits == 32 else "<u8")
            if ish.ishmem_putmem(addr, a.ctypes.data, bits // 8, to):
                fails.append(f"pe{pe} p: {ish.last_error()}")

        if "waittest" in scenarios:
            for tn, (bits, signed) in SYNC_TYPES.items():
                test_fn, wait_fn = getattr(ish, f"ishmem_{tn}_test"), getattr(ish, f"ishmem_{tn}_wait_until")
                for cmp in (EQ, NE, GT, GE, LT, LE):
                    before, cval, after = flip_case(bits, signed, cmp)
                    tag = f"pe{pe} {tn} {CMP_NAMES[cmp]}"
                    set_u64(ivar, 0x5A5A5A5A5A5A5A5A)  # a 32-bit variable's neighbour word must not matter
                    hip.upload(ivar, np.array([before & ((1 << bits) - 1)], dtype="<u4" if bits == 32 else "<u8"))
                    ish.ishmem_barrier_all()
                    if test_fn(ivar, cmp, cval) != 0:
                        fails.append(f"{tag}: test is 1 before the peer's p ({ish.last_error()})")
                    ish.ishmem_sync_all()  # every PE has tested before any variable flips
                    p_value(ivar, after, bits, nxt)
                    if wait_fn(ivar, cmp, cval):
                        fails.append(f"{tag}: wait_until failed: {ish.last_error()}")
                    if test_fn(ivar, cmp, cval) != 1:
                        fails.append(f"{tag}: test is 0 after the peer's p ({ish.last_error()})")
                    rc, v = ish.wait_until(ivar, ish.TYPENAMES[tn], cmp, cval)
                    if rc or ((v - after) & ((1 << bits) - 1)):
                        fails.append(f"{tag}: wait_until returned rc={rc} value {v:#x}, want {after:#x}")
                    ish.ishmem_barrier_all()

        if "sigops" in scenarios:
            set_u64(sigA, 5)
            ish.ishmem_barrier_all()
            if ish.ishmemx_signal_set(sigA, 41 + pe, nxt):
                fails.append(f"pe{pe} signal_set: {ish.last_error()}")
            ish.ishmem_barrier_all()
            if ish.signal_fetch(sigA) != (0, 41 + prv):
                fails.append(f"pe{pe} after signal_set: fetch {ish.signal_fetch(sigA)}")
            ish.ishmem_barrier_all()
            if ish.ishmemx_signal_add(sigA, (1 << 40) + 2, nxt):
                fails.append(f"pe{pe} signal_add: {ish.last_error()}")
            rc, v = ish.wait_until(sigA, "uint64", GT, 1 << 40)
            if rc or v != 41 + prv + (1 << 40) + 2 or ish.ishmem_signal_fetch(sigA) != v:
                fails.append(f"pe{pe} after signal_add: rc={rc} value {v}")
            ish.ishmem_barrier_all()

        def chain_enqueue(st, B, out, G):
            # origin: put_signal to the next PE.  target: wait for the signal, consume dest with plain
            # loads, put the first copy back to the origin with a signal of its own, and reset its signal
            # word (a put_signal of no bytes to itself).  origin: wait for the echo, reset that word too.
            r = ish.put_signal_on_stream(dbuf + GUARD, sbuf, B, sigA, 1, SET, nxt, st)
            r = r or ish.signal_wait_until_on_stream(sigA, EQ, 1, valw, st, ret=retw)
            r = r or L.ishmemi_c_read_all_u32(out, dbuf + GUARD, B // 4, G, st)
            r = r or ish.put_signal_on_stream(tbuf + GUARD, out, B, sigB, 1, SET, prv, st)
            r = r or ish.put_signal_on_stream(0, 0, 0, sigA, 0, SET, pe, st)
            r = r or ish.wait_until_on_stream(sigB, "uint64", GE, 1, 0, 0, st)
            r = r or ish.put_signal_on_stream(0, 0, 0, sigB, 0, SET, pe, st)
            if r:
                fails.append(f"pe{pe} chain enqueue: {ish.last_error()}")

        def chain_round(tag, launch, st, B, out, G):
            seedc[0] += 1
            seed = seedc[0]
            hip.upload(sbuf, payload("random", seed, B, pe, nxt))
            for buf in (dbuf, tbuf):
                hip.upload(buf, np.full(GUARD + B + GUARD, 0xA5, np.uint8))
            hip.memset(retw, 0xFF, 4)
            set_u64(valw, 0)
            ish.ishmem_barrier_all()
            launch()
            hip.stream_synchronize(st)
            if int(hip.download(retw, 1, np.int32)[0]) != 0 or int(hip.download(valw, 1, np.uint64)[0]) != 1:
                fails.append(f"pe{pe} {tag}: *ret {hip.download(retw, 1, np.int32)[0]}, *ret_value "
                             f"{hip.download(valw, 1, np.uint64)[0]}")
            g = np.full(GUARD, 0xA5, np.uint8)
            for name, buf, body in (("dest", dbuf, payload("random", seed, B, prv, pe)),
                                    ("echo", tbuf, payload("random", seed, B, pe, nxt))):
                if not np.array_equal(hip.download(buf, GUARD + B + GUARD, np.uint8), np.concatenate([g, body, g])):
                    fails.append(f"pe{pe} {tag}: {name} is wrong")
            got = hip.download(out, G * B, np.uint8).reshape(G, B)
            if not all(np.array_equal(got[b], payload("random", seed, B, prv, pe)) for b in range(G)):
                fails.append(f"pe{pe} {tag}: the consumer kernel read stale bytes")
            if ish.signal_fetch(sigA) != (0, 0) or ish.signal_fetch(sigB) != (0, 0):
                fails.append(f"pe{pe} {tag}: the handshake was not reset")
            ish.ishmem_barrier_all()

        if "chain" in scenarios or "graph" in scenarios:
            B, G = 300_000, 4
            out = ish.ishmem_align(256, G * B)  # symmetric: the echo's source is classified without a HIP call
            st = hip.stream_create()
            set_u64(sigA, 0)
            set_u64(sigB, 0)
            ish.ishmem_barrier_all()
            if "chain" in scenarios:
                for rep in range(2):
                    chain_round(f"chain eager {rep}", lambda: chain_enqueue(st, B, out, G), st, B, out, G)
            if "graph" in scenarios:
                with hip.Graph(st) as g:
                    chain_enqueue(st, B, out, G)
                for rep in range(2):
                    chain_round(f"graph replay {rep}", g.launch, st, B, out, G)
                del g
            hip.stream_destroy(st)
            ish.ishmem_free(out)

        if "thread" in scenarios:
            # PE 0's main thread blocks in signal_wait_until while a second thread of PE 0 issues the put
            # and the put_signal that PE 1 (PE 0 itself when alone) waits for before it signals back: a
            # wait that kept the library's lock would end in the timeout error.
            B = 4096
            peer = 1 % npes
            seedc[0] += 1
            seed = seedc[0]
            set_u64(sigA, 0)
            set_u64(sigB, 0)
            hip.upload(dbuf, np.full(2 * B, 0xA5, np.uint8))
            hip.upload(sbuf, payload("random", seed, 2 * B, 0, peer))
            ish.ishmem_barrier_all()
            t0 = time.monotonic()
            if pe == 0:
                go = threading.Event()
                terr: list[str] = []

                def second_thread():
                    go.wait()
                    if ish.ishmem_putmem(dbuf, sbuf, B, peer):
                        terr.append(f"put: {ish.last_error()}")
                    if ish.ishmem_putmem_signal(dbuf + B, sbuf + B, B, sigB, 1, SET, peer):
                        terr.append(f"put_signal: {ish.last_error()}")
                    if npes == 1 and ish.ishmemx_signal_set(sigA, 7, 0):
                        terr.append(f"signal_set: {ish.last_error()}")

                th = threading.Thread(target=second_thread)
                th.start()
                go.set()
                v = ish.ishmem_signal_wait_until(sigA, EQ, 7)
                th.join()
                if v != 7 or terr:
                    fails.append(f"pe0 thread: wait returned {v} ({ish.last_error()}) {terr}")
            if pe == peer:
                rc, v = ish.wait_until(sigB, "uint64", EQ, 1)
                if rc:
                    fails.append(f"pe{pe} thread: wait for PE 0's second thread: {ish.last_error()}")
                if not np.array_equal(hip.download(dbuf, 2 * B, np.uint8), payload("random", seed, 2 * B, 0, peer)):
                    fails.append(f"pe{pe} thread: wrong bytes from PE 0's second thread")
                if npes > 1 and ish.ishmemx_signal_set(sigA, 7, 0):
                    fails.append(f"pe{pe} thread: signal back: {ish.last_error()}")
            if time.monotonic() - t0 > 10.0:
                fails.append(f"pe{pe} thread: took {time.monotonic() - t0:.1f} s")
            ish.ishmem_barrier_all()

        if "argfail" in scenarios:
            B = 1000
            plain = hip.malloc(B)
            errs0 = L.ishmemi_c_error_count()
            base, size, used = ctypes.c_void_p(), ctypes.c_size_t(), ctypes.c_size_t()
            L.ishmemi_c_heap_info(ctypes.byref(base), ctypes.byref(size), ctypes.byref(used))
            heap_end = base.value + size.value
            puts = (ish.ishmem_putmem_signal, ish.ishmem_putmem_signal_nbi,
                    lambda d, s, n, sg, v, op, p: ish.put_signal_on_stream(d, s, n, sg, v, op, p, 0))
            set_u64(sigA, 0)
            cases = [
                ("pe -1", lambda f: f(dbuf, sbuf, B, sigA, 1, SET, -1), "outside [0"),
                ("pe npes", lambda f: f(dbuf, sbuf, B, sigA, 1, SET, npes), "outside [0"),
                ("sig_op 2", lambda f: f(dbuf, sbuf, B, sigA, 1, 2, nxt), "sig_op"),
                ("sig_op -1", lambda f: f(dbuf, sbuf, 0, sigA, 1, -1, nxt), "sig_op"),
                ("sig misaligned", lambda f: f(dbuf, sbuf, B, sigA + 4, 1, SET, nxt), "8-byte aligned"),
                ("sig outside heap", lambda f: f(dbuf, sbuf, B, plain, 1, SET, nxt), "not inside the symmetric heap"),
                ("sig null", lambda f: f(dbuf, sbuf, B, 0, 1, SET, nxt), "sig_addr"),
                ("null dest", lambda f: f(0, sbuf, B, sigA, 1, SET, nxt), "null pointer"),
                ("dest outside heap", lambda f: f(plain, sbuf, B, sigA, 1, SET, nxt), "not inside the symmetric heap"),
                ("dest runs past the heap", lambda f: f(heap_end - 8, sbuf, B, sigA, 1, SET, nxt),
                 "not inside the symmetric heap"),
            ]
            for tag, call, word in cases:
                for f in puts:
                    rc = call(f)
                    if rc == 0:
                        fails.append(f"pe{pe} argfail {tag}: returned 0")
                    elif word not in ish.last_error():
                        fails.append(f"pe{pe} argfail {tag}: message '{ish.last_error()}' lacks '{word}'")
            page = np.zeros(B, np.uint8)
            for f in puts[1:]:
                if f(dbuf, page.ctypes.data, B, sigA, 1, SET, nxt) == 0 or "not device-accessible" not in ish.last_error():
                    fails.append(f"pe{pe} argfail pageable source: not refused ('{ish.last_error()}')")
            more = [
                ("signal_set pe", lambda: ish.ishmemx_signal_set(sigA, 1, npes), "outside [0"),
                ("signal_add misaligned", lambda: ish.ishmemx_signal_add(sigA + 2, 1, nxt), "8-byte aligned"),
                ("signal_op op", lambda: L.ishmemi_c_signal_op(sigA, 1, 7, nxt), "sig_op"),
                ("fetch outside heap", lambda: ish.signal_fetch(plain)[0], "not inside the symmetric heap"),
                ("wait cmp 0", lambda: ish.wait_until(sigA, "uint64", 0, 1)[0], "cmp"),
                ("wait cmp 7", lambda: ish.wait_until(sigA, "int32", 7, 1)[0], "cmp"),
                ("test cmp 9", lambda: ish.test(sigA, "int64", 9, 1)[0], "cmp"),
                ("wait dtype float", lambda: ish.wait_until(sigA, "float", EQ, 1)[0], "dtype"),
                ("wait dtype int16", lambda: ish.wait_until(sigA, "int16", EQ, 1)[0], "dtype"),
                ("wait misaligned", lambda: ish.wait_until(sigA + 4, "uint64", EQ, 1)[0], "8-byte aligned"),
                ("test misaligned", lambda: ish.test(sigA + 2, "uint32", EQ, 1)[0], "4-byte aligned"),
                ("wait outside heap", lambda: ish.wait_until(plain, "uint64", EQ, 1)[0], "not inside the symmetric heap"),
                ("wait_on_stream cmp", lambda: ish.wait_until_on_stream(sigA, "uint64", 0, 1, 0, 0, 0), "cmp"),
                ("wait_on_stream null", lambda: ish.wait_until_on_stream(0, "uint64", EQ, 1, 0, 0, 0), "ivar"),
            ]
            for tag, call, word in more:
                rc = call()
                if rc == 0:
                    fails.append(f"pe{pe} argfail {tag}: returned 0")
                elif word not in ish.last_error():
                    fails.append(f"pe{pe} argfail {tag}: message '{ish.last_error()}' lacks '{word}'")
            if L.ishmemi_c_error_count() != errs0:
                fails.append(f"pe{pe} argfail: error count moved")
            ish.ishmem_barrier_all()
            if ish.signal_fetch(sigA) != (0, 0):
                fails.append(f"pe{pe} argfail: a refused call updated the signal: {ish.signal_fetch(sigA)}")
            hip.free(plain)
            put_signal_case("after argfail", 4099, SET)

        if "bounded" in scenarios:
            # Runs with ISHMEM_TIMEOUT_MS=300: a wait for a word nobody writes returns with an error.
            set_u64(sigA, 3)
            errs0 = L.ishmemi_c_error_count()
            t0 = time.monotonic()
            rc, v = ish.wait_until(sigA, "uint64", EQ, 99)
            dt = time.monotonic() - t0
            if rc == 0 or "timed out" not in ish.last_error() or v != 3 or dt > 5.0 or dt < 0.25:
                fails.append(f"pe{pe} bounded host wait: rc={rc} value {v} after {dt:.2f} s: '{ish.last_error()}'")
            if L.ishmemi_c_error_count() != errs0 + 1:
                fails.append(f"pe{pe} bounded host wait: error count {L.ishmemi_c_error_count()} != {errs0 + 1}")
            st = hip.stream_create()
            hip.memset(retw, 0, 4)
            t0 = time.monotonic()
            if ish.wait_until_on_stream(sigA, "uint64", GT, 99, valw, retw, st):
                fails.append(f"pe{pe} bounded on_stream: {ish.last_error()}")
            hip.stream_synchronize(st)
            dt = time.monotonic() - t0
            if int(hip.download(retw, 1, np.int32)[0]) == 0 or dt > 5.0:
                fails.append(f"pe{pe} bounded on_stream: *ret {hip.download(retw, 1, np.int32)[0]} after {dt:.2f} s")
            if L.ishmemi_c_error_count() != errs0 + 2:
                fails.append(f"pe{pe} bounded on_stream: error count {L.ishmemi_c_error_count()} != {errs0 + 2}")
            hip.stream_destroy(st)
            expected_errors = 1  # the host wait's; resync clears the device's word
            ish.set_param("timeout_ms", 20000)
            if ish.resync() != 0:
                fails.append(f"pe{pe} resync failed: {ish.last_error()}")
            put_signal_case("after a timed-out wait", 4099, SET)

        ish.ishmem_barrier_all()
        if L.ishmemi_c_error_count() != expected_errors:
            fails.append(f"pe{pe}: device error count {L.ishmemi_c_error_count()}")
        for b in (words, tbuf, dbuf, sbuf):
            ish.ishmem_free(b)
        ish.ishmem_finalize()
    except Exception:
        fails.append(f"pe{pe} exception:\n{traceback.format_exc()}")
    q.put((pe, fails))

"""Worker body of the multi-PE atomic-memory-operation GPU tests (tests/test_gpu_amo.py): one process =
one PE, all PEs on one GPU, symmetric heaps mapped into each other over HIP IPC.

Expected values come from amo_model, Python integers masked to the width (pinned by known answers in
tests/test_amo.py).  Every PE targets (me + 1) % p unless stated, on a 64-byte line of the target that
this origin owns: the target word between two guard words of the same width, so a 64-bit operation on
a 32-bit type shows in a guard.  Failures are returned as strings through the queue.
"""
from __future__ import annotations

import os
import threading
import traceback

import numpy as np

EQ, GE = 1, 4
FETCHING = ("fetch", "compare_swap", "swap", "fetch_inc", "fetch_add", "fetch_and", "fetch_or", "fetch_xor")
OPS = ("fetch", "set", "compare_swap", "swap", "fetch_inc", "inc", "fetch_add", "add", "fetch_and", "and", "fetch_or",
       "or", "fetch_xor", "xor")
INT_DTYPES = {"int32": 4, "uint32": 4, "int64": 8, "uint64": 8}
FLOAT_DTYPES = {"float": 4, "double": 8}
FLOAT_OPS = ("fetch", "set", "swap")
GUARD32, GUARD64 = 0xA5A5A5A5, 0xA5A5A5A5A5A5A5A5
# (old, value, cond) per width.  32-bit: 0x7FFFFFFF + 1 and 0xFFFFFFFF + 1, masks with bits in both
# 16-bit halves; compare_swap matches in the first and third triple and misses in the second, whose
# cond equals the word in the low half only.  64-bit: the carry out of the low half, an operand with
# bits in both halves, the same hit / miss pattern.
OPERANDS = {
    4: [(0x7FFFFFFF, 1, 0x7FFFFFFF), (0xFFFFFFFF, 1, 0x7FFFFFFF), (0xF0F00F0F, 0xFF0000FF, 0xF0F00F0F)],
    8: [(0x00000000FFFFFFFF, 1, 0x00000000FFFFFFFF), (0x1234567890ABCDEF, 0x8000000100000002, 0x0234567890ABCDEF),
        (0xF0F0F0F00F0F0F0F, 0xFF00FF0000FF00FF, 0xF0F0F0F00F0F0F0F)],
}
# float / double travel as bits: 1.0, -0.0 and a quiet NaN with a payload.
FLOAT_OPERANDS = {
    4: [(0x3F800000, 0x80000000, 0), (0x80000000, 0x7FC12345, 0), (0x7FC12345, 0x3F800000, 0)],
    8: [(0x3FF0000000000000, 0x8000000000000000, 0), (0x8000000000000000, 0x7FF80000DEADBEEF, 0),
        (0x7FF80000DEADBEEF, 0x3FF0000000000000, 0)],
}


def amo_model(op: str, width: int, old: int, value: int, cond: int) -> tuple[int, int]:
    """(new, fetched) of one AMO on a `width`-byte word holding `old`; fetched is 0 for a
    non-fetching operation (what the C ABI reports)."""
    m = (1 << (8 * width)) - 1
    old, value, cond = old & m, value & m, cond & m
    base = op[6:] if op.startswith("fetch_") else op
    if base == "fetch":
        new = old
    elif base in ("set", "swap"):
        new = value
    elif base == "compare_swap":
        new = value if old == cond else old
    elif base == "inc":
        new = (old + 1) & m
    elif base == "add":
        new = (old + value) & m
    elif base == "and":
        new = old & value
    elif base == "or":
        new = old | value
    elif base == "xor":
        new = old ^ value
    else:
        raise ValueError(op)
    return new, (old if op in FETCHING else 0)


def call_args(op: str, value: int, cond: int) -> tuple:
    """The [value], [cond] part of a Python atomic_<op> call."""
    if op == "compare_swap":
        return (cond, value)
    if op in ("fetch", "fetch_inc", "inc"):
        return ()
    return (value,)


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
        from tests.signal_worker import round_pattern

        ish.init(pe, npes, 0, key)
        L = ish.lib()
        nxt, prv = (pe + 1) % npes, (pe - 1) % npes
        lines = ish.ishmem_align(256, 64 * 16)   # line j: the words origin j owns on this PE
        shared = ish.ishmem_align(256, 256)      # words every PE updates (on PE 0)
        gath = ish.ishmem_align(256, 16 * 128 * 8)  # [origin][128] u64 gathered on PE 0
        fheap = ish.ishmem_align(256, 32 * 8)    # an _nbi fetch array in the heap
        mine = lines + 64 * pe                   # this origin's line, as a symmetric address

        def np_t(width):
            return "<u4" if width == 4 else "<u8"

        def word_at(width):
            """Offset of the target word in the line: 12 for 4 bytes (off the 8-byte grid), 16 for 8."""
            return 12 if width == 4 else 16

        def prepare(width, old, to):
            """guard | word = old | guard on this origin's line of PE `to` (a blocking put from host memory)."""
            g = GUARD32 if width == 4 else GUARD64
            a = np.array([g, old & ((1 << 8 * width) - 1), g], dtype=np_t(width))
            if ish.ishmem_putmem(mine + word_at(width) - width, a.ctypes.data, 3 * width, to):
                fails.append(f"pe{pe} prepare: {ish.last_error()}")

        def check(tag, width, want, to):
            a = np.zeros(3, dtype=np_t(width))
            if ish.ishmem_getmem(a.ctypes.data, mine + word_at(width) - width, 3 * width, to):
                fails.append(f"pe{pe} {tag}: get: {ish.last_error()}")
            g = GUARD32 if width == 4 else GUARD64
            if int(a[0]) != g or int(a[2]) != g:
                fails.append(f"pe{pe} {tag}: a guard word changed: {int(a[0]):#x} {int(a[2]):#x}")
            if int(a[1]) != want:
                fails.append(f"pe{pe} {tag}: word {int(a[1]):#x}, want {want:#x}")

        def set_word(addr, v, width=8):
            hip.upload(addr, np.array([v & ((1 << 8 * width) - 1)], dtype=np_t(width)))

        def gather_check(tag, vals, want_sorted, final_addr, final_dtype, final_want):
            """Every PE's fetched values to row pe of PE 0's gath; PE 0 checks the multiset and the word."""
            a = np.array(vals, dtype="<u8")
            if ish.ishmem_putmem(gath + pe * 128 * 8, a.ctypes.data, a.nbytes, 0):
                fails.append(f"pe{pe} {tag}: put: {ish.last_error()}")
            ish.ishmem_barrier_all()
            if pe == 0:
                got = hip.download(gath, 16 * 128, np.uint64).reshape(16, 128)[:npes, :len(vals)].ravel()
                if sorted(int(x) for x in got) != want_sorted:
                    fails.append(f"pe0 {tag}: the fetched values are not each of the expected ones once")
                rc, v = ish.atomic_fetch(final_addr, final_dtype, 0)
                if rc or v != final_want:
                    fails.append(f"pe0 {tag}: final word rc={rc} {v:#x}, want {final_want:#x}")
            ish.ishmem_barrier_all()

        if "matrix" in scenarios:
            for dtypes, ops, table in ((INT_DTYPES, OPS, OPERANDS), (FLOAT_DTYPES, FLOAT_OPS, FLOAT_OPERANDS)):
                for dt, width in dtypes.items():
                    for op in ops:
                        for old, value, cond in table[width]:
                            tag = f"{op} {dt} old={old:#x} value={value:#x} cond={cond:#x}"
                            prepare(width, old, nxt)
                            rc, f = getattr(ish, f"atomic_{op}")(mine + word_at(width), dt, *call_args(op, value, cond), nxt)
                            new, fetched = amo_model(op, width, old, value, cond)
                            if rc or f != fetched:
                                fails.append(f"pe{pe} {tag}: rc={rc} fetched {f:#x}, want {fetched:#x} {ish.last_error()}")
                            check(tag, width, new, nxt)
            ish.ishmem_barrier_all()

        if "contended" in scenarios:
            ctr = shared
            for tag, dt, width, step in (("fetch_add int32", "int32", 4, 1), ("fetch_inc uint32", "uint32", 4, None),
                                         ("fetch_add uint64", "uint64", 8, 0x100000001)):
                if pe == 0:
                    set_word(ctr, 0)
                ish.ishmem_barrier_all()
                vals = []
                for _ in range(64):
                    rc, f = ish.atomic_fetch_inc(ctr, dt, 0) if step is None else ish.atomic_fetch_add(ctr, dt, step, 0)
                    if rc:
                        fails.append(f"pe{pe} contended {tag}: {ish.last_error()}")
                    vals.append(f)
                s = step or 1
                gather_check(f"contended {tag}", vals, [k * s for k in range(64 * npes)], ctr, dt, 64 * npes * s)
            # compare_swap increment loop: a failed attempt means somebody else succeeded.
            if pe == 0:
                set_word(ctr, 0)
            ish.ishmem_barrier_all()
            vals = []
            for i in range(16):
                rc, cur = ish.atomic_fetch(ctr, "int64", 0)
                for attempt in range(4096):
                    rc2, f = ish.atomic_compare_swap(ctr, "int64", cur, cur + 1, 0)
                    if rc or rc2:
                        fails.append(f"pe{pe} contended compare_swap: {ish.last_error()}")
                        break
                    if f == cur:
                        vals.append(cur)
                        break
                    cur = f
                else:
                    fails.append(f"pe{pe} contended compare_swap: increment {i} used up its 4096 attempts")
            vals += [1 << 63] * (16 - len(vals))  # a failed increment shows in the check
            gather_check("contended compare_swap", vals, list(range(16 * npes)), ctr, "int64", 16 * npes)

        if "nbi" in scenarios:
            N = 32
            fdev = hip.malloc(N * 8)
            fpin = hip.host_malloc(N * 8)
            sentinel = 0x5EA15EA15EA15EA1
            for kind, fbuf in (("heap", fheap), ("device", fdev), ("pinned", fpin)):
                for dt, width in (("uint32", 4), ("int64", 8)):
                    m = (1 << 8 * width) - 1
                    for op in FETCHING:
                        old0 = OPERANDS[width][2][0]
                        prepare(width, old0, nxt)
                        hip.upload(fbuf, np.full(N, sentinel, dtype="<u8"))
                        cur, want = old0, []
                        for i in range(N):
                            value = (OPERANDS[width][1][1] * (i + 1) + i) & m
                            cond = cur if i % 2 == 0 else cur ^ (1 << (8 * width - 1))  # hit, then a miss in the high half
                            rc = getattr(ish, f"atomic_{op}_nbi")(fbuf + i * width, mine + word_at(width), dt,
                                                                  *call_args(op, value, cond), nxt)
                            if rc:
                                fails.append(f"pe{pe} nbi {op} {dt} {kind}: {ish.last_error()}")
                            cur, f = amo_model(op, width, cur, value, cond)
                            want.append(f)
                        ish.ishmem_quiet()
                        got = hip.download(fbuf, N * width // 8, np.uint64).view(np_t(width))
                        if [int(x) for x in got] != want:
                            fails.append(f"pe{pe} nbi {op} {dt} {kind}: fetched values differ from the model's after quiet")
                        rest = hip.download(fbuf + N * width, N - N * width // 8, np.uint64) if width == 4 else []
                        if any(int(x) != sentinel for x in rest):
                            fails.append(f"pe{pe} nbi {op} {dt} {kind}: wrote past the {N} fetch words")
                        check(f"nbi {op} {dt} {kind}", width, cur, nxt)
            # a pageable fetch is refused and changes nothing
            page = np.full(1, sentinel, dtype="<u8")
            prepare(8, 77, nxt)
            rc = ish.atomic_fetch_add_nbi(page.ctypes.data, mine + word_at(8), "uint64", 5, nxt)
            if rc == 0 or "not device-accessible" not in ish.last_error():
                fails.append(f"pe{pe} nbi pageable fetch: not refused ('{ish.last_error()}')")
            ish.ishmem_quiet()
            check("nbi pageable fetch", 8, 77, nxt)
            if int(page[0]) != sentinel:
                fails.append(f"pe{pe} nbi pageable fetch: the fetch word changed")
            hip.host_free(fpin)
            hip.free(fdev)
            ish.ishmem_barrier_all()

        if "ordering" in scenarios:
            # In round r the origin fills its source with a pattern of r, issues the put, ishmem_fence,
            # then one AMO on the target's flag.  The target warms its caches with dest's old lines from
            # 16 workgroups, waits for the flag on the host, and 16 workgroups then read dest with plain
            # loads: each must see round r in every word.  No barrier between the put and the check.
            G, MAXB = 16, 1 << 20
            sbuf = ish.ishmem_align(256, MAXB)
            dbuf = ish.ishmem_align(256, MAXB + 64)
            for form in ("put_nbi fence atomic_add", "put atomic_set"):
                for B in (4096, MAXB):
                    n = B // 4
                    out = hip.malloc(G * B)
                    flag = dbuf + B  # directly after dest
                    hip.upload(dbuf, np.zeros(B + 64, np.uint8))
                    ish.ishmem_barrier_all()
                    for r in range(1, 5):
                        hip.upload(sbuf, round_pattern(r, pe, n))
                        if L.ishmemi_c_read_all_u32(out, dbuf, n, G, None):
                            fails.append(f"pe{pe} ordering warm: {ish.last_error()}")
                        hip.synchronize()
                        if form.startswith("put_nbi"):
                            rc = ish.ishmem_putmem_nbi(dbuf, sbuf, B, nxt)
                            ish.ishmem_fence()
                            rc = rc or ish.atomic_add(flag, "uint64", 1, nxt)[0]
                        else:
                            rc = ish.ishmem_putmem(dbuf, sbuf, B, nxt)
                            rc = rc or ish.atomic_set(flag, "uint64", r, nxt)[0]
                        if rc:
                            fails.append(f"pe{pe} ordering {form}: {ish.last_error()}")
                        rc, v = ish.wait_until(flag, "uint64", GE, r)
                        if rc or v != r:
                            fails.append(f"pe{pe} ordering {form} B={B} round {r}: wait rc={rc} value {v}: {ish.last_error()}")
                        L.ishmemi_c_read_all_u32(out, dbuf, n, G, None)
                        got = hip.download(out, G * n, np.uint32).reshape(G, n)
                        want = round_pattern(r, prv, n)
                        stale = [b for b in range(G) if not np.array_equal(got[b], want)]
                        if stale:
                            fails.append(f"pe{pe} ordering {form} B={B} round {r}: workgroups {stale} read "
                                         f"{int(np.count_nonzero(got != want[None, :]))} words that are not round {r}'s")
                        ish.ishmem_quiet()     # this PE's own put is complete before its source is refilled
                        ish.ishmem_sync_all()  # round r + 1 must not overwrite a dest that is still being checked
                    hip.free(out)
                    ish.ishmem_barrier_all()
            ish.ishmem_free(dbuf)
            ish.ishmem_free(sbuf)

        if "fanin" in scenarios:
            ctr = shared + 8
            for dt, width in (("int32", 4), ("uint64", 8)):
                if pe == 0:
                    set_word(ctr, 0)
                ish.ishmem_barrier_all()
                if pe != 0 and ish.atomic_inc(ctr, dt, 0)[0]:
                    fails.append(f"pe{pe} fanin inc: {ish.last_error()}")
                if pe == 0:
                    rc, v = ish.wait_until(ctr, dt, GE, npes - 1)
                    rc2, f = ish.atomic_fetch(ctr, dt, 0)
                    if rc or rc2 or v != npes - 1 or f != npes - 1:
                        fails.append(f"pe0 fanin {dt}: wait rc={rc} value {v}, fetch rc={rc2} {f}, want {npes - 1}")
                ish.ishmem_barrier_all()

        if "threads" in scenarios:
            prepare(8, 0, nxt)
            got: list[list[int]] = [[], []]
            terr: list[str] = []

            def body(k):
                for _ in range(64):
                    rc, f = ish.atomic_fetch_add(mine + word_at(8), "int64", 1, nxt)
                    if rc:
                        terr.append(ish.last_error())
                    got[k].append(f)

            ths = [threading.Thread(target=body, args=(k,)) for k in range(2)]
            for t in ths:
                t.start()
            for t in ths:
                t.join()
            if terr or sorted(got[0] + got[1]) != list(range(128)):
                fails.append(f"pe{pe} threads: the 128 fetched values are not 0 .. 127 each once {terr[:1]}")
            check("threads", 8, 128, nxt)
            ish.ishmem_barrier_all()

        if "argfail" in scenarios:
            plain = hip.malloc(64)
            errs0 = L.ishmemi_c_error_count()
            prepare(8, 0x1111, nxt)
            w = mine + word_at(8)
            AMO = ish.AMO_OPS
            cases = [
                ("pe -1", lambda: ish.atomic_fetch_add(w, "int64", 1, -1)[0], "outside [0"),
                ("pe npes", lambda: ish.atomic_set(w, "int64", 1, npes)[0], "outside [0"),
                ("nbi pe npes", lambda: ish.atomic_swap_nbi(fheap, w, "int64", 1, npes), "outside [0"),
                ("op 14", lambda: ish.amo(14, "int64", w, 1, 0, nxt)[0], "op 14"),
                ("op -1", lambda: ish.amo(-1, "int64", w, 1, 0, nxt)[0], "op -1"),
                ("nbi op 99", lambda: ish.amo_nbi(99, "int64", fheap, w, 1, 0, nxt), "op 99"),
                ("nbi set", lambda: ish.amo_nbi(AMO["set"], "int64", fheap, w, 1, 0, nxt), "_nbi form"),
                ("nbi add", lambda: ish.amo_nbi(AMO["add"], "int64", fheap, w, 1, 0, nxt), "_nbi form"),
                ("nbi inc", lambda: ish.amo_nbi(AMO["inc"], "int64", fheap, w, 1, 0, nxt), "_nbi form"),
                ("nbi xor", lambda: ish.amo_nbi(AMO["xor"], "int64", fheap, w, 1, 0, nxt), "_nbi form"),
                ("float fetch_add", lambda: ish.atomic_fetch_add(w, "float", 1, nxt)[0], "float and double"),
                ("double compare_swap", lambda: ish.atomic_compare_swap(w, "double", 1, 2, nxt)[0], "float and double"),
                ("float xor", lambda: ish.atomic_xor(w, "float", 1, nxt)[0], "float and double"),
                ("double fetch_inc_nbi", lambda: ish.atomic_fetch_inc_nbi(fheap, w, "double", nxt), "float and double"),
                ("int8", lambda: ish.atomic_fetch(w, "int8", nxt)[0], "dtype"),
                ("uint16", lambda: ish.atomic_add(w, "uint16", 1, nxt)[0], "dtype"),
                ("dtype name", lambda: ish.atomic_add(w, "no such type", 1, nxt)[0], "dtype"),
                ("null dest", lambda: ish.atomic_inc(0, "int64", nxt)[0], "dest is null"),
                ("64-bit op on a 4-byte phase", lambda: ish.atomic_fetch_or(w + 4, "uint64", 1, nxt)[0], "8-byte aligned"),
                ("32-bit op misaligned", lambda: ish.atomic_fetch_or(w + 2, "uint32", 1, nxt)[0], "4-byte aligned"),
                ("dest outside the heap", lambda: ish.atomic_swap(plain, "int64", 1, nxt)[0], "not inside the symmetric heap"),
                ("null fetch", lambda: ish.atomic_fetch_add_nbi(0, w, "int64", 1, nxt), "fetch is null"),
                ("misaligned fetch", lambda: ish.atomic_fetch_add_nbi(fheap + 4, w, "int64", 1, nxt), "fetch is not aligned"),
            ]
            for tag, call, word in cases:
                rc = call()
                if rc == 0:
                    fails.append(f"pe{pe} argfail {tag}: returned 0")
                elif word not in ish.last_error():
                    fails.append(f"pe{pe} argfail {tag}: message '{ish.last_error()}' lacks '{word}'")
            if L.ishmemi_c_error_count() != errs0:
                fails.append(f"pe{pe} argfail: error count moved")
            ish.ishmem_quiet()
            check("argfail", 8, 0x1111, nxt)
            hip.free(plain)
            rc, f = ish.atomic_fetch_add(w, "int64", 1, nxt)  # the library works afterwards
            if rc or f != 0x1111:
                fails.append(f"pe{pe} after argfail: rc={rc} fetched {f:#x}")
            ish.ishmem_barrier_all()

        ish.ishmem_barrier_all()
        if L.ishmemi_c_error_count() != 0:
            fails.append(f"pe{pe}: device error count {L.ishmemi_c_error_count()}")
        for b in (fheap, gath, shared, lines):
            ish.ishmem_free(b)
        ish.ishmem_finalize()
    except Exception:
        fails.append(f"pe{pe} exception:\n{traceback.format_exc()}")
    q.put((pe, fails))

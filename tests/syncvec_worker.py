"""Worker body of the multi-PE GPU tests of the vector waits and tests (tests/test_gpu_syncvec.py): one
process = one PE, all PEs on one GPU, as tests/signal_worker.py.  Every PE writes to (me + 1) % p, so
with one PE it writes to itself.  The expectations come from the model in tests/syncvec_cases.py; the
`any` rotor is per PE and starts at 0 in a fresh process, and the worker follows it through every
call.  Failures are returned as strings through the queue.
"""
from __future__ import annotations

import os
import threading
import time
import traceback

import numpy as np

from tests.signal_worker import CMP_NAMES, EQ, GT, NE, SET, SYNC_TYPES, round_pattern
from tests.syncvec_cases import CHUNK, OPS, SIZE_MAX, case_values, model, size_cases, status_array, type_cases

GUARD_IDX = 0xDEADBEEFCAFEF00D  # indices entries the call must not write
MAXN = CHUNK + 64


def run(pe: int, npes: int, key: str, scenarios: list[str], q, env: dict | None = None, hb=None) -> None:
    fails: list[str] = []
    try:
        for k, v in (env or {}).items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v[pe] if isinstance(v, list) else v)
        import ishmem_amd as ish
        from ishmem_amd import hip

        ish.init(pe, npes, 0, key)
        L = ish.lib()
        nxt, prv = (pe + 1) % npes, (pe - 1) % npes
        # ivars sit 64 bytes into `arena`, between words of 0x5A
        arena = ish.ishmem_align(256, 64 + MAXN * 8 + 64)
        ivars = arena + 64
        words = ish.ishmem_align(256, 256)  # marker signal, *ret, *result
        marker, retw, resw = words, words + 8, words + 16
        dev_status, dev_cv, dev_idx = hip.malloc(MAXN * 4), hip.malloc(MAXN * 8), hip.malloc((MAXN + 4) * 8)
        rotor = [0]
        expected_errors = 0

        def fail(msg):
            fails.append(f"pe{pe} {msg}")

        def set_ivars(values, bits):
            """The whole arena: 0x5A bytes around the variables."""
            dt = "<u4" if bits == 32 else "<u8"
            body = np.array([v & ((1 << bits) - 1) for v in values], dtype=dt).view(np.uint8)
            buf = np.full(64 + MAXN * 8 + 64, 0x5A, np.uint8)
            buf[64:64 + len(body)] = body
            hip.upload(arena, buf)

        def put_elems(first, vals, bits, to):
            """Blocking put of consecutive elements from a host array (the pageable path)."""
            a = np.array([v & ((1 << bits) - 1) for v in vals], dtype="<u4" if bits == 32 else "<u8")
            if ish.ishmem_putmem(ivars + first * (bits // 8), a.ctypes.data, a.nbytes, to):
                fail(f"put: {ish.last_error()}")

        class Side:
            """status / cmp_values / indices of one call, in pageable host memory or in device memory."""

            def __init__(self, n, status, cvs, bits, where):
                self.n, self.where = n, where
                self.h_status = np.array(status, dtype=np.int32) if status is not None else None
                self.h_cv = np.array(cvs, dtype="<u4" if bits == 32 else "<u8") if cvs is not None else None
                self.h_idx = np.full(n + 4, GUARD_IDX, dtype=np.uint64)
                if where == "device":
                    if status is not None and n:
                        hip.upload(dev_status, self.h_status)
                    if cvs is not None and n:
                        hip.upload(dev_cv, self.h_cv)
                    hip.upload(dev_idx, self.h_idx)

            def status(self):
                return 0 if self.h_status is None else (dev_status if self.where == "device" else self.h_status.ctypes.data)

            def cv(self):
                return 0 if self.h_cv is None else (dev_cv if self.where == "device" else self.h_cv.ctypes.data)

            def idx(self):
                return dev_idx if self.where == "device" else self.h_idx.ctypes.data

            def indices(self):
                return hip.download(dev_idx, self.n + 4, np.uint64) if self.where == "device" else self.h_idx

        def one_shot(tag, tn, bits, signed, cmp, n, sk, vector, seed, where):
            values, cv = case_values(n, bits, signed, cmp, seed, vector)
            status = status_array(sk, n, seed)
            set_ivars(values, bits)
            for op in OPS:
                want = model(op, values, status, cmp, cv, bits, signed, rotor[0])
                if want.blocks:
                    continue  # the snapshot would make this wait block; its test form runs
                side = Side(n, status, cv if vector else None, bits, where)
                name = f"ishmem_{tn}_{op}{'_vector' if vector else ''}"
                fn = getattr(ish, name)
                c = side.cv() if vector else cv
                errs = L.ishmemi_c_error_count()
                got = fn(ivars, n, side.idx(), side.status(), cmp, c) if op.endswith("some") else fn(ivars, n, side.status(), cmp, c)
                if op == "wait_until_all":
                    got = 1 if got == 0 else 0  # the name returns the status
                where_tag = f"{tag} {name} {CMP_NAMES[cmp]} n={n} status={sk} arrays={where}"
                if got != want.result:
                    fail(f"{where_tag}: returned {got}, want {want.result} ({ish.last_error()})")
                if op.endswith("some"):
                    idx = side.indices()
                    if list(idx[:want.result]) != want.indices or not np.all(idx[want.result:] == GUARD_IDX):
                        fail(f"{where_tag}: indices {list(idx[:8])}... want {want.indices[:8]}... and guards behind them")
                if L.ishmemi_c_error_count() != errs:
                    fail(f"{where_tag}: error count moved")
                rotor[0] = want.rotor

        if "types" in scenarios:
            for k, (tn, bits, signed, cmp, n, sk, vector, seed) in enumerate(type_cases()):
                one_shot("types", tn, bits, signed, cmp, n, sk, vector, seed, "device" if k % 2 else "host")

        if "sizes" in scenarios:
            for k, (tn, bits, signed, cmp, n, sk, vector, seed) in enumerate(size_cases()):
                for where in ("host", "device"):
                    one_shot("sizes", tn, bits, signed, cmp, n, sk, vector, seed + (where == "device"), where)
            # the C ABI itself: nelems == 0 with null arrays, and a result pointer of null
            for mode, want in ((0, 1), (1, SIZE_MAX), (2, 0), (3, 1), (4, SIZE_MAX), (5, 0)):
                if ish.sync_vector(mode, "int32", 0, 0, 0, 0, EQ, 1) != (0, want):
                    fail(f"empty mode {mode}: {ish.sync_vector(mode, 'int32', 0, 0, 0, 0, EQ, 1)} {ish.last_error()}")
            if L.ishmemi_c_sync_vector(3, ish.DTYPES["int32"], ivars, 4, None, None, EQ, 1, None, None):
                fail(f"null result pointer: {ish.last_error()}")

        def marker_reset():
            hip.upload(words, np.zeros(4, dtype="<u8"))
            hip.memset(retw, 0xFF, 4)

        def marker_value():
            return int(hip.download(marker, 1, np.uint64)[0])

        def host_sync():
            hb.wait(60)

        # An on-stream wait occupies its stream, and HIP may place other streams of the same process on
        # its hardware queue, so what such a wait waits for is written by ANOTHER process:
        # one PE at a time waits on a stream, its predecessor writes, and the PEs meet at a host-side
        # barrier (no GPU work of the waiter's while its wait is pending).  With one PE there is no other
        # process; the blocking forms, which are time-sliced, run at every PE count.
        turns = [(w, (w - 1) % npes) for w in range(npes)] if npes > 1 else []

        if "all" in scenarios:
            # wait_until_all must not return while one element of the wait set is unsatisfied.
            st = hip.stream_create()
            for n, bits, tn in ((65, 32, "int32"), (CHUNK + 1, 64, "uint64")):
                excluded = [3, n - 2]
                last = n - 1  # past the first wave / in the second chunk
                status = [1 if i in excluded else 0 for i in range(n)]
                np_dt = np.uint32 if bits == 32 else np.uint64

                def reset():
                    set_ivars([0] * n, bits)
                    marker_reset()
                    hip.upload(dev_status, np.array(status, dtype=np.int32))
                    ish.ishmem_barrier_all()

                def put_all_but_last(to):
                    put_elems(0, [7] * 3, bits, to)
                    put_elems(4, [7] * (n - 2 - 4), bits, to)

                def check_excluded(tag):
                    got = hip.download(ivars, n, np_dt)
                    if any(int(got[i]) != 0 for i in excluded):
                        fail(f"{tag}: an excluded element was written")

                # blocking, in a second host thread of every PE
                tag = f"all blocking n={n}"
                reset()
                result: list = []
                th = threading.Thread(target=lambda: result.append(
                    ish.sync_vector("wait_until_all", tn, ivars, n, 0, dev_status, GT, 6)))
                th.start()
                put_all_but_last(nxt)
                ish.ishmem_barrier_all()  # this PE's predecessor has put too
                th.join(0.05)
                if not th.is_alive():
                    fail(f"{tag}: returned {result} before the last element was written")
                ish.ishmem_barrier_all()  # every PE has looked
                put_elems(last, [7], bits, nxt)
                th.join(15)
                if th.is_alive() or result != [(0, 1)]:
                    fail(f"{tag}: returned {result} ({ish.last_error()})")
                check_excluded(tag)
                ish.ishmem_barrier_all()
                # on a stream, followed by a marker write
                for w, wr in turns:
                    tag = f"all on_stream n={n}"
                    reset()
                    if pe == w:
                        rc = ish.sync_vector_on_stream("wait_until_all", tn, ivars, n, 0, dev_status, GT, 6, 0, 0, retw, st)
                        rc = rc or ish.put_signal_on_stream(0, 0, 0, marker, 1, SET, pe, st)  # the marker behind the wait
                        if rc:
                            fail(f"{tag}: enqueue: {ish.last_error()}")
                    host_sync()
                    if pe == wr:
                        put_all_but_last(w)
                    host_sync()
                    if pe == w and hip.stream_query(st):
                        fail(f"{tag}: the stream got past the wait before the last element was written")
                    host_sync()
                    if pe == wr:
                        put_elems(last, [7], bits, w)
                    if pe == w:
                        hip.stream_synchronize(st)
                        if int(hip.download(retw, 1, np.int32)[0]) != 0 or marker_value() != 1:
                            fail(f"{tag}: *ret {hip.download(retw, 1, np.int32)[0]}, marker {marker_value()}")
                        check_excluded(tag)
                    ish.ishmem_barrier_all()
                # on a stream with the wait set already satisfied (every PE count)
                vals = [0 if i in excluded else 7 for i in range(n)]
                set_ivars(vals, bits)
                marker_reset()
                if ish.sync_vector_on_stream("wait_until_all", tn, ivars, n, 0, dev_status, GT, 6, 0, 0, retw, st) or \
                        ish.put_signal_on_stream(0, 0, 0, marker, 1, SET, pe, st):
                    fail(f"all on_stream satisfied n={n}: enqueue: {ish.last_error()}")
                hip.stream_synchronize(st)
                if int(hip.download(retw, 1, np.int32)[0]) != 0 or marker_value() != 1:
                    fail(f"all on_stream satisfied n={n}: *ret {hip.download(retw, 1, np.int32)[0]}, marker {marker_value()}")
                ish.ishmem_barrier_all()
            # An element that moves on after it satisfied EQ: seen once is enough.
            n = 65

            def flip_back(to, sync):
                put_elems(0, [1], 64, to)
                for _ in range(3):  # many polling passes (and slices of the blocking form) see element 0 == 1
                    sync()
                put_elems(0, [2], 64, to)
                put_elems(1, [1] * (n - 1), 64, to)

            set_ivars([0] * n, 64)
            ish.ishmem_barrier_all()
            result = []
            th = threading.Thread(target=lambda: result.append(ish.sync_vector("wait_until_all", "int64", ivars, n, 0, 0, EQ, 1)))
            th.start()
            flip_back(nxt, ish.ishmem_barrier_all)
            th.join(15)
            if th.is_alive() or result != [(0, 1)]:
                fail(f"all flips back blocking: returned {result} ({ish.last_error()})")
            ish.ishmem_barrier_all()
            for w, wr in turns:
                set_ivars([0] * n, 64)
                marker_reset()
                ish.ishmem_barrier_all()
                if pe == w and ish.sync_vector_on_stream("wait_until_all", "int64", ivars, n, 0, 0, EQ, 1, 0, 0, retw, st):
                    fail(f"all flips back on_stream: enqueue: {ish.last_error()}")
                host_sync()
                if pe == wr:
                    flip_back(w, hip.synchronize)
                if pe == w:
                    hip.stream_synchronize(st)
                    if int(hip.download(retw, 1, np.int32)[0]) != 0:
                        fail(f"all flips back on_stream: *ret {hip.download(retw, 1, np.int32)[0]}")
                ish.ishmem_barrier_all()
            hip.stream_destroy(st)

        if "anysome" in scenarios:
            n, bits, tn = CHUNK + 44, 64, "uint64"
            for k in (0, n - 1, n // 2, CHUNK):
                set_ivars([0] * n, bits)
                hip.upload(dev_idx, np.full(n + 4, GUARD_IDX, dtype=np.uint64))
                ish.ishmem_barrier_all()
                put_elems(k, [5], bits, nxt)
                got = ish.sync_vector("wait_until_any", tn, ivars, n, 0, 0, NE, 0)
                rotor[0] = k
                if got != (0, k):
                    fail(f"any k={k}: {got} ({ish.last_error()})")
                got = ish.sync_vector("wait_until_some", tn, ivars, n, dev_idx, 0, NE, 0)
                idx = hip.download(dev_idx, n + 4, np.uint64)
                if got != (0, 1) or int(idx[0]) != k or not np.all(idx[1:] == GUARD_IDX):
                    fail(f"some k={k}: {got}, indices {list(idx[:3])}")
                ish.ishmem_barrier_all()
            # k excluded and written: the call waits for j (blocking, in a second host thread)
            for op, k, j in (("wait_until_any", 7, CHUNK + 3), ("wait_until_some", CHUNK + 9, 2)):
                set_ivars([0] * n, bits)
                status = np.zeros(n, dtype=np.int32)
                status[k] = 1
                hip.upload(dev_status, status)
                hip.upload(dev_idx, np.full(n + 4, GUARD_IDX, dtype=np.uint64))
                ish.ishmem_barrier_all()
                result: list = []
                th = threading.Thread(target=lambda: result.append(ish.sync_vector(op, tn, ivars, n, dev_idx, dev_status, EQ, 5)))
                th.start()
                put_elems(k, [5], bits, nxt)
                ish.ishmem_barrier_all()
                th.join(0.05)
                if not th.is_alive():
                    fail(f"{op}: returned {result} for the excluded element {k}")
                ish.ishmem_barrier_all()
                put_elems(j, [5], bits, nxt)
                th.join(15)
                if op == "wait_until_any":
                    rotor[0] = j
                    if th.is_alive() or result != [(0, j)]:
                        fail(f"any excluded: {result}, want {j} ({ish.last_error()})")
                else:
                    idx = hip.download(dev_idx, n + 4, np.uint64)
                    if th.is_alive() or result != [(0, 1)] or int(idx[0]) != j or not np.all(idx[1:] == GUARD_IDX):
                        fail(f"some excluded: {result} indices {list(idx[:3])}, want [{j}] ({ish.last_error()})")
                ish.ishmem_barrier_all()
            # Fairness: with every element satisfied, consecutive any calls visit each non-excluded one once.
            for N in (5, CHUNK + 44):
                set_ivars([9] * N, bits)
                excl = {1, N - 2}
                status = np.array([1 if i in excl else 0 for i in range(N)], dtype=np.int32)
                seen = []
                for c in range(N - len(excl)):
                    op = "wait_until_any" if c % 2 == 0 else "test_any"
                    rc, r = ish.sync_vector(op, tn, ivars, N, 0, status.ctypes.data, EQ, 9)
                    want = model(op, [9] * N, list(status), EQ, 9, bits, False, rotor[0])
                    if rc or r != want.result:
                        fail(f"fairness N={N} call {c}: {(rc, r)}, the model says {want.result}")
                    rotor[0] = want.rotor
                    seen.append(r)
                if sorted(seen) != [i for i in range(N) if i not in excl]:
                    fail(f"fairness N={N}: {len(set(seen))} distinct indices in {len(seen)} calls")
            ish.ishmem_barrier_all()

        if "graph" in scenarios:
            # One captured consumer step, wait_until_some_on_stream + a kernel that copies what it
            # reported; replayed with other elements written and other status contents each time.
            n, bits, tn = 8, 64, "uint64"
            st = hip.stream_create()
            # symmetric memory: classified without a HIP call while the capture is open
            garr = ish.ishmem_align(256, 1024)
            g_status, g_idx, snap = garr, garr + 256, garr + 512
            set_ivars([0] * n, bits)
            hip.upload(g_status, np.zeros(n, dtype=np.int32))
            hip.upload(g_idx, np.full(n + 4, GUARD_IDX, dtype=np.uint64))
            ish.ishmem_barrier_all()
            with hip.Graph(st) as g:
                r = ish.sync_vector_on_stream("wait_until_some", tn, ivars, n, g_idx, g_status, NE, 0, 0, resw, retw, st)
                r = r or L.ishmemi_c_read_all_u32(snap, g_idx, 2 * n, 1, st)
                if r:
                    fail(f"graph capture: {ish.last_error()}")

            def replay_result():
                hip.stream_synchronize(st)
                cnt, ret = int(hip.download(resw, 1, np.uint64)[0]), int(hip.download(retw, 1, np.int32)[0])
                return cnt, ret, [int(x) for x in hip.download(snap, n, np.uint64)[:min(cnt, n)]]

            # replay 1: elements 1 and 5 are there before the launch
            put_elems(1, [3], bits, nxt)
            put_elems(5, [3], bits, nxt)
            ish.ishmem_barrier_all()
            hip.memset(retw, 0xFF, 4)
            g.launch()
            if replay_result() != (2, 0, [1, 5]):
                fail(f"graph replay 1: {replay_result()}")
            # the consumer marks them: the replay reads the new contents of status and finds nothing left
            # to wait for but element 6, which only the writer of this turn supplies
            status = np.zeros(n, dtype=np.int32)
            status[[1, 5]] = 1
            hip.upload(g_status, status)
            ish.ishmem_barrier_all()
            if npes == 1:
                put_elems(6, [4], bits, nxt)  # one PE: written before the launch
                hip.memset(retw, 0xFF, 4)
                g.launch()
                if replay_result() != (1, 0, [6]):
                    fail(f"graph replay 2: {replay_result()}")
            for w, wr in turns:
                if pe == w:
                    hip.memset(retw, 0xFF, 4)
                    g.launch()
                host_sync()
                if pe == w and hip.stream_query(st):
                    fail("graph replay 2: returned for elements its status excludes")
                host_sync()
                if pe == wr:
                    put_elems(6, [4], bits, w)
                if pe == w and replay_result() != (1, 0, [6]):
                    fail(f"graph replay 2: {replay_result()}")
                ish.ishmem_barrier_all()
            del g
            hip.stream_destroy(st)
            ish.ishmem_free(garr)
            ish.ishmem_barrier_all()

        if "payload" in scenarios:
            # Every PE puts a payload with a signal into its own slot on EVERY PE; the target learns of
            # them through the vector wait alone, and a kernel launched then must see every payload.
            B, G = 16384, 4
            nw = B // 4
            slots = ish.ishmem_align(256, npes * B)
            sigs = ish.ishmem_align(256, npes * 8)
            sbuf = ish.ishmem_align(256, B)
            out = hip.malloc(G * npes * B)
            hip.upload(sigs, np.zeros(npes, dtype="<u8"))
            hip.upload(slots, np.full(npes * B, 0xA5, np.uint8))
            ish.ishmem_barrier_all()
            for r, form in ((1, "all"), (2, "some"), (3, "any")):
                hip.upload(sbuf, round_pattern(r, pe, nw))
                L.ishmemi_c_read_all_u32(out, slots, npes * nw, G, None)  # warm, stale lines
                hip.synchronize()
                ish.ishmem_barrier_all()  # nobody overwrites a slot that is still being checked
                for t in range(npes):
                    if ish.ishmem_putmem_signal(slots + pe * B, sbuf, B, sigs + pe * 8, r, SET, (pe + 1 + t) % npes):
                        fail(f"payload put_signal: {ish.last_error()}")
                arrived: list[int] = []
                if form == "all":
                    if ish.sync_vector("wait_until_all", "uint64", sigs, npes, 0, 0, EQ, r) != (0, 1):
                        fail(f"payload wait_until_all: {ish.last_error()}")
                    arrived = list(range(npes))
                else:
                    status = np.zeros(npes, dtype=np.int32)
                    idx = np.zeros(npes, dtype=np.uint64)
                    while len(arrived) < npes:
                        if form == "some":
                            rc, cnt = ish.sync_vector("wait_until_some", "uint64", sigs, npes, idx.ctypes.data, status.ctypes.data, EQ, r)
                            new = [int(x) for x in idx[:cnt]]
                        else:
                            rc, w = ish.sync_vector("wait_until_any", "uint64", sigs, npes, 0, status.ctypes.data, EQ, r)
                            new = [w]
                            rotor[0] = w if rc == 0 and w != SIZE_MAX else rotor[0]
                        if rc or not new or any(status[i] for i in new if i < npes) or max(new) >= npes:
                            fail(f"payload {form}: rc={rc} new={new} status={list(status)} ({ish.last_error()})")
                            break
                        # a kernel launched now sees the payloads these signals announce
                        L.ishmemi_c_read_all_u32(out, slots, npes * nw, G, None)
                        got = hip.download(out, G * npes * nw, np.uint32).reshape(G, npes, nw)
                        for i in new:
                            if not all(np.array_equal(got[b, i], round_pattern(r, i, nw)) for b in range(G)):
                                fail(f"payload {form} round {r}: origin {i}'s payload is stale after its signal")
                            status[i] = 1
                        arrived += new
                if form == "all":
                    L.ishmemi_c_read_all_u32(out, slots, npes * nw, G, None)
                    got = hip.download(out, G * npes * nw, np.uint32).reshape(G, npes, nw)
                    for i in range(npes):
                        if not all(np.array_equal(got[b, i], round_pattern(r, i, nw)) for b in range(G)):
                            fail(f"payload all round {r}: origin {i}'s payload is stale after wait_until_all")
                ish.ishmem_barrier_all()
            hip.free(out)
            for b in (sbuf, sigs, slots):
                ish.ishmem_free(b)

        if "argfail" in scenarios:
            import ctypes
            plain = hip.malloc(4096)
            base, size, used = ctypes.c_void_p(), ctypes.c_size_t(), ctypes.c_size_t()
            L.ishmemi_c_heap_info(ctypes.byref(base), ctypes.byref(size), ctypes.byref(used))
            heap_end = base.value + size.value
            errs0 = L.ishmemi_c_error_count()
            set_ivars([1] * 8, 64)
            hip.upload(dev_idx, np.full(MAXN + 4, GUARD_IDX, dtype=np.uint64))
            page = np.zeros(16, dtype=np.int64)
            V = ish.SYNC_VECTOR_FLAG
            sv, svs = ish.sync_vector, ish.sync_vector_on_stream
            cases = [
                ("mode 6", lambda: sv(6, "int64", ivars, 4, 0, 0, EQ, 1)[0], "mode"),
                ("mode -1", lambda: sv(-1, "int64", ivars, 4, 0, 0, EQ, 1)[0], "mode"),
                ("dtype float", lambda: sv("test_all", "float", ivars, 4, 0, 0, EQ, 1)[0], "dtype"),
                ("dtype int16", lambda: sv("wait_until_any", "int16", ivars, 4, 0, 0, EQ, 1)[0], "dtype"),
                ("cmp 0", lambda: sv("wait_until_all", "int64", ivars, 4, 0, 0, 0, 1)[0], "cmp"),
                ("cmp 7", lambda: sv("test_some", "int64", ivars, 4, dev_idx, 0, 7, 1)[0], "cmp"),
                ("ivars null", lambda: sv("test_any", "int64", 0, 4, 0, 0, EQ, 1)[0], "ivars is null"),
                ("ivars misaligned", lambda: sv("test_all", "int64", ivars + 4, 4, 0, 0, EQ, 1)[0], "8-byte aligned"),
                ("ivars misaligned 32", lambda: sv("test_all", "uint32", ivars + 2, 4, 0, 0, EQ, 1)[0], "4-byte aligned"),
                ("ivars outside", lambda: sv("test_all", "int64", plain, 4, 0, 0, EQ, 1)[0], "not inside the symmetric heap"),
                ("ivars runs past", lambda: sv("test_all", "int64", heap_end - 16, 3, 0, 0, EQ, 1)[0], "not inside the symmetric heap"),
                ("ivars wraps", lambda: sv("test_all", "int64", ivars, (1 << 62), 0, 0, EQ, 1)[0], "not inside the symmetric heap"),
                ("some without indices", lambda: sv("wait_until_some", "int64", ivars, 4, 0, 0, EQ, 1)[0], "indices is null"),
                ("test_some without indices", lambda: sv("test_some", "int64", ivars, 4, 0, 0, EQ, 1)[0], "indices is null"),
                ("vector without cmp_values", lambda: sv(0 | V, "int64", ivars, 4, 0, 0, EQ, 1)[0], "cmp_values is null"),
                ("name without cmp_values", lambda: 0 if ish.ishmem_long_test_any_vector(ivars, 4, 0, EQ, 0) != SIZE_MAX else 1,
                 "cmp_values is null"),
                ("on_stream test mode", lambda: svs("test_all", "int64", ivars, 4, 0, 0, EQ, 1, 0, 0, 0, 0), "no on-stream form"),
                ("on_stream cmp", lambda: svs("wait_until_all", "int64", ivars, 4, 0, 0, 9, 1, 0, 0, 0, 0), "cmp"),
                ("on_stream ivars", lambda: svs("wait_until_any", "int64", plain, 4, 0, 0, EQ, 1, 0, 0, 0, 0), "not inside"),
                ("on_stream indices", lambda: svs("wait_until_some", "int64", ivars, 4, 0, 0, EQ, 1, 0, 0, 0, 0), "indices is null"),
                ("on_stream vector", lambda: svs(1 | V, "int64", ivars, 4, 0, 0, EQ, 1, 0, 0, 0, 0), "cmp_values is null"),
                ("on_stream pageable status", lambda: svs("wait_until_all", "int64", ivars, 4, 0, page.ctypes.data, EQ, 1, 0, 0, 0, 0),
                 "status is not device-accessible"),
                ("on_stream pageable cmp_values", lambda: svs("wait_until_all", "int64", ivars, 4, 0, 0, EQ, 0, page.ctypes.data, 0, 0, 0),
                 "cmp_values is not device-accessible"),
                ("on_stream pageable indices", lambda: svs("wait_until_some", "int64", ivars, 4, page.ctypes.data, 0, EQ, 1, 0, 0, 0, 0),
                 "indices is not device-accessible"),
                ("on_stream pageable result", lambda: svs("wait_until_any", "int64", ivars, 4, 0, 0, EQ, 1, 0, page.ctypes.data, 0, 0),
                 "result is not device-accessible"),
            ]
            for tag, call, word in cases:
                rc = call()
                if rc == 0:
                    fail(f"argfail {tag}: returned 0")
                elif word not in ish.last_error():
                    fail(f"argfail {tag}: message '{ish.last_error()}' lacks '{word}'")
            if L.ishmemi_c_error_count() != errs0:
                fail("argfail: error count moved")
            hip.synchronize()
            if not np.all(hip.download(dev_idx, MAXN + 4, np.uint64) == GUARD_IDX):
                fail("argfail: a refused call wrote indices")
            # the library still works, and the refused any calls did not move the rotor
            want = model("test_any", [1] * 8, None, EQ, 1, 64, True, rotor[0])
            if sv("test_any", "int64", ivars, 8, 0, 0, EQ, 1) != (0, want.result):
                fail(f"argfail: test_any afterwards, want {want.result}: {ish.last_error()}")
            rotor[0] = want.rotor
            hip.free(plain)
            ish.ishmem_barrier_all()

        if "bounded" in scenarios:
            # Runs with ISHMEM_TIMEOUT_MS=300: waits on words nobody writes return with an error.
            n = CHUNK + 1
            set_ivars([3] * n, 64)
            hip.upload(dev_idx, np.full(n + 4, GUARD_IDX, dtype=np.uint64))
            errs0 = L.ishmemi_c_error_count()
            for c, (op, want) in enumerate((("wait_until_all", 0), ("wait_until_any", SIZE_MAX), ("wait_until_some", 0))):
                t0 = time.monotonic()
                rc, r = ish.sync_vector(op, "int64", ivars, n, dev_idx, 0, EQ, 99)
                dt = time.monotonic() - t0
                if rc == 0 or "timed out" not in ish.last_error() or r != want or dt > 5.0 or dt < 0.25:
                    fail(f"bounded host {op}: rc={rc} result {r} after {dt:.2f} s: '{ish.last_error()}'")
                if L.ishmemi_c_error_count() != errs0 + c + 1:
                    fail(f"bounded host {op}: error count {L.ishmemi_c_error_count()} != {errs0 + c + 1}")
            # tests of the same words are no errors
            if ish.sync_vector("test_all", "int64", ivars, n, 0, 0, EQ, 99) != (0, 0) or \
                    ish.sync_vector("test_any", "int64", ivars, n, 0, 0, EQ, 99) != (0, SIZE_MAX) or \
                    L.ishmemi_c_error_count() != errs0 + 3:
                fail(f"bounded: a test that found nothing counted as an error ({ish.last_error()})")
            st = hip.stream_create()
            for op in ("wait_until_all", "wait_until_any", "wait_until_some"):
                hip.memset(retw, 0, 4)
                hip.upload(resw, np.array([12345], dtype="<u8"))
                t0 = time.monotonic()
                if ish.sync_vector_on_stream(op, "int64", ivars, n, dev_idx, 0, GT, 99, 0, resw, retw, st):
                    fail(f"bounded on_stream {op}: {ish.last_error()}")
                hip.stream_synchronize(st)
                dt = time.monotonic() - t0
                res = int(hip.download(resw, 1, np.uint64)[0])
                if int(hip.download(retw, 1, np.int32)[0]) == 0 or dt > 5.0 or res != (SIZE_MAX if op == "wait_until_any" else 0):
                    fail(f"bounded on_stream {op}: *ret {hip.download(retw, 1, np.int32)[0]} result {res} after {dt:.2f} s")
            if L.ishmemi_c_error_count() != errs0 + 4:  # the device-API error word counts once
                fail(f"bounded on_stream: error count {L.ishmemi_c_error_count()} != {errs0 + 4}")
            if not np.all(hip.download(dev_idx, n + 4, np.uint64) == GUARD_IDX):
                fail("bounded: a timed-out some wrote indices")
            hip.stream_destroy(st)
            expected_errors = 3  # the host waits'; resync clears the device's word
            ish.set_param("timeout_ms", 20000)
            if ish.resync() != 0:
                fail(f"resync failed: {ish.last_error()}")
            ish.ishmem_barrier_all()
            set_ivars([0], 64)
            ish.ishmem_barrier_all()
            put_elems(0, [77], 64, nxt)
            if ish.wait_until(ivars, "int64", EQ, 77) != (0, 77):
                fail(f"bounded: scalar wait afterwards: {ish.last_error()}")
            if ish.sync_vector("wait_until_all", "int64", ivars, 1, 0, 0, EQ, 77) != (0, 1):
                fail(f"bounded: wait_until_all afterwards: {ish.last_error()}")

        ish.ishmem_barrier_all()
        if L.ishmemi_c_error_count() != expected_errors:
            fail(f"device error count {L.ishmemi_c_error_count()}")
        for p in (dev_status, dev_cv, dev_idx):
            hip.free(p)
        for b in (words, arena):
            ish.ishmem_free(b)
        ish.ishmem_finalize()
    except Exception:
        fails.append(f"pe{pe} exception:\n{traceback.format_exc()}")
    q.put((pe, fails))

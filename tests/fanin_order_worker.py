"""The one PE of tests/test_gpu_fanin_order.py, in a process of its own (run_pes of
tests/test_gpu_multi.py): the pytest process itself never opens the GPU, so the co-located
multi-PE tests that run after this module find the device as they do without it.

Scenarios (each a function below; a failed assertion is reported with its case):
  vector  - body sizes of 0, 1, 63, 64, 65, 4097 16-B items and 1 MiB + one element, dest 4 / 12 B
            (float) or 8 B (double) off the 16-B grid with the sources on the same phase, so head
            and tail are non-empty: copy, combine with 2 and with 3 sources;
  shifted - a source on another 16-B phase: the realigned kernel from 1 KiB (the last workgroup
            partial) and the element-granular path below it, copy and 2-source combine;
  rule    - set_param "fanin_order" 0 with the lower bound at 0: get_param "last_fanin_order"
            after each launch of a sequence, stream capture and replay included.
Every result is bit-exact against numpy, with guard bytes before and after dest, under
fanin_order 1 (ascending) and 2 (descending).
"""
import os
import traceback

import numpy as np

PAD = 64
GUARD = 0xA5
NP = {"float": np.float32, "double": np.float64}
ORDERS = (1, 2)


def values(seed: int, n: int, dtype: str) -> np.ndarray:
    """Small integers as floating point: every partial sum is exact, so the fold order numpy uses
    and the kernel's agree bit for bit."""
    return np.random.default_rng(seed).integers(-1000, 1000, n).astype(NP[dtype])


def run_case(ish, bufs, op: str, dtype: str, nbytes: int, dest_off: int, src_offs: list[int], order: int):
    """One launch with dest at `dest_off` and source j at src_offs[j] bytes past a 256-B boundary
    (after PAD guard bytes); checks dest bit for bit and the guard bytes around it."""
    from ishmem_amd import hip
    (d, *s), cap = bufs
    es = np.dtype(NP[dtype]).itemsize
    assert nbytes % es == 0 and PAD + 16 + nbytes + PAD <= cap
    n = nbytes // es
    k = len(src_offs)
    xs = [values(1000 * order + 10 * n + j, n, dtype) for j in range(k)]
    for j in range(k):
        hip.upload(s[j] + PAD + src_offs[j], xs[j])
    span = PAD + dest_off + nbytes + PAD
    hip.memset(d, GUARD, span)
    ish.set_param("fanin_order", order)
    if op == "copy":
        r = ish.reduce_on_stream("sum", dtype, d + PAD + dest_off, s[0] + PAD + src_offs[0], n, None, 0)
    else:
        r = ish.combine("sum", dtype, d + PAD + dest_off, [s[j] + PAD + src_offs[j] for j in range(k)], n)
    what = (op, dtype, nbytes, dest_off, src_offs, order)
    assert r == 0, (what, ish.last_error())
    assert ish.get_param("last_fanin_order") == order - 1, what
    hip.synchronize()
    raw = hip.download(d, span, np.uint8)
    want = xs[0]
    for x in xs[1:]:
        want = want + x  # left to right, as the kernel folds
    lo, hi = PAD + dest_off, PAD + dest_off + nbytes
    assert np.array_equal(raw[lo:hi], want.view(np.uint8)), what
    assert (raw[:lo] == GUARD).all() and (raw[hi:] == GUARD).all(), what


OPS = [("copy", 1), ("combine", 2), ("combine", 3)]
# (dtype, dest offsets from the 16-B grid): element-aligned, head and tail both non-empty.
SAME_PHASE = [("float", (4, 12)), ("double", (8,))]
BODY_ITEMS = (0, 1, 63, 64, 65, 4097)


def vector(ish, bufs):
    for order in ORDERS:
        for op, k in OPS:
            for dtype, offs in SAME_PHASE:
                es = np.dtype(NP[dtype]).itemsize
                for off in offs:
                    for items in BODY_ITEMS:
                        nbytes = (16 - off) + 16 * items + es  # head up to the grid, the body, one tail element
                        run_case(ish, bufs, op, dtype, nbytes, off, [off] * k, order)
                    run_case(ish, bufs, op, dtype, (1 << 20) + es, off, [off] * k, order)  # 1 MiB + one element
                run_case(ish, bufs, op, dtype, (1 << 20) + es, 0, [0] * k, order)


def shifted(ish, bufs):
    for order in ORDERS:
        # The copy is a byte copy, so any source shift is element-aligned.  1 KiB: the realigned
        # kernel's entry; 20 004 B: three 8 KiB workgroups, the last partial; 1 MiB + 4 B; below
        # 1 KiB the element-granular path (1000 B: 15 full blocks and 40 items).
        for shift in (1, 4, 12):
            for dest_off in (0, 4):
                for nbytes in (1024, 20_004, (1 << 20) + 4, 1000, 4):
                    run_case(ish, bufs, "copy", "float", nbytes, dest_off, [(dest_off + shift) % 16], order)
        # combine needs the element's alignment: one shifted source and one on dest's phase, then both shifted.
        for dtype, shifts in (("float", (4, 12)), ("double", (8,))):
            es = np.dtype(NP[dtype]).itemsize
            for sh in shifts:
                for dest_off in (0, es):
                    srcs = [(dest_off + sh) % 16, dest_off]
                    for nbytes in (1024, 20_000 + es, (1 << 20) + es, 1000, es):
                        run_case(ish, bufs, "combine", dtype, nbytes, dest_off, srcs, order)
                    run_case(ish, bufs, "combine", dtype, 20_000 + es, dest_off, [(dest_off + sh) % 16] * 2, order)


# ---- the rule ---------------------------------------------------------------------------------
def copy(ish, d, s, n, stream=0):
    assert ish.reduce_on_stream("sum", "float", d, s, n, None, stream) == 0, ish.last_error()
    return ish.get_param("last_fanin_order")


def rule(ish, bufs):
    from ishmem_amd import hip
    (a, b, c, d), _ = bufs
    ish.set_param("fanin_order", 0)
    ish.set_param("fanin_order_min_bytes", 0)
    n = 4096
    x = values(1, n, "float")
    hip.upload(b, x)
    hip.upload(d, x + 1)
    copy(ish, c, d, n)  # whatever ran before, the record now holds c and d only
    assert [copy(ish, a, b, n) for _ in range(3)] == [0, 1, 0]  # first forward, then alternating
    assert copy(ish, c, d, n) == 0          # disjoint new buffers
    assert copy(ish, c, d, n) == 1          # the same again
    assert copy(ish, a, c, n) == 0          # the last dest as the new source flips
    assert copy(ish, b + 64, a, n) == 1     # and again, into a range overlapping an earlier source
    hip.synchronize()
    assert np.array_equal(hip.download(b + 64, n, np.float32), x + 1)
    # combine: the same record and rule; an in-place combine (dest is a source) is exempt.
    for want in (0, 1):
        assert ish.combine("sum", "float", c, [a, d], n) == 0
        assert ish.get_param("last_fanin_order") == want
    assert ish.combine("sum", "float", c, [c, d], n) == 0
    assert ish.get_param("last_fanin_order") == 0
    assert ish.combine("sum", "float", c, [a, d], n) == 0
    assert ish.get_param("last_fanin_order") == 0  # flips the record (1), not the exempt launch
    hip.synchronize()
    assert np.array_equal(hip.download(c, n, np.float32), (x + 1) + (x + 1))

    # below the bound: forward, record untouched
    ish.set_param("fanin_order_min_bytes", 4 * n)
    before = copy(ish, a, b, n)
    assert copy(ish, a, b, n) == 1 - before
    ish.set_param("fanin_order_min_bytes", 4 * n + 1)
    assert copy(ish, a, b, n) == 0 and copy(ish, a, b, n) == 0
    ish.set_param("fanin_order_min_bytes", 4 * n)
    assert copy(ish, a, b, n) == before
    ish.set_param("fanin_order_min_bytes", 0)

    # under stream capture: forward, record untouched, the replay's result correct
    n = 20_001
    st = hip.stream_create()
    try:
        copy(ish, a, b, n, st)
        assert copy(ish, a, b, n, st) == 1 - copy(ish, a, b, n, st)
        before = ish.get_param("last_fanin_order")
        hip.stream_synchronize(st)
        x = values(7, n, "float")
        with hip.Graph(st) as g:
            assert copy(ish, a, b, n, st) == 0  # a graph would bake the order in: ascending
        assert copy(ish, a, b, n, st) == 1 - before  # the record is as it was before the capture
        hip.stream_synchronize(st)
        hip.upload(b, x)
        hip.memset(a, GUARD, 4 * n + PAD)
        g.launch(st)
        hip.stream_synchronize(st)
        raw = hip.download(a, 4 * n + PAD, np.uint8)
        assert np.array_equal(raw[:4 * n], x.view(np.uint8)) and (raw[4 * n:] == GUARD).all()
        del g
    finally:
        hip.stream_destroy(st)


SCENARIOS = {"vector": vector, "shifted": shifted, "rule": rule}


def run(pe: int, npes: int, key: str, scenarios: list[str], q, env: dict | None = None) -> None:
    fails: list[str] = []
    try:
        for k, v in (env or {}).items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        import ishmem_amd as ish
        ish.init(pe, npes, 0, key)
        nb = (1 << 20) + 4096
        ptrs = [ish.ishmem_align(256, nb) for _ in range(4)]  # dest and three sources
        if not all(ptrs):
            fails.append(f"heap allocation: {ish.last_error()}")
        else:
            for name in scenarios:
                try:
                    SCENARIOS[name](ish, (ptrs, nb))
                except AssertionError:
                    fails.append(f"{name}: " + traceback.format_exc()[-1500:])
            for p in reversed(ptrs):
                ish.ishmem_free(p)
        ish.ishmem_finalize()
    except Exception:
        fails.append("worker: " + traceback.format_exc()[-1500:])
    q.put((pe, fails))

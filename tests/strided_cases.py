"""Case tables and expected results of the strided / blocked put / get tests (tests/strided_worker.py,
tests/test_gpu_strided.py), pinned on the CPU by tests/test_strided.py.

A case is (elem_bytes, dst, sst, bsize, nblocks): block b of bsize elements goes from
source + b * sst to dest + b * dst (element strides); iput / iget are bsize == 1.  Expected results
are numpy index arithmetic: `byte_index` lists the bytes a side touches, in transfer order.
"""
from __future__ import annotations

import numpy as np

GUARD = 64
SENTINEL = 0xA5
MAX_BLOCKS = 32      # ISHMEM_MAX_BLOCKS of the suite
TILE_ITEMS = 256 * 4  # items per workgroup per grid-stride step (kRmaBlock * kRmaUnroll)
# Every workgroup of a 32-workgroup grid runs its loop twice; one item is left for a third step.
LOOP_TWICE = 2 * MAX_BLOCKS * TILE_ITEMS + 1

WIDTHS = [1, 2, 4, 8, 16]
IPUT_STRIDES = [(1, 1), (2, 3), (3, 2), (7, 1), (1, 5)]
IPUT_NELEMS = [0, 1, 2, 63, 64, 65, 1025, LOOP_TWICE]

IB_BSIZES = [1, 2, 5, 16, 33, 1027]
IB_NBLOCKS = [0, 1, 2, 3, 65]
IB_WIDTHS = [1, 4, 16]


def iput_cases() -> list[tuple[int, int, int, int, int]]:
    return [(es, dst, sst, 1, n) for es in WIDTHS for dst, sst in IPUT_STRIDES for n in IPUT_NELEMS]


def ib_stride_pairs(bsize: int) -> list[tuple[int, int]]:
    """(dst, sst) from {bsize, bsize + 1, 2 * bsize + 3} with the two differing."""
    s = [bsize, bsize + 1, 2 * bsize + 3]
    return [(d, t) for d in s for t in s if d != t]


def ib_cases() -> list[tuple[int, int, int, int, int]]:
    return [(es, dst, sst, bs, nb) for es in IB_WIDTHS for bs in IB_BSIZES for dst, sst in ib_stride_pairs(bs)
            for nb in IB_NBLOCKS]


def offset_cases() -> list[tuple[int, int, tuple[int, int, int, int, int]]]:
    """(source byte offset, dest byte offset, case) for byte-wide elements: every pair of offsets
    0..15 with a shape whose block length and strides are multiples of 16 (the item is then set by the
    offsets alone: 16 B at (0, 0), 8 B at (8, 0), ... 1 B at odd offsets) and with a walking shape."""
    walk = [(1, 5, 3, 2, 3), (1, 34, 50, 33, 3), (1, 20, 17, 16, 65), (1, 9, 7, 5, 2), (1, 2048, 1030, 1027, 2)]
    out = []
    n = 0
    for soff in range(16):
        for doff in range(16):
            out.append((soff, doff, (1, 48, 64, 32, 5)))
            out.append((soff, doff, walk[n % len(walk)]))
            n += 1
    return out


def tester_calls(nelems: int) -> list[tuple[int, int, int, int, int, int]]:
    """The reference ibput tester's pair of calls for `nelems` elements, as (dest element offset,
    source element offset, dst, sst, bsize, nblocks).  For nelems == 3 the second call has a zero
    source stride and an empty block: it is refused and moves nothing."""
    calls = [(0, 0, nelems // 2 if nelems > 1 else 1, 1, 1, 2 if nelems > 1 else 1)]
    if nelems > 2:
        calls.append((1, 2, nelems // 2, nelems // 2 - 1, nelems // 2 - 1, 2))
    return calls


TESTER_NELEMS = [1, 2, 3, 16, 1024]
# The reference's int_iput_device test: arrays of 20 ints, 5 elements, dst = 3, sst = 2.
INT_IPUT_DEVICE = dict(array=20, dst=3, sst=2, nelems=5)


def strides_valid(dst: int, sst: int, bsize: int) -> bool:
    return dst >= 1 and sst >= 1 and dst >= bsize and sst >= bsize


def extent(stride: int, bsize: int, nblocks: int, es: int) -> int:
    """Bytes from a side's first to one past its last byte."""
    if nblocks == 0 or bsize == 0:
        return 0
    return ((nblocks - 1) * stride + bsize) * es


def byte_index(stride: int, bsize: int, nblocks: int, es: int) -> np.ndarray:
    """Byte offsets a side touches, in transfer order."""
    elems = (np.arange(nblocks, dtype=np.int64)[:, None] * stride + np.arange(bsize, dtype=np.int64)[None, :]).reshape(-1)
    return (elems[:, None] * es + np.arange(es, dtype=np.int64)[None, :]).reshape(-1)


def apply(dest: np.ndarray, source: np.ndarray, case: tuple[int, int, int, int, int], doff: int = 0, soff: int = 0) -> None:
    """dest (bytes) after the transfer `case` from source (bytes), both given from the pointers' bases
    plus byte offsets."""
    es, dst, sst, bsize, nblocks = case
    if nblocks == 0 or bsize == 0:
        return
    dest[doff + byte_index(dst, bsize, nblocks, es)] = source[soff + byte_index(sst, bsize, nblocks, es)]


def plan(dest: int, source: int, dst: int, sst: int, bsize: int, nblocks: int, es: int) -> tuple[int, int, bool]:
    """Restatement of the library's layout rule: (item bytes, items per block, contiguous)."""
    block = bsize * es
    vals = [dest, source, block] + ([dst * es, sst * es] if nblocks > 1 else [])
    w = 16
    while any(v % w for v in vals):
        w //= 2
    return w, block // w, nblocks <= 1 or (dst == bsize and sst == bsize)

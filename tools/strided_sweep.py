#!/usr/bin/env python3
"""Strided / blocked put and get against their two alternatives (dev tool): 2 co-located PEs (one
process per PE on device 0).

For element widths --widths (4 and 16 bytes), block lengths --blocks (1, 16, 256, 4096 elements; 1 is
iput / iget, the others ibput / ibget) and payloads --min-bytes .. --max-bytes by powers of four, PE 0
times, to / from PE 1's heap, with both strides twice the block length:
  put / get  the strided transfer, ibput_on_stream / ibget_on_stream;
  contig     ONE contiguous put_on_stream of the same payload bytes: the ceiling;
  loop       nblocks contiguous ishmem_putmem_nbi calls and one ishmem_quiet, what a user writes
             without the strided forms (skipped above --loop-max-calls calls per transfer).
put, get and contig are timed with HIP events around `iters` back-to-back stream-ordered calls; loop
with a host clock around the calls and their quiet (its cost is the host's, call by call).  The four
are interleaved round by round after a warm-up; the figure is the median over the rounds with the
quartiles as the spread.  PE 1 waits on the host meanwhile.  Each strided shape is checked once
(bit-exact: the first and last blocks and the gap after the first).  Writes CSV under
profiles/strided/ (--out) and prints it.

These are co-located numbers: both PEs share one GPU's HBM and there is no xGMI hop in them.
"""
from __future__ import annotations

import argparse
import multiprocessing as mp
import os
import sys
import time
import uuid
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

TILE = 16 << 20  # the source repeats with this period


def source_bytes(member: int, lo: int, hi: int) -> np.ndarray:
    """Bytes [lo, hi) of member `member`'s source: a multiplicative hash of (member, index mod TILE)."""
    i = np.arange(lo, hi, dtype=np.uint64) % np.uint64(TILE)
    return (((i + np.uint64(member * 0x9E3779B1)) * np.uint64(2654435761)) >> np.uint64(13)).astype(np.uint8)


def payloads(lo: int, hi: int) -> list[int]:
    out = []
    while lo <= hi:
        out.append(lo)
        lo *= 4
    return out


def worker(pe: int, npes: int, key: str, args, q, hb) -> None:
    import ishmem_amd as ish
    from ishmem_amd import hip

    ish.init(pe, npes, 0, key)
    ext_max = 2 * args.max_bytes
    src = ish.ishmem_align(256, ext_max + 256)
    dst = ish.ishmem_align(256, ext_max + 256)
    tile = source_bytes(pe, 0, min(TILE, ext_max))
    for lo in range(0, ext_max, TILE):
        hip.upload(src + lo, tile[:min(TILE, ext_max - lo)])
    st = hip.stream_create()
    other = (pe + 1) % npes
    rows = []
    for es in args.widths:
        for bsize in args.blocks:
            for B in payloads(args.min_bytes, args.max_bytes):
                bb = bsize * es
                if B < bb:
                    continue
                nblocks, stride = B // bb, 2 * bsize
                ops = {"put": lambda: ish.ibput_on_stream(dst, src, stride, stride, bsize, nblocks, es, other, st),
                       "get": lambda: ish.ibget_on_stream(dst, src, stride, stride, bsize, nblocks, es, other, st),
                       "contig": lambda: ish.put_on_stream(dst, src, B, other, st)}
                loop = nblocks <= args.loop_max_calls

                def loop_call():
                    for b in range(nblocks):
                        ish.ishmem_putmem_nbi(dst + b * stride * es, src + b * stride * es, bb, other)
                    ish.ishmem_quiet()
                # Warm up and check the strided forms: put lands in PE 1's dst, get in PE 0's.
                ok = {"contig": 1, "loop": 1}
                for name in ("put", "get"):
                    hip.memset(dst, 0, min(ext_max, 2 * B))
                    ish.ishmem_barrier_all()
                    if pe == 0:
                        for _ in range(args.warmup):
                            if ops[name]():
                                raise RuntimeError(ish.last_error())
                        hip.stream_synchronize(st)
                    ish.ishmem_barrier_all()
                    good = True
                    if pe == (1 if name == "put" else 0):
                        owner = 0 if name == "put" else 1
                        last = (nblocks - 1) * stride * es
                        for lo, hi, zero in ((0, bb, False), (bb, 2 * bb, True), (last, last + bb, False)):
                            got = hip.download(dst + lo, hi - lo, np.uint8)
                            want = np.zeros(hi - lo, np.uint8) if zero else source_bytes(owner, lo, hi)
                            good = good and np.array_equal(got, want)
                    ok[name] = int(good)
                    ish.ishmem_barrier_all()
                if pe == 0:
                    for _ in range(args.warmup):
                        ops["contig"]()
                        if loop:
                            loop_call()
                    hip.stream_synchronize(st)
                iters = max(2, min(args.iters, (2 << 30) // B))
                times = {name: [] for name in ("put", "get", "contig", "loop")}
                for _ in range(args.rounds):
                    for name, call in ops.items():  # interleaved: the same process, stream and minute
                        if pe == 0:
                            e0, e1 = hip.Event(), hip.Event()
                            e0.record(st)
                            for _ in range(iters):
                                call()
                            e1.record(st)
                            hip.stream_synchronize(st)
                            times[name].append(e0.elapsed_ms(e1) * 1000.0 / iters)
                    if pe == 0 and loop:
                        t0 = time.perf_counter()
                        loop_call()
                        times["loop"].append((time.perf_counter() - t0) * 1e6)
                hb.wait()  # PE 1 waits on the host: no polling kernel shares the GPU with the timed calls
                ish.ishmem_barrier_all()
                rows.append((es, bsize, B, nblocks, times, ok))
    ish.ishmem_barrier_all()
    ish.ishmem_finalize()
    q.put((pe, rows))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--widths", type=int, nargs="+", default=[4, 16])
    ap.add_argument("--blocks", type=int, nargs="+", default=[1, 16, 256, 4096])
    ap.add_argument("--min-bytes", type=int, default=4 << 10)
    ap.add_argument("--max-bytes", type=int, default=256 << 20)
    ap.add_argument("--loop-max-calls", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=20, help="calls per timed window (fewer at large sizes)")
    ap.add_argument("--rounds", type=int, default=5, help="timed windows per operation and shape")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "strided"))
    ap.add_argument("--tag", default="sweep")
    args = ap.parse_args()
    out = Path(args.out)
    out.mkdir(parents=True, exist_ok=True)
    npes = 2
    os.environ.setdefault("ISHMEM_SYMMETRIC_SIZE", "3G")
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    hb = ctx.Barrier(npes)
    key = f"str{uuid.uuid4().hex[:10]}"
    procs = [ctx.Process(target=worker, args=(pe, npes, key, args, q, hb)) for pe in range(npes)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=1100) for _ in range(npes))
    for p in procs:
        p.join(timeout=60)
    lines = ["pes,elem_bytes,block_elems,bytes,nblocks,op,us_median,us_q1,us_q3,GiBps,frac_of_contig,speedup_vs_loop,ok"]
    for i, (es, bsize, B, nblocks, times, ok) in enumerate(res[0]):
        med = {op: float(np.percentile(t, 50)) for op, t in times.items() if t}
        for op, t in times.items():
            if not t:
                continue
            q1, q3 = (float(np.percentile(t, x)) for x in (25, 75))
            good = min(res[pe][i][5][op] for pe in range(npes))
            frac = f"{med['contig'] / med[op]:.3f}" if op in ("put", "get") else ""
            vs = f"{med['loop'] / med[op]:.1f}" if op in ("put", "get") and "loop" in med else ""
            lines.append(f"{npes},{es},{bsize},{B},{nblocks},{op},{med[op]:.2f},{q1:.2f},{q3:.2f},"
                         f"{B / 2**30 / (med[op] * 1e-6):.2f},{frac},{vs},{good}")
    text = "\n".join(lines) + "\n"
    (out / f"{args.tag}_p{npes}.csv").write_text(text)
    print(text, flush=True)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""put and get against the local copy of the same size (dev tool): 2 co-located PEs (one process per
PE on device 0), B = --min-bytes .. --max-bytes by powers of two.

PE 0 moves B bytes to / from PE 1's heap with put_on_stream / get_on_stream while PE 1 waits on the
host, and copies B bytes inside its own heap with the fan-in copy kernel (ishmemi_c_combine with
one source: the kernel bench.py's 1-PE path runs).  All three move 2 B of HBM traffic per payload
byte on the one GPU, so the copy in the same process, stream and minute is the yardstick.  The three
are interleaved round by round, each round timed with HIP events after a warm-up; the figure is the
median over the rounds with the quartiles as the spread.  --repeat runs the whole sweep again in the
same processes, which gives the copy's own run-to-run spread.  Up to --a2a-max-bytes a 2-PE alltoall of
the same block size is timed too (both PEs take part), for orientation at small sizes.  Results are
checked (bit-exact, the first and last 64 KiB) once per size.  Writes CSV under profiles/rma/ (--out)
and prints it.

These are co-located numbers: both PEs share one GPU's HBM and there is no xGMI hop in them.
"""
from __future__ import annotations

import argparse
import multiprocessing as mp
import os
import sys
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


def worker(pe: int, npes: int, key: str, args, q, hb) -> None:
    import ishmem_amd as ish
    from ishmem_amd import hip

    ish.init(pe, npes, 0, key)
    for kv in args.param:
        name, val = kv.split("=", 1)
        ish.set_param(name, int(val))
    bmax = args.max_bytes
    src = ish.ishmem_align(256, bmax + args.src_offset + 256) + args.src_offset
    dst = ish.ishmem_align(256, bmax + args.dst_offset + 256) + args.dst_offset
    a2a_max = min(args.a2a_max_bytes, bmax // 2)
    tile = source_bytes(pe, 0, min(TILE, bmax))
    for lo in range(0, bmax, TILE):
        hip.upload(src + lo, tile[:min(TILE, bmax - lo)])
    st = hip.stream_create()
    other = (pe + 1) % npes
    rows = []

    def edges(B):
        return {(0, min(B, 65536)), (max(0, B - 65536), B)}

    for rep in range(args.repeat):
        B = args.min_bytes
        while B <= bmax:
            solo = {"put": lambda: ish.put_on_stream(dst, src, B, other, st),
                    "get": lambda: ish.get_on_stream(dst, src, B, other, st),
                    "copy": lambda: ish.combine("or", "uint8", dst, [src], B, st)}
            # Warm up and check: put lands in the other PE's dst, get and copy in this PE's.
            ok = {}
            for name, call in solo.items():
                hip.memset(dst, 0, B)
                ish.ishmem_barrier_all()
                if pe == 0:
                    for _ in range(args.warmup):
                        if call():
                            raise RuntimeError(ish.last_error())
                    hip.stream_synchronize(st)
                ish.ishmem_barrier_all()
                checker, owner = (1, 0) if name == "put" else (0, 1 if name == "get" else 0)
                good = True
                if pe == checker:
                    for lo, hi in edges(B):
                        good = good and np.array_equal(hip.download(dst + lo, hi - lo, np.uint8), source_bytes(owner, lo, hi))
                ok[name] = int(good)
                ish.ishmem_barrier_all()
            iters = max(2, min(args.iters, (4 << 30) // max(1, B)))
            times = {name: [] for name in solo}
            # PE 1 waits on the HOST (hb, a process barrier) while PE 0 times: a PE waiting in
            # ishmem_barrier_all keeps a polling kernel on the shared GPU, and PE 0's launches then
            # take turns with it (a first run of this tool showed 4 us calls flipping to 22-28 us).
            for _ in range(args.rounds):
                for name, call in solo.items():  # interleaved: the same process, stream and minute
                    if pe == 0:
                        e0, e1 = hip.Event(), hip.Event()
                        e0.record(st)
                        for _ in range(iters):
                            call()
                        e1.record(st)
                        hip.stream_synchronize(st)
                        times[name].append(e0.elapsed_ms(e1) * 1000.0 / iters)
                    else:
                        times[name].append(0.0)
            hb.wait()
            ish.ishmem_barrier_all()
            if B <= a2a_max:  # both PEs: a 2-PE alltoall of B-byte blocks, for orientation
                call = lambda: ish.alltoall_on_stream(dst, src, B, None, st)
                for _ in range(args.warmup):
                    call()
                hip.stream_synchronize(st)
                ish.ishmem_barrier_all()
                times["alltoall"] = []
                ok["alltoall"] = 1
                for _ in range(args.rounds):
                    e0, e1 = hip.Event(), hip.Event()
                    e0.record(st)
                    for _ in range(iters):
                        call()
                    e1.record(st)
                    hip.stream_synchronize(st)
                    times["alltoall"].append(e0.elapsed_ms(e1) * 1000.0 / iters)
                ish.ishmem_barrier_all()
            rows.append((rep, B, times, ok))
            B *= 2
    ish.ishmem_barrier_all()
    ish.ishmem_finalize()
    q.put((pe, rows))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--min-bytes", type=int, default=8)
    ap.add_argument("--max-bytes", type=int, default=1 << 30)
    ap.add_argument("--a2a-max-bytes", type=int, default=1 << 20)
    ap.add_argument("--iters", type=int, default=20, help="calls per timed window (fewer at large sizes)")
    ap.add_argument("--rounds", type=int, default=7, help="timed windows per operation and size")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeat", type=int, default=2, help="whole sweeps per process (run-to-run spread)")
    ap.add_argument("--src-offset", type=int, default=0)
    ap.add_argument("--dst-offset", type=int, default=0)
    ap.add_argument("--param", action="append", default=[], metavar="NAME=VALUE")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "rma"))
    ap.add_argument("--tag", default="sweep")
    args = ap.parse_args()
    out = Path(args.out)
    out.mkdir(parents=True, exist_ok=True)
    npes = 2
    os.environ.setdefault("ISHMEM_SYMMETRIC_SIZE", "3G")
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    hb = ctx.Barrier(npes)
    key = f"rma{uuid.uuid4().hex[:10]}"
    procs = [ctx.Process(target=worker, args=(pe, npes, key, args, q, hb)) for pe in range(npes)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=900) for _ in range(npes))
    for p in procs:
        p.join(timeout=60)
    lines = ["pes,rep,bytes,op,us_median,us_q1,us_q3,GiBps,frac_of_copy,ok"]
    for i, (rep, B, times, _) in enumerate(res[0]):
        copy_med = float(np.percentile(times["copy"], 50))
        for op in times:
            # put / get / copy: PE 0's times; alltoall: per round the slower PE.
            per_round = np.max(np.array([res[pe][i][2][op] for pe in range(npes)]), axis=0)
            med, q1, q3 = (float(np.percentile(per_round, x)) for x in (50, 25, 75))
            ok = min(res[pe][i][3][op] for pe in range(npes))
            frac = f"{copy_med / med:.3f}" if op in ("put", "get") else ""
            lines.append(f"{npes},{rep},{B},{op},{med:.2f},{q1:.2f},{q3:.2f},{B / 2**30 / (med * 1e-6):.2f},{frac},{ok}")
    text = "\n".join(lines) + "\n"
    (out / f"{args.tag}_p{npes}.csv").write_text(text)
    print(text, flush=True)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""alltoall against fcollect of the same block size (dev tool): TEAM_WORLD of --pes co-located PEs
(one process per PE on device 0), B = --min-bytes .. --max-bytes by powers of two.

The two collectives move the same bytes per member ((p-1)·B remote and B local read, p·B written), so
fcollect on the same kernels is the yardstick.  Both are enqueued on one stream of the same process,
interleaved round by round (alltoall, fcollect, alltoall, ...), each round timed with HIP events
after a warm-up of every shape; the figure per collective is the median over the rounds of the
slowest PE's time, with the quartiles as the spread.  --repeat runs the whole sweep again in the same
processes, which gives fcollect's own run-to-run spread.  Results are checked (bit-exact) once per
size.  Writes CSV under profiles/alltoall/ (--out) and prints it.

These are co-located numbers: every PE shares one GPU's HBM and there is no xGMI hop in them.
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


def source_bytes(member: int, lo: int, hi: int) -> np.ndarray:
    """Bytes [lo, hi) of member `member`'s source: a multiplicative hash of (member, index)."""
    i = np.arange(lo, hi, dtype=np.uint64)
    return (((i + np.uint64(member * 0x9E3779B1)) * np.uint64(2654435761)) >> np.uint64(13)).astype(np.uint8)


def worker(pe: int, npes: int, key: str, args, q) -> None:
    import ishmem_amd as ish
    from ishmem_amd import hip

    ish.init(pe, npes, 0, key)
    for kv in args.param:
        name, val = kv.split("=", 1)
        ish.set_param(name, int(val))
    bmax = args.max_bytes
    src = ish.ishmem_align(256, npes * bmax + args.src_offset + 256) + args.src_offset
    dst = ish.ishmem_align(256, npes * bmax + args.dst_offset + 256) + args.dst_offset
    chunk = 16 << 20
    for lo in range(0, npes * bmax, chunk):
        hip.upload(src + lo, source_bytes(pe, lo, min(lo + chunk, npes * bmax)))
    st = hip.stream_create()
    rows = []
    for rep in range(args.repeat):
        B = args.min_bytes
        while B <= bmax:
            calls = {"alltoall": lambda: ish.alltoall_on_stream(dst, src, B, None, st),
                     "fcollect": lambda: ish.fcollect_on_stream(dst, src, B, None, st)}
            # Warm both shapes up and check them: the first and last 64 KiB of every block.
            ok = {}
            for name, call in calls.items():
                for _ in range(args.warmup):
                    if call():
                        raise RuntimeError(ish.last_error())
                hip.stream_synchronize(st)
                good = True
                for j in range(npes):
                    base = pe * B if name == "alltoall" else 0  # where member j's source holds this block
                    for lo, hi in {(0, min(B, 65536)), (max(0, B - 65536), B)}:
                        got = hip.download(dst + j * B + lo, hi - lo, np.uint8)
                        good = good and np.array_equal(got, source_bytes(j, base + lo, base + hi))
                ok[name] = int(good)
            iters = max(2, min(args.iters, (256 << 20) // max(1, npes * B)))
            times = {name: [] for name in calls}
            ish.ishmem_barrier_all()
            for _ in range(args.rounds):
                for name, call in calls.items():  # interleaved: the same process, stream and minute
                    e0, e1 = hip.Event(), hip.Event()
                    e0.record(st)
                    for _ in range(iters):
                        call()
                    e1.record(st)
                    hip.stream_synchronize(st)
                    times[name].append(e0.elapsed_ms(e1) * 1000.0 / iters)
            rows.append((rep, B, {k: v for k, v in times.items()}, ok))
            B *= 2
    ish.ishmem_barrier_all()
    ish.ishmem_finalize()
    q.put((pe, rows))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--pes", type=int, nargs="+", default=[2, 4, 8])
    ap.add_argument("--min-bytes", type=int, default=8)
    ap.add_argument("--max-bytes", type=int, default=64 << 20)
    ap.add_argument("--iters", type=int, default=20, help="calls per timed window (fewer at large sizes)")
    ap.add_argument("--rounds", type=int, default=7, help="timed windows per collective and size")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeat", type=int, default=2, help="whole sweeps per process (run-to-run spread)")
    ap.add_argument("--src-offset", type=int, default=0)
    ap.add_argument("--dst-offset", type=int, default=0)
    ap.add_argument("--param", action="append", default=[], metavar="NAME=VALUE")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "alltoall"))
    ap.add_argument("--tag", default="sweep")
    args = ap.parse_args()
    out = Path(args.out)
    out.mkdir(parents=True, exist_ok=True)
    header = "pes,rep,block_bytes,coll,us_median,us_q1,us_q3,algbw_GiBps,ok"
    for npes in args.pes:
        os.environ.setdefault("ISHMEM_SYMMETRIC_SIZE", "4G")
        ctx = mp.get_context("spawn")
        q = ctx.Queue()
        key = f"a2a{uuid.uuid4().hex[:10]}"
        procs = [ctx.Process(target=worker, args=(pe, npes, key, args, q)) for pe in range(npes)]
        for p in procs:
            p.start()
        res = dict(q.get(timeout=900) for _ in range(npes))
        for p in procs:
            p.join(timeout=60)
        lines = [header]
        for i, (rep, B, _, _) in enumerate(res[0]):
            for coll in ("alltoall", "fcollect"):
                # Per round the slowest PE; over the rounds the median and quartiles.
                per_round = np.max(np.array([res[pe][i][2][coll] for pe in range(npes)]), axis=0)
                med, q1, q3 = (float(np.percentile(per_round, x)) for x in (50, 25, 75))
                ok = min(res[pe][i][3][coll] for pe in range(npes))
                lines.append(f"{npes},{rep},{B},{coll},{med:.2f},{q1:.2f},{q3:.2f},"
                             f"{npes * B / 2**30 / (med * 1e-6):.2f},{ok}")
        text = "\n".join(lines) + "\n"
        (out / f"{args.tag}_p{npes}.csv").write_text(text)
        print(text, flush=True)


if __name__ == "__main__":
    main()

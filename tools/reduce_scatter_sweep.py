#!/usr/bin/env python3
"""reduce-scatter against the reduce over the same source (dev tool): TEAM_WORLD of --pes co-located
PEs (one process per PE on device 0), float sum, B = --blocks bytes per block.

There is no earlier number for the call: the yardstick is the only way to get the same bytes without
it, ishmem_float_sum_reduce over p * nreduce elements, of which the caller keeps one block.  Both are
enqueued on one stream of the same process, interleaved window by window (reduce-scatter, reduce,
reduce-scatter, ...), each window timed with HIP events after a warm-up of both shapes; consecutive
calls rotate through --rotate buffer sets (as many as fit --rotate-bytes), so small sizes are not
timed on lines the previous call left in the caches.  The figure per collective is the median over
the windows of the slowest PE's time, with the quartiles as the spread; --repeat runs the whole
sweep again in the same processes.  Once per size the reduce-scatter's dest is compared bit for bit
with block `me` of the reduce's dest (first and last 64 KiB).  Writes CSV under
profiles/reduce_scatter/ (--out) and prints it.

Byte model, co-located, per PE: the reduce-scatter reads p blocks and writes one, (p + 1) * B; the
phased reduce reads p chunks, writes one, then reads p - 1 and writes p - 1 more: (3p - 1) * B for the
same B = N / p.  Launches: two barriers and one grid against three barriers and two grids.

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


def source_floats(member: int, n: int) -> np.ndarray:
    """Member `member`'s n source values in [-1, 1): a multiplicative hash of (member, index)."""
    i = np.arange(n, dtype=np.uint64)
    h = ((i + np.uint64(member * 0x9E3779B1 + 1)) * np.uint64(2654435761)) & np.uint64(0xFFFFFF)
    return (h.astype(np.float32) / np.float32(1 << 23)) - np.float32(1.0)


def worker(pe: int, npes: int, key: str, args, q) -> None:
    import ishmem_amd as ish
    from ishmem_amd import hip

    ish.init(pe, npes, 0, key)
    for kv in args.param:
        name, val = kv.split("=", 1)
        ish.set_param(name, int(val))
    st = hip.stream_create()
    rows = []
    for B in args.blocks:
        n = B // 4
        total = npes * n
        rot = max(1, min(args.rotate, args.rotate_bytes // ((2 * npes + 1) * B)))
        sets = []
        x = source_floats(pe, total)
        for _ in range(rot):
            s, dr, ds = (ish.ishmem_align(256, total * 4), ish.ishmem_align(256, total * 4), ish.ishmem_align(256, B))
            hip.upload(s, x)
            sets.append((s, dr, ds))
        turn = {"reduce_scatter": 0, "reduce": 0}

        def call(name):
            s, dr, ds = sets[turn[name] % rot]
            turn[name] += 1
            if name == "reduce_scatter":
                return ish.reduce_scatter_on_stream("sum", "float", ds, s, n, None, st)
            return ish.reduce_on_stream("sum", "float", dr, s, total, None, st)

        for rep in range(args.repeat):
            for name in turn:
                for _ in range(max(args.warmup, rot)):  # every buffer set of both shapes
                    if call(name):
                        raise RuntimeError(ish.last_error())
            hip.stream_synchronize(st)
            ok = 1
            for s, dr, ds in sets[:1]:
                for lo, hi in {(0, min(n, 16384)), (max(0, n - 16384), n)}:
                    a = hip.download(ds + lo * 4, hi - lo, np.uint32)
                    b = hip.download(dr + (pe * n + lo) * 4, hi - lo, np.uint32)
                    ok = ok and int(np.array_equal(a, b))
            iters = max(2, min(args.iters, args.window_bytes // max(1, total * 4)))
            times = {name: [] for name in turn}
            ish.ishmem_barrier_all()
            for _ in range(args.rounds):
                for name in turn:  # interleaved: the same process, stream and minute
                    e0, e1 = hip.Event(), hip.Event()
                    e0.record(st)
                    for _ in range(iters):
                        call(name)
                    e1.record(st)
                    hip.stream_synchronize(st)
                    times[name].append(e0.elapsed_ms(e1) * 1000.0 / iters)
            rows.append((rep, B, times, ok, rot))
        ish.ishmem_barrier_all()
        for s, dr, ds in reversed(sets):
            for b_ in (ds, dr, s):
                ish.ishmem_free(b_)
    ish.ishmem_barrier_all()
    ish.ishmem_finalize()
    q.put((pe, rows))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--pes", type=int, nargs="+", default=[2, 4])
    ap.add_argument("--blocks", type=int, nargs="+", default=[4 << 10, 64 << 10, 1 << 20, 16 << 20, 128 << 20],
                    help="bytes per block (B)")
    ap.add_argument("--iters", type=int, default=20, help="calls per timed window (fewer at large sizes)")
    ap.add_argument("--window-bytes", type=int, default=4 << 30, help="source bytes per timed window at most")
    ap.add_argument("--rounds", type=int, default=7, help="timed windows per collective and size")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeat", type=int, default=3, help="whole measurements per size (run-to-run spread)")
    ap.add_argument("--rotate", type=int, default=8, help="buffer sets to rotate through at most")
    ap.add_argument("--rotate-bytes", type=int, default=3 << 30, help="heap bytes for the rotating sets")
    ap.add_argument("--param", action="append", default=[], metavar="NAME=VALUE")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "reduce_scatter"))
    ap.add_argument("--tag", default="sweep")
    args = ap.parse_args()
    out = Path(args.out)
    out.mkdir(parents=True, exist_ok=True)
    header = "pes,rep,block_bytes,coll,us_median,us_q1,us_q3,model_bytes_per_pe,model_GBps,rotating_sets,ok"
    for npes in args.pes:
        os.environ.setdefault("ISHMEM_SYMMETRIC_SIZE", "6G")
        ctx = mp.get_context("spawn")
        q = ctx.Queue()
        key = f"rs{uuid.uuid4().hex[:10]}"
        procs = [ctx.Process(target=worker, args=(pe, npes, key, args, q)) for pe in range(npes)]
        for p in procs:
            p.start()
        res = dict(q.get(timeout=900) for _ in range(npes))
        for p in procs:
            p.join(timeout=60)
        lines = [header]
        for i, (rep, B, _, _, rot) in enumerate(res[0]):
            for coll in ("reduce_scatter", "reduce"):
                # Per window the slowest PE; over the windows the median and quartiles.
                per_round = np.max(np.array([res[pe][i][2][coll] for pe in range(npes)]), axis=0)
                med, q1, q3 = (float(np.percentile(per_round, x)) for x in (50, 25, 75))
                ok = min(res[pe][i][3] for pe in range(npes))
                model = (npes + 1) * B if coll == "reduce_scatter" else (3 * npes - 1) * B
                lines.append(f"{npes},{rep},{B},{coll},{med:.2f},{q1:.2f},{q3:.2f},{model},"
                             f"{model / 1e9 / (med * 1e-6):.1f},{rot},{ok}")
        text = "\n".join(lines) + "\n"
        (out / f"{args.tag}_p{npes}.csv").write_text(text)
        print(text, flush=True)


if __name__ == "__main__":
    main()

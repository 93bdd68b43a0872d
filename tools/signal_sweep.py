#!/usr/bin/env python3
"""put_signal hand-off latency against put + team sync, and the fused kernel against the two-launch
path (dev tool): 2 co-located PEs (one process per PE on device 0), B = --min-bytes .. --max-bytes by
powers of two.

Hand-off (ops handoff_*): a payload of B bytes goes from PE 0 to PE 1 and one of B bytes comes back,
`iters` times, all enqueued up front on one stream per PE; PE 0 times its window with HIP events and
the one-way figure is the window / (2 * iters): from the origin's put_signal_on_stream until the
target's signal_wait_until_on_stream has completed, averaged over both directions.
  handoff_fused       put_signal_on_stream -> signal_wait_until_on_stream, put_signal_fused_max_bytes = 4 MiB
  handoff_two_launch  the same with put_signal_fused_max_bytes = 0 (put grid, then the signal kernel)
  handoff_put_sync    what a user had to write before: put_on_stream + team_sync_on_stream on the
                      origin, team_sync_on_stream on the target
Per call (ops call_*): PE 0 issues `iters` calls back to back on its stream while PE 1 waits on the
HOST (a process barrier, no polling kernel on the shared GPU: DESIGN.md §3b records why):
  call_put, call_put_signal_fused, call_put_signal_two_launch
The operations of one size are interleaved round by round in the same processes, streams and minute;
the figure is the median over --rounds windows with the quartiles as the spread; --repeat runs the
whole sweep again in the same processes.  The payload is checked (bit-exact, first and last 64 KiB)
once per size and hand-off op.  Writes CSV under profiles/signal/ (--out) and prints it.

These are co-located numbers: both PEs share one GPU and there is no xGMI hop in them.
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

FUSED_ALL = 4 << 20
HANDOFF = ("handoff_fused", "handoff_two_launch", "handoff_put_sync")
CALLS = ("call_put", "call_put_signal_fused", "call_put_signal_two_launch")


def source_bytes(member: int, lo: int, hi: int) -> np.ndarray:
    i = np.arange(lo, hi, dtype=np.uint64)
    return (((i + np.uint64(member * 0x9E3779B1)) * np.uint64(2654435761)) >> np.uint64(13)).astype(np.uint8)


def worker(pe: int, npes: int, key: str, args, q, hb) -> None:
    try:
        run(pe, npes, key, args, q, hb)
    except BaseException as e:  # the other PE must not sit in the process barrier for ever
        hb.abort()
        q.put((pe, f"{type(e).__name__}: {e}"))


def run(pe: int, npes: int, key: str, args, q, hb) -> None:
    import ishmem_amd as ish
    from ishmem_amd import hip

    ish.init(pe, npes, 0, key)
    bmax = args.max_bytes
    src = ish.ishmem_align(256, bmax + 256)
    dst = ish.ishmem_align(256, bmax + 256)
    sig = ish.ishmem_align(256, 256)
    hip.upload(src, source_bytes(pe, 0, bmax))
    hip.memset(sig, 0, 8)
    st = hip.stream_create()
    other = 1 - pe
    W = ish.ISHMEM_TEAM_WORLD
    k = [0]  # the signal value: both PEs run the same loops, so they count alike
    rows = []

    def must(rc):
        if rc:
            raise RuntimeError(ish.last_error())

    def handoff(op, B, iters):
        if op != "handoff_put_sync":
            ish.set_param("put_signal_fused_max_bytes", FUSED_ALL if op == "handoff_fused" else 0)
        for _ in range(iters):
            if op == "handoff_put_sync":
                if pe == 0:
                    must(ish.put_on_stream(dst, src, B, other, st))
                    must(ish.team_sync_on_stream(W, None, st))
                    must(ish.team_sync_on_stream(W, None, st))
                else:
                    must(ish.team_sync_on_stream(W, None, st))
                    must(ish.put_on_stream(dst, src, B, other, st))
                    must(ish.team_sync_on_stream(W, None, st))
                continue
            k[0] += 1
            if pe == 0:
                must(ish.put_signal_on_stream(dst, src, B, sig, k[0], ish.ISHMEM_SIGNAL_SET, other, st))
                must(ish.signal_wait_until_on_stream(sig, ish.ISHMEM_CMP_EQ, k[0], 0, st))
            else:
                must(ish.signal_wait_until_on_stream(sig, ish.ISHMEM_CMP_EQ, k[0], 0, st))
                must(ish.put_signal_on_stream(dst, src, B, sig, k[0], ish.ISHMEM_SIGNAL_SET, other, st))

    def call(op, B, iters):
        if op != "call_put":
            ish.set_param("put_signal_fused_max_bytes", FUSED_ALL if op == "call_put_signal_fused" else 0)
        for _ in range(iters):
            if op == "call_put":
                must(ish.put_on_stream(dst, src, B, other, st))
            else:
                k[0] += 1
                must(ish.put_signal_on_stream(dst, src, B, sig, k[0], ish.ISHMEM_SIGNAL_SET, other, st))

    def timed(fn, op, B, iters):
        e0, e1 = hip.Event(), hip.Event()
        e0.record(st)
        fn(op, B, iters)
        e1.record(st)
        hip.stream_synchronize(st)
        return e0.elapsed_ms(e1) * 1000.0

    for rep in range(args.repeat):
        B = args.min_bytes
        while B <= bmax:
            ok = {}
            for op in HANDOFF:  # warm up and check
                hip.memset(dst, 0, B)
                hb.wait()
                handoff(op, B, args.warmup)
                hip.stream_synchronize(st)
                hb.wait()
                good = True
                for lo, hi in {(0, min(B, 65536)), (max(0, B - 65536), B)}:
                    good = good and np.array_equal(hip.download(dst + lo, hi - lo, np.uint8), source_bytes(other, lo, hi))
                ok[op] = int(good)
            times = {op: [] for op in HANDOFF + CALLS}
            for _ in range(args.rounds):
                for op in HANDOFF:  # interleaved: the same processes, streams and minute
                    hb.wait()
                    times[op].append(timed(handoff, op, B, args.iters) / (2 * args.iters))
                for op in CALLS:
                    hb.wait()
                    if pe == 0:
                        call(op, B, args.warmup)
                        times[op].append(timed(call, op, B, args.iters) / args.iters)
                    else:  # PE 1 idles on the host; it counts the signal values PE 0 uses
                        if op != "call_put":
                            k[0] += args.warmup + args.iters
                        times[op].append(0.0)
                    hb.wait()
                    ok[op] = 1
            rows.append((rep, B, times, ok))
            B *= 2
    hb.wait()
    ish.ishmem_barrier_all()
    ish.ishmem_finalize()
    q.put((pe, rows))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--min-bytes", type=int, default=8)
    ap.add_argument("--max-bytes", type=int, default=4 << 20)
    ap.add_argument("--iters", type=int, default=20, help="hand-offs (there and back) or calls per timed window")
    ap.add_argument("--rounds", type=int, default=7, help="timed windows per operation and size")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeat", type=int, default=2, help="whole sweeps per process (run-to-run spread)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "signal"))
    ap.add_argument("--tag", default="sweep")
    args = ap.parse_args()
    out = Path(args.out)
    out.mkdir(parents=True, exist_ok=True)
    npes = 2
    os.environ.setdefault("ISHMEM_SYMMETRIC_SIZE", "256M")
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    hb = ctx.Barrier(npes)
    key = f"sig{uuid.uuid4().hex[:10]}"
    procs = [ctx.Process(target=worker, args=(pe, npes, key, args, q, hb)) for pe in range(npes)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=600) for _ in range(npes))
    for p in procs:
        p.join(timeout=60)
    if any(isinstance(r, str) for r in res.values()):
        raise SystemExit(f"a PE failed: {res}")
    lines = ["pes,rep,bytes,op,us_median,us_q1,us_q3,vs_put_sync,ok"]
    for i, (rep, B, times, _) in enumerate(res[0]):
        base = float(np.percentile(times["handoff_put_sync"], 50))
        for op in times:
            med, q1, q3 = (float(np.percentile(times[op], x)) for x in (50, 25, 75))  # PE 0's windows
            ok = min(res[pe][i][3][op] for pe in range(npes))
            ratio = f"{med / base:.3f}" if op.startswith("handoff") else ""
            lines.append(f"{npes},{rep},{B},{op},{med:.2f},{q1:.2f},{q3:.2f},{ratio},{ok}")
    text = "\n".join(lines) + "\n"
    (out / f"{args.tag}_p{npes}.csv").write_text(text)
    print(text, flush=True)


if __name__ == "__main__":
    main()

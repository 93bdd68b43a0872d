#!/usr/bin/env python3
"""Cost of the atomic memory operations (dev tool): 2 co-located PEs (one process per PE on device 0).

Host (ops host_*): PE 0 issues `iters` calls back to back and times the window on the host clock
(the calls are blocking; the _nbi form is timed with its quiet), to its peer and to itself, while PE 1
waits on the host (a process barrier, no polling kernel on the shared GPU):
  host_signal_add           ishmemi_c_signal_op(ADD): the existing call of the same shape
  host_atomic_add           blocking, no fetched value
  host_atomic_fetch_add     blocking, the value comes back through the pinned host word
  host_atomic_fetch_add_nbi + quiet after every call
The operations are interleaved round by round in the same processes and minute; the figure is the
median over --rounds windows with the quartiles as the spread.
Device (ops dev_*): tools/amo_device_bench.hip, fetching atomics per microsecond on a peer's word from
1 wave, 1 workgroup, 64 and 256 workgroups, on one word and on one word per wave.
Writes CSV under profiles/amo/ (--out) and prints it.

These are co-located numbers: both PEs share one GPU and there is no xGMI hop in them.
"""
from __future__ import annotations

import argparse
import multiprocessing as mp
import os
import subprocess
import sys
import time
import uuid
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

HOST_OPS = ("host_signal_add", "host_atomic_add", "host_atomic_fetch_add", "host_atomic_fetch_add_nbi")
DEV_EXE = ROOT / "build" / "tools" / "amo_device_bench"


def build_device_bench() -> Path:
    src = ROOT / "tools" / "amo_device_bench.hip"
    lib = ROOT / "ishmem_amd" / "libishmem_amd.so"
    if DEV_EXE.exists() and all(d.stat().st_mtime <= DEV_EXE.stat().st_mtime for d in (src, lib)):
        return DEV_EXE
    DEV_EXE.parent.mkdir(parents=True, exist_ok=True)
    subprocess.run(["hipcc", "--offload-arch=gfx950", "-O2", "-std=c++20", f"-I{ROOT / 'include'}", str(src),
                    f"-L{lib.parent}", "-lishmem_amd", f"-Wl,-rpath,{lib.parent}", "-o", str(DEV_EXE)], check=True)
    return DEV_EXE


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
    word = ish.ishmem_align(256, 256)
    fetch = ish.ishmem_align(256, 256)
    hip.memset(word, 0, 256)
    ish.ishmem_barrier_all()

    def must(rc):
        if rc:
            raise RuntimeError(ish.last_error())

    def call(op, to):
        if op == "host_signal_add":
            must(ish.ishmemx_signal_add(word, 1, to))
        elif op == "host_atomic_add":
            must(ish.atomic_add(word, "uint64", 1, to)[0])
        elif op == "host_atomic_fetch_add":
            must(ish.atomic_fetch_add(word, "uint64", 1, to)[0])
        else:
            must(ish.atomic_fetch_add_nbi(fetch, word, "uint64", 1, to))
            must(ish.ishmem_quiet())

    times = {(op, tgt): [] for op in HOST_OPS for tgt in ("peer", "self")}
    for r in range(args.rounds + 1):  # round 0 warms up
        for tgt in ("peer", "self"):
            for op in HOST_OPS:
                hb.wait()
                if pe == 0:
                    to = 1 if tgt == "peer" else 0
                    t0 = time.perf_counter()
                    for _ in range(args.iters):
                        call(op, to)
                    dt = (time.perf_counter() - t0) * 1e6 / args.iters
                    if r:
                        times[(op, tgt)].append(dt)
                hb.wait()
    hb.wait()
    ish.ishmem_barrier_all()
    total = int(hip.download(word, 1, np.uint64)[0])
    ish.ishmem_finalize()
    q.put((pe, (times, total)))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200, help="calls per timed window")
    ap.add_argument("--rounds", type=int, default=9, help="timed windows per operation")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "amo"))
    ap.add_argument("--tag", default="sweep")
    args = ap.parse_args()
    out = Path(args.out)
    out.mkdir(parents=True, exist_ok=True)
    npes = 2
    os.environ.setdefault("ISHMEM_SYMMETRIC_SIZE", "256M")
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    hb = ctx.Barrier(npes)
    key = f"amo{uuid.uuid4().hex[:10]}"
    procs = [ctx.Process(target=worker, args=(pe, npes, key, args, q, hb)) for pe in range(npes)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=600) for _ in range(npes))
    for p in procs:
        p.join(timeout=60)
    if any(isinstance(r, str) for r in res.values()):
        raise SystemExit(f"a PE failed: {res}")
    times, _ = res[0]
    want = 4 * (args.rounds + 1) * args.iters  # every op adds 1 per call to each target's word
    ok = int(all(res[pe][1] == want for pe in range(npes)))
    lines = ["pes,op,target,figure,median,q1,q3,vs_signal_add,ok"]
    for tgt in ("peer", "self"):
        base = float(np.percentile(times[("host_signal_add", tgt)], 50))
        for op in HOST_OPS:
            med, q1, q3 = (float(np.percentile(times[(op, tgt)], x)) for x in (50, 25, 75))
            lines.append(f"{npes},{op},{tgt},us_per_call,{med:.2f},{q1:.2f},{q3:.2f},{med / base:.3f},{ok}")
    # the device program, PEs as processes of their own
    exe = build_device_bench()
    key = f"amod{uuid.uuid4().hex[:10]}"
    devs = []
    for pe in range(npes):
        env = {**os.environ, "ISHMEM_PE": str(pe), "ISHMEM_NPES": str(npes), "ISHMEM_DEVICE": "0", "ISHMEM_BOOTSTRAP_KEY": key}
        env.pop("HSA_ENABLE_IPC_MODE_LEGACY", None)
        devs.append(subprocess.Popen([str(exe)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = []
    for p in devs:
        try:
            o, _ = p.communicate(timeout=300)
        except subprocess.TimeoutExpired:
            p.kill()
            o, _ = p.communicate()
        outs.append((p.returncode, o))
    if any(rc for rc, _ in outs):
        raise SystemExit(f"the device program failed: {outs}")
    for ln in outs[0][1].splitlines():
        if ln.startswith("AMODEV,"):
            _, shape, words, lanes, ops, med, q1, q3, rate = ln.split(",")
            lines.append(f"{npes},dev_fetch_add_{shape}_{lanes}_lanes,peer_{words},us_per_kernel_of_{ops}_lane_ops,{med},{q1},{q3},,1")
            lines.append(f"{npes},dev_fetch_add_{shape}_{lanes}_lanes,peer_{words},lane_ops_per_us,{rate},,,,1")
    text = "\n".join(lines) + "\n"
    (out / f"{args.tag}_p{npes}.csv").write_text(text)
    print(text, flush=True)


if __name__ == "__main__":
    main()

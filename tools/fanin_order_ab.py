"""Measurements behind the local fan-in's block order, one process per library:

    python tools/fanin_order_ab.py --label new --legs cold,copy,combine [--lib PATH] [--root DIR]

  cold    - a 1 GiB copy forced ascending and forced descending, interleaved, each timed launch
            after an unrelated 1 GiB buffer pair was streamed through (nothing of the operands is
            left in the Infinity Cache): what a wrong guess of the rule costs;
  copy    - back-to-back one-member float sum reduces (copies) of --sizes-mib per operand, each
            order mode in turn, --reps rounds interleaved: ms per call;
  combine - the same for dst = a + b.
Modes: auto (set_param "fanin_order" 0 with the lower bound at 0), fwd (1), rev (2); a library
without the parameter (--root / --lib of an older build) runs its only order as "default".
Prints one JSON line per leg.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
from pathlib import Path


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", default="new")
    ap.add_argument("--legs", default="cold,copy,combine")
    ap.add_argument("--sizes-mib", default="16,32,64,128,256,512,1024,2048,4096")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cold-launches", type=int, default=12)
    ap.add_argument("--root", default=str(Path(__file__).resolve().parents[1]),
                    help="tree whose ishmem_amd package is imported")
    ap.add_argument("--lib", default=None, help="library to load instead of the tree's (ISHMEM_AMD_LIB)")
    args = ap.parse_args()
    sizes = [int(x) << 20 for x in args.sizes_mib.split(",")]
    legs = args.legs.split(",")
    if args.lib:
        os.environ["ISHMEM_AMD_LIB"] = str(Path(args.lib).resolve())
    nsrc = 2 if "combine" in legs else 1
    os.environ.setdefault("ISHMEM_SYMMETRIC_SIZE", str((nsrc + 1) * max(sizes + [1 << 30]) + (1 << 30)))
    sys.path.insert(0, args.root)
    import ishmem_amd as ish
    from ishmem_amd import hip

    ish.init(0, 1, 0, None)
    has_param = ish.set_param("fanin_order", 0) == 0
    modes = {"auto": 0, "fwd": 1, "rev": 2} if has_param else {"default": None}
    if has_param:
        ish.set_param("fanin_order_min_bytes", 0)
    big = max(sizes + [1 << 30])
    dst, a, b = ish.ishmem_malloc(big), ish.ishmem_malloc(big), ish.ishmem_malloc(big) if nsrc == 2 else 0
    assert dst and a and (b or nsrc == 1), ish.last_error()
    hip.memset(a, 1, big)
    if b:
        hip.memset(b, 2, big)
    st = hip.stream_create()

    def launch(kind: str, nbytes: int) -> None:
        n = nbytes // 4
        r = (ish.reduce_on_stream("sum", "float", dst, a, n, None, st) if kind == "copy"
             else ish.combine("sum", "float", dst, [a, b], n, st))
        if r:
            raise RuntimeError(ish.last_error())

    def set_mode(m) -> None:
        if m is not None:
            ish.set_param("fanin_order", m)

    def timed(kind: str, nbytes: int, iters: int) -> float:
        for _ in range(3):
            launch(kind, nbytes)
        e0, e1 = hip.Event(), hip.Event()
        e0.record(st)
        for _ in range(iters):
            launch(kind, nbytes)
        e1.record(st)
        hip.stream_synchronize(st)
        return e0.elapsed_ms(e1) / iters

    if "cold" in legs and has_param:
        fa, fb = hip.malloc(1 << 30), hip.malloc(1 << 30)
        hip.memset(fa, 3, 1 << 30)
        out = {"fwd": [], "rev": []}
        for _ in range(args.cold_launches):
            for name in ("fwd", "rev"):
                set_mode(1)
                ish.combine("sum", "float", fb, [fa], (1 << 30) // 4, st)  # the flush: 2 GiB of unrelated traffic
                set_mode(modes[name])
                e0, e1 = hip.Event(), hip.Event()
                e0.record(st)
                launch("copy", 1 << 30)
                e1.record(st)
                hip.stream_synchronize(st)
                out[name].append(round(e0.elapsed_ms(e1), 5))
        hip.free(fa)
        hip.free(fb)
        print(json.dumps({"label": args.label, "leg": "cold", "bytes": 1 << 30, "ms": out}), flush=True)

    for kind in ("copy", "combine"):
        if kind not in legs:
            continue
        rows = []
        for nbytes in sizes:
            iters = max(10, min(200, (16 << 30) // nbytes))
            ms = {k: [] for k in modes}
            for _ in range(args.reps):
                for name, m in modes.items():
                    set_mode(m)
                    ms[name].append(round(timed(kind, nbytes, iters), 5))
            rows.append({"bytes": nbytes, "iters": iters, "ms": ms})
        print(json.dumps({"label": args.label, "leg": kind, "rows": rows}), flush=True)
    hip.stream_destroy(st)
    ish.ishmem_finalize()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())

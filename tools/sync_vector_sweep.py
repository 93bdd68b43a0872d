"""Host cost of the vector waits and tests against the scalar wait they replace.

One PE, N already-satisfied uint64 variables, N in {1, 8, 64, 256}.  Timed per call, on the host clock:
  wait_until_all / wait_until_some / test_all   one vector call (one kernel launch);
  scalar x N                                    N successive ishmem_uint64_wait_until calls, the only
                                                way to wait for N words before, in the same process.
The four are measured in alternating windows (window = REPS calls of each, in turn), WINDOWS times, so
a drift of the shared host hits all of them alike.  Reported: the median over all calls, the
quartiles, the minimum, and the spread of the per-window medians.  Nothing here is a pass bar.

  python tools/sync_vector_sweep.py [--out profiles/sync_vector/sweep.csv]
"""
from __future__ import annotations

import argparse
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

SIZES = [1, 8, 64, 256]
WINDOWS, REPS, WARM = 7, 40, 20


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "sync_vector" / "sweep.csv"))
    args = ap.parse_args()
    import ishmem_amd as ish
    from ishmem_amd import hip

    ish.init(0, 1, 0, None)
    nmax = max(SIZES)
    ivars = ish.ishmem_align(256, nmax * 8)
    indices = hip.malloc(nmax * 8)
    hip.upload(ivars, np.full(nmax, 5, dtype="<u8"))
    EQ = ish.ISHMEM_CMP_EQ

    def scalar(n):
        for i in range(n):
            if ish.ishmem_uint64_wait_until(ivars + 8 * i, EQ, 5):
                raise RuntimeError(ish.last_error())

    def vector(op, want):
        def call(n):
            if ish.sync_vector(op, "uint64", ivars, n, indices, 0, EQ, 5) != (0, want(n)):
                raise RuntimeError(f"{op}: {ish.last_error()}")
        return call

    forms = {"wait_until_all": vector("wait_until_all", lambda n: 1), "wait_until_some": vector("wait_until_some", lambda n: n),
             "test_all": vector("test_all", lambda n: 1), "scalar_x_N": scalar}
    rows = ["form,nelems,calls,median_us,q25_us,q75_us,min_us,window_median_lo_us,window_median_hi_us"]
    for n in SIZES:
        samples = {k: [] for k in forms}
        wmed = {k: [] for k in forms}
        for name, fn in forms.items():
            for _ in range(WARM):
                fn(n)
        for _ in range(WINDOWS):
            for name, fn in forms.items():
                win = []
                for _ in range(REPS):
                    t0 = time.perf_counter()
                    fn(n)
                    win.append((time.perf_counter() - t0) * 1e6)
                samples[name] += win
                wmed[name].append(statistics.median(win))
        for name in forms:
            s = sorted(samples[name])
            q = statistics.quantiles(s, n=4)
            rows.append(f"{name},{n},{len(s)},{statistics.median(s):.2f},{q[0]:.2f},{q[2]:.2f},{s[0]:.2f},"
                        f"{min(wmed[name]):.2f},{max(wmed[name]):.2f}")
    hip.free(indices)
    ish.ishmem_free(ivars)
    ish.ishmem_finalize()
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("\n".join(rows) + "\n")
    print("\n".join(rows))
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""bench.py's plain run on the GPU: `--steps` timed steps, the lean result line, and
`--dump-outputs` — the dest of the last timed step as DIR/dest_pe0.npy, whole when it fits the
dump's budget and as the fixed windows of bench.dump_windows above it — compared bit for bit with
the closed-form fold of the input pattern (ishmem_amd/selfcheck.py; 1 PE: dest = source)."""
import importlib.util
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
MOVED_LEGS = ("combine", "cpu_baseline_pes", "cpu_baseline_mpich", "e2e_host", "e2e_host_pageable")


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", ROOT / "bench.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# 4 MiB: dumped whole.  13 Mi + 5 elements (odd, above the 12 Mi-element budget): sampled windows.
@pytest.mark.parametrize("nelems", [1 << 20, (13 << 20) + 5], ids=["whole", "sampled"])
def test_plain_run_is_lean_and_dumps_the_timed_dest(tmp_path, nelems):
    from ishmem_amd import selfcheck as sc
    b = _bench()
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--nelems", str(nelems), "--dump-outputs", str(tmp_path / "out")],
                       cwd=str(ROOT), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["full"] is False
    assert d["unit"] == "GiB/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert abs(d["value"] - nelems * 4 / 2**30 / (d["ms_per_step"] / 1000.0)) <= 1e-9 * d["value"]
    assert d["cpu_baseline"] is None and not [k for k in MOVED_LEGS if k in d]
    assert sorted(p.name for p in (tmp_path / "out").iterdir()) == ["dest_pe0.npy"]
    got = np.load(tmp_path / "out" / "dest_pe0.npy")
    wins = b.dump_windows(nelems, 1)
    assert got.dtype == np.float32 and got.size == sum(m for _, m in wins) == d["outputs"]["elements"]
    assert got.nbytes <= b.DUMP_MAX_BYTES and d["outputs"]["sampled"] == (len(wins) > 1)
    want = np.concatenate([sc.pattern_expected("sum", np.float32, 1, lo, m) for lo, m in wins])
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))

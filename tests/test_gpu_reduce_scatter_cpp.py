"""The reduce-scatter extension through the C++ names, host and device
(tests/cpp/reduce_scatter_patterns.hip): the reference tester's reduce patterns, sliced; host blocking
and on-stream, work_group by a 1024-thread block and by a 64-lane tile, the one-thread form; the world
team and a strided team; aligned and misaligned dest; device reduce-scatters alternating with a device
reduce of the same team; guard bytes round dest.  Both host paths."""
from pathlib import Path

import pytest

from tests.test_gpu_cpp import build_exe, run_exe

ROOT = Path(__file__).resolve().parents[1]
RS_EXE = ROOT / "build" / "reduce_scatter_patterns"


def test_reduce_scatter_program_builds():
    assert build_exe(ROOT / "tests/cpp/reduce_scatter_patterns.hip", RS_EXE).exists()


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["default", "barrier"])
@pytest.mark.parametrize("npes", [2, 4])
def test_cpp_reduce_scatter_patterns(npes, path, monkeypatch):
    if path == "barrier":
        monkeypatch.setenv("ISHMEM_LL_MAX_BYTES", "0")  # run_exe hands the environment to every PE
    else:
        monkeypatch.delenv("ISHMEM_LL_MAX_BYTES", raising=False)
    run_exe(build_exe(ROOT / "tests/cpp/reduce_scatter_patterns.hip", RS_EXE), npes)

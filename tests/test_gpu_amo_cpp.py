"""Atomic memory operations from inside kernels, through the C++ names (tests/cpp/amo_patterns.hip):
contended fetch_inc / fetch_add on one word and on words and PEs that diverge inside a wave, bit
masks, a compare_swap lock around plain counters, float / double swap rings, the _nbi device forms,
every thread's atomic_inc with the leader's wait_until, a bad pe, and a few host names."""
from pathlib import Path

import pytest

from tests.test_gpu_cpp import build_exe, run_exe

ROOT = Path(__file__).resolve().parents[1]
AMO_EXE = ROOT / "build" / "amo_patterns"


def test_amo_program_builds():
    assert build_exe(ROOT / "tests/cpp/amo_patterns.hip", AMO_EXE).exists()


@pytest.mark.gpu
@pytest.mark.parametrize("npes", [2, 3])
def test_cpp_amo_patterns(npes):
    run_exe(build_exe(ROOT / "tests/cpp/amo_patterns.hip", AMO_EXE), npes, timeout=120)

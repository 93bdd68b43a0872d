"""put_signal, wait_until and test from inside kernels, through the C++ names
(tests/cpp/signal_patterns.hip): the in-kernel ping-pong by a block, a 64-lane tile and single
work-items with warm consumers, device wait_until / test against a peer's device p, the ADD fan-in,
the host names, and device waits that time out instead of hanging."""
from pathlib import Path

import pytest

from tests.test_gpu_cpp import build_exe, run_exe

ROOT = Path(__file__).resolve().parents[1]
SIGNAL_EXE = ROOT / "build" / "signal_patterns"


def test_signal_program_builds():
    assert build_exe(ROOT / "tests/cpp/signal_patterns.hip", SIGNAL_EXE).exists()


@pytest.mark.gpu
@pytest.mark.parametrize("npes", [2, 3])
def test_cpp_signal_patterns(npes):
    run_exe(build_exe(ROOT / "tests/cpp/signal_patterns.hip", SIGNAL_EXE), npes)


@pytest.mark.gpu
@pytest.mark.parametrize("npes", [2])
def test_cpp_device_waits_are_bounded(npes, monkeypatch):
    # The program itself sets ISHMEM_TIMEOUT_MS=300 in this mode (run_exe fixes the variable).
    monkeypatch.setenv("SIGNAL_PATTERNS_BOUNDED", "1")
    run_exe(build_exe(ROOT / "tests/cpp/signal_patterns.hip", SIGNAL_EXE), npes, timeout=120)

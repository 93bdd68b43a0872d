"""The vector waits and tests from inside kernels, through the C++ names
(tests/cpp/sync_vector_patterns.hip): an in-kernel fan-in consumed by a wait_until_some loop with warm
consumers, wait_until_all and a test_any polling loop, each by a block, a 64-lane tile and one
work-item; the host names; and device waits that time out instead of hanging."""
from pathlib import Path

import pytest

from tests.test_gpu_cpp import build_exe, run_exe

ROOT = Path(__file__).resolve().parents[1]
SYNCVEC_EXE = ROOT / "build" / "sync_vector_patterns"
SRC = ROOT / "tests/cpp/sync_vector_patterns.hip"


def test_sync_vector_program_builds():
    assert build_exe(SRC, SYNCVEC_EXE).exists()


@pytest.mark.gpu
@pytest.mark.parametrize("npes", [2, 3])
def test_cpp_sync_vector_patterns(npes):
    run_exe(build_exe(SRC, SYNCVEC_EXE), npes)


@pytest.mark.gpu
@pytest.mark.parametrize("npes", [2])
def test_cpp_device_vector_waits_are_bounded(npes, monkeypatch):
    # The program itself sets ISHMEM_TIMEOUT_MS=300 in this mode (run_exe fixes the variable).
    monkeypatch.setenv("SYNC_VECTOR_BOUNDED", "1")
    run_exe(build_exe(SRC, SYNCVEC_EXE), npes, timeout=120)

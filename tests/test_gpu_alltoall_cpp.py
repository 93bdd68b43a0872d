"""alltoall through the C++ names, host and device (tests/cpp/alltoall_patterns.hip): the reference
test's aligned sizes and offset sweep, element sizes 1 / 2 / 4 / 8 and alltoallmem, in five modes
(host blocking, on-stream, work_group by a block, by a wavefront tile, single thread)."""
from pathlib import Path

import pytest

from tests.test_gpu_cpp import build_exe, run_exe

ROOT = Path(__file__).resolve().parents[1]
A2A_EXE = ROOT / "build" / "alltoall_patterns"


def test_alltoall_program_builds():
    assert build_exe(ROOT / "tests/cpp/alltoall_patterns.hip", A2A_EXE).exists()


@pytest.mark.gpu
@pytest.mark.parametrize("npes", [2, 3])
def test_cpp_reference_style_alltoall_tests(npes):
    run_exe(build_exe(ROOT / "tests/cpp/alltoall_patterns.hip", A2A_EXE), npes)

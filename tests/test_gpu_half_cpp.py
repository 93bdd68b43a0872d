"""The 16-bit floating-point reductions through the C++ names (tests/cpp/half_patterns.hip): typed and
generic host names, the on-stream names, the _work_group forms by a thread block and by a 64-lane
tile and the one-work-item form, on TEAM_WORLD and on a strided team whose team index is not the PE
number; expected values from a host restatement of tests/half_model.py."""
from pathlib import Path

import pytest

from tests.test_gpu_cpp import build_exe, run_exe

ROOT = Path(__file__).resolve().parents[1]
HALF_EXE = ROOT / "build" / "half_patterns"


def build_half_patterns() -> Path:
    return build_exe(ROOT / "tests/cpp/half_patterns.hip", HALF_EXE)


def test_half_program_builds():
    assert build_half_patterns().exists()


@pytest.mark.gpu
@pytest.mark.parametrize("npes", [2, 3, 5])
def test_half_cpp_and_device_forms(npes):
    run_exe(build_half_patterns(), npes, timeout=240)

"""Strided / blocked put / get through the C++ names, host and device (tests/cpp/strided_patterns.hip):
the reference ibput tester's pairs of calls, int_iput_device's shape and larger strided and blocked
shapes for six types and the five sized forms in six modes (host blocking, on-stream, work_group by a
block, by a 64-lane tile, single threads, a multi-workgroup kernel); the whole dest arena is compared."""
from pathlib import Path

import pytest

from tests.test_gpu_cpp import build_exe, run_exe

ROOT = Path(__file__).resolve().parents[1]
STRIDED_EXE = ROOT / "build" / "strided_patterns"


def test_strided_program_builds():
    assert build_exe(ROOT / "tests/cpp/strided_patterns.hip", STRIDED_EXE).exists()


@pytest.mark.gpu
@pytest.mark.parametrize("npes", [2, 3])
def test_cpp_reference_style_strided_tests(npes):
    run_exe(build_exe(ROOT / "tests/cpp/strided_patterns.hip", STRIDED_EXE), npes)

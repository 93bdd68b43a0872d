"""put / get through the C++ names, host and device (tests/cpp/rma_patterns.hip): the reference
tests' aligned sizes and offset sweep for six types, mem and the sized forms in seven modes (host
blocking, host _nbi + quiet, on-stream, work_group by a block, by a 64-lane tile, single threads, a
multi-workgroup kernel), p / g for all 23 typenames, and the in-kernel warm-cache hand-off."""
from pathlib import Path

import pytest

from tests.test_gpu_cpp import build_exe, run_exe

ROOT = Path(__file__).resolve().parents[1]
RMA_EXE = ROOT / "build" / "rma_patterns"


def test_rma_program_builds():
    assert build_exe(ROOT / "tests/cpp/rma_patterns.hip", RMA_EXE).exists()


@pytest.mark.gpu
@pytest.mark.parametrize("npes", [2, 3])
def test_cpp_reference_style_rma_tests(npes):
    run_exe(build_exe(ROOT / "tests/cpp/rma_patterns.hip", RMA_EXE), npes)

"""Device-initiated collectives on wide and strided teams (tests/cpp/device_teams.hip): the folds,
copies and barriers of include/ishmemx_device.h at team widths 2, 5 and 8 (a second, a partial and a
carried member batch), on teams with start != 0 and stride != 1, from non-members, at byte offsets
that take the element-wise arms as the whole body, with guard bytes round every dest; checked
bit-exactly against the oracle's fold in team order."""
from pathlib import Path

import pytest

from tests.test_gpu_cpp import build_exe, run_exe

ROOT = Path(__file__).resolve().parents[1]
TEAMS_EXE = ROOT / "build" / "device_teams"


def test_device_teams_program_builds():
    assert build_exe(ROOT / "tests/cpp/device_teams.hip", TEAMS_EXE).exists()


@pytest.mark.gpu
@pytest.mark.parametrize("npes", [2, 5, 8])
def test_device_collectives_on_wide_and_strided_teams(npes):
    run_exe(build_exe(ROOT / "tests/cpp/device_teams.hip", TEAMS_EXE), npes)

"""GPU tests of team epochs past 2^31, across the 32-bit wrap and one full period later
(tests/epoch_worker.py, model and tables in tests/epoch_cases.py).

The suite's collectives otherwise run at epochs of a few thousand.  Here a test hook of the
test-hooks library ages a team without running its launches, and every path and form then runs with
one member arriving 50 ms late, bit-exact against the oracle: a flag row, ring granule or claim word
that an old launch left behind and a new launch takes for its own lets the early members read the
late member's previous source.  2 and 3 PEs on one GPU, TEAM_WORLD and a split team that ages alone.
"""
import pytest

from tests import epoch_worker
from tests.test_gpu_topology import TESTHOOKS, run_pes

pytestmark = pytest.mark.gpu

ENV = {**TESTHOOKS, "ISHMEM_TIMEOUT_MS": 5000, "ISHMEM_SYMMETRIC_SIZE": "256M", "ISHMEM_STAGING_SIZE": "1M",
       "ISHMEM_STAGING_SLOTS": 2, "ISHMEM_MAX_BLOCKS": None, "ISHMEM_LL_MAX_BYTES": None,
       "ISHMEM_PHASED_MIN_BYTES": None, "ISHMEM_ONESHOT_P2_MAX_BYTES": None, "HSA_ENABLE_IPC_MODE_LEGACY": None}

NPES = [2, 3]


def run(npes: int, scenario: str) -> None:
    run_pes(npes, epoch_worker.run, (scenario,), ENV, timeout=180.0)


@pytest.mark.parametrize("npes", NPES)
def test_host_launch_count_bounds_the_epoch_advance_of_every_path_and_form(npes):
    run(npes, "counts")


@pytest.mark.parametrize("npes", NPES)
def test_every_path_waits_for_a_late_member_past_2_to_the_31_launches(npes):
    run(npes, "past31")


@pytest.mark.parametrize("npes", NPES)
def test_mixed_calls_across_the_epoch_wrap(npes):
    run(npes, "wrap")


@pytest.mark.parametrize("npes", NPES)
def test_granule_and_claim_words_one_full_period_later(npes):
    run(npes, "period")


@pytest.mark.parametrize("npes", NPES)
def test_refresh_every_seven_launches_under_mixed_calls_then_resync(npes):
    run(npes, "trigger")

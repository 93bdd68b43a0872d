"""The 16-bit floating-point reductions (half, bfloat16) across several PEs: scenario "half" of
tests/half_worker.py once per way of forcing a path, with the settings
tests/test_gpu_special_values.py uses for that path.  Every fold site must give the team-order fold
acc = x_0; acc = rn_T(f32(acc) OP f32(x_j)) of tests/half_model.py: rounded after every step, from
member 0's own value, never rotated for sum / prod (3 and 8 members are where a rotated fold
differs bitwise), with no flushed subnormal.
"""
import pytest

from tests import half_worker
from tests import staged_cases as sc
from tests.test_gpu_multi import LL_ENV, run_pes

pytestmark = pytest.mark.gpu

PERSISTENT = {"ISHMEM_LL_MAX_BYTES": 0, "ISHMEM_PHASED_MIN_BYTES": -1}
PHASED = {"ISHMEM_PHASED_MIN_BYTES": 0, "ISHMEM_LL_MAX_BYTES": 0, "ISHMEM_ONESHOT_P2_MAX_BYTES": 0}


def run_half(npes, scenarios, env=None, timeout=200):
    run_pes(npes, scenarios, env=env, timeout=timeout, worker=half_worker.run)


@pytest.mark.parametrize("npes", [2, 3, 4])
@pytest.mark.parametrize("ll", ["cap", "on"])
def test_half_granule_path(npes, ll):
    # The granule exchange (fold8: four 16-bit elements per item, two per granule word).
    run_half(npes, ["half"], env={"ISHMEM_LL_MAX_BYTES": LL_ENV[ll]})


def test_half_two_pe_persistent_rs_ag():
    run_half(2, ["half"], env={**PERSISTENT, "ISHMEM_ONESHOT_P2_MAX_BYTES": 0})


@pytest.mark.parametrize("npes", [3, 4])
@pytest.mark.parametrize("fold", ["whole_array", "persistent"])
def test_half_three_four_pes_no_granule_no_phased(npes, fold):
    # whole_array: the run-time team-size fold at 3 (team order for sum / prod), rs_tile<4> at 4;
    # persistent: the fold bound at 0 (nodirect).
    run_half(npes, ["half"] + (["nodirect"] if fold == "persistent" else []), env=PERSISTENT)


@pytest.mark.parametrize("npes", [3, 4])
def test_half_persistent_element_granular_shifted(npes):
    run_half(npes, ["half", "nodirect", "arshift0"], env=PERSISTENT)


@pytest.mark.parametrize("direct", ["on", "off"])
def test_half_two_pe_whole_array_fold(direct):
    run_half(2, ["half"] + (["nodirect"] if direct == "off" else []), env=PERSISTENT)


@pytest.mark.parametrize("npes", [2, 3, 4])
@pytest.mark.parametrize("shifted", ["unaligned_loads", "realigned"])
def test_half_phased_path(npes, shifted):
    # realigned: the realigning reduce-scatter kernel under a three-workgroup cap.
    run_half(npes, ["half"] + (["realigncap"] if shifted == "realigned" else []), env=PHASED)


@pytest.mark.parametrize("path", ["ll", "phased"])
def test_half_eight_pes(path):
    env = {"ISHMEM_LL_MAX_BYTES": 65536} if path == "ll" else PHASED
    run_half(8, ["half"], env={**env, "ISHMEM_MAX_BLOCKS": 8}, timeout=300)


def test_half_staged_pipeline_two_slots():
    # 1 MiB staging region, two slots: a bfloat16 sum and a half prod over 2 c + 3 elements of the
    # type's chunk, pageable buffers, 2 PEs.
    run_half(2, ["staged"], env={"ISHMEM_STAGING_SIZE": sc.STAGING, "ISHMEM_STAGING_SLOTS": 2,
                                 "STAGED_WANT_BYTES": sc.STAGING, "STAGED_WANT_SLOTS": 2,
                                 "ISHMEM_STAGED_COPY_KERNEL": None}, timeout=120)


@pytest.mark.parametrize("npes", [2, 3])
def test_half_scans_are_refused_on_every_pe(npes):
    # A sum scan with ids 16 / 17 returns non-zero on every PE before anything is launched; the
    # team's next reduce still pairs up.
    run_half(npes, ["refuse"], timeout=120)

"""NaN, infinities, signed zeros, overflow and subnormals through the multi-PE reduce (DESIGN.md
"Special values"): scenario "special" of tests/mp_worker.py, once per way of forcing a path, with
the settings tests/test_gpu_multi.py already uses for that path.  Every fold site loads member 0
and folds the rest in its own way; each must keep max / min = fmax / fmin, sum = +=, prod = *=
from member 0's own value, with no identity seed and no flushed subnormal.

The scenario runs float and double x max / min / sum / prod at n = 5, 1027 and 4099: out of place,
on a stream, in place (aligned and one element off the 16-B grid), on shifted 16-B phases with guard
bytes, on a strided team, on a team of one, from host buffers, and one in-place float case at
262,147 elements.
"""
import pytest

from tests.test_gpu_multi import LL_ENV, run_pes

pytestmark = pytest.mark.gpu

PERSISTENT = {"ISHMEM_LL_MAX_BYTES": 0, "ISHMEM_PHASED_MIN_BYTES": -1}
PHASED = {"ISHMEM_PHASED_MIN_BYTES": 0, "ISHMEM_LL_MAX_BYTES": 0, "ISHMEM_ONESHOT_P2_MAX_BYTES": 0}


@pytest.mark.parametrize("npes", [2, 3, 4])
@pytest.mark.parametrize("ll", ["cap", "on"])
def test_special_values_granule_path(npes, ll):
    # The granule exchange (fold8 per granule); cap: the default threshold, on: 64 KiB.
    run_pes(npes, ["special"], env={"ISHMEM_LL_MAX_BYTES": LL_ENV[ll]}, timeout=200)


def test_special_values_two_pe_persistent_rs_ag():
    # Two members on the persistent reduce-scatter + all-gather kernel (no one-shot fold).
    run_pes(2, ["special"], env={**PERSISTENT, "ISHMEM_ONESHOT_P2_MAX_BYTES": 0}, timeout=200)


@pytest.mark.parametrize("npes", [3, 4])
@pytest.mark.parametrize("fold", ["whole_array", "persistent"])
def test_special_values_three_four_pes_no_granule_no_phased(npes, fold):
    # whole_array: disjoint and in-place reduces take the whole-array fold (run-time team-size fold
    # at 3, rs_tile<4> at 4); persistent: the fold bound at 0 (nodirect), the persistent kernel.
    run_pes(npes, ["special"] + (["nodirect"] if fold == "persistent" else []), env=PERSISTENT, timeout=200)


@pytest.mark.parametrize("npes", [3, 4])
def test_special_values_persistent_element_granular_shifted(npes):
    # Sources on another 16-B phase than dest on the persistent kernel's element-granular
    # instantiation (ar_shifted 0).
    run_pes(npes, ["special", "nodirect", "arshift0"], env=PERSISTENT, timeout=200)


@pytest.mark.parametrize("direct", ["on", "off"])
def test_special_values_two_pe_whole_array_fold(direct):
    # on: barrier + one fold grid + barrier; off: the persistent kernel's one-shot mode.
    run_pes(2, ["special"] + (["nodirect"] if direct == "off" else []), env=PERSISTENT, timeout=200)


@pytest.mark.parametrize("npes", [2, 3, 4])
@pytest.mark.parametrize("shifted", ["unaligned_loads", "realigned"])
def test_special_values_phased_path(npes, shifted):
    # Barrier, reduce-scatter grid, barrier, all-gather.  Sources on another 16-B phase than dest:
    # unaligned 16-B loads (the default) or the realigning reduce-scatter kernel (realigncap:
    # phase_unaligned 0, at most three workgroups so its grid-stride loop runs too).
    run_pes(npes, ["special"] + (["realigncap"] if shifted == "realigned" else []), env=PHASED, timeout=200)


@pytest.mark.parametrize("path", ["ll", "phased"])
def test_special_values_eight_pes(path):
    # p = 8: 8-way granule rings and the register-staged rs_tile<8> (the 1 MiB in-place case), then
    # the phased path at P = 8; small grids so eight PEs' kernels stay resident on one GPU.
    env = {"ISHMEM_LL_MAX_BYTES": 65536} if path == "ll" else PHASED
    run_pes(8, ["special"], env={**env, "ISHMEM_MAX_BLOCKS": 8}, timeout=300)

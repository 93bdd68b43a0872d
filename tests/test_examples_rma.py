"""The reference's examples/2_get.cpp as a HIP program (examples/get.hip): its device call
`ishmem_int_g(&src[id], next_pe)` is unchanged.  Built on the CPU, run on the GPU."""
import pytest

from tests.test_examples import build_example, run_example


def test_get_example_builds():
    assert build_example("get").exists()


@pytest.mark.gpu
@pytest.mark.parametrize("npes", [2, 3])
def test_get_example(npes):
    outs = run_example(build_example("get"), npes)
    assert "successfully received the data using ISHMEM get" in outs[0]

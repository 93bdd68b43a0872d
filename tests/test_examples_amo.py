"""The reference's examples/3_library_apis.cpp with its whole test kernel as a HIP program
(examples/library_apis_amo.hip): the put / get ring, broadcast, ishmem_int32_atomic_fetch_add,
ishmem_int32_atomic_xor, reduce, every thread's ishmem_int_atomic_inc and the leader's
ishmem_int_wait_until, device calls unchanged.  Built on the CPU, run on the GPU."""
import pytest

from tests.test_examples import build_example, run_example


def test_library_apis_amo_example_builds():
    assert build_example("library_apis_amo").exists()


@pytest.mark.gpu
@pytest.mark.parametrize("npes", [2, 3])
def test_library_apis_amo_example(npes):
    outs = run_example(build_example("library_apis_amo"), npes)
    assert "SUCCESS - verified put/get/amo/broadcast/reduce/sync" in outs[0]

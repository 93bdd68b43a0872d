"""The local fan-in's block order (set_param "fanin_order": 1 ascending, 2 descending) and the rule
that picks it (0), on one PE.

The PE runs in a child process (tests/fanin_order_worker.py, which lists the cases), as the
multi-PE tests' PEs do: this module sorts before the co-located 8-PE tests, and a pytest process
that has opened the GPU itself (a context, a stream, a replayed graph) would stay on the device
beside their eight PEs.
"""
import pytest

from tests import fanin_order_worker
from tests.test_gpu_multi import run_pes

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("scenario", ["vector", "shifted"])
def test_results_are_bit_exact_in_both_orders(scenario):
    run_pes(1, [scenario], timeout=120, worker=fanin_order_worker.run)


def test_rule_on_launches():
    run_pes(1, ["rule"], timeout=120, worker=fanin_order_worker.run)

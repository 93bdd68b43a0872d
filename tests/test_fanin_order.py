"""The rule that picks a local fan-in's block order, as the pure function the runtime calls
(ishmemi_c_fanin_order through ishmem_amd.FaninOrder).  No GPU: the same sequences
tests/test_gpu_fanin_order.py runs against the library's launches."""
import ctypes

import ishmem_amd as ish

A, B, C, D = 0x10_0000, 0x20_0000, 0x30_0000, 0x40_0000  # disjoint 1 MiB apart
N = 16384


def test_first_forward_then_alternating_on_the_same_buffers():
    f = ish.FaninOrder()
    assert [f(A, [B], N) for _ in range(4)] == [0, 1, 0, 1]


def test_disjoint_buffers_run_forward_and_become_the_record():
    f = ish.FaninOrder()
    assert [f(A, [B], N), f(A, [B], N)] == [0, 1]
    assert f(C, [D], N) == 0
    assert f(C, [D], N) == 1
    assert f(A, [B], N) == 0  # only the last launch is remembered


def test_last_dest_as_the_new_source_flips():
    f = ish.FaninOrder()
    assert f(C, [D], N) == 0 and f(C, [D], N) == 1
    assert f(A, [C], N) == 0
    assert f(B + 64, [A], N) == 1
    assert f(D, [B], N) == 0  # B + 64 .. overlaps B ..
    assert f(C, [A, D + N - 1], N) == 1  # a partial overlap of any source
    assert f(C + N, [A + N, D + 2 * N], N) == 0  # adjacent ranges do not overlap


def test_capture_small_payloads_and_overlap_run_forward_and_leave_the_record():
    f = ish.FaninOrder()
    assert f(A, [B], N) == 0 and f(A, [B], N) == 1
    assert f(A, [B], N, capturing=True) == 0
    assert f(A, [B], N, min_bytes=N + 1) == 0
    assert f(A, [A + 16], N) == 0           # dest overlaps its source
    assert f(A, [A, B], N) == 0             # in place
    assert f(C, [D], N, capturing=True) == 0
    assert f(A, [B], N, min_bytes=N) == 0   # the record still says (A, B) ran descending


def test_another_stream_does_not_flip():
    f = ish.FaninOrder()
    assert f(A, [B], N, stream=0x100) == 0
    assert f(A, [B], N, stream=0x200) == 0
    assert f(A, [B], N, stream=0x200) == 1


def test_forced_orders():
    f = ish.FaninOrder()
    assert [f(A, [B], N, mode=1) for _ in range(2)] == [0, 0]
    assert [f(A, [B], N, mode=2) for _ in range(2)] == [1, 1]
    assert f(A, [B], N) == 0  # automatic again: the opposite of the last (forced) launch
    assert f(A, [B], N, mode=2, capturing=True) == 1 and f(A, [B], N) == 1  # forced, nothing learned


def test_argument_checks():
    L = ish.lib()
    rec = (ctypes.c_uint64 * 37)()
    r = (ctypes.c_uint64 * 4)(A, A + N, B, B + N)
    assert L.ishmemi_c_fanin_order(None, 0, 0, 0, None, r, 2, N) == -1
    assert L.ishmemi_c_fanin_order(ctypes.addressof(rec), 3, 0, 0, None, r, 2, N) == -1
    assert L.ishmemi_c_fanin_order(ctypes.addressof(rec), 0, 0, 0, None, r, 0, N) == -1
    assert L.ishmemi_c_fanin_order(ctypes.addressof(rec), 0, 0, 0, None, r, 18, N) == -1
    f = ish.FaninOrder()
    srcs = [B + 2 * N * j for j in range(16)]
    assert [f(A, srcs, N), f(A, srcs, N)] == [0, 1]  # dest + 16 sources fit the record


def test_parameters_without_a_gpu():
    assert ish.get_param("fanin_order") == 0
    bound = ish.get_param("fanin_order_min_bytes")
    assert bound > 0
    try:
        assert ish.set_param("fanin_order", 2) == 0 and ish.get_param("fanin_order") == 2
        assert ish.set_param("fanin_order", 3) != 0 and ish.get_param("fanin_order") == 2
        assert ish.set_param("fanin_order_min_bytes", 12345) == 0
        assert ish.get_param("fanin_order_min_bytes") == 12345
    finally:
        ish.set_param("fanin_order", 0)
        ish.set_param("fanin_order_min_bytes", bound)
    assert ish.get_param("last_fanin_order") in (0, 1)

"""The 16-bit floating-point fold on the GPU, one process, through the C ABI:
  * the local combine unit on EVERY pair (a, b) with a over all 65,536 encodings and b over the
    partner list of tests/half_model.py, per type and op, against the numpy model under its
    comparison rule (NaN matches NaN, mixed-sign zero extremes exempt, the rest bit-exact) — aligned
    (the 16-B vector kernel), with a source 2 and 14 bytes off dest's 16-B phase (the realigned
    kernel and, with dest itself off the grid, the head / tail elements), and with three sources
    (the run-time source count, folded in source order);
  * the 1-PE reduce: a bit-exact copy, signalling NaNs and payloads included.
"""
import numpy as np
import pytest

from tests import half_model as hm

pytestmark = pytest.mark.gpu

ARITH = ("max", "min", "sum", "prod")


@pytest.fixture(scope="module")
def ish():
    import ishmem_amd
    ishmem_amd.init(0, 1, 0, None)
    yield ishmem_amd
    ishmem_amd.ishmem_finalize()


@pytest.fixture(scope="module")
def pairs():
    """kind -> (a, b): all encodings tiled against the partner list (3.1 M elements, 6 MiB each)."""
    out = {}
    a = np.arange(1 << 16, dtype=np.uint16)
    for kind in hm.KINDS:
        b = hm.partners(kind)
        out[kind] = (np.tile(a, b.size), np.repeat(b, a.size))
    return out


@pytest.fixture(scope="module")
def bufs(ish):
    from ishmem_amd import hip
    nbytes = 48 * (1 << 16) * 2 + 256
    ptrs = [hip.malloc(nbytes) for _ in range(4)]
    yield ptrs
    for p in ptrs:
        hip.free(p)


def _check(kind, op, srcs, got):
    # every NaN and every exempt zero of these cases is counted by the model; the caps are for the
    # multi-PE tables (here a is EVERY encoding, NaNs included, by construction)
    fails = hm.compare(kind, op, srcs, got, caps=False)
    assert not fails, f"{kind} {op}: {fails[0]}"


@pytest.mark.parametrize("op", ARITH)
@pytest.mark.parametrize("kind", hm.KINDS)
def test_combine_every_pattern_against_the_partner_list(ish, pairs, bufs, kind, op):
    from ishmem_amd import hip
    a, b = pairs[kind]
    n = a.size
    pa, pb, pd, _ = bufs
    # (offset of a, of b, of dest) in bytes from a 16-B boundary
    for oa, ob, od in ((0, 0, 0), (2, 0, 0), (0, 14, 0), (2, 2, 2)):
        hip.upload(pa + oa, a)
        hip.upload(pb + ob, b)
        hip.memset(pd, 0xA5, n * 2 + 64)
        assert ish.combine(op, kind, pd + od, [pa + oa, pb + ob], n) == 0, ish.last_error()
        hip.synchronize()
        raw = hip.download(pd, n + 32, np.uint16)
        _check(kind, op, [a, b], raw[od // 2:od // 2 + n].copy())
        assert (raw[:od // 2] == 0xA5A5).all() and (raw[od // 2 + n:] == 0xA5A5).all(), (kind, op, oa, ob, od)


@pytest.mark.parametrize("op", ARITH)
@pytest.mark.parametrize("kind", hm.KINDS)
def test_combine_three_sources_fold_in_source_order(ish, pairs, bufs, kind, op):
    from ishmem_amd import hip
    a, b = pairs[kind]
    n = 8 << 16  # every encoding against eight partners
    a, b = a[:n], b[16 * (1 << 16):16 * (1 << 16) + n]  # the ulp fractions and neighbours of the list
    c = np.roll(b, 1 << 16)
    pa, pb, pd, pc = bufs
    for x, p in ((a, pa), (b, pb), (c, pc)):
        hip.upload(p, x)
    assert ish.combine(op, kind, pd, [pa, pb, pc], n) == 0, ish.last_error()
    hip.synchronize()
    _check(kind, op, [a, b, c], hip.download(pd, n, np.uint16))
    if op in ("sum", "prod"):  # the order matters on these inputs, so a rotated fold would show
        assert (hm.fold(kind, op, [b, c, a]) != hm.fold(kind, op, [a, b, c])).any()


@pytest.mark.parametrize("kind", hm.KINDS)
def test_one_pe_reduce_is_a_bit_exact_copy(ish, bufs, kind):
    from ishmem_amd import hip
    for n in (1, 7, 8, 9, 4099):
        x = hm.copy_source(kind, n)
        s, d = ish.ishmem_malloc(n * 2 + 32), ish.ishmem_malloc(n * 2 + 64)
        for off in (0, 2):
            for op in ARITH:
                hip.upload(s + off, x)
                hip.memset(d, 0xA5, n * 2 + 64)
                assert ish.reduce(op, kind, d + 16 + off, s + off, n) == 0, ish.last_error()
                raw = hip.download(d, n + 32, np.uint16)
                lo = 8 + off // 2
                assert np.array_equal(raw[lo:lo + n], x), (kind, op, n, off)
                assert (raw[:lo] == 0xA5A5).all() and (raw[lo + n:] == 0xA5A5).all(), (kind, op, n, off)
        # in place, and from a pageable host buffer through the staging pipeline
        hip.upload(s, x)
        assert getattr(ish, f"ishmemx_{kind}_sum_reduce")(s, s, n) == 0, ish.last_error()
        assert np.array_equal(hip.download(s, n, np.uint16), x)
        h = np.zeros(n, np.uint16)
        assert ish.reduce("max", kind, h.ctypes.data, x.ctypes.data, n) == 0, ish.last_error()
        assert np.array_equal(h, x)
        ish.ishmem_free(d)
        ish.ishmem_free(s)


def test_bitwise_ops_and_scans_are_refused(ish):
    s = ish.ishmem_malloc(64)
    for kind in hm.KINDS:
        for op in ("and", "or", "xor"):
            assert ish.reduce(op, kind, s, s, 4) != 0 and "invalid (op, dtype)" in ish.last_error()
            assert ish.combine(op, kind, s, [s, s], 4) != 0 and "invalid (op, dtype)" in ish.last_error()
        assert ish.scan(kind, True, s, s, 4) != 0 and "invalid dtype" in ish.last_error()
    ish.ishmem_free(s)

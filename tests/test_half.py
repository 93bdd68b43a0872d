"""The 16-bit floating-point reductions without a GPU: the C ABI's ids, sizes and validity matrix,
the refusal of the ids by every entry that is not a reduction, the Python and C++ names, the numpy
model of the contract (tests/half_model.py) pinned against numpy's float16 and torch's CPU bfloat16
arithmetic on every bit pattern, and the coverage and caps of the 16-bit special table."""
import ctypes
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import ishmem_amd as ish
from tests import half_model as hm

ROOT = Path(__file__).resolve().parents[1]
INCLUDE = ROOT / "include"
HALF, BF16 = 16, 17
ARITH = ("max", "min", "sum", "prod")


# ---- ABI ----------------------------------------------------------------------------------------
def test_ids_sizes_and_validity_matrix():
    L = ish.lib()
    L.ishmemi_c_dtype_size.restype = ctypes.c_size_t
    assert ish.DTYPES["half"] == HALF and ish.DTYPES["bfloat16"] == BF16
    assert hm.DTYPE_ID == {"half": HALF, "bfloat16": BF16}
    text = (INCLUDE / "ishmem_capi.h").read_text()
    assert "ISHMEMI_DT_HALF = 16" in text and "ISHMEMI_DT_BFLOAT16 = 17" in text and "ISHMEMI_DT_COUNT = 10" in text
    assert L.ishmemi_c_dtype_size(HALF) == 2 and L.ishmemi_c_dtype_size(BF16) == 2
    for dt in [-1, *range(10, 16), 18, 19, 32, 255, 1 << 20]:
        assert L.ishmemi_c_dtype_size(dt) == 0, dt
    for op, code in ish.OPS.items():
        for dt in (HALF, BF16):
            assert L.ishmemi_c_op_dtype_valid(code, dt) == (1 if op in ARITH else 0), (op, dt)
        for dt in [-1, *range(10, 16), 18]:
            assert L.ishmemi_c_op_dtype_valid(code, dt) == 0, (op, dt)
    for dt in (HALF, BF16):
        assert L.ishmemi_c_op_dtype_valid(-1, dt) == 0 and L.ishmemi_c_op_dtype_valid(7, dt) == 0
    # the ten types keep their matrix
    for name, dt in ish.DTYPES.items():
        if dt < 10:
            for op, code in ish.OPS.items():
                want = 0 if name in ("float", "double") and op in ("and", "or", "xor") else 1
                assert L.ishmemi_c_op_dtype_valid(code, dt) == want, (op, name)


def test_every_entry_that_is_not_a_reduction_refuses_the_ids():
    assert not ish.initialized()
    L = ish.lib()
    v, r, f, z = ctypes.c_uint64(0), ctypes.c_int(0), ctypes.c_uint64(0), ctypes.c_size_t(0)
    EQ = ish.ISHMEM_CMP_EQ
    for dt in (HALF, BF16):
        calls = {
            "scan": lambda: L.ishmemi_c_scan(0, dt, 1, None, None, 4),
            "scan_on_stream": lambda: L.ishmemi_c_scan_on_stream(0, dt, 0, None, None, 4, None, None),
            "amo": lambda: L.ishmemi_c_amo(ish.AMO_OPS["fetch"], dt, None, 1, 0, 0, ctypes.byref(f)),
            "amo_nbi": lambda: L.ishmemi_c_amo_nbi(ish.AMO_OPS["swap"], dt, None, None, 1, 0, 0),
            "wait_until": lambda: L.ishmemi_c_wait_until(None, dt, EQ, 1, ctypes.byref(v)),
            "wait_until_on_stream": lambda: L.ishmemi_c_wait_until_on_stream(None, dt, EQ, 1, None, None, None),
            "test": lambda: L.ishmemi_c_test(None, dt, EQ, 1, ctypes.byref(r)),
            "sync_vector": lambda: L.ishmemi_c_sync_vector(0, dt, None, 4, None, None, EQ, 1, None, ctypes.byref(z)),
            "sync_vector_on_stream": lambda: L.ishmemi_c_sync_vector_on_stream(0, dt, None, 4, None, None, EQ, 1, None,
                                                                                None, None, None),
        }
        for name, call in calls.items():
            assert call() != 0, (name, dt)
            assert ish.last_error(), (name, dt)
    # ... and the reductions do not refuse the pair: before init they fail for that reason instead
    for dt in (HALF, BF16):
        assert L.ishmemi_c_reduce(0, ish.OPS["sum"], dt, None, None, 4) != 0
        assert "initialized" in ish.last_error()
        assert L.ishmemi_c_combine(ish.OPS["and"], dt, None, None, 2, 4, None) != 0
        assert "invalid (op, dtype)" in ish.last_error()


def test_scans_keep_their_own_dtype_check():
    src = (ROOT / "ishmem_amd" / "csrc" / "runtime.cpp").read_text()
    assert "op_dtype_valid(ISHMEMI_OP_SUM" not in src  # scans would start accepting ids 16 / 17
    assert src.count("scan_dtype_valid(") >= 2


# ---- names --------------------------------------------------------------------------------------
def _names():
    host = [f"ishmemx_{t}_{op}_reduce" for t in hm.KINDS for op in ARITH]
    return host, [n + "_on_stream" for n in host]


def test_python_names():
    host, on_stream = _names()
    # 2 types x 4 ops, each with and without a team argument: 16 host and 16 on-stream call forms
    assert len(host) == 8 and len(on_stream) == 8
    assert sorted(ish.HALF_NAMES) == sorted(host + on_stream)
    for n in host + on_stream:
        assert callable(getattr(ish, n)), n
        for older in (ish.API_NAMES, ish.SIGNAL_NAMES, ish.RMA_NAMES, ish.STRIDED_NAMES, ish.SYNC_VECTOR_NAMES,
                      ish.AMO_NAMES):
            assert n not in older, n
    assert not ish.initialized()
    for n in host:
        assert getattr(ish, n)(0, 0, 4) != 0 and getattr(ish, n)(ish.ISHMEM_TEAM_WORLD, 0, 0, 4) != 0
        with pytest.raises(TypeError):
            getattr(ish, n)(0, 0)
    for n in on_stream:
        assert getattr(ish, n)(0, 0, 4, 0, 0) != 0 and getattr(ish, n)(ish.ISHMEM_TEAM_WORLD, 0, 0, 4, 0, 0) != 0
    assert ish.reduce("sum", "bfloat16", 0, 0, 4) != 0 and ish.reduce_on_stream("max", "half", 0, 0, 4, 0, 0) != 0


CXX = r"""
#include "ishmemx.h"
static_assert(sizeof(ishmemx_half_t) == 2 && sizeof(ishmemx_bfloat16_t) == 2, "2-byte types");
static_assert(ishmemi_cxx::dtype_of<ishmemx_half_t>() == 16 && ishmemi_cxx::dtype_of<ishmemx_bfloat16_t>() == 17, "ids");
static_assert(ishmemi_cxx::dtype_of<float>() == 8 && ishmemi_cxx::dtype_of<unsigned short>() == 5, "old ids");
template <typename T> int all(T *d, const T *s, hipStream_t st, int *ret, hipEvent_t ev)
{
    int r = 0;
#define ONE(TN, OP) \
    r += ishmemx_##TN##_##OP##_reduce(d, s, 4) + ishmemx_##TN##_##OP##_reduce(ISHMEM_TEAM_WORLD, d, s, 4) + \
         ishmemx_##TN##_##OP##_reduce_on_stream(d, s, 4, ret, st) + \
         ishmemx_##TN##_##OP##_reduce_on_stream(ISHMEM_TEAM_WORLD, d, s, 4, ret, st) + \
         ishmemx_##TN##_##OP##_reduce_on_stream(d, s, 4, ret, st, &ev, 1, ev) + \
         ishmemx_##TN##_##OP##_reduce_on_stream(ISHMEM_TEAM_WORLD, d, s, 4, ret, st, &ev, 1, ev) + \
         ishmem_##OP##_reduce(d, s, 4) + ishmemx_##OP##_reduce_on_stream(ISHMEM_TEAM_WORLD, d, s, 4, ret, st);
#define FOUR(TN) ONE(TN, max) ONE(TN, min) ONE(TN, sum) ONE(TN, prod)
    if constexpr (sizeof(T) == 2 && ishmemi_cxx::fp16_kind<T>() == 1) { FOUR(half) }
    else { FOUR(bfloat16) }
    return r;
}
int main()
{
    ishmemx_half_t h[4] = {};
    ishmemx_bfloat16_t b[4] = {};
    /* not initialised: every call fails, none crashes */
    const int r = all(h, h, nullptr, nullptr, nullptr) + all(b, b, nullptr, nullptr, nullptr);
    return r == 2 * 4 * 8 ? 0 : 1;
}
"""


def test_host_names_compile_as_plain_cxx_and_fail_cleanly_before_init(tmp_path):
    gxx = shutil.which("g++") or shutil.which("c++")
    if gxx is None:
        pytest.skip("no host C++ compiler")
    src = tmp_path / "half_names.cpp"
    src.write_text(CXX)
    exe = tmp_path / "half_names"
    subprocess.run([gxx, "-std=c++17", "-Wall", "-Werror", f"-I{INCLUDE}", str(src), "-o", str(exe),
                    f"-L{ROOT / 'ishmem_amd'}", "-lishmem_amd", f"-Wl,-rpath,{ROOT / 'ishmem_amd'}"], check=True)
    assert subprocess.run([str(exe)]).returncode == 0


# ---- the model, pinned independently --------------------------------------------------------------
def _pairs(kind):
    a = np.arange(1 << 16, dtype=np.uint16)
    b = hm.partners(kind)
    return np.tile(a, b.size), np.repeat(b, a.size)


def _same(kind, op, a, b, want, got):
    """uint16 views equal, NaN payloads aside, mixed-sign zero extremes aside.  Signalling NaNs
    entering an op are outside the contract (numpy's and torch's fmax / fmin return the NaN quieted
    where the model, like fmaxf under the default environment, may return the other operand)."""
    quiet = (hm.QNAN[kind] & ~hm.INF[kind]) & 0xFFFF
    snan = (hm.isnan(kind, a) & ((a & quiet) == 0)) | (hm.isnan(kind, b) & ((b & quiet) == 0))
    assert 0 < snan.sum() < 0.02 * a.size
    nan = hm.isnan(kind, want)
    ex = hm.zero_exempt(kind, op, [a, b], want)
    ok = snan | np.where(nan, hm.isnan(kind, got), np.where(ex, hm.iszero(got), want == got))
    bad = np.nonzero(~ok)[0]
    assert bad.size == 0, (f"{kind} {op}: {bad.size} differ, first a={int(a[bad[0]]):#06x} b={int(b[bad[0]]):#06x} "
                           f"model {int(want[bad[0]]):#06x} other {int(got[bad[0]]):#06x}")


def test_partner_list():
    for kind in hm.KINDS:
        b = hm.partners(kind)
        assert b.size == 48 and len(set(b.tolist())) == 48
        for need in (0x0000, 0x8000, 0x0001, 0x8001, hm.INF[kind], hm.INF[kind] | 0x8000, hm.QNAN[kind],
                     hm.INF[kind] - 1, hm.enc(kind, 1.0), hm.enc(kind, -1.0)):
            assert need in b.tolist(), (kind, hex(need))


@pytest.mark.parametrize("op", ARITH)
def test_model_equals_numpy_float16_on_every_pattern(op):
    a, b = _pairs("half")
    x, y = a.view(np.float16), b.view(np.float16)
    with np.errstate(all="ignore"):
        other = {"max": np.fmax, "min": np.fmin, "sum": np.add, "prod": np.multiply}[op](x, y)
    assert other.dtype == np.float16
    _same("half", op, a, b, hm.binop("half", op, a, b), other.view(np.uint16))


@pytest.mark.parametrize("op", ARITH)
def test_model_equals_torch_cpu_bfloat16_on_every_pattern(op):
    torch = pytest.importorskip("torch")
    a, b = _pairs("bfloat16")
    x = torch.from_numpy(a.view(np.int16).copy()).view(torch.bfloat16)
    y = torch.from_numpy(b.view(np.int16).copy()).view(torch.bfloat16)
    other = {"max": torch.fmax, "min": torch.fmin, "sum": torch.add, "prod": torch.mul}[op](x, y)
    assert other.dtype == torch.bfloat16
    _same("bfloat16", op, a, b, hm.binop("bfloat16", op, a, b), other.view(torch.int16).numpy().view(np.uint16))


def test_widen_narrow_round_trip_and_known_roundings():
    for kind in hm.KINDS:
        a = np.arange(1 << 16, dtype=np.uint16)
        back = hm.narrow(kind, hm.widen(kind, a))
        nan = hm.isnan(kind, a)
        assert np.array_equal(back[~nan], a[~nan]) and hm.isnan(kind, back[nan]).all()
    e = hm.enc
    # hand-derived: ties to even both ways, overflow by rounding, the largest finite kept
    assert hm.binop("half", "sum", [0x3C00], [0x1000])[0] == 0x3C00        # 1 + 2^-11 -> 1
    assert hm.binop("half", "sum", [0x3C01], [0x1000])[0] == 0x3C02        # 1 + 2^-10 + 2^-11 -> 1 + 2^-9
    assert hm.binop("half", "sum", [0x7BFF], [0x4C00])[0] == 0x7C00        # 65504 + 16 -> inf
    assert hm.binop("half", "sum", [0x7BFF], [0x4800])[0] == 0x7BFF        # 65504 + 8 -> 65504
    assert hm.binop("half", "sum", [0x03FF], [0x0001])[0] == 0x0400        # subnormals add exactly
    assert hm.binop("half", "prod", [0x0001], [0x3800])[0] == 0x0000       # 2^-24 / 2: tie to even, zero
    assert hm.binop("half", "prod", [0x0003], [0x3800])[0] == 0x0002       # 1.5 x 2^-24: tie to even, up
    assert hm.binop("bfloat16", "sum", [0x3F80], [0x3B80])[0] == 0x3F80    # 1 + 2^-8 -> 1
    assert hm.binop("bfloat16", "sum", [0x3F81], [0x3B80])[0] == 0x3F82    # 1 + 2^-7 + 2^-8 -> 1 + 2^-6
    assert hm.binop("bfloat16", "sum", [0x7F7F], [0x7B00])[0] == 0x7F80    # max + half an ulp -> inf
    assert hm.binop("bfloat16", "sum", [0x7F7F], [0x7A80])[0] == 0x7F7F    # max + a quarter ulp -> max
    assert hm.binop("bfloat16", "sum", [0x8000], [0x8000])[0] == 0x8000    # -0 + -0
    assert hm.isnan("bfloat16", hm.binop("bfloat16", "sum", [0x7F80], [0xFF80]))[0]
    assert hm.binop("bfloat16", "max", [0x7FC0], [0x3F80])[0] == 0x3F80    # NaN is missing data
    assert e("half", 1.0) == 0x3C00 and e("bfloat16", 1.0) == 0x3F80 and e("half", 65504.0) == 0x7BFF
    # a fold is the ops in team order, rounded every step: (1 + u/2) + u/2 stays 1, u/2 + u/2 + 1 does not
    u2, one = e("half", 2.0 ** -11), e("half", 1.0)
    assert hm.fold("half", "sum", [np.array([one], np.uint16), np.array([u2], np.uint16), np.array([u2], np.uint16)])[0] == one
    assert hm.fold("half", "sum", [np.array([u2], np.uint16), np.array([u2], np.uint16), np.array([one], np.uint16)])[0] == one + 1


# ---- table coverage and caps ------------------------------------------------------------------------
SIZES = (1, 7, 8, 9, 1027, 4099)


@pytest.mark.parametrize("kind", hm.KINDS)
def test_table_rows_produce_what_their_names_say(kind):
    def result(op, name, p=2):
        rows = hm.table(kind, op)
        i = [r[0] for r in rows].index(name)
        srcs = hm.sources(kind, op, p, len(rows), 0)
        return int(hm.fold(kind, op, srcs)[i]), rows[i]
    c, e = hm.consts(kind), lambda v: hm.enc(kind, v)
    u = c["ulp"]
    assert result("sum", "tie rounded down")[0] == e(1.0)
    assert result("sum", "tie rounded up")[0] == e(1 + 2 * u)
    assert result("sum", "overflow by rounding")[0] == hm.INF[kind]
    assert result("sum", "finite just below overflow")[0] == e(c["max"])
    assert result("sum", "subnormal in, subnormal out")[0] == e(4 * c["sub"])
    assert result("sum", "largest subnormal + smallest = smallest normal")[0] == e(c["tiny"])
    assert hm.isnan(kind, np.array([result("sum", "inf - inf")[0]], np.uint16))[0]
    assert result("sum", "all -0")[0] == 0x8000
    assert result("sum", "all -0", 3)[0] == 0x8000
    assert result("prod", "tie rounded down")[0] == e(1.5 + 4 * u)
    assert result("prod", "tie rounded up")[0] == e(1.5 + 2 * u)
    assert result("prod", "overflow")[0] == hm.INF[kind]
    assert result("prod", "normal to subnormal")[0] == e(c["tiny"] / 2)
    assert result("prod", "subnormal tie to even (up)")[0] == e(2 * c["sub"])
    assert result("prod", "subnormal tie to even (zero)")[0] == 0
    assert hm.isnan(kind, np.array([result("prod", "inf x 0")[0]], np.uint16))[0]
    assert result("max", "NaN is missing data")[0] == e(1.0) and result("min", "NaN is missing data")[0] == e(1.0)
    assert result("max", "subnormal against zero")[0] == e(c["sub"])
    assert result("min", "negative subnormal against zero")[0] == e(c["sub"]) | 0x8000
    if kind == "bfloat16":
        got, row = result("prod", "product in the float32 subnormal range")
        x = float(hm.widen(kind, [row[1]])[0]) * float(hm.widen(kind, [row[2]])[0])  # exact in double
        assert 0 < x < 2.0 ** -126 and got == int(hm.narrow(kind, np.array([np.float32(x)]))[0])
        got, row = result("prod", "product rounded in float32 first")
        x = float(hm.widen(kind, [row[1]])[0]) * float(hm.widen(kind, [row[2]])[0])
        assert 0 < x < 2.0 ** -126 and float(np.float32(x)) != x  # the float32 product itself rounds


@pytest.mark.parametrize("kind", hm.KINDS)
@pytest.mark.parametrize("op", ARITH)
def test_table_meets_every_lane_and_every_member_and_stays_under_the_caps(kind, op):
    rows = hm.table(kind, op)
    R = len(rows)
    assert R % 2 == 1
    for p in (2, 3, 4, 8):
        n = 4099
        i = np.arange(n)
        in_table, rowi, rot = hm.layout(R, p, n)
        for row in range(R):
            sel = in_table & (rowi == row)
            assert set((i[sel] % 8).tolist()) == set(range(8)), (row, p)       # every lane of a 16-B item
            assert set(rot[sel].tolist()) == set(range(p)), (row, p)            # the special entry on every member
        for n in SIZES + (262_147,):
            srcs = hm.sources(kind, op, p, n)
            assert all(s.dtype == np.uint16 and s.size == n for s in srcs)
            stats = {}
            ref = hm.fold(kind, op, srcs)
            assert hm.compare_ref(kind, op, srcs, ref, ref, stats) == [], (p, n)
            assert stats["nan"] <= hm.NAN_CAP * n and stats["zero_exempt"] <= hm.ZERO_CAP * n, (p, n, stats)
            if n >= 1027:
                assert stats["nan"] > 0
                assert (op in ("max", "min")) == (stats["zero_exempt"] > 0)
        # a rotated sum / prod fold differs from the team-order one somewhere at 3 and 8 members:
        # the table and the random values can tell the two apart
        if op in ("sum", "prod") and p in (3, 8):
            srcs = hm.sources(kind, op, p, 4099)
            rotated = hm.fold(kind, op, srcs[1:] + srcs[:1])
            assert (rotated != hm.fold(kind, op, srcs)).any()


def test_compare_rule():
    kind = "bfloat16"
    srcs = hm.sources(kind, "max", 3, 1027)
    ref = hm.fold(kind, "max", srcs)
    got = ref.copy()
    nan = np.nonzero(hm.isnan(kind, ref))[0]
    ex = np.nonzero(hm.zero_exempt(kind, "max", srcs, ref))[0]
    assert nan.size and ex.size
    got[nan[0]] = 0xFFC1          # another NaN: fine
    got[ex[0]] ^= 0x8000          # the other zero: fine
    assert hm.compare(kind, "max", srcs, got) == []
    got[nan[0]] = 0x7F80          # infinity where a NaN belongs
    assert len(hm.compare(kind, "max", srcs, got)) == 1
    got = ref.copy()
    plain = np.nonzero(~hm.isnan(kind, ref) & ~hm.zero_exempt(kind, "max", srcs, ref))[0]
    got[plain[3]] ^= 1
    assert "1 of 1027" in hm.compare(kind, "max", srcs, got)[0]
    assert hm.compare(kind, "sum", srcs, np.full(1027, 0x7FC0, np.uint16))  # NaN everywhere cannot pass
    assert hm.compare(kind, "max", srcs, ref.astype(np.int16))              # wrong type

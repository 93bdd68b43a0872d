"""put_signal, signal operations and wait_until / test without a GPU: the C ABI before init, the Python
names, the host C++ names (g++, linked against the library), the device API (hipcc, gfx950, compile
only), the comparison helper of the GPU worker and the threshold's environment variable."""
import ctypes
import re
import shutil
import subprocess
import sys
from pathlib import Path

import pytest

import ishmem_amd as ish
from ishmem_amd import _lib
from tests.signal_worker import EQ, GE, GT, LE, LT, NE, SYNC_TYPES, cmp_holds, flip_case
from tests.test_launcher import ENV_PROBE, clean_env

ROOT = Path(__file__).resolve().parents[1]
INCLUDE = ROOT / "include"

C_NAMES = ["ishmemi_c_put_signal", "ishmemi_c_put_signal_nbi", "ishmemi_c_put_signal_on_stream", "ishmemi_c_signal_op",
           "ishmemi_c_signal_fetch", "ishmemi_c_wait_until", "ishmemi_c_test", "ishmemi_c_wait_until_on_stream"]


def test_not_initialised_calls_fail_with_a_reason():
    assert not ish.initialized()
    L = ish.lib()
    v, r = ctypes.c_uint64(0), ctypes.c_int(0)
    calls = {
        "ishmemi_c_put_signal": lambda f: f(None, None, 8, None, 1, 0, 0),
        "ishmemi_c_put_signal_nbi": lambda f: f(None, None, 0, None, 1, 0, 0),  # nbytes == 0 is no success either
        "ishmemi_c_put_signal_on_stream": lambda f: f(None, None, 8, None, 1, 0, 0, None),
        "ishmemi_c_signal_op": lambda f: f(None, 1, 1, 0),
        "ishmemi_c_signal_fetch": lambda f: f(None, ctypes.byref(v)),
        "ishmemi_c_wait_until": lambda f: f(None, ish.DTYPES["uint64"], EQ, 1, ctypes.byref(v)),
        "ishmemi_c_test": lambda f: f(None, ish.DTYPES["int32"], NE, 1, ctypes.byref(r)),
        "ishmemi_c_wait_until_on_stream": lambda f: f(None, ish.DTYPES["int64"], GT, 1, None, None, None),
    }
    assert sorted(calls) == sorted(C_NAMES)
    for name, call in calls.items():
        assert call(getattr(L, name)) != 0, name
        assert "not initialized" in ish.last_error(), name
    for call in (lambda: ish.ishmem_putmem_signal(0, 0, 8, 0, 1, 0, 0), lambda: ish.ishmem_putmem_signal_nbi(0, 0, 8, 0, 1, 0, 0),
                 lambda: ish.put_signal_on_stream(0, 0, 8, 0, 1, 0, 0, 0), lambda: ish.ishmemx_signal_set(0, 1, 0),
                 lambda: ish.ishmemx_signal_add(0, 1, 0), lambda: ish.signal_fetch(0)[0],
                 lambda: ish.wait_until(0, "uint64", EQ, 1)[0], lambda: ish.test(0, "int32", EQ, 1)[0],
                 lambda: ish.wait_until_on_stream(0, "uint64", EQ, 1, 0, 0, 0),
                 lambda: ish.signal_wait_until_on_stream(0, EQ, 1, 0, 0), lambda: ish.ishmem_int_wait_until(0, EQ, 1)):
        assert call() != 0
        assert "not initialized" in ish.last_error()
    assert ish.ishmem_signal_fetch(0) == 0 and ish.ishmem_signal_wait_until(0, EQ, 1) == 0
    assert ish.ishmem_uint64_test(0, EQ, 1) == 0


def test_python_names_exist_for_every_typename():
    want = ["ishmem_putmem_signal", "ishmem_putmem_signal_nbi", "ishmem_signal_fetch", "ishmem_signal_wait_until",
            "ishmemx_signal_set", "ishmemx_signal_add"]
    assert len(ish.ARITH_TYPENAMES) == 23 and len(ish.SYNC_TYPENAMES) == 12
    assert sorted(ish.SYNC_TYPENAMES) == sorted(SYNC_TYPES)
    for tn in ish.ARITH_TYPENAMES:
        want += [f"ishmem_{tn}_put_signal", f"ishmem_{tn}_put_signal_nbi"]
    for bits in (8, 16, 32, 64, 128):
        want += [f"ishmem_put{bits}_signal", f"ishmem_put{bits}_signal_nbi"]
    for tn in ish.SYNC_TYPENAMES:
        want += [f"ishmem_{tn}_wait_until", f"ishmem_{tn}_test"]
        assert ish.TYPENAMES[tn] == ("" if SYNC_TYPES[tn][1] else "u") + f"int{SYNC_TYPES[tn][0]}"
    assert sorted(want) == sorted(ish.SIGNAL_NAMES)
    for name in want:
        fn = getattr(ish, name)
        assert fn.__name__ == name
    assert ish.ishmem_float_put_signal(0, 0, 1, 0, 1, 0, 0) != 0  # not initialised
    assert not set(ish.SIGNAL_NAMES) & set(ish.API_NAMES)
    for name in ("put_signal_on_stream", "wait_until_on_stream", "signal_wait_until_on_stream", "wait_until", "test",
                 "signal_fetch"):
        assert callable(getattr(ish, name))
    assert (ish.ISHMEM_CMP_EQ, ish.ISHMEM_CMP_NE, ish.ISHMEM_CMP_GT, ish.ISHMEM_CMP_GE, ish.ISHMEM_CMP_LT,
            ish.ISHMEM_CMP_LE) == (1, 2, 3, 4, 5, 6)
    assert (ish.ISHMEM_SIGNAL_SET, ish.ISHMEM_SIGNAL_ADD) == (0, 1)
    names = [p[0] for p in _lib.PROTOTYPES]
    assert all(n in names for n in C_NAMES)
    header = (INCLUDE / "ishmem_capi.h").read_text()
    assert all(f"{n}(" in header for n in C_NAMES)


def test_comparison_helper():
    # int32 -1 against 0, versus uint32 0xFFFFFFFF against 0 (the same bits).
    signed = {EQ: False, NE: True, GT: False, GE: False, LT: True, LE: True}
    unsigned = {EQ: False, NE: True, GT: True, GE: True, LT: False, LE: False}
    for cmp in (EQ, NE, GT, GE, LT, LE):
        assert cmp_holds(-1, cmp, 0, 32, True) == signed[cmp]
        assert cmp_holds(0xFFFFFFFF, cmp, 0, 32, True) == signed[cmp]
        assert cmp_holds(0xFFFFFFFF, cmp, 0, 32, False) == unsigned[cmp]
        assert cmp_holds(-1, cmp, 0, 32, False) == unsigned[cmp]
    # int64 / uint64 values that differ only above bit 32.
    a, b = 7, 7 + (1 << 32)
    less = {EQ: False, NE: True, GT: False, GE: False, LT: True, LE: True}
    for cmp in (EQ, NE, GT, GE, LT, LE):
        for sg in (True, False):
            assert cmp_holds(a, cmp, b, 64, sg) == less[cmp]
            assert cmp_holds(a, cmp, b, 32, sg) == (cmp in (EQ, GE, LE))  # what a 32-bit comparison would say
    # the top bit of a 64-bit value: negative when signed
    assert cmp_holds(7 + (1 << 63), GT, 7, 64, False) and cmp_holds(7 + (1 << 63), LT, 7, 64, True)
    # every flip case of the GPU test: false before, true after, in the variable's own type
    for bits, sg in set(SYNC_TYPES.values()):
        for cmp in (EQ, NE, GT, GE, LT, LE):
            before, cval, after = flip_case(bits, sg, cmp)
            assert not cmp_holds(before, cmp, cval, bits, sg) and cmp_holds(after, cmp, cval, bits, sg)
    # ... and the cases where the wrong signedness or the low half alone would answer differently
    assert cmp_holds(flip_case(32, True, GE)[0], GE, 0, 32, False)
    assert not cmp_holds(flip_case(32, False, GT)[2], GT, 0x7FFFFFFF, 32, True)
    assert not cmp_holds(flip_case(64, False, NE)[2], NE, flip_case(64, False, NE)[1], 32, False)


@pytest.mark.parametrize("value,bad", [("64K", False), (" 4MiB ", False), ("0", False), ("65536", False),
                                       ("64KQ", True), ("lots", True), ("16MB x", True)])
def test_fused_threshold_variable_parses_strictly(value, bad):
    out = subprocess.run([sys.executable, "-c", ENV_PROBE, str(ROOT)],
                         env=clean_env(ISHMEM_PUT_SIGNAL_FUSED_MAX_BYTES=value), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    line = out.stdout.strip().splitlines()[-1]
    if bad:
        assert line.startswith("rc=1|") and "ISHMEM_PUT_SIGNAL_FUSED_MAX_BYTES" in line, line
    else:
        assert "ISHMEM_PUT_SIGNAL_FUSED_MAX_BYTES" not in line, line
    assert "not a supported variable" not in out.stderr


def test_fused_threshold_parameter():
    assert ish.get_param("put_signal_fused_max_bytes") > 0
    assert ish.get_param("put_signal_fused_max_bytes") <= 4 << 20


HOST_CXX = r'''
#include <ishmem.h>
#include <ishmemx.h>
#include <cstdio>
#include <cstring>
static int bad = 0, n = 0;
static void expect_reason(const char *what) {
    ++n;
    if (!std::strstr(ishmemi_c_last_error(), "not initialized")) { ++bad; std::printf("%s: %s\n", what, ishmemi_c_last_error()); }
}
#define V(call) do { call; expect_reason(#call); } while (0)
#define I(call) do { if ((call) == 0) { ++bad; std::printf("%s returned 0\n", #call); } expect_reason(#call); } while (0)
int main() {
    float *d = nullptr; const float *s = nullptr;
    long *ld = nullptr; const long *ls = nullptr;
    uint64_t *sig = nullptr;
    hipStream_t st = nullptr;
    hipEvent_t deps[1] = {nullptr};
    static_assert(ISHMEM_CMP_EQ == 1 && ISHMEM_CMP_NE == 2 && ISHMEM_CMP_GT == 3 && ISHMEM_CMP_GE == 4 &&
                  ISHMEM_CMP_LT == 5 && ISHMEM_CMP_LE == 6 && ISHMEM_SIGNAL_SET == 0 && ISHMEM_SIGNAL_ADD == 1, "values");
    V(ishmem_float_put_signal(d, s, 1, sig, 1, ISHMEM_SIGNAL_SET, 0));
    V(ishmem_size_put_signal((size_t *) nullptr, (const size_t *) nullptr, 1, sig, 1, ISHMEM_SIGNAL_ADD, 0));
    V(ishmem_ptrdiff_put_signal_nbi((ptrdiff_t *) nullptr, (const ptrdiff_t *) nullptr, 1, sig, 1, ISHMEM_SIGNAL_SET, 0));
    V(ishmem_char_put_signal_nbi((char *) nullptr, (const char *) nullptr, 1, sig, 1, ISHMEM_SIGNAL_SET, 0));
    V(ishmem_put_signal(ld, ls, 1, sig, 1, ISHMEM_SIGNAL_SET, 0));
    V(ishmem_put_signal_nbi(ld, ls, 1, sig, 1, ISHMEM_SIGNAL_ADD, 0));
    V(ishmem_put8_signal(d, s, 1, sig, 1, ISHMEM_SIGNAL_SET, 0));
    V(ishmem_put16_signal(d, s, 1, sig, 1, ISHMEM_SIGNAL_SET, 0));
    V(ishmem_put32_signal_nbi(d, s, 1, sig, 1, ISHMEM_SIGNAL_SET, 0));
    V(ishmem_put64_signal(d, s, 1, sig, 1, ISHMEM_SIGNAL_SET, 0));
    V(ishmem_put128_signal_nbi(d, s, 1, sig, 1, ISHMEM_SIGNAL_SET, 0));
    V(ishmem_putmem_signal(d, s, 4, sig, 1, ISHMEM_SIGNAL_SET, 0));
    V(ishmem_putmem_signal_nbi(d, s, 4, sig, 1, ISHMEM_SIGNAL_SET, 0));
    V((void) ishmem_signal_fetch(sig));
    V((void) ishmem_signal_wait_until(sig, ISHMEM_CMP_EQ, 1));
    V(ishmemx_signal_set(sig, 1, 0));
    V(ishmemx_signal_add(sig, 1, 0));
    V(ishmem_int_wait_until((int *) nullptr, ISHMEM_CMP_EQ, 1));
    V(ishmem_long_wait_until((long *) nullptr, ISHMEM_CMP_NE, 1L));
    V(ishmem_longlong_wait_until((long long *) nullptr, ISHMEM_CMP_GT, 1LL));
    V(ishmem_uint_wait_until((unsigned int *) nullptr, ISHMEM_CMP_GE, 1u));
    V(ishmem_ulong_wait_until((unsigned long *) nullptr, ISHMEM_CMP_LT, 1ul));
    V(ishmem_ulonglong_wait_until((unsigned long long *) nullptr, ISHMEM_CMP_LE, 1ull));
    V(ishmem_int32_wait_until((int32_t *) nullptr, ISHMEM_CMP_EQ, 1));
    V(ishmem_int64_wait_until((int64_t *) nullptr, ISHMEM_CMP_EQ, 1));
    V(ishmem_uint32_wait_until((uint32_t *) nullptr, ISHMEM_CMP_EQ, 1));
    V(ishmem_uint64_wait_until((uint64_t *) nullptr, ISHMEM_CMP_EQ, 1));
    V(ishmem_size_wait_until((size_t *) nullptr, ISHMEM_CMP_EQ, 1));
    V(ishmem_ptrdiff_wait_until((ptrdiff_t *) nullptr, ISHMEM_CMP_EQ, 1));
    V(ishmem_wait_until(ld, ISHMEM_CMP_EQ, 1L));
    V((void) ishmem_int_test((int *) nullptr, ISHMEM_CMP_EQ, 1));
    V((void) ishmem_long_test((long *) nullptr, ISHMEM_CMP_EQ, 1L));
    V((void) ishmem_longlong_test((long long *) nullptr, ISHMEM_CMP_EQ, 1LL));
    V((void) ishmem_uint_test((unsigned int *) nullptr, ISHMEM_CMP_EQ, 1u));
    V((void) ishmem_ulong_test((unsigned long *) nullptr, ISHMEM_CMP_EQ, 1ul));
    V((void) ishmem_ulonglong_test((unsigned long long *) nullptr, ISHMEM_CMP_EQ, 1ull));
    V((void) ishmem_int32_test((int32_t *) nullptr, ISHMEM_CMP_EQ, 1));
    V((void) ishmem_int64_test((int64_t *) nullptr, ISHMEM_CMP_EQ, 1));
    V((void) ishmem_uint32_test((uint32_t *) nullptr, ISHMEM_CMP_EQ, 1));
    V((void) ishmem_uint64_test((uint64_t *) nullptr, ISHMEM_CMP_EQ, 1));
    V((void) ishmem_size_test((size_t *) nullptr, ISHMEM_CMP_EQ, 1));
    V((void) ishmem_ptrdiff_test((ptrdiff_t *) nullptr, ISHMEM_CMP_EQ, 1));
    V((void) ishmem_test(ld, ISHMEM_CMP_EQ, 1L));
    I(ishmemx_float_put_signal_on_stream(d, s, 1, sig, 1, ISHMEM_SIGNAL_SET, 0, st));
    I(ishmemx_double_put_signal_nbi_on_stream((double *) nullptr, (const double *) nullptr, 1, sig, 1, ISHMEM_SIGNAL_SET, 0, st));
    I(ishmemx_put_signal_on_stream(ld, ls, 1, sig, 1, ISHMEM_SIGNAL_SET, 0, st));
    I(ishmemx_put_signal_nbi_on_stream(ld, ls, 1, sig, 1, ISHMEM_SIGNAL_SET, 0, st));
    I(ishmemx_putmem_signal_on_stream(d, s, 4, sig, 1, ISHMEM_SIGNAL_SET, 0, st));
    I(ishmemx_putmem_signal_nbi_on_stream(d, s, 4, sig, 1, ISHMEM_SIGNAL_SET, 0, st));
    I(ishmemx_put64_signal_on_stream(d, s, 1, sig, 1, ISHMEM_SIGNAL_SET, 0, st));
    I(ishmemx_put128_signal_nbi_on_stream(d, s, 1, sig, 1, ISHMEM_SIGNAL_SET, 0, st));
    I(ishmemx_int_put_signal_on_stream((int *) nullptr, (const int *) nullptr, 1, sig, 1, ISHMEM_SIGNAL_SET, 0, st, deps, 0, nullptr));
    I(ishmemx_put_signal_on_stream(ld, ls, 1, sig, 1, ISHMEM_SIGNAL_SET, 0, st, deps, 0, nullptr));
    I(ishmemx_putmem_signal_on_stream(d, s, 4, sig, 1, ISHMEM_SIGNAL_SET, 0, st, deps, 0, nullptr));
    I(ishmemx_signal_wait_until_on_stream(sig, ISHMEM_CMP_EQ, 1, (uint64_t *) nullptr, st));
    I(ishmemx_signal_wait_until_on_stream(sig, ISHMEM_CMP_EQ, 1, (uint64_t *) nullptr, st, deps, 0, nullptr));
    I(ishmemx_int_wait_until_on_stream((int *) nullptr, ISHMEM_CMP_EQ, 1, st));
    I(ishmemx_uint64_wait_until_on_stream((uint64_t *) nullptr, ISHMEM_CMP_EQ, 1, st));
    I(ishmemx_ptrdiff_wait_until_on_stream((ptrdiff_t *) nullptr, ISHMEM_CMP_EQ, 1, st, deps, 0, nullptr));
    I(ishmemx_size_wait_until_on_stream((size_t *) nullptr, ISHMEM_CMP_EQ, 1, st));
    I(ishmemx_wait_until_on_stream(ld, ISHMEM_CMP_EQ, 1L, st));
    std::printf("%d %d\n", n, bad);
    return 0;
}
'''


def test_host_cxx_names_compile_link_and_fail_before_init(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed for the host C++ names"
    src = tmp_path / "t.cpp"
    src.write_text(HOST_CXX)
    exe = tmp_path / "t"
    subprocess.run([gxx, "-std=c++17", "-Wall", "-Werror", f"-I{INCLUDE}", str(src), "-o", str(exe),
                    f"-L{_lib.LIB_PATH.parent}", f"-Wl,-rpath,{_lib.LIB_PATH.parent}", "-lishmem_amd"],
                   check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    calls = len(re.findall(r"^    [VI]\(", HOST_CXX, re.M))
    assert calls == 61  # 43 void / value-returning calls, 18 on-stream calls
    assert out.stdout.split()[-2:] == [str(calls), "0"], out.stdout


def test_device_forms_compile_for_gfx950(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert Path(hipcc).exists(), "hipcc is needed for the device API"
    src = tmp_path / "t.hip"
    src.write_text(r'''
#include <hip/hip_cooperative_groups.h>
#include <ishmem.h>
#include <ishmemx.h>
namespace cg = cooperative_groups;
__global__ void k(int *dst, const int *src, double *fd, const double *fs, uint64_t *sig, long *lv, int pe, long *out) {
    auto grp = cg::this_thread_block();
    auto wave = cg::tiled_partition<64>(grp);
    long acc = 0;
    // a thread block
    ishmemx_int_put_signal_work_group(dst, src, 3, sig, 1, ISHMEM_SIGNAL_SET, pe, grp);
    ishmemx_double_put_signal_nbi_work_group(fd, fs, 3, sig, 1, ISHMEM_SIGNAL_ADD, pe, grp);
    ishmemx_put_signal_work_group(fd, fs, 3, sig, 1, ISHMEM_SIGNAL_SET, pe, grp);
    ishmemx_put_signal_nbi_work_group(dst, src, 3, sig, 1, ISHMEM_SIGNAL_SET, pe, grp);
    ishmemx_putmem_signal_work_group(dst, src, 12, sig, 1, ISHMEM_SIGNAL_SET, pe, grp);
    ishmemx_putmem_signal_nbi_work_group(dst, src, 12, sig, 1, ISHMEM_SIGNAL_SET, pe, grp);
    ishmemx_put8_signal_work_group(dst, src, 12, sig, 1, ISHMEM_SIGNAL_SET, pe, grp);
    ishmemx_put16_signal_nbi_work_group(dst, src, 6, sig, 1, ISHMEM_SIGNAL_SET, pe, grp);
    ishmemx_put32_signal_nbi_work_group(dst, src, 3, sig, 1, ISHMEM_SIGNAL_SET, pe, grp);
    ishmemx_put64_signal_work_group(fd, fs, 3, sig, 1, ISHMEM_SIGNAL_SET, pe, grp);
    ishmemx_put128_signal_nbi_work_group(fd, fs, 1, sig, 1, ISHMEM_SIGNAL_SET, pe, grp);
    acc += (long) ishmemx_signal_wait_until_work_group(sig, ISHMEM_CMP_GE, 1, grp);
    ishmemx_int_wait_until_work_group(dst, ISHMEM_CMP_EQ, 1, grp);
    ishmemx_long_wait_until_work_group(lv, ISHMEM_CMP_NE, 1L, grp);
    ishmemx_longlong_wait_until_work_group((long long *) lv, ISHMEM_CMP_GT, 1LL, grp);
    ishmemx_uint_wait_until_work_group((unsigned int *) dst, ISHMEM_CMP_GE, 1u, grp);
    ishmemx_ulong_wait_until_work_group((unsigned long *) lv, ISHMEM_CMP_LT, 1ul, grp);
    ishmemx_ulonglong_wait_until_work_group((unsigned long long *) lv, ISHMEM_CMP_LE, 1ull, grp);
    ishmemx_int32_wait_until_work_group((int32_t *) dst, ISHMEM_CMP_EQ, 1, grp);
    ishmemx_int64_wait_until_work_group((int64_t *) lv, ISHMEM_CMP_EQ, 1, grp);
    ishmemx_uint32_wait_until_work_group((uint32_t *) dst, ISHMEM_CMP_EQ, 1, grp);
    ishmemx_uint64_wait_until_work_group(sig, ISHMEM_CMP_EQ, 1, grp);
    ishmemx_size_wait_until_work_group((size_t *) lv, ISHMEM_CMP_EQ, 1, grp);
    ishmemx_ptrdiff_wait_until_work_group((ptrdiff_t *) lv, ISHMEM_CMP_EQ, 1, grp);
    ishmemx_wait_until_work_group(lv, ISHMEM_CMP_EQ, 1L, grp);
    acc += ishmemx_int_test_work_group(dst, ISHMEM_CMP_EQ, 1, grp);
    acc += ishmemx_long_test_work_group(lv, ISHMEM_CMP_EQ, 1L, grp);
    acc += ishmemx_longlong_test_work_group((long long *) lv, ISHMEM_CMP_EQ, 1LL, grp);
    acc += ishmemx_uint_test_work_group((unsigned int *) dst, ISHMEM_CMP_EQ, 1u, grp);
    acc += ishmemx_ulong_test_work_group((unsigned long *) lv, ISHMEM_CMP_EQ, 1ul, grp);
    acc += ishmemx_ulonglong_test_work_group((unsigned long long *) lv, ISHMEM_CMP_EQ, 1ull, grp);
    acc += ishmemx_int32_test_work_group((int32_t *) dst, ISHMEM_CMP_EQ, 1, grp);
    acc += ishmemx_int64_test_work_group((int64_t *) lv, ISHMEM_CMP_EQ, 1, grp);
    acc += ishmemx_uint32_test_work_group((uint32_t *) dst, ISHMEM_CMP_EQ, 1, grp);
    acc += ishmemx_uint64_test_work_group(sig, ISHMEM_CMP_EQ, 1, grp);
    acc += ishmemx_size_test_work_group((size_t *) lv, ISHMEM_CMP_EQ, 1, grp);
    acc += ishmemx_ptrdiff_test_work_group((ptrdiff_t *) lv, ISHMEM_CMP_EQ, 1, grp);
    acc += ishmemx_test_work_group(lv, ISHMEM_CMP_EQ, 1L, grp);
    // a 64-lane tile
    if (grp.thread_rank() < 64) {
        ishmemx_size_put_signal_work_group((size_t *) fd, (const size_t *) fs, 3, sig, 1, ISHMEM_SIGNAL_SET, pe, wave);
        ishmemx_uint8_put_signal_nbi_work_group((uint8_t *) dst, (const uint8_t *) src, 3, sig, 1, ISHMEM_SIGNAL_ADD, pe, wave);
        ishmemx_put_signal_work_group(dst, src, 3, sig, 1, ISHMEM_SIGNAL_SET, pe, wave);
        ishmemx_putmem_signal_nbi_work_group(dst, src, 12, sig, 1, ISHMEM_SIGNAL_SET, pe, wave);
        ishmemx_put32_signal_work_group(dst, src, 3, sig, 1, ISHMEM_SIGNAL_SET, pe, wave);
        acc += (long) ishmemx_signal_wait_until_work_group(sig, ISHMEM_CMP_EQ, 1, wave);
        ishmemx_int_wait_until_work_group(dst, ISHMEM_CMP_EQ, 1, wave);
        ishmemx_ptrdiff_wait_until_work_group((ptrdiff_t *) lv, ISHMEM_CMP_EQ, 1, wave);
        ishmemx_uint64_wait_until_work_group(sig, ISHMEM_CMP_EQ, 1, wave);
        acc += ishmemx_int_test_work_group(dst, ISHMEM_CMP_EQ, 1, wave);
        acc += ishmemx_size_test_work_group((size_t *) lv, ISHMEM_CMP_EQ, 1, wave);
        acc += ishmemx_test_work_group(lv, ISHMEM_CMP_EQ, 1L, wave);
    }
    // single work-items, each with its own arguments
    const int t = grp.thread_rank();
    ishmem_int_put_signal(dst + t, src + t, 1, sig + t, 1, ISHMEM_SIGNAL_SET, pe);
    ishmem_double_put_signal_nbi(fd + t, fs + t, 1, sig + t, 1, ISHMEM_SIGNAL_ADD, pe);
    ishmem_put_signal(fd + t, fs + t, 1, sig + t, 1, ISHMEM_SIGNAL_SET, pe);
    ishmem_put_signal_nbi(dst + t, src + t, 1, sig + t, 1, ISHMEM_SIGNAL_SET, pe);
    ishmem_putmem_signal(dst + t, src + t, 4, sig + t, 1, ISHMEM_SIGNAL_SET, pe);
    ishmem_putmem_signal_nbi(dst + t, src + t, 4, sig + t, 1, ISHMEM_SIGNAL_SET, pe);
    ishmem_put16_signal(dst + t, src + t, 2, sig + t, 1, ISHMEM_SIGNAL_SET, pe);
    ishmem_put128_signal_nbi(fd + 2 * t, fs + 2 * t, 1, sig + t, 1, ISHMEM_SIGNAL_SET, pe);
    ishmemx_signal_set(sig + t, 1, pe);
    ishmemx_signal_add(sig + t, 1, pe);
    acc += (long) ishmem_signal_fetch(sig + t);
    acc += (long) ishmem_signal_wait_until(sig + t, ISHMEM_CMP_EQ, 2);
    ishmem_int_wait_until(dst + t, ISHMEM_CMP_EQ, 1);
    ishmem_uint64_wait_until(sig + t, ISHMEM_CMP_EQ, 1);
    ishmem_ptrdiff_wait_until((ptrdiff_t *) lv + t, ISHMEM_CMP_EQ, 1);
    ishmem_wait_until(lv + t, ISHMEM_CMP_EQ, 1L);
    acc += ishmem_int_test(dst + t, ISHMEM_CMP_EQ, 1);
    acc += ishmem_size_test((size_t *) lv + t, ISHMEM_CMP_EQ, 1);
    acc += ishmem_test(lv + t, ISHMEM_CMP_EQ, 1L);
    out[t] = acc;
}
int main() { return 0; }
''')
    subprocess.run([hipcc, "--offload-arch=gfx950", "-std=c++20", f"-I{INCLUDE}", "-c", str(src), "-o",
                    str(tmp_path / "t.o")], check=True)

"""put / get without a GPU: the C ABI before init, the Python names, the host C++ names (g++, linked
against the library), the device API (hipcc, gfx950, compile only) and the expected-result helper."""
import shutil
import subprocess
from pathlib import Path

import numpy as np

import ishmem_amd as ish
from ishmem_amd import _lib
from tests.rma_worker import LOOP_TWICE, MAX_BLOCKS, TILE_BYTES, expected_word, payload

ROOT = Path(__file__).resolve().parents[1]
INCLUDE = ROOT / "include"

C_NAMES = ["ishmemi_c_put", "ishmemi_c_get", "ishmemi_c_put_nbi", "ishmemi_c_get_nbi", "ishmemi_c_put_on_stream",
           "ishmemi_c_get_on_stream", "ishmemi_c_quiet", "ishmemi_c_fence", "ishmemi_c_quiet_on_stream"]


def test_not_initialised_calls_fail_with_a_reason():
    assert not ish.initialized()
    L = ish.lib()
    for name in C_NAMES:
        fn = getattr(L, name)
        if name.endswith(("quiet", "fence")):
            rc = fn()
        elif name == "ishmemi_c_quiet_on_stream":
            rc = fn(None)
        elif name.endswith("on_stream"):
            rc = fn(None, None, 8, 0, None)
        else:
            rc = fn(None, None, 8, 0)
        assert rc != 0, name
        assert "not initialized" in ish.last_error(), name
    # nbytes == 0 before init is still "not initialized", not a success
    assert L.ishmemi_c_put(None, None, 0, 0) != 0
    for call in (lambda: ish.ishmem_putmem(0, 0, 8, 0), lambda: ish.ishmem_getmem_nbi(0, 0, 8, 0),
                 lambda: ish.put_on_stream(0, 0, 8, 0, 0), lambda: ish.get_on_stream(0, 0, 8, 0, 0),
                 lambda: ish.quiet_on_stream(0), ish.ishmem_quiet, ish.ishmem_fence):
        assert call() != 0
        assert "not initialized" in ish.last_error()


def test_python_names_exist_for_every_typename():
    assert len(ish.ARITH_TYPENAMES) == 23
    want = ["ishmem_putmem", "ishmem_getmem", "ishmem_putmem_nbi", "ishmem_getmem_nbi"]
    for tn in ish.ARITH_TYPENAMES:
        want += [f"ishmem_{tn}_put", f"ishmem_{tn}_get", f"ishmem_{tn}_put_nbi", f"ishmem_{tn}_get_nbi"]
    for bits in (8, 16, 32, 64, 128):
        want += [f"ishmem_put{bits}", f"ishmem_get{bits}", f"ishmem_put{bits}_nbi", f"ishmem_get{bits}_nbi"]
    assert sorted(want) == sorted(ish.RMA_NAMES)
    for name in want:
        fn = getattr(ish, name)
        assert fn.__name__ == name
        assert fn(0, 0, 1, 0) != 0  # not initialised
    for name in ("ishmem_quiet", "ishmem_fence", "put_on_stream", "get_on_stream", "quiet_on_stream"):
        assert callable(getattr(ish, name))
    names = [p[0] for p in _lib.PROTOTYPES]
    assert all(n in names for n in C_NAMES)
    header = (INCLUDE / "ishmem_capi.h").read_text()
    assert all(f"{n}(" in header for n in C_NAMES)


def test_expected_result_helper():
    # The tester's word (ishmem_tester.h:1118-1149).
    assert int(expected_word(5, 1, 2, 0)) == (5 << 48) + (0x81 << 40) + (0x82 << 32)
    assert int(expected_word(3, 0, 1, 2)) == (3 << 48) + (0x80 << 40) + (0x81 << 32) + 2
    w = expected_word(16, 2, 0, np.arange(4))
    assert [int(x) for x in w] == [(16 << 48) + (0x82 << 40) + (0x80 << 32) + i for i in range(4)]
    b = payload("tester", 0, 20, 1, 2)
    assert b.dtype == np.uint8 and b.size == 20
    assert int(b[:8].view("<u8")[0]) == (20 << 48) + (0x81 << 40) + (0x82 << 32)
    assert int(b[8:16].view("<u8")[0]) == (20 << 48) + (0x81 << 40) + (0x82 << 32) + 1
    assert payload("tester", 0, 0, 0, 0).size == 0
    r = payload("random", 7, 33, 0, 1)
    assert np.array_equal(r, payload("random", 7, 33, 0, 1)) and not np.array_equal(r, payload("random", 7, 33, 1, 0))
    # The size at which every workgroup of a 32-workgroup grid runs its loop at least twice.
    assert TILE_BYTES == 256 * 4 * 16 and LOOP_TWICE // TILE_BYTES >= 2 * MAX_BLOCKS


def test_host_cxx_names_compile_link_and_fail_before_init(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed for the host C++ names"
    src = tmp_path / "t.cpp"
    src.write_text(r'''
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
    hipStream_t st = nullptr;
    hipEvent_t deps[1] = {nullptr};
    V(ishmem_float_put(d, s, 1, 0));  V(ishmem_float_get(d, s, 1, 0));            // typed
    V(ishmem_size_put((size_t *) nullptr, (const size_t *) nullptr, 1, 0));
    V(ishmem_ptrdiff_get((ptrdiff_t *) nullptr, (const ptrdiff_t *) nullptr, 1, 0));
    V(ishmem_put(ld, ls, 1, 0));      V(ishmem_get(ld, ls, 1, 0));               // generic
    V(ishmem_put8(d, s, 1, 0));       V(ishmem_get16(d, s, 1, 0));               // sized
    V(ishmem_put32(d, s, 1, 0));      V(ishmem_get64(d, s, 1, 0));
    V(ishmem_put128(d, s, 1, 0));     V(ishmem_get128(d, s, 1, 0));
    V(ishmem_putmem(d, s, 4, 0));     V(ishmem_getmem(d, s, 4, 0));              // mem
    V(ishmem_float_put_nbi(d, s, 1, 0)); V(ishmem_float_get_nbi(d, s, 1, 0));    // _nbi
    V(ishmem_put_nbi(ld, ls, 1, 0));  V(ishmem_get_nbi(ld, ls, 1, 0));
    V(ishmem_put64_nbi(d, s, 1, 0));  V(ishmem_get8_nbi(d, s, 1, 0));
    V(ishmem_putmem_nbi(d, s, 4, 0)); V(ishmem_getmem_nbi(d, s, 4, 0));
    V(ishmem_float_p(d, 1.0f, 0));    V((void) ishmem_float_g(s, 0));            // p / g
    V(ishmem_p(ld, 1L, 0));           V((void) ishmem_g(ls, 0));
    V(ishmem_uint8_p((uint8_t *) nullptr, (uint8_t) 1, 0));
    V((void) ishmem_double_g((const double *) nullptr, 0));
    V(ishmem_quiet());                V(ishmem_fence());                         // ordering
    I(ishmemx_float_put_on_stream(d, s, 1, 0, st));                              // on a stream
    I(ishmemx_float_get_on_stream(d, s, 1, 0, st));
    I(ishmemx_float_put_nbi_on_stream(d, s, 1, 0, st));
    I(ishmemx_put_on_stream(ld, ls, 1, 0, st));
    I(ishmemx_get_nbi_on_stream(ld, ls, 1, 0, st));
    I(ishmemx_putmem_on_stream(d, s, 4, 0, st));
    I(ishmemx_getmem_nbi_on_stream(d, s, 4, 0, st));
    I(ishmemx_put64_on_stream(d, s, 1, 0, st));
    I(ishmemx_get128_nbi_on_stream(d, s, 1, 0, st));
    I(ishmemx_quiet_on_stream(st));
    I(ishmemx_double_put_on_stream((double *) nullptr, (const double *) nullptr, 1, 0, st, deps, 0, nullptr));
    I(ishmemx_get_on_stream(ld, ls, 1, 0, st, deps, 0, nullptr));
    I(ishmemx_putmem_on_stream(d, s, 4, 0, st, deps, 0, nullptr));
    I(ishmemx_quiet_on_stream(st, deps, 0, nullptr));
    std::printf("%d %d\n", n, bad);
    return 0;
}
''')
    exe = tmp_path / "t"
    subprocess.run([gxx, "-std=c++17", f"-I{INCLUDE}", str(src), "-o", str(exe),
                    f"-L{_lib.LIB_PATH.parent}", f"-Wl,-rpath,{_lib.LIB_PATH.parent}", "-lishmem_amd"],
                   check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split()[-2:] == ["44", "0"], out.stdout  # 30 void calls, 14 on-stream calls


def test_device_forms_compile_for_gfx950(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert Path(hipcc).exists(), "hipcc is needed for the device API"
    src = tmp_path / "t.hip"
    src.write_text(r'''
#include <hip/hip_cooperative_groups.h>
#include <ishmem.h>
#include <ishmemx.h>
namespace cg = cooperative_groups;
__global__ void k(int *dst, const int *src, double *fd, const double *fs, int pe, long *out) {
    auto grp = cg::this_thread_block();
    auto wave = cg::tiled_partition<64>(grp);
    // a thread block
    ishmemx_int_put_work_group(dst, src, 3, pe, grp);
    ishmemx_int_get_work_group(dst, src, 3, pe, grp);
    ishmemx_double_put_nbi_work_group(fd, fs, 3, pe, grp);
    ishmemx_double_get_nbi_work_group(fd, fs, 3, pe, grp);
    ishmemx_put_work_group(fd, fs, 3, pe, grp);
    ishmemx_get_nbi_work_group(fd, fs, 3, pe, grp);
    ishmemx_putmem_work_group(dst, src, 12, pe, grp);
    ishmemx_getmem_nbi_work_group(dst, src, 12, pe, grp);
    ishmemx_put64_work_group(fd, fs, 3, pe, grp);
    ishmemx_get128_nbi_work_group(fd, fs, 1, pe, grp);
    ishmemx_quiet_work_group(grp);
    ishmemx_fence_work_group(grp);
    // a 64-lane tile
    if (grp.thread_rank() < 64) {
        ishmemx_size_put_work_group((size_t *) fd, (const size_t *) fs, 3, pe, wave);
        ishmemx_uint8_get_work_group((uint8_t *) dst, (const uint8_t *) src, 3, pe, wave);
        ishmemx_put_nbi_work_group(dst, src, 3, pe, wave);
        ishmemx_getmem_work_group(dst, src, 12, pe, wave);
        ishmemx_put32_work_group(dst, src, 3, pe, wave);
        ishmemx_quiet_work_group(wave);
        ishmemx_fence_work_group(wave);
    }
    // single threads, each with its own arguments
    const int t = grp.thread_rank();
    ishmem_int_put(dst + t, src + t, 1, pe);
    ishmem_int_get(dst + t, src + t, 1, pe);
    ishmem_put(fd + t, fs + t, 1, pe);
    ishmem_get_nbi(fd + t, fs + t, 1, pe);
    ishmem_putmem(dst + t, src + t, 4, pe);
    ishmem_getmem_nbi(dst + t, src + t, 4, pe);
    ishmem_put16(dst + t, src + t, 2, pe);
    ishmem_get8_nbi(dst + t, src + t, 4, pe);
    ishmem_long_put_nbi((long *) fd + t, (const long *) fs + t, 1, pe);
    // p / g
    ishmem_int_p(dst + t, t, pe);
    ishmem_double_p(fd + t, 1.0, pe);
    ishmem_p((short *) dst + t, (short) t, pe);
    ishmem_char_p((char *) dst + t, (char) t, pe);
    long acc = ishmem_int_g(src + t, pe) + (long) ishmem_double_g(fs + t, pe) + ishmem_g((const short *) src + t, pe) +
               ishmem_uint8_g((const uint8_t *) src + t, pe) + (long) ishmem_uint64_g((const uint64_t *) fs + t, pe);
    ishmem_quiet();
    ishmem_fence();
    out[t] = acc;
}
int main() { return 0; }
''')
    subprocess.run([hipcc, "--offload-arch=gfx950", "-std=c++20", f"-I{INCLUDE}", "-c", str(src), "-o",
                    str(tmp_path / "t.o")], check=True)

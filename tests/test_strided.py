"""Strided / blocked put / get without a GPU: the layout rule (ishmemi_c_strided_plan) against a numpy
restatement, the C ABI before init, the Python names, the host C++ names (g++, linked against the
library), the device names (hipcc, gfx950, compile only) and the GPU tests' case tables."""
import ctypes
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import ishmem_amd as ish
from ishmem_amd import _lib
from tests import strided_cases as sc

ROOT = Path(__file__).resolve().parents[1]
INCLUDE = ROOT / "include"
C_NAMES = ["ishmemi_c_ibput", "ishmemi_c_ibget", "ishmemi_c_ibput_on_stream", "ishmemi_c_ibget_on_stream"]


@pytest.mark.parametrize("es", range(1, 17))
def test_plan_matches_the_layout_rule(es):
    L = ish.lib()
    w, ipb, cont = ctypes.c_int(), ctypes.c_size_t(), ctypes.c_int()
    base = 1 << 20
    n = 0
    for bsize in (1, 2, 3, 4, 5, 16, 33):
        strides = (bsize, bsize + 1, 2 * bsize + 3, 64)
        for dst in strides:
            for sst in strides:
                if dst < bsize or sst < bsize:
                    continue
                for nblocks in (1, 2, 65):
                    for doff in range(16):
                        for soff in range(16):
                            d, s = base + doff, 3 * base + soff
                            assert L.ishmemi_c_strided_plan(d, s, dst, sst, bsize, nblocks, es, ctypes.byref(w),
                                                            ctypes.byref(ipb), ctypes.byref(cont)) == 0
                            want = sc.plan(d, s, dst, sst, bsize, nblocks, es)
                            assert (w.value, ipb.value, bool(cont.value)) == want, (d, s, dst, sst, bsize, nblocks, es)
                            n += 1
    assert n > 10000


def test_plan_properties():
    # The item divides everything an address is built from; one block ignores the strides.
    for d, s, dst, sst, bsize, nblocks, es in [(4096, 8192, 8, 12, 4, 9, 4), (4096 + 4, 8192, 8, 12, 4, 9, 4),
                                                (4096, 8192, 7, 9, 5, 3, 1), (4096, 8192 + 8, 4, 4, 2, 100, 8),
                                                (4096, 8192, 3, 5, 1, 10, 16), (4096, 8192, 3, 5, 1, 10, 1)]:
        w, ipb, cont = ish.strided_plan(d, s, dst, sst, bsize, nblocks, es)
        assert w in (1, 2, 4, 8, 16) and ipb * w == bsize * es
        assert all(v % w == 0 for v in (d, s, dst * es, sst * es))
        w2 = min(16, 2 * w)
        assert w == 16 or any(v % w2 for v in (d, s, dst * es, sst * es, bsize * es))
    assert ish.strided_plan(4096, 8192, 8, 12, 4, 9, 4) == (16, 1, False)    # an aligned float block: 16-B items
    assert ish.strided_plan(4096, 8192, 64, 80, 16, 9, 4) == (16, 4, False)
    assert ish.strided_plan(4096, 8192, 3, 5, 1, 100, 1) == (1, 1, False)    # a uint8 iput moves bytes
    assert ish.strided_plan(4096, 8192, 7, 7, 7, 100, 4)[2] is True          # both strides == bsize: contiguous
    assert ish.strided_plan(4096, 8192, 1, 1, 1, 100, 4) == (4, 1, True)
    assert ish.strided_plan(4096, 8192, 1001, 3, 1, 1, 16) == (16, 1, True)  # one block: the strides do not count
    assert ish.strided_plan(4096, 8192, 1001, 3, 2, 1, 8) == ish.strided_plan(4096, 8192, 2, 2, 2, 1, 8) == (16, 1, True)
    w, ipb, cont = ctypes.c_int(), ctypes.c_size_t(), ctypes.c_int()
    L = ish.lib()
    assert L.ishmemi_c_strided_plan(4096, 8192, 1, 1, 1, 1, 0, ctypes.byref(w), ctypes.byref(ipb), ctypes.byref(cont)) != 0
    assert L.ishmemi_c_strided_plan(4096, 8192, -1, 1, 1, 2, 4, ctypes.byref(w), ctypes.byref(ipb), ctypes.byref(cont)) != 0
    assert L.ishmemi_c_strided_plan(4096, 8192, 1, 1, 1, 1, 4, None, ctypes.byref(ipb), ctypes.byref(cont)) != 0


def test_not_initialised_calls_fail_with_a_reason():
    assert not ish.initialized()
    L = ish.lib()
    for name in C_NAMES:
        fn = getattr(L, name)
        args = (None, None, 2, 3, 1, 8, 4, 0) + ((None,) if name.endswith("on_stream") else ())
        assert fn(*args) != 0, name
        assert "not initialized" in ish.last_error(), name
        # an empty call, or bad arguments, before init is still "not initialized"
        assert fn(*((None, None, 0, -1, 1, 0, 3, -1) + args[8:])) != 0
        assert "not initialized" in ish.last_error(), name
    for call in (lambda: ish.ibput(0, 0, 2, 2, 1, 8, 4, 0), lambda: ish.ibget(0, 0, 2, 2, 1, 8, 4, 0),
                 lambda: ish.ibput_on_stream(0, 0, 2, 2, 1, 8, 4, 0, 0), lambda: ish.ibget_on_stream(0, 0, 2, 2, 1, 8, 4, 0, 0)):
        assert call() != 0
        assert "not initialized" in ish.last_error()


def test_python_names_exist_for_every_typename_and_size():
    assert len(ish.ARITH_TYPENAMES) == 23
    want = []
    for tn in ish.ARITH_TYPENAMES:
        want += [f"ishmem_{tn}_iput", f"ishmem_{tn}_iget", f"ishmemx_{tn}_ibput", f"ishmemx_{tn}_ibget"]
    for bits in (8, 16, 32, 64, 128):
        want += [f"ishmem_iput{bits}", f"ishmem_iget{bits}", f"ishmemx_ibput{bits}", f"ishmemx_ibget{bits}"]
    assert sorted(want) == sorted(ish.STRIDED_NAMES) and len(want) == 4 * 28
    for name in want:
        fn = getattr(ish, name)
        assert fn.__name__ == name
        rc = fn(0, 0, 2, 2, 1, 3, 0) if "_ib" in name else fn(0, 0, 2, 2, 3, 0)
        assert rc != 0 and "not initialized" in ish.last_error()  # not initialised
    for name in ("ibput", "ibget", "ibput_on_stream", "ibget_on_stream", "strided_plan"):
        assert callable(getattr(ish, name))
    assert not any(n in ish.API_NAMES for n in want)
    names = [p[0] for p in _lib.PROTOTYPES]
    header = (INCLUDE / "ishmem_capi.h").read_text()
    for n in C_NAMES + ["ishmemi_c_strided_plan"]:
        assert n in names and f"{n}(" in header


def test_case_tables():
    assert sc.LOOP_TWICE == 2 * 32 * 1024 + 1 and sc.TILE_ITEMS == 1024 and sc.MAX_BLOCKS == 32
    iput = sc.iput_cases()
    assert len(iput) == 5 * 5 * 8 and all(c[3] == 1 for c in iput)
    assert {c[0] for c in iput} == {1, 2, 4, 8, 16} and {(c[1], c[2]) for c in iput} == {(1, 1), (2, 3), (3, 2), (7, 1), (1, 5)}
    assert {c[4] for c in iput} == {0, 1, 2, 63, 64, 65, 1025, 65537}
    ib = sc.ib_cases()
    assert len(ib) == 3 * 6 * 6 * 5
    for es, dst, sst, bs, nb in ib:
        assert dst != sst and {dst, sst} <= {bs, bs + 1, 2 * bs + 3} and bs in (1, 2, 5, 16, 33, 1027) and nb in (0, 1, 2, 3, 65)
    # The offset sweep meets every item width, the 16-B path included.
    off = sc.offset_cases()
    assert {(s, d) for s, d, _ in off} == {(s, d) for s in range(16) for d in range(16)}
    widths = {sc.plan(4096 + d, 8192 + s, c[1], c[2], c[3], c[4], c[0])[0] for s, d, c in off}
    assert widths == {1, 2, 4, 8, 16}
    assert all(sc.strides_valid(c[1], c[2], c[3]) for _, _, c in off)
    # The reference tester's pair of calls.
    assert sc.tester_calls(1) == [(0, 0, 1, 1, 1, 1)]
    assert sc.tester_calls(2) == [(0, 0, 1, 1, 1, 2)]
    assert sc.tester_calls(16) == [(0, 0, 8, 1, 1, 2), (1, 2, 8, 7, 7, 2)]
    assert not sc.strides_valid(*sc.tester_calls(3)[1][2:5])


def test_expected_result_helper():
    assert sc.extent(3, 1, 5, 4) == 52 and sc.extent(3, 1, 0, 4) == 0 and sc.extent(7, 5, 1, 2) == 10
    assert list(sc.byte_index(3, 1, 3, 2)) == [0, 1, 6, 7, 12, 13]
    assert list(sc.byte_index(4, 2, 2, 1)) == [0, 1, 4, 5]
    # int_iput_device: target[i * 3] = source[i * 2] for 5 ints, every other int unchanged.
    src = np.arange(20, dtype="<i4")
    dst = np.full(20, -1, "<i4")
    want = dst.copy()
    for i in range(5):
        want[i * 3] = src[i * 2]
    d8 = dst.view(np.uint8).copy()
    sc.apply(d8, src.view(np.uint8), (4, 3, 2, 1, 5))
    assert np.array_equal(d8.view("<i4"), want)
    # blocked, with offsets
    d8 = np.zeros(64, np.uint8)
    sc.apply(d8, np.arange(64, dtype=np.uint8), (2, 5, 3, 2, 3), doff=4, soff=1)
    want = np.zeros(64, np.uint8)
    for b in range(3):
        for k in range(4):
            want[4 + b * 10 + k] = 1 + b * 6 + k
    assert np.array_equal(d8, want)


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
#define TYPED(TN, TYPE, U1, U2)                                                              \
    V(ishmem_##TN##_iput((TYPE *) nullptr, (const TYPE *) nullptr, 2, 3, 1, 0));             \
    V(ishmem_##TN##_iget((TYPE *) nullptr, (const TYPE *) nullptr, 2, 3, 1, 0));             \
    V(ishmemx_##TN##_ibput((TYPE *) nullptr, (const TYPE *) nullptr, 2, 3, 2, 1, 0));        \
    V(ishmemx_##TN##_ibget((TYPE *) nullptr, (const TYPE *) nullptr, 2, 3, 2, 1, 0));        \
    I(ishmemx_##TN##_iput_on_stream((TYPE *) nullptr, (const TYPE *) nullptr, 2, 3, 1, 0, st)); \
    I(ishmemx_##TN##_iget_on_stream((TYPE *) nullptr, (const TYPE *) nullptr, 2, 3, 1, 0, st)); \
    I(ishmemx_##TN##_ibput_on_stream((TYPE *) nullptr, (const TYPE *) nullptr, 2, 3, 2, 1, 0, st)); \
    I(ishmemx_##TN##_ibget_on_stream((TYPE *) nullptr, (const TYPE *) nullptr, 2, 3, 2, 1, 0, st)); \
    I(ishmemx_##TN##_ibput_on_stream((TYPE *) nullptr, (const TYPE *) nullptr, 2, 3, 2, 1, 0, st, deps, 0, nullptr));
#define SIZED(BITS)                                                                          \
    V(ishmem_iput##BITS(d, s, 2, 3, 1, 0));           V(ishmem_iget##BITS(d, s, 2, 3, 1, 0)); \
    V(ishmemx_ibput##BITS(d, s, 2, 3, 2, 1, 0));      V(ishmemx_ibget##BITS(d, s, 2, 3, 2, 1, 0)); \
    I(ishmemx_iput##BITS##_on_stream(d, s, 2, 3, 1, 0, st));                                 \
    I(ishmemx_iget##BITS##_on_stream(d, s, 2, 3, 1, 0, st, deps, 0, nullptr));               \
    I(ishmemx_ibput##BITS##_on_stream(d, s, 2, 3, 2, 1, 0, st, deps, 0, nullptr));           \
    I(ishmemx_ibget##BITS##_on_stream(d, s, 2, 3, 2, 1, 0, st));
int main() {
    float *d = nullptr; const float *s = nullptr;
    long *ld = nullptr; const long *ls = nullptr;
    hipStream_t st = nullptr;
    hipEvent_t deps[1] = {nullptr};
    ISHMEMI_CXX_ARITH_TYPES(TYPED, _, _)                                               // 23 x 9
    SIZED(8) SIZED(16) SIZED(32) SIZED(64) SIZED(128)                                  // 5 x 8
    V(ishmem_iput(ld, ls, 2, 3, 1, 0));               V(ishmem_iget(ld, ls, 2, 3, 1, 0));  // generic
    V(ishmemx_ibput(ld, ls, 2, 3, 2, 1, 0));          V(ishmemx_ibget(ld, ls, 2, 3, 2, 1, 0));
    I(ishmemx_iput_on_stream(ld, ls, 2, 3, 1, 0, st));
    I(ishmemx_iget_on_stream(ld, ls, 2, 3, 1, 0, st, deps, 0, nullptr));
    I(ishmemx_ibput_on_stream(ld, ls, 2, 3, 2, 1, 0, st));
    I(ishmemx_ibget_on_stream(ld, ls, 2, 3, 2, 1, 0, st, deps, 0, nullptr));
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
    assert out.stdout.split()[-2:] == [str(23 * 9 + 5 * 8 + 8), "0"], out.stdout


def test_device_names_compile_for_gfx950(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert Path(hipcc).exists(), "hipcc is needed for the device API"
    src = tmp_path / "t.hip"
    src.write_text(r'''
#include <hip/hip_cooperative_groups.h>
#include <ishmem.h>
#include <ishmemx.h>
namespace cg = cooperative_groups;
#define TYPED(TN, TYPE, U1, U2)                                                              \
    ishmem_##TN##_iput((TYPE *) d + t, (const TYPE *) s + t, 2, 3, 4, pe);                   \
    ishmem_##TN##_iget((TYPE *) d + t, (const TYPE *) s + t, 2, 3, 4, pe);                   \
    ishmemx_##TN##_ibput((TYPE *) d + t, (const TYPE *) s + t, 2, 3, 2, 4, pe);              \
    ishmemx_##TN##_ibget((TYPE *) d + t, (const TYPE *) s + t, 2, 3, 2, 4, pe);              \
    ishmemx_##TN##_iput_work_group((TYPE *) d, (const TYPE *) s, 2, 3, 4, pe, grp);          \
    ishmemx_##TN##_iget_work_group((TYPE *) d, (const TYPE *) s, 2, 3, 4, pe, grp);          \
    ishmemx_##TN##_ibput_work_group((TYPE *) d, (const TYPE *) s, 2, 3, 2, 4, pe, grp);      \
    ishmemx_##TN##_ibget_work_group((TYPE *) d, (const TYPE *) s, 2, 3, 2, 4, pe, grp);
#define SIZED(BITS)                                                                          \
    ishmem_iput##BITS(d + 16 * t, s + 16 * t, 2, 3, 4, pe);                                  \
    ishmem_iget##BITS(d + 16 * t, s + 16 * t, 2, 3, 4, pe);                                  \
    ishmemx_ibput##BITS(d + 16 * t, s + 16 * t, 2, 3, 2, 4, pe);                             \
    ishmemx_ibget##BITS(d + 16 * t, s + 16 * t, 2, 3, 2, 4, pe);                             \
    ishmemx_iput##BITS##_work_group(d, s, 2, 3, 4, pe, grp);                                 \
    ishmemx_iget##BITS##_work_group(d, s, 2, 3, 4, pe, wave);                                \
    ishmemx_ibput##BITS##_work_group(d, s, 2, 3, 2, 4, pe, wave);                            \
    ishmemx_ibget##BITS##_work_group(d, s, 2, 3, 2, 4, pe, grp);
__global__ void k(char *d, const char *s, int pe) {
    auto grp = cg::this_thread_block();
    auto wave = cg::tiled_partition<64>(grp);
    const int t = grp.thread_rank();
    ISHMEMI_CXX_ARITH_TYPES(TYPED, _, _)
    SIZED(8) SIZED(16) SIZED(32) SIZED(64) SIZED(128)
    // generic templates, a 64-lane tile and the library's own group tags
    ishmem_iput((double *) d + t, (const double *) s + t, 2, 3, 4, pe);
    ishmem_iget((short *) d + t, (const short *) s + t, 2, 3, 4, pe);
    ishmemx_ibput((double *) d + t, (const double *) s + t, 2, 3, 2, 4, pe);
    ishmemx_ibget((short *) d + t, (const short *) s + t, 2, 3, 2, 4, pe);
    ishmemx_iput_work_group((float *) d, (const float *) s, 2, 3, 4, pe, wave);
    ishmemx_iget_work_group((float *) d, (const float *) s, 2, 3, 4, pe, grp);
    ishmemx_ibput_work_group((float *) d, (const float *) s, 2, 3, 2, 4, pe, grp);
    ishmemx_ibget_work_group((float *) d, (const float *) s, 2, 3, 2, 4, pe, ishmemx_dev::wavefront);
    ishmemx_float_ibput_work_group((float *) d, (const float *) s, 2, 3, 2, 4, pe, ishmemx_dev::work_group);
}
int main() { return 0; }
''')
    subprocess.run([hipcc, "--offload-arch=gfx950", "-std=c++20", f"-I{INCLUDE}", "-c", str(src), "-o",
                    str(tmp_path / "t.o")], check=True)

"""alltoall without a GPU: the C ABI before init, the Python names, the host C++ names (g++, linked
against the library) and the device API (hipcc, gfx950, compile only)."""
import shutil
import subprocess
from pathlib import Path

import numpy as np

import ishmem_amd as ish
from ishmem_amd import _lib
from tests.alltoall_worker import expected_dest, member_source, pattern_block

ROOT = Path(__file__).resolve().parents[1]
INCLUDE = ROOT / "include"


def test_not_initialised_calls_fail_with_a_reason():
    assert not ish.initialized()
    L = ish.lib()
    assert L.ishmemi_c_alltoall(0, None, None, 8) != 0
    assert "not initialized" in ish.last_error()
    assert L.ishmemi_c_alltoall_on_stream(0, None, None, 8, None, None) != 0
    assert "not initialized" in ish.last_error()
    assert ish.ishmem_alltoallmem(0, 0, 0) != 0
    assert ish.alltoall_on_stream(0, 0, 0, None, 0) != 0
    assert "not initialized" in ish.last_error()


def test_python_names_exist_for_every_typename():
    assert len(ish.ARITH_TYPENAMES) == 23
    for tn in ish.ARITH_TYPENAMES:
        fn = getattr(ish, f"ishmem_{tn}_alltoall")
        assert fn.__name__ == f"ishmem_{tn}_alltoall"
        assert fn(0, 0, 1) != 0 and fn(ish.ISHMEM_TEAM_WORLD, 0, 0, 1) != 0  # both overloads; not initialised
        assert f"ishmem_{tn}_alltoall" not in ish.API_NAMES
    assert callable(ish.ishmem_alltoallmem) and callable(ish.alltoall_on_stream)
    names = [p[0] for p in _lib.PROTOTYPES]
    assert "ishmemi_c_alltoall" in names and "ishmemi_c_alltoall_on_stream" in names


def test_expected_result_helpers():
    # The tester's word (test/unit/alltoall.cpp:47-90) and the transposition, on a 3-member team.
    w = pattern_block(5, 1, 2, 8).view("<u8")[0]
    assert int(w) == (5 << 48) + (0x81 << 40) + (0x82 << 32)
    assert pattern_block(3, 0, 1, 20).view(np.uint8).size == 20
    assert int(pattern_block(3, 0, 1, 24).view("<u8")[2]) == (3 << 48) + (0x80 << 40) + (0x81 << 32) + 2
    p, B = 3, 7
    for kind in ("tester", "random"):
        src = [member_source(kind, 11, B, f, p, B) for f in range(p)]
        assert all(s.size == p * B for s in src)
        for me in range(p):
            want = np.concatenate([src[j][me * B:(me + 1) * B] for j in range(p)])
            assert np.array_equal(expected_dest(kind, 11, B, me, p, B), want)


def test_host_cxx_names_compile_link_and_fail_before_init(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed for the host C++ names"
    src = tmp_path / "t.cpp"
    src.write_text(r'''
#include <ishmem.h>
#include <ishmemx.h>
#include <cstdio>
int main() {
    float *d = nullptr; const float *s = nullptr;
    long *ld = nullptr; const long *ls = nullptr;
    hipStream_t st = nullptr;
    hipEvent_t deps[1] = {nullptr};
    int r[16], n = 0;
    r[n++] = ishmem_float_alltoall(d, s, 1);                                    // typed
    r[n++] = ishmem_float_alltoall(ISHMEM_TEAM_WORLD, d, s, 1);                 // typed, team
    r[n++] = ishmem_size_alltoall((size_t *) nullptr, (const size_t *) nullptr, 1);
    r[n++] = ishmem_alltoall(ld, ls, 1);                                        // generic
    r[n++] = ishmem_alltoall(ISHMEM_TEAM_WORLD, ld, ls, 1);                     // generic, team
    r[n++] = ishmem_alltoallmem((void *) d, (const void *) s, 4);               // mem
    r[n++] = ishmem_alltoallmem(ISHMEM_TEAM_WORLD, (void *) d, (const void *) s, 4);
    r[n++] = ishmemx_float_alltoall_on_stream(d, s, 1, nullptr, st);            // on-stream
    r[n++] = ishmemx_float_alltoall_on_stream(ISHMEM_TEAM_WORLD, d, s, 1, nullptr, st);
    r[n++] = ishmemx_alltoall_on_stream(ld, ls, 1, nullptr, st);
    r[n++] = ishmemx_alltoall_on_stream(ISHMEM_TEAM_WORLD, ld, ls, 1, nullptr, st);
    r[n++] = ishmemx_alltoallmem_on_stream((void *) d, (const void *) s, 4, nullptr, st);
    r[n++] = ishmemx_alltoallmem_on_stream(ISHMEM_TEAM_WORLD, (void *) d, (const void *) s, 4, nullptr, st);
    r[n++] = ishmemx_double_alltoall_on_stream(ISHMEM_TEAM_WORLD, (double *) nullptr, (const double *) nullptr, 1,
                                               nullptr, st, deps, 0, nullptr);  // deps / done
    r[n++] = ishmemx_alltoall_on_stream(ISHMEM_TEAM_WORLD, ld, ls, 1, nullptr, st, deps, 0, nullptr);
    r[n++] = ishmemx_alltoallmem_on_stream(ISHMEM_TEAM_WORLD, (void *) d, (const void *) s, 4, nullptr, st, deps, 0,
                                           nullptr);
    int bad = 0;
    for (int i = 0; i < n; ++i) bad += r[i] == 0;
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
    assert out.stdout.split() == ["16", "0"]


def test_device_forms_compile_for_gfx950(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert Path(hipcc).exists(), "hipcc is needed for the device API"
    src = tmp_path / "t.hip"
    src.write_text(r'''
#include <hip/hip_cooperative_groups.h>
#include <ishmem.h>
#include <ishmemx.h>
namespace cg = cooperative_groups;
__global__ void k(int *dst, const int *src, double *fd, const double *fs, ishmem_team_t team, int *rc) {
    auto grp = cg::this_thread_block();
    auto wave = cg::tiled_partition<64>(grp);
    int r = 0;
    // a thread block
    r |= ishmemx_int_alltoall_work_group(dst, src, 3, grp);
    r |= ishmemx_int_alltoall_work_group(team, dst, src, 3, grp);
    r |= ishmemx_alltoall_work_group(fd, fs, 3, grp);
    r |= ishmemx_alltoall_work_group(team, fd, fs, 3, grp);
    r |= ishmemx_alltoallmem_work_group(dst, src, 12, grp);
    r |= ishmemx_alltoallmem_work_group(team, dst, src, 12, grp);
    // a wavefront tile
    if (grp.thread_rank() < 64) {
        r |= ishmemx_double_alltoall_work_group(fd, fs, 3, wave);
        r |= ishmemx_size_alltoall_work_group(team, (size_t *) fd, (const size_t *) fs, 3, wave);
        r |= ishmemx_alltoall_work_group(team, dst, src, 3, wave);
        r |= ishmemx_alltoallmem_work_group(team, dst, src, 12, wave);
    }
    // a single thread
    if (grp.thread_rank() == 0) {
        r |= ishmem_int_alltoall(dst, src, 3);
        r |= ishmem_int_alltoall(team, dst, src, 3);
        r |= ishmem_alltoall(fd, fs, 3);
        r |= ishmem_alltoall(team, fd, fs, 3);
        r |= ishmem_alltoallmem(dst, src, 12);
        r |= ishmem_alltoallmem(team, dst, src, 12);
        *rc = r;
    }
}
int main() { return 0; }
''')
    subprocess.run([hipcc, "--offload-arch=gfx950", "-std=c++20", f"-I{INCLUDE}", "-c", str(src), "-o",
                    str(tmp_path / "t.o")], check=True)

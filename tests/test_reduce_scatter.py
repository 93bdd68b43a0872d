"""The reduce-scatter extension without a GPU: the C ABI before init, the Python names, the slicing
helper of the GPU tests, the host C++ names (g++, linked against the library) and the device forms
(hipcc, gfx950, compile only)."""
import shutil
import subprocess
from pathlib import Path

import numpy as np

import ishmem_amd as ish
import oracle
from ishmem_amd import _lib
from tests import half_model as hm
from tests import reduce_scatter_worker as rsw

ROOT = Path(__file__).resolve().parents[1]
INCLUDE = ROOT / "include"


def test_not_initialised_calls_fail_with_a_reason():
    assert not ish.initialized()
    L = ish.lib()
    assert L.ishmemi_c_reduce_scatter(0, 5, 8, None, None, 8) != 0
    assert "not initialized" in ish.last_error()
    assert L.ishmemi_c_reduce_scatter_on_stream(0, 5, 8, None, None, 8, None, None) != 0
    assert "not initialized" in ish.last_error()
    assert L.ishmemi_c_reduce_scatter_on_stream_deps(0, 5, 8, None, None, 8, None, None, None, 0, None) != 0
    assert "not initialized" in ish.last_error()
    assert ish.reduce_scatter("sum", "float", 0, 0, 1) != 0
    assert ish.reduce_scatter_on_stream("sum", "bfloat16", 0, 0, 1, None, 0) != 0
    assert "not initialized" in ish.last_error()
    names = [p[0] for p in _lib.PROTOTYPES]
    for n in ("ishmemi_c_reduce_scatter", "ishmemi_c_reduce_scatter_on_stream", "ishmemi_c_reduce_scatter_on_stream_deps"):
        assert n in names


def test_python_names_exist_for_the_whole_matrix():
    want = []
    for op, tns in ish.TYPENAMES_FOR_OP.items():
        for tn in [*tns, *(ish.HALF_TYPENAMES if op in ("max", "min", "sum", "prod") else [])]:
            want += [f"ishmemx_{tn}_{op}_reduce_scatter", f"ishmemx_{tn}_{op}_reduce_scatter_on_stream"]
    assert len(want) == 2 * (14 * 3 + 23 * 4 + 2 * 4)
    assert sorted(ish.REDUCE_SCATTER_NAMES) == sorted(want)
    for name in want:
        fn = getattr(ish, name)
        assert fn.__name__ == name
        if name.endswith("_on_stream"):  # both overloads; not initialised
            assert fn(0, 0, 1, None, 0) != 0 and fn(ish.ISHMEM_TEAM_WORLD, 0, 0, 1, None, 0) != 0
        else:
            assert fn(0, 0, 1) != 0 and fn(ish.ISHMEM_TEAM_WORLD, 0, 0, 1) != 0
    older = set(ish.API_NAMES) | set(ish.HALF_NAMES) | set(ish.AMO_NAMES)
    assert not older & set(ish.REDUCE_SCATTER_NAMES)
    for bad in ("ishmemx_float_and_reduce_scatter", "ishmemx_half_xor_reduce_scatter"):
        assert not hasattr(ish, bad)


def test_slicing_helper_on_a_hand_built_three_member_case():
    # 3 members, 2 elements per block: member j's source is [10 j + 0 .. 10 j + 5].
    p, n = 3, 2
    srcs = [np.arange(6, dtype=np.int32) + 10 * j for j in range(p)]
    full = rsw.full_fold("sum", "int32", srcs)
    assert full.tolist() == [30, 33, 36, 39, 42, 45]
    assert [rsw.block_of(full, k, n).tolist() for k in range(p)] == [[30, 33], [36, 39], [42, 45]]
    for k in range(p):
        by_hand = sum(s[k * n:(k + 1) * n] for s in srcs)
        assert not rsw.mismatches("sum", "int32", srcs, full, by_hand.astype(np.int32), k, n)
    # the next member's block, and a dropped last element, are told apart
    assert rsw.mismatches("sum", "int32", srcs, full, rsw.block_of(full, 1, n), 0, n)
    assert rsw.mismatches("sum", "int32", srcs, full, rsw.block_of(full, 0, n)[:1], 0, n)
    # float sum: the team-order fold (member 0 first), not the reverse order
    f = [np.array([1e8, 1.0, 0.0], np.float32), np.array([-1e8, 1.0, 0.0], np.float32), np.array([1.0, 1.0, 0.0], np.float32)]
    full = rsw.full_fold("sum", "float", f)
    assert full[0] == np.float32(1.0)  # (1e8 - 1e8) + 1; the reverse order gives 0
    assert rsw.mismatches("sum", "float", f, full, np.array([0.0], np.float32), 0, 1)
    # the 16-bit types go through the model and its comparison rule
    h = rsw.sources("sum", "bfloat16", 3, 64, 5)
    assert all(s.dtype == np.uint16 and s.size == 3 * 64 for s in h)
    full = rsw.full_fold("sum", "bfloat16", h)
    assert np.array_equal(full, hm.fold("bfloat16", "sum", h))
    assert not rsw.mismatches("sum", "bfloat16", h, full, rsw.block_of(full, 2, 64), 2, 64)
    assert rsw.mismatches("sum", "bfloat16", h, full, rsw.block_of(full, 1, 64), 2, 64)


def test_block_sizes_and_inputs():
    for es in (1, 2, 4, 8):
        sizes = rsw.block_sizes(es)
        it = 16 // es
        assert {1, it + 1, 1027, 64 * it - 1, 64 * it + 1, 4099 * it, 1024 // es - 1} <= set(sizes)
        assert max(sizes) * es * 8 < 1 << 20  # the largest source per PE, 8 members
        assert (1024 // es - 1) * es < rsw.REALIGN_MIN
    assert (1027 * 4) % 16 and (1027 * 2) % 16 and (1027 * 8) % 16  # members' blocks on different phases
    for op, lo, hi in (("prod", 0.5, 2.0), ("sum", -1.0, 1.0)):
        for s in rsw.sources(op, "double", 3, 100, 1):
            assert s.size == 300 and (s >= lo).all() and (s < hi).all()
    a, b = rsw.sources("xor", "uint64", 2, 50, 3)
    assert a.dtype == np.uint64 and not np.array_equal(a, b)
    assert oracle.valid(oracle.OPS["sum"], oracle.DTYPES["float"])


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
    ishmemx_half_t *hd = nullptr; const ishmemx_half_t *hs = nullptr;
    ishmemx_bfloat16_t *bd = nullptr; const ishmemx_bfloat16_t *bs = nullptr;
    hipStream_t st = nullptr;
    hipEvent_t deps[1] = {nullptr};
    int r[32], n = 0;
    r[n++] = ishmemx_float_sum_reduce_scatter(d, s, 1);                                   // typed
    r[n++] = ishmemx_float_sum_reduce_scatter(ISHMEM_TEAM_WORLD, d, s, 1);                // typed, team
    r[n++] = ishmemx_size_xor_reduce_scatter((size_t *) nullptr, (const size_t *) nullptr, 1);
    r[n++] = ishmemx_long_max_reduce_scatter(ld, ls, 1);
    r[n++] = ishmemx_prod_reduce_scatter(ld, ls, 1);                                      // generic
    r[n++] = ishmemx_min_reduce_scatter(ISHMEM_TEAM_WORLD, d, s, 1);                      // generic, team
    r[n++] = ishmemx_float_sum_reduce_scatter_on_stream(d, s, 1, nullptr, st);            // on-stream
    r[n++] = ishmemx_float_sum_reduce_scatter_on_stream(ISHMEM_TEAM_WORLD, d, s, 1, nullptr, st);
    r[n++] = ishmemx_and_reduce_scatter_on_stream(ld, ls, 1, nullptr, st);
    r[n++] = ishmemx_or_reduce_scatter_on_stream(ISHMEM_TEAM_WORLD, ld, ls, 1, nullptr, st);
    r[n++] = ishmemx_double_prod_reduce_scatter_on_stream((double *) nullptr, (const double *) nullptr, 1, nullptr, st,
                                                          deps, 0, nullptr);              // deps / done
    r[n++] = ishmemx_double_prod_reduce_scatter_on_stream(ISHMEM_TEAM_WORLD, (double *) nullptr,
                                                          (const double *) nullptr, 1, nullptr, st, deps, 0, nullptr);
    r[n++] = ishmemx_sum_reduce_scatter_on_stream(ISHMEM_TEAM_WORLD, ld, ls, 1, nullptr, st, deps, 0, nullptr);
    r[n++] = ishmemx_half_sum_reduce_scatter(hd, hs, 1);                                  // the 16-bit types
    r[n++] = ishmemx_half_max_reduce_scatter(ISHMEM_TEAM_WORLD, hd, hs, 1);
    r[n++] = ishmemx_bfloat16_prod_reduce_scatter(bd, bs, 1);
    r[n++] = ishmemx_bfloat16_min_reduce_scatter_on_stream(ISHMEM_TEAM_WORLD, bd, bs, 1, nullptr, st);
    r[n++] = ishmemx_bfloat16_sum_reduce_scatter_on_stream(bd, bs, 1, nullptr, st, deps, 0, nullptr);
    r[n++] = ishmemx_sum_reduce_scatter(hd, hs, 1);                                       // generic, 16-bit
    r[n++] = ishmemx_max_reduce_scatter_on_stream(ISHMEM_TEAM_WORLD, bd, bs, 1, nullptr, st);
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
    assert out.stdout.split() == ["20", "0"]


def test_device_forms_compile_for_gfx950(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert Path(hipcc).exists(), "hipcc is needed for the device API"
    src = tmp_path / "t.hip"
    src.write_text(r'''
#include <hip/hip_cooperative_groups.h>
#include <ishmem.h>
#include <ishmemx.h>
namespace cg = cooperative_groups;
__global__ void k(int *dst, const int *src, double *fd, const double *fs, ishmemx_half_t *hd, const ishmemx_half_t *hs,
                  ishmemx_bfloat16_t *bd, const ishmemx_bfloat16_t *bs, ishmem_team_t team, int *rc) {
    auto grp = cg::this_thread_block();
    auto wave = cg::tiled_partition<64>(grp);
    int r = 0;
    // a thread block
    r |= ishmemx_int_sum_reduce_scatter_work_group(dst, src, 3, grp);
    r |= ishmemx_int32_xor_reduce_scatter_work_group(team, dst, src, 3, grp);
    r |= ishmemx_prod_reduce_scatter_work_group(fd, fs, 3, grp);
    r |= ishmemx_min_reduce_scatter_work_group(team, fd, fs, 3, grp);
    r |= ishmemx_half_sum_reduce_scatter_work_group(hd, hs, 3, grp);
    r |= ishmemx_bfloat16_max_reduce_scatter_work_group(team, bd, bs, 3, grp);
    // a wavefront tile
    if (grp.thread_rank() < 64) {
        r |= ishmemx_double_max_reduce_scatter_work_group(fd, fs, 3, wave);
        r |= ishmemx_size_or_reduce_scatter_work_group(team, (size_t *) fd, (const size_t *) fs, 3, wave);
        r |= ishmemx_sum_reduce_scatter_work_group(team, dst, src, 3, wave);
        r |= ishmemx_bfloat16_prod_reduce_scatter_work_group(bd, bs, 3, wave);
        r |= ishmemx_sum_reduce_scatter_work_group(team, (_Float16 *) hd, (const _Float16 *) hs, 3, wave);
    }
    // a single thread
    if (grp.thread_rank() == 0) {
        r |= ishmemx_int_sum_reduce_scatter(dst, src, 3);
        r |= ishmemx_int32_and_reduce_scatter(team, dst, src, 3);
        r |= ishmemx_prod_reduce_scatter(fd, fs, 3);
        r |= ishmemx_max_reduce_scatter(team, fd, fs, 3);
        r |= ishmemx_half_min_reduce_scatter(hd, hs, 3);
        r |= ishmemx_bfloat16_sum_reduce_scatter(team, bd, bs, 3);
        *rc = r;
    }
}
int main() { return 0; }
''')
    subprocess.run([hipcc, "--offload-arch=gfx950", "-std=c++20", f"-I{INCLUDE}", "-c", str(src), "-o",
                    str(tmp_path / "t.o")], check=True)

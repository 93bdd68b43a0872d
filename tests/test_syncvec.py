"""The vector waits and tests (wait_until_all / any / some, test_all / any / some, _vector forms)
without a GPU: the Python model of tests/syncvec_cases.py against hand-written expectations, the C ABI
before init, the Python names, the host C++ names (g++, linked against the library) and the device API
(hipcc, gfx950, compile only)."""
import ctypes
import re
import shutil
import subprocess
from pathlib import Path

import ishmem_amd as ish
from ishmem_amd import _lib
from tests.signal_worker import EQ, GE, GT, LE, LT, NE, SYNC_TYPES, flip_case
from tests.syncvec_cases import (CHUNK, CMPS, OPS, SIZE_MAX, SIZES, case_values, model, size_cases, status_array,
                                 type_cases, wait_set)

ROOT = Path(__file__).resolve().parents[1]
INCLUDE = ROOT / "include"
C_NAMES = ["ishmemi_c_sync_vector", "ishmemi_c_sync_vector_on_stream"]
C_TYPES = {"int": "int", "long": "long", "longlong": "long long", "uint": "unsigned int", "ulong": "unsigned long",
           "ulonglong": "unsigned long long", "int32": "int32_t", "int64": "int64_t", "uint32": "uint32_t",
           "uint64": "uint64_t", "size": "size_t", "ptrdiff": "ptrdiff_t"}


def test_model_signedness_and_width_traps():
    # int32 -1 against 0 and uint32 0xFFFFFFFF against 0 are the same bits
    for op, signed_r, unsigned_r in (("test_all", 0, 1), ("test_any", SIZE_MAX, 0), ("test_some", 0, 1)):
        assert model(op, [0xFFFFFFFF], None, GT, 0, 32, True).result == signed_r
        assert model(op, [0xFFFFFFFF], None, GT, 0, 32, False).result == unsigned_r
    # 64-bit values that differ only above bit 32: a comparison of the low halves would call them equal
    a, b = 7, 7 + (1 << 32)
    assert model("test_all", [a, a], None, EQ, b, 64, False).result == 0
    assert model("test_some", [a, b, a], None, LT, b, 64, True).indices == [0, 2]
    assert model("test_any", [b, a], None, EQ, [a, b], 64, True).result == SIZE_MAX  # _vector: element-wise
    assert model("test_any", [b, a], None, EQ, [b, b], 64, True).result == 0
    # the top bit of a 64-bit value is a sign only when signed
    assert model("test_all", [7 + (1 << 63)], None, GT, 7, 64, False).result == 1
    assert model("test_all", [7 + (1 << 63)], None, GT, 7, 64, True).result == 0
    # every flip case: `before` never satisfies, `after` always does, in the variable's own type
    for bits, signed in set(SYNC_TYPES.values()):
        for cmp in CMPS:
            before, cval, after = flip_case(bits, signed, cmp)
            assert model("test_all", [after, after], None, cmp, cval, bits, signed).result == 1
            assert model("test_some", [before, after, before], None, cmp, cval, bits, signed).indices == [1]
            assert model("wait_until_any", [before, before], None, cmp, cval, bits, signed).blocks


def test_model_empty_wait_set_and_exclusion():
    for status, values in ((None, []), ([1, 2], [5, 5]), ([7], [0])):
        for op, want in (("wait_until_all", 1), ("test_all", 1), ("wait_until_any", SIZE_MAX), ("test_any", SIZE_MAX),
                         ("wait_until_some", 0), ("test_some", 0)):
            o = model(op, values, status, EQ, 99, 64, False, rotor=3)
            assert (o.result, o.indices, o.blocks, o.rotor) == (want, [], False, 3), (op, status)
    # an excluded element neither satisfies nor holds up
    assert model("wait_until_all", [1, 0, 1], [0, 1, 0], EQ, 1, 32, True).result == 1
    assert model("wait_until_all", [1, 0, 1], [0, 0, 0], EQ, 1, 32, True).blocks
    assert model("test_any", [1, 0], [1, 0], EQ, 1, 32, True).result == SIZE_MAX
    assert model("test_some", [1, 1, 1, 1], [0, 1, 0, 9], EQ, 1, 32, True).indices == [0, 2]
    assert wait_set(4, [0, 1, 0, 9]) == [0, 2] and wait_set(2, None) == [0, 1]
    assert status_array("null", 5, 0) is None and not any(status_array("zero", 5, 0)) and all(status_array("all", 5, 0))
    for n in (2, 5, 65):
        for seed in range(3):
            st = status_array("mixed", n, seed)
            assert 0 < sum(1 for x in st if x) < n or n == 2


def test_model_some_is_ascending_and_any_rotates():
    vals = [1] * 7
    assert model("test_some", vals, None, EQ, 1, 32, True).indices == list(range(7))
    assert model("wait_until_some", [0, 1, 0, 1, 1], None, NE, 0, 64, False).indices == [1, 3, 4]
    # the scan starts behind the index last returned, modulo nelems: N calls visit every element once
    rotor, seen = 0, []
    for _ in range(7):
        o = model("wait_until_any", vals, None, EQ, 1, 32, True, rotor)
        rotor = o.rotor
        seen.append(o.result)
    assert seen == [1, 2, 3, 4, 5, 6, 0]
    # excluded elements are skipped; a rotor left by a longer array wraps
    st = [0, 1, 0, 0, 1]
    rotor, seen = 11, []
    for _ in range(3):
        o = model("test_any", [1] * 5, st, EQ, 1, 32, True, rotor)
        rotor = o.rotor
        seen.append(o.result)
    assert seen == [2, 3, 0]
    # no match leaves the rotor alone
    assert model("test_any", [0, 0], None, EQ, 1, 32, True, rotor=1).rotor == 1
    assert model("test_any", [0, 1, 1], None, EQ, 1, 32, True, rotor=1).result == 2
    assert model("test_any", [1, 1, 0], None, EQ, 1, 32, True, rotor=1).result == 0


def test_case_tables_cover_what_the_gpu_tests_claim():
    tc, sc = type_cases(), size_cases()
    assert {(c[0], c[3], c[6]) for c in tc} == {(tn, cmp, v) for tn in SYNC_TYPES for cmp in CMPS for v in (False, True)}
    assert {c[4] for c in sc} == set(SIZES) and {0, 1, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1} == set(SIZES)
    assert {(c[4], c[5], c[6]) for c in sc} == {(n, sk, v) for n in SIZES for sk in ("null", "zero", "mixed", "all")
                                                for v in (False, True)}
    header = (ROOT / "ishmem_amd/csrc/kernels.h").read_text()
    assert re.search(r"kSyncUnroll = (\d+);", header) and 64 * int(re.search(r"kSyncUnroll = (\d+);", header).group(1)) == CHUNK
    # both answers occur among the elements of a case, and the _vector form differs from the scalar one somewhere
    outcomes = set()
    for tn, bits, signed, cmp, n, sk, vector, seed in tc:
        values, cv = case_values(n, bits, signed, cmp, seed, vector)
        o = model("test_some", values, status_array(sk, n, seed), cmp, cv, bits, signed)
        outcomes.add(0 < o.result < n)
        assert isinstance(cv, list) == vector
    assert outcomes == {True, False}  # "all" status cases give 0, the others a proper subset


def test_c_symbols_are_declared_exported_and_bound():
    lib = ish.lib()
    header = (INCLUDE / "ishmem_capi.h").read_text()
    names = [p[0] for p in _lib.PROTOTYPES]
    nm = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], capture_output=True, text=True).stdout
    for n in C_NAMES:
        assert f"{n}(" in header and n in names and hasattr(lib, n) and re.search(rf" T {n}\b", nm), n
    codes = dict(re.findall(r"#define ISHMEMI_C_SYNC_(\w+) (\d+)", header))
    assert codes == {"WAIT_ALL": "0", "WAIT_ANY": "1", "WAIT_SOME": "2", "TEST_ALL": "3", "TEST_ANY": "4", "TEST_SOME": "5",
                     "VECTOR": "16"}
    assert {f"ISHMEMI_C_SYNC_{'WAIT' if k.startswith('wait') else 'TEST'}_{k.rsplit('_', 1)[1].upper()}": str(v)
            for k, v in ish.SYNC_MODES.items()} == {f"ISHMEMI_C_SYNC_{k}": v for k, v in codes.items() if k != "VECTOR"}
    assert ish.SYNC_VECTOR_FLAG == 16 and ish.SIZE_MAX == SIZE_MAX
    # the rotor pointer is the context's last member
    ctx = header[header.index("typedef struct {"):header.index("} ishmemi_c_device_ctx_t;")]
    assert ctx.strip().splitlines()[-1].strip().startswith("uint64_t *sync_rotor;")


def test_python_names_and_not_initialised_calls():
    assert not ish.initialized()
    want = [f"ishmem_{tn}_{op}{v}" for tn in ish.SYNC_TYPENAMES for op in OPS for v in ("", "_vector")]
    assert len(want) == 144 and sorted(want) == sorted(ish.SYNC_VECTOR_NAMES)
    assert list(ish.SYNC_MODES) == OPS
    # the earlier lists keep their contents
    assert len(ish.SIGNAL_NAMES) == 6 + 23 * 2 + 5 * 2 + 12 * 2
    assert not set(ish.SYNC_VECTOR_NAMES) & (set(ish.SIGNAL_NAMES) | set(ish.API_NAMES))
    assert not [n for n in ish.SIGNAL_NAMES + ish.API_NAMES if re.search(r"_(all|any|some)(_vector)?$", n)]
    L = ish.lib()
    r = ctypes.c_size_t(5)
    for mode in range(6):
        for vec in (0, 16):
            assert L.ishmemi_c_sync_vector(mode | vec, ish.DTYPES["int64"], None, 4, None, None, EQ, 1, None, ctypes.byref(r)) != 0
            assert "not initialized" in ish.last_error(), mode
            assert r.value == (SIZE_MAX if mode in (1, 4) else 0)
            assert L.ishmemi_c_sync_vector_on_stream(mode | vec, ish.DTYPES["uint32"], None, 4, None, None, NE, 1, None, None,
                                                     None, None) != 0
            assert "not initialized" in ish.last_error(), mode
    assert L.ishmemi_c_sync_vector(99, 0, None, 0, None, None, 0, 0, None, None) != 0 and "not initialized" in ish.last_error()
    for name in want:
        fn = getattr(ish, name)
        assert fn.__name__ == name
        op = name.split("_", 2)[2]
        got = fn(0, 3, 0, 0, EQ, 1) if "some" in op else fn(0, 3, 0, EQ, 1)
        assert "not initialized" in ish.last_error(), name
        # wait_until_all reports the status; the others their "nothing found" value
        assert got == (SIZE_MAX if "any" in op else 0) or (op.startswith("wait_until_all") and got != 0), name
    for op in OPS:
        assert ish.sync_vector(op, "int32", 0, 1, 0, 0, EQ, 1)[0] != 0 and "not initialized" in ish.last_error()
        assert ish.sync_vector_on_stream(op, "int32", 0, 1, 0, 0, EQ, 1, 0, 0, 0, 0) != 0
        assert "not initialized" in ish.last_error()


def host_cxx_source() -> tuple[str, int]:
    """Every host form for every typename (12 blocking operations, 6 on-stream waits and the deps / done
    overload of each on-stream wait), the templates once; each call must fail with "not initialized"."""
    lines, n = [], 0
    for tn, ty in C_TYPES.items():
        p, cv, cvs = f"({ty} *) nullptr", f"({ty}) 1", f"(const {ty} *) nullptr"
        for vec, c in (("", cv), ("_vector", cvs)):
            lines += [f"    V(ishmem_{tn}_wait_until_all{vec}({p}, 3, st, ISHMEM_CMP_EQ, {c}));",
                      f"    A(ishmem_{tn}_wait_until_any{vec}({p}, 3, st, ISHMEM_CMP_NE, {c}));",
                      f"    Z(ishmem_{tn}_wait_until_some{vec}({p}, 3, idx, st, ISHMEM_CMP_GT, {c}));",
                      f"    Z((size_t) ishmem_{tn}_test_all{vec}({p}, 3, st, ISHMEM_CMP_GE, {c}));",
                      f"    A(ishmem_{tn}_test_any{vec}({p}, 3, st, ISHMEM_CMP_LT, {c}));",
                      f"    Z(ishmem_{tn}_test_some{vec}({p}, 3, idx, st, ISHMEM_CMP_LE, {c}));",
                      f"    I(ishmemx_{tn}_wait_until_all{vec}_on_stream({p}, 3, st, ISHMEM_CMP_EQ, {c}, stream));",
                      f"    I(ishmemx_{tn}_wait_until_any{vec}_on_stream({p}, 3, st, ISHMEM_CMP_EQ, {c}, ret, stream));",
                      f"    I(ishmemx_{tn}_wait_until_some{vec}_on_stream({p}, 3, idx, st, ISHMEM_CMP_EQ, {c}, ret, stream));",
                      f"    I(ishmemx_{tn}_wait_until_all{vec}_on_stream({p}, 3, st, ISHMEM_CMP_EQ, {c}, stream, deps, 0, nullptr));",
                      f"    I(ishmemx_{tn}_wait_until_any{vec}_on_stream({p}, 3, st, ISHMEM_CMP_EQ, {c}, ret, stream, deps, 0, nullptr));",
                      f"    I(ishmemx_{tn}_wait_until_some{vec}_on_stream({p}, 3, idx, st, ISHMEM_CMP_EQ, {c}, ret, stream, deps, 0, nullptr));"]
            n += 12
    lines += ["    V(ishmem_wait_until_all(lp, 3, st, ISHMEM_CMP_EQ, 1L));",
              "    A(ishmem_wait_until_any_vector(lp, 3, st, ISHMEM_CMP_EQ, (const long *) lp));",
              "    Z(ishmem_wait_until_some(lp, 3, idx, st, ISHMEM_CMP_EQ, 1L));",
              "    Z((size_t) ishmem_test_all_vector(lp, 3, st, ISHMEM_CMP_EQ, (const long *) lp));",
              "    A(ishmem_test_any(lp, 3, st, ISHMEM_CMP_EQ, 1L));",
              "    Z(ishmem_test_some_vector(lp, 3, idx, st, ISHMEM_CMP_EQ, (const long *) lp));",
              "    I(ishmemx_wait_until_all_on_stream(lp, 3, st, ISHMEM_CMP_EQ, 1L, stream));",
              "    I(ishmemx_wait_until_any_vector_on_stream(lp, 3, st, ISHMEM_CMP_EQ, (const long *) lp, ret, stream));",
              "    I(ishmemx_wait_until_some_on_stream(lp, 3, idx, st, ISHMEM_CMP_EQ, 1L, ret, stream, deps, 0, nullptr));"]
    n += 9
    body = "\n".join(lines)
    return r'''
#include <ishmem.h>
#include <ishmemx.h>
#include <cstdio>
#include <cstring>
#include <type_traits>
static int bad = 0, n = 0;
static void expect_reason(const char *what) {
    ++n;
    if (!std::strstr(ishmemi_c_last_error(), "not initialized")) { ++bad; std::printf("%s: %s\n", what, ishmemi_c_last_error()); }
}
#define V(call) do { static_assert(std::is_void<decltype(call)>::value, "void"); call; expect_reason(#call); } while (0)
#define A(call) do { static_assert(std::is_same<decltype(call), size_t>::value, "size_t"); \
                     if ((call) != SIZE_MAX) { ++bad; std::printf("%s did not return SIZE_MAX\n", #call); } expect_reason(#call); } while (0)
#define Z(call) do { if ((call) != 0) { ++bad; std::printf("%s did not return 0\n", #call); } expect_reason(#call); } while (0)
#define I(call) do { if ((call) == 0) { ++bad; std::printf("%s returned 0\n", #call); } expect_reason(#call); } while (0)
int main() {
    const int *st = nullptr;
    size_t *idx = nullptr, *ret = nullptr;
    long *lp = nullptr;
    hipStream_t stream = nullptr;
    hipEvent_t deps[1] = {nullptr};
    static_assert(std::is_same<decltype(ishmem_int_test_all((int *) nullptr, 0, st, 1, 1)), int>::value, "test_all returns int");
    static_assert(std::is_same<decltype(ishmem_size_wait_until_some_vector((size_t *) nullptr, 0, idx, st, 1, (const size_t *) nullptr)),
                               size_t>::value, "some returns size_t");
''' + body + r'''
    // nelems == 0 is the empty wait set only for an initialised library
    std::printf("%d %d\n", n, bad);
    return 0;
}
''', n


def test_host_cxx_names_compile_link_and_fail_before_init(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed for the host C++ names"
    text, calls = host_cxx_source()
    assert calls == 12 * 2 * 12 + 9
    src = tmp_path / "t.cpp"
    src.write_text(text)
    exe = tmp_path / "t"
    subprocess.run([gxx, "-std=c++17", "-Wall", "-Werror", f"-I{INCLUDE}", str(src), "-o", str(exe),
                    f"-L{_lib.LIB_PATH.parent}", f"-Wl,-rpath,{_lib.LIB_PATH.parent}", "-lishmem_amd"], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split()[-2:] == [str(calls), "0"], out.stdout[-2000:]


def device_source() -> str:
    """Every device form: one work-item and a thread block for every typename, a 64-lane tile and the
    library's tags for three of them, the templates once."""
    def forms(tn, ty, suffix, grp):
        g = f", {grp}" if grp else ""
        pre = "ishmemx" if grp else "ishmem"
        out = []
        for vec, c in (("", f"({ty}) 1"), ("_vector", f"(const {ty} *) cv")):
            p = f"({ty} *) iv"
            out += [f"    {pre}_{tn}_wait_until_all{vec}{suffix}({p}, n, st, ISHMEM_CMP_EQ, {c}{g});",
                    f"    acc += {pre}_{tn}_wait_until_any{vec}{suffix}({p}, n, st, ISHMEM_CMP_NE, {c}{g});",
                    f"    acc += {pre}_{tn}_wait_until_some{vec}{suffix}({p}, n, idx, st, ISHMEM_CMP_GT, {c}{g});",
                    f"    acc += (size_t) {pre}_{tn}_test_all{vec}{suffix}({p}, n, st, ISHMEM_CMP_GE, {c}{g});",
                    f"    acc += {pre}_{tn}_test_any{vec}{suffix}({p}, n, st, ISHMEM_CMP_LT, {c}{g});",
                    f"    acc += {pre}_{tn}_test_some{vec}{suffix}({p}, n, idx, st, ISHMEM_CMP_LE, {c}{g});"]
        return out
    kernels = []
    for tn, ty in C_TYPES.items():
        body = forms(tn, ty, "_work_group", "grp") + forms(tn, ty, "", "")
        if tn in ("int", "uint64", "ptrdiff"):
            body += ["    if (grp.thread_rank() < 64) {"] + forms(tn, ty, "_work_group", "wave") + ["    }"]
        kernels.append(f"__global__ void k_{tn}(void *iv, const void *cv, size_t n, size_t *idx, const int *st, size_t *out) {{\n"
                       "    auto grp = cg::this_thread_block();\n    auto wave = cg::tiled_partition<64>(grp);\n"
                       "    size_t acc = 0;\n" + "\n".join(body) + "\n    (void) wave;\n    out[grp.thread_rank()] = acc;\n}\n")
    return r'''
#include <hip/hip_cooperative_groups.h>
#include <ishmem.h>
#include <ishmemx.h>
namespace cg = cooperative_groups;
''' + "\n".join(kernels) + r'''
__global__ void k_generic(long *lv, const long *lc, size_t n, size_t *idx, const int *st, size_t *out) {
    auto grp = cg::this_thread_block();
    size_t acc = 0;
    ishmem_wait_until_all(lv, n, st, ISHMEM_CMP_EQ, 1L);
    acc += ishmem_wait_until_any_vector(lv, n, st, ISHMEM_CMP_EQ, lc);
    acc += ishmem_test_some(lv, n, idx, st, ISHMEM_CMP_EQ, 1L);
    ishmemx_wait_until_all_vector_work_group(lv, n, st, ISHMEM_CMP_EQ, lc, grp);
    acc += ishmemx_wait_until_some_work_group(lv, n, idx, st, ISHMEM_CMP_EQ, 1L, ishmemx_dev::work_group);
    acc += ishmemx_test_any_work_group(lv, n, st, ISHMEM_CMP_EQ, 1L, ishmemx_dev::wavefront);
    acc += (size_t) ishmemx_test_all_vector_work_group(lv, n, st, ISHMEM_CMP_EQ, lc, ishmemx_dev::thread);
    out[grp.thread_rank()] = acc;
}
int main() { return 0; }
'''


def test_device_forms_compile_for_gfx950(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert Path(hipcc).exists(), "hipcc is needed for the device API"
    src = tmp_path / "t.hip"
    text = device_source()
    assert len(re.findall(r"_work_group\(", text)) == 12 * 12 + 3 * 12 + 4 and text.count("ishmem_uint32_test_some_vector(") == 1
    src.write_text(text)
    subprocess.run([hipcc, "--offload-arch=gfx950", "-std=c++20", "-O1", f"-I{INCLUDE}", "-c", str(src), "-o",
                    str(tmp_path / "t.o")], check=True)

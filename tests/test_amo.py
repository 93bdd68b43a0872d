"""The atomic memory operations without a GPU: the C ABI before init, the Python names, the model the
GPU tests take their expected values from, the set of C++ names of the host and the device header
against the committed list (tests/golden/amo_names.txt), a host program that calls every typed name
(g++, linked against the library), a device translation unit that calls every typed name and every
template (hipcc, gfx950, compile only), and the templates' type lists refusing a wrong type."""
import ctypes
import re
import shutil
import subprocess
from pathlib import Path

import pytest

import ishmem_amd as ish
from ishmem_amd import _lib
from tests.amo_worker import FETCHING, OPS, amo_model

ROOT = Path(__file__).resolve().parents[1]
INCLUDE = ROOT / "include"
GOLDEN = ROOT / "tests" / "golden" / "amo_names.txt"
NAME_RE = re.compile(r"\bishmem_\w*atomic_\w+")

BIT = {"uint": "unsigned int", "ulong": "unsigned long", "ulonglong": "unsigned long long", "int32": "int32_t",
       "int64": "int64_t", "uint32": "uint32_t", "uint64": "uint64_t"}
STD = {**BIT, "int": "int", "long": "long", "longlong": "long long", "size": "size_t", "ptrdiff": "ptrdiff_t"}
EXT = {**STD, "float": "float", "double": "double"}
EXT_OPS = ["fetch", "set", "swap", "fetch_nbi", "swap_nbi"]
STD_OPS = ["compare_swap", "fetch_inc", "inc", "fetch_add", "add", "compare_swap_nbi", "fetch_inc_nbi", "fetch_add_nbi"]
BIT_OPS = ["fetch_and", "fetch_or", "fetch_xor", "and", "or", "xor", "fetch_and_nbi", "fetch_or_nbi", "fetch_xor_nbi"]


def hipcc() -> str:
    exe = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert Path(exe).exists(), "hipcc is needed for the device API"
    return exe


def golden_names() -> list[str]:
    lines = GOLDEN.read_text().splitlines()
    assert lines[0].startswith("#") and "reference" in lines[0]
    return [ln for ln in lines[1:] if ln.strip()]


def matrix() -> list[tuple[str, str, str]]:
    """(typename, C type, op) of the issue's table: 229 typed names."""
    out = []
    for ops, types in ((EXT_OPS, EXT), (STD_OPS, STD), (BIT_OPS, BIT)):
        out += [(tn, t, op) for op in ops for tn, t in types.items()]
    return out


def call_text(name: str, op: str, ctype: str, dest: str, fetch: str) -> str:
    """One call of `name` with the reference's signature for `op` (src/amo.cpp:93-134, :230-253)."""
    base = op[:-4] if op.endswith("_nbi") else op
    one = f"({ctype}) 1"
    args = [dest]
    if base == "compare_swap":
        args += [one, one]
    elif base not in ("fetch", "fetch_inc", "inc"):
        args += [one]
    if op.endswith("_nbi"):
        return f"{name}({', '.join([fetch] + args + ['pe'])});"
    if base in FETCHING:
        return f"(void) {name}({', '.join(args + ['pe'])});"
    return f"{name}({', '.join(args + ['pe'])});"


def test_the_matrix_is_the_committed_list():
    typed = {f"ishmem_{tn}_atomic_{op}" for tn, _, op in matrix()}
    generic = {f"ishmem_atomic_{op}" for op in EXT_OPS + STD_OPS + BIT_OPS}
    assert len(typed) == 229 and len(generic) == 22
    names = golden_names()
    assert len(names) == len(set(names)) == 251
    assert set(names) == typed | generic
    assert not [n for n in names if "schar" in n]


def test_not_initialised_calls_fail_with_a_reason():
    assert not ish.initialized()
    L = ish.lib()
    f = ctypes.c_uint64(7)
    assert L.ishmemi_c_amo(ish.AMO_OPS["fetch_add"], ish.DTYPES["int32"], None, 1, 0, 0, ctypes.byref(f)) != 0
    assert "not initialized" in ish.last_error() and f.value == 7
    assert L.ishmemi_c_amo_nbi(ish.AMO_OPS["swap"], ish.DTYPES["double"], None, None, 1, 0, 0) != 0
    assert "not initialized" in ish.last_error()
    assert L.ishmemi_c_amo(99, 0, None, 1, 0, 0, None) != 0 and "not initialized" in ish.last_error()
    for name in ish.AMO_NAMES:
        op = name[len("atomic_"):]
        nbi = op.endswith("_nbi")
        base = op[:-4] if nbi else op
        args = [0] * (1 if nbi else 0) + [0, "uint64"]
        args += [1, 2] if base == "compare_swap" else [] if base in ("fetch", "fetch_inc", "inc") else [1]
        r = getattr(ish, name)(*args, 0)
        assert (r != 0) if nbi else (r[0] != 0 and r[1] == 0), name
        assert "not initialized" in ish.last_error(), name


def test_python_names_exist():
    assert list(ish.AMO_OPS) == list(OPS) and sorted(ish.AMO_OPS.values()) == list(range(14))
    assert tuple(ish.AMO_FETCHING) == FETCHING
    want = [f"atomic_{op}" for op in OPS] + [f"atomic_{op}_nbi" for op in FETCHING]
    assert sorted(want) == sorted(ish.AMO_NAMES) and len(want) == 22
    for name in want:
        assert getattr(ish, name).__name__ == name
    assert callable(ish.amo) and callable(ish.amo_nbi)
    names = [p[0] for p in _lib.PROTOTYPES]
    header = (INCLUDE / "ishmem_capi.h").read_text()
    for n in ("ishmemi_c_amo", "ishmemi_c_amo_nbi"):
        assert n in names and f"{n}(" in header
    for op, code in ish.AMO_OPS.items():
        assert re.search(rf"#define ISHMEMI_C_AMO_{op.upper()} {code}\b", header), op


def test_model_known_answers():
    assert amo_model("fetch_add", 4, 0xFFFFFFFF, 1, 0) == (0, 0xFFFFFFFF)  # a 32-bit wrap
    assert amo_model("add", 4, 0xFFFFFFFF, 1, 0) == (0, 0)
    assert amo_model("fetch_inc", 4, 0x7FFFFFFF, 99, 0) == (0x80000000, 0x7FFFFFFF)
    assert amo_model("fetch_add", 8, 0x00000000FFFFFFFF, 1, 0) == (0x0000000100000000, 0x00000000FFFFFFFF)  # a 64-bit carry
    assert amo_model("inc", 8, 0xFFFFFFFFFFFFFFFF, 0, 0) == (0, 0)
    assert amo_model("fetch_add", 8, 0x1234567890ABCDEF, 0x8000000100000002, 0) == (0x9234567990ABCDF1, 0x1234567890ABCDEF)
    # compare_swap: a hit, and a miss whose cond differs from the word in the high half only
    assert amo_model("compare_swap", 8, 0x1234567890ABCDEF, 5, 0x1234567890ABCDEF) == (5, 0x1234567890ABCDEF)
    assert amo_model("compare_swap", 8, 0x1234567890ABCDEF, 5, 0x0234567890ABCDEF) == (0x1234567890ABCDEF, 0x1234567890ABCDEF)
    assert amo_model("compare_swap", 4, 0xFFFFFFFF, 5, 0x7FFFFFFF) == (0xFFFFFFFF, 0xFFFFFFFF)
    # a 32-bit operation sees the low 32 bits of its operands only
    assert amo_model("compare_swap", 4, 0xFFFFFFFF, 5, 0x1FFFFFFFF) == (5, 0xFFFFFFFF)
    # and / or / xor with bits in both halves
    old, v = 0xF0F0F0F00F0F0F0F, 0xFF00FF0000FF00FF
    assert amo_model("fetch_and", 8, old, v, 0) == (0xF000F000000F000F, old)
    assert amo_model("fetch_or", 8, old, v, 0) == (0xFFF0FFF00FFF0FFF, old)
    assert amo_model("fetch_xor", 8, old, v, 0) == (0x0FF00FF00FF00FF0, old)
    assert amo_model("and", 8, old, v, 0) == (0xF000F000000F000F, 0)
    assert amo_model("or", 4, 0xF0F00F0F, 0xFF0000FF, 0) == (0xFFF00FFF, 0)
    assert amo_model("xor", 4, 0xF0F00F0F, 0xFF0000FF, 0) == (0x0FF00FF0, 0)
    assert amo_model("fetch", 8, 7, 9, 9) == (7, 7) and amo_model("set", 8, 7, 9, 0) == (9, 0)
    assert amo_model("swap", 4, 0x80000000, 0x7FC12345, 0) == (0x7FC12345, 0x80000000)
    with pytest.raises(ValueError):
        amo_model("fetch_mul", 8, 1, 1, 1)


def preprocessed_names(cmd: list[str]) -> set[str]:
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    return set(NAME_RE.findall(out.stdout))


def test_host_header_has_exactly_the_committed_names():
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed for the host C++ names"
    got = preprocessed_names([gxx, "-std=c++17", "-E", "-x", "c++", f"-I{INCLUDE}", str(INCLUDE / "ishmem.h")])
    want = set(golden_names())
    assert not want - got, f"missing: {sorted(want - got)[:10]}"
    assert not got - want, f"extra: {sorted(got - want)[:10]}"


def test_device_header_has_exactly_the_committed_names():
    got = preprocessed_names([hipcc(), "--offload-arch=gfx950", "-std=c++20", "--cuda-device-only", "-E", "-x", "hip",
                              f"-I{INCLUDE}", str(INCLUDE / "ishmemx_device.h")])
    want = set(golden_names())
    assert not want - got, f"missing: {sorted(want - got)[:10]}"
    assert not got - want, f"extra: {sorted(got - want)[:10]}"


def test_host_cxx_names_compile_link_and_fail_before_init(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed for the host C++ names"
    calls = [call_text(f"ishmem_{tn}_atomic_{op}", op, t, f"({t} *) nullptr", f"({t} *) nullptr") for tn, t, op in matrix()]
    assert len(calls) == 229
    body = "\n".join(f"    V({c[:-1]});" for c in calls)
    src = tmp_path / "t.cpp"
    src.write_text(r'''
#include <ishmem.h>
#include <cstdio>
#include <cstring>
static int bad = 0, n = 0;
static void expect_reason(const char *what) {
    ++n;
    if (!std::strstr(ishmemi_c_last_error(), "not initialized")) { ++bad; std::printf("%s: %s\n", what, ishmemi_c_last_error()); }
}
#define V(call) do { call; expect_reason(#call); } while (0)
int main() {
    const int pe = 0;
''' + body + r'''
    // a fetching name returns T() after a failure
    if (ishmem_double_atomic_swap((double *) nullptr, 2.5, pe) != 0.0 || ishmem_long_atomic_fetch_add((long *) nullptr, 3L, pe) != 0L) ++bad;
    if (ishmem_atomic_fetch((float *) nullptr, pe) != 0.0f || ishmem_atomic_compare_swap((size_t *) nullptr, (size_t) 1, (size_t) 2, pe) != 0) ++bad;
    std::printf("%d %d\n", n, bad);
    return 0;
}
''')
    exe = tmp_path / "t"
    subprocess.run([gxx, "-std=c++17", "-Wall", "-Werror", f"-I{INCLUDE}", str(src), "-o", str(exe),
                    f"-L{_lib.LIB_PATH.parent}", f"-Wl,-rpath,{_lib.LIB_PATH.parent}", "-lishmem_amd"], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split()[-2:] == ["229", "0"], out.stdout


def test_device_forms_compile_for_gfx950(tmp_path):
    lines = []
    for tn, t, op in matrix():
        lines.append("    " + call_text(f"ishmem_{tn}_atomic_{op}", op, t, f"({t} *) p + t", f"({t} *) f + t"))
    # every template on legal types: unsigned long is in all three lists, double in EXT, int in STD
    for ops, types in ((EXT_OPS, ("unsigned long", "double", "int")), (STD_OPS, ("unsigned long", "int", "ptrdiff_t")),
                       (BIT_OPS, ("unsigned long", "int64_t", "uint32_t"))):
        for op in ops:
            for t in types:
                lines.append("    " + call_text(f"ishmem_atomic_{op}<{t}>", op, t, f"({t} *) p + t", f"({t} *) f + t"))
    src = tmp_path / "t.hip"
    src.write_text("#include <ishmem.h>\n__global__ void k(char *p, char *f, int pe)\n{\n    const int t = threadIdx.x;\n" +
                   "\n".join(lines) + "\n    ishmem_quiet();\n}\nint main() { return 0; }\n")
    subprocess.run([hipcc(), "--offload-arch=gfx950", "-std=c++20", "-Wall", "-Werror", f"-I{INCLUDE}", "-c", str(src), "-o",
                    str(tmp_path / "t.o")], check=True)


WRONG = {"fetch_add_float": ("float", "ishmem_atomic_fetch_add<float>(p, 1.0f, 0)", "unsigned long",
                             "ishmem_atomic_fetch_add<unsigned long>(p, 1ul, 0)"),
         "fetch_and_int": ("int", "ishmem_atomic_fetch_and<int>(p, 1, 0)", "unsigned int",
                           "ishmem_atomic_fetch_and<unsigned int>(p, 1u, 0)")}


@pytest.mark.parametrize("side", ["host", "device"])
@pytest.mark.parametrize("case", sorted(WRONG))
def test_templates_refuse_a_type_outside_their_list(tmp_path, case, side):
    """ishmem_atomic_fetch_add<float> and ishmem_atomic_fetch_and<int> do not compile; the same line
    with a listed type does, so it is the type list that refuses."""
    bad_t, bad_call, good_t, good_call = WRONG[case]
    for t, call, ok in ((good_t, good_call, True), (bad_t, bad_call, False)):
        if side == "host":
            src = tmp_path / f"t{int(ok)}.cpp"
            src.write_text(f"#include <ishmem.h>\nint main() {{ {t} *p = nullptr; (void) {call}; return 0; }}\n")
            cmd = [shutil.which("g++") or "g++", "-std=c++17", "-fsyntax-only", f"-I{INCLUDE}", str(src)]
        else:
            src = tmp_path / f"t{int(ok)}.hip"
            src.write_text(f"#include <ishmem.h>\n__global__ void k({t} *p) {{ (void) {call}; }}\nint main() {{ return 0; }}\n")
            cmd = [hipcc(), "--offload-arch=gfx950", "-std=c++20", f"-I{INCLUDE}", "-c", str(src), "-o", str(tmp_path / "t.o")]
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        if ok:
            assert out.returncode == 0, out.stderr[-2000:]
        else:
            assert out.returncode != 0, f"{call} compiled"
            assert "static assertion failed" in out.stderr or "static_assert" in out.stderr, out.stderr[-2000:]

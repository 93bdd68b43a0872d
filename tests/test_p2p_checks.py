"""The runtime's shared point-to-point argument helpers at their boundaries, without a GPU:
tests/cpp/p2p_checks.cpp compiles runtime.cpp into a stand-alone program, calls check_pe, peer_range,
peer_address, check_sig_op, sync_word_error and rma_args on a hand-made state and compares every
message with the literal text the entry points have always reported (the GPU workers' argument-error
tables pin the same texts through the real entry points)."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]


def build_p2p_checks() -> Path:
    src = ROOT / "tests" / "cpp" / "p2p_checks.cpp"
    exe = ROOT / "build" / "tests" / "p2p_checks"
    lib = ROOT / "ishmem_amd" / "libishmem_amd.so"
    deps = [src, lib, *sorted((ROOT / "ishmem_amd" / "csrc").glob("*")), *sorted((ROOT / "include").glob("*.h"))]
    if exe.exists() and all(d.stat().st_mtime <= exe.stat().st_mtime for d in deps):
        return exe
    exe.parent.mkdir(parents=True, exist_ok=True)
    # The kernels' launchers and the bootstrap come from the library; runtime.cpp is in the program.
    subprocess.run(["hipcc", "--offload-arch=gfx950", "-O1", "-std=c++20", "-Wall", "-Wno-unused-function",
                    f"-I{ROOT / 'include'}", f"-I{ROOT / 'ishmem_amd' / 'csrc'}", str(src),
                    f"-L{lib.parent}", "-lishmem_amd", f"-Wl,-rpath,{lib.parent}", "-o", str(exe)], check=True)
    return exe


def test_p2p_check_helpers_at_their_boundaries():
    out = subprocess.run([str(build_p2p_checks())], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "p2p_checks OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]

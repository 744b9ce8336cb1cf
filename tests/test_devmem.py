"""The batch's owned device buffers (csrc/rs_devmem.h) without a GPU: tests/csrc/devmem_check.cpp defines the few HIP functions the
header calls on top of malloc -- counting the live blocks, failing the k-th allocation on demand -- and asserts the ownership rules:
sizes, replace-on-success, failures that change nothing, moves, the all-or-none family at every k, nothing live at exit.  Built with
AddressSanitizer and UndefinedBehaviorSanitizer, without the HIP runtime; a stand-alone program run as a child process with leak
detection on.  The child gets this process's environment as it is, with ASAN_OPTIONS added: nothing is added to the preload and
nothing taken from it, and the sanitizer runtimes are linked statically so that the program does not depend on what is preloaded."""
import os
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]


def test_devmem_ownership_rules_under_the_sanitizers(tmp_path):
    exe = tmp_path / "devmem_check"
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "tests/csrc/devmem_check.cpp",
           "-o", str(exe)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "devmem_check: ok" in r.stdout

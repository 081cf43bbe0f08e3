"""csrc/dispatch.h on the CPU: tests/dispatch_host.cpp walks every run-time value the launchers pass to dispatch_hl,
dispatch_1to4, dispatch_bool and dispatch_dtype and checks the compile-time value that reaches the lambda, and compares
persistent_bx / persistent_bx_ceil with the clamps they replace.  The header is plain C++17, so any host compiler
builds it; none at all is a failure, not a skip."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _host_compiler():
    for cxx in (os.environ.get("CXX"), "g++", "c++", "clang++", "hipcc"):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    return None


def test_dispatch_header_on_the_host(tmp_path):
    cxx = _host_compiler()
    assert cxx, "no host C++ compiler found (CXX, g++, c++, clang++, hipcc)"
    exe = str(tmp_path / "dispatch_host")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe,
                            os.path.join(ROOT, "tests", "dispatch_host.cpp")], capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "dispatch_host: ok" in run.stdout

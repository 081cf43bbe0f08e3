"""csrc/workspace.h on the CPU: tests/workspace_host.cpp walks one sequence of regions over a NULL base (the size query)
and over a real buffer (the carve) and checks that both give the same offsets and total, that every region has the
alignment it asked for and starts behind the one before it, that empty regions and reserve() cost what they say, that
2^40-element walks do not wrap, and round_up / is_aligned at their boundaries.  The header is plain C++17, so any host
compiler builds it; none at all is a failure, not a skip."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _host_compiler():
    for cxx in (os.environ.get("CXX"), "g++", "c++", "clang++", "hipcc"):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    return None


def test_workspace_header_on_the_host(tmp_path):
    cxx = _host_compiler()
    assert cxx, "no host C++ compiler found (CXX, g++, c++, clang++, hipcc)"
    exe = str(tmp_path / "workspace_host")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe,
                            os.path.join(ROOT, "tests", "workspace_host.cpp")], capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "workspace_host: ok" in run.stdout

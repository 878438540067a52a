"""The host side of a gemm plan (csrc/srlx_gemm_plan.h) without a GPU and without HIP: tests/host/gemm_plan_host.cpp is a stand-alone program
that includes only that header; this test builds it with the host C++ compiler and runs it -- under AddressSanitizer and UndefinedBehaviorSanitizer where a
one-line trial program links with them, plain otherwise.  Nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def _compile(cxx, flags, source, exe):
    return subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *flags, "-I", os.path.join(ROOT, "simple_distributed_rl_amd", "csrc"),
                           source, "-o", exe], capture_output=True, text=True, timeout=120)


def test_plan_builder_bounds_grid_and_wgrad_table(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.fail("no host C++ compiler (CXX, c++, g++ or clang++)")
    trial = tmp_path / "trial.cpp"
    trial.write_text("int main() { return 0; }\n")
    flags = SANITIZE if _compile(cxx, SANITIZE, str(trial), str(tmp_path / "trial")).returncode == 0 else []
    print(f"GEMM-PLAN host build: {cxx} {' '.join(flags) or '(no sanitizer links here)'}")
    exe = str(tmp_path / "gemm_plan_host")
    built = _compile(cxx, flags, os.path.join(ROOT, "tests", "host", "gemm_plan_host.cpp"), exe)
    assert built.returncode == 0, built.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(run.stdout + run.stderr)
    assert run.returncode == 0 and "all checks passed" in run.stdout

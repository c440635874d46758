"""The row split of the f16x3 NT GEMM's launchers (csrc/nt_plan.h: which launch
takes which rows of rb_gemm_nt_h / _act / _dact) against a recorded table, on
the host alone.

tests/golden/nt_plan_sweep.txt.gz is the output of the three launchers' host
arithmetic as it stood before nt_plan.h replaced it (copied into a stand-alone
program, the CU count a parameter, each launch replaced by a record of its
kernel arguments and grid), over kind x M x R x C x wide x bias at 256, 304 and
64 CUs plus dact's n_parts bound.  tools/nt_plan_check.cpp prints the same
sweep from nt_plan()."""
import gzip
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_equals_the_recorded_launcher_arithmetic(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)),
               None)
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path / "nt_plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-o", exe,
                    os.path.join(ROOT, "tools", "nt_plan_check.cpp")], check=True)
    got = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()
    with gzip.open(os.path.join(ROOT, "tests", "golden", "nt_plan_sweep.txt.gz"), "rt") as f:
        want = f.read().splitlines()
    assert len(want) == 40416
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w
    # the fused entries never take the few-rows kernel (it has no epilogue)
    assert not any(w.split(" : ")[1].startswith("few") for w in want if not w.startswith("plain"))
    # every path and every refusal is in the table
    paths = {w.split(" : ")[1].split()[0] for w in want}
    assert paths == {"main", "tail", "both", "few", "few_main", "error"}
    errors = {w.split(" : error ")[1] for w in want if " : error " in w}
    assert errors == {
        "rb_gemm_nt_h: C % 128 != 0 needs R <= 1024",
        "rb_gemm_nt_h_act: shape or alignment without a wide-epilogue launch",
        "rb_gemm_nt_h_dact: shape or alignment without a wide-epilogue launch",
        "rb_gemm_nt_h_dact: dpart has too few rows",
    }

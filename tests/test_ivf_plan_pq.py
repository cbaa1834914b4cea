"""CPU: the per-query width of the IVF planner (csrc/ivf_plan.h) through tests/ivf_plan_pq_check.cpp, a stand-alone host program built
with AddressSanitizer + UBSan where the machine has their runtimes and run once: width 0 is the plan as it was, field for field, over
the sweep of tests/ivf_plan_check.cpp; width m adds the documented suspect bitmap, hash bitset and LDS tag block and nothing else, and
no route's LDS passes 160 KB."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_program_passes_and_the_sanitizers_report_nothing(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "g++ not found: the planner's check needs a C++ compiler"
    exe = str(tmp_path / "ivf_plan_pq_check")
    cmd = [cxx, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "radad_retrievalaugmenteddeepfakeaudiodetection_amd", "csrc"),
           os.path.join(ROOT, "tests", "ivf_plan_pq_check.cpp"), "-o", exe]
    san = subprocess.run(cmd + ["-fsanitize=address,undefined"], capture_output=True, text=True)
    if san.returncode != 0:
        assert "sanitize" in san.stderr or "asan" in san.stderr or "ubsan" in san.stderr, san.stderr      # anything else is a real error
        print("ivf_plan_pq_check: no sanitizer runtimes on this machine, built WITHOUT -fsanitize=address,undefined")
        subprocess.run(cmd, check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    assert "ivf_plan_pq_check: ok" in run.stdout and "FAILED" not in run.stdout
    assert "runtime error" not in run.stderr and "Sanitizer" not in run.stderr, run.stderr[-3000:]

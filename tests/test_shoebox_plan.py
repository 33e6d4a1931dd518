"""CPU: the host's decisions about a summation-integration job (csrc/shoebox_plan.hpp: which tables and jobs are refused and why, the
index over the boxes' z-ranges against a brute-force filter, the bytes of device state) as a plain C++ program under the address and
undefined-behaviour sanitizers; tests/shoebox_plan_check.cc lists what it holds."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-std=c++20", "-ffp-contract=off", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
INCLUDES = ["-I", os.path.join(ROOT, "fast-feedback-service_amd", "csrc")]


def test_refusals_and_index_queries_hold_and_sanitizers_are_clean(tmp_path):
    exe = tmp_path / "shoebox_plan_check"
    subprocess.run(["g++", *FLAGS, *INCLUDES, os.path.join(ROOT, "tests", "shoebox_plan_check.cc"), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    failures = [line for line in run.stdout.splitlines() if line.startswith("FAIL")]
    assert not failures, failures[:10]
    assert run.returncode == 0 and run.stderr == "" and run.stdout.splitlines()[-1] == "OK", (run.returncode, run.stderr[-2000:])

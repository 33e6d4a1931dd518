"""CPU: the host's decisions about a scan prediction (csrc/predict_plan.hpp: every refusal of ffs_ctx_predict, its text and the untouched
state; h_max against brute force on 200 random settings; the candidate numbering's round trip; the centring absences; the BOX_REFUSED flag
against ffs_ctx_shoebox_begin's own rule) as a plain C++ program under the address and undefined-behaviour sanitizers;
tests/predict_plan_check.cc lists what it holds."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-std=c++20", "-ffp-contract=off", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
INCLUDES = ["-I", os.path.join(ROOT, "fast-feedback-service_amd", "csrc")]


def test_refusals_candidate_box_and_numbering_hold_and_sanitizers_are_clean(tmp_path):
    exe = tmp_path / "predict_plan_check"
    subprocess.run(["g++", *FLAGS, *INCLUDES, os.path.join(ROOT, "tests", "predict_plan_check.cc"), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    failures = [line for line in run.stdout.splitlines() if line.startswith("FAIL")]
    assert not failures, failures[:10]
    assert run.returncode == 0 and run.stderr == "" and run.stdout.splitlines()[-1] == "OK", (run.returncode, run.stderr[-2000:])

"""CPU: the arithmetic of rotation sweeps and of the exchange between GPUs (csrc/sweep_plan.hpp) is a header without HIP: the stack's growth and
room rules, where a batch's strong-pixel lists land and its append table, the finish's tables and launch sizes, which records are
reflections, in which order the gathered spot rows arrive -- the one layout the library writes by and the driver reads by -- and the two
transport decisions.  tests/sweep_plan_check.cc holds each against a restatement over small exhaustive spaces (rank orders such as devices
1,0,1 included, which a one-GPU machine cannot run), in its own process under the address and undefined-behaviour sanitizers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-std=c++20", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
INCLUDES = ["-I", os.path.join(ROOT, "fast-feedback-service_amd", "csrc"), "-I", os.path.join(ROOT, "include")]


def test_placement_room_finish_plan_classification_gather_layout_and_transport(tmp_path):
    exe = tmp_path / "sweep_plan_check"
    subprocess.run(["g++", *FLAGS, *INCLUDES, os.path.join(ROOT, "tests", "sweep_plan_check.cc"), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    failures = [line for line in run.stdout.splitlines() if line.startswith("FAIL")]
    assert not failures, failures[:10]
    assert run.returncode == 0 and run.stderr == "" and run.stdout.splitlines()[-1] == "OK", (run.returncode, run.stderr[-2000:])

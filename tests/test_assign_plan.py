"""CPU: csrc/assign_plan.hpp as a plain C++ program (tests/assign_plan_check.cc): every refusal of the assignment entries with its text, the
key table's size, the bytes of a setting, the pass boundaries and the launches' shapes.  No HIP header is needed to compile it."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fast-feedback-service_amd", "csrc")


def test_the_plan_as_a_program(tmp_path):
    exe = str(tmp_path / "assign_plan_check")
    subprocess.run(["g++", "-std=c++20", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC,
                    os.path.join(ROOT, "tests", "assign_plan_check.cc"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout == "ok\n" and run.stderr == "", (run.stdout[-3000:], run.stderr[-3000:])

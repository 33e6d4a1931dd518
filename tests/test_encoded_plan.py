"""CPU: what the host decides about a batch of encoded frames (csrc/encoded_plan.hpp) is plain arithmetic in a header without HIP:
bitshuffle's blocking, the chunk checks and their texts, where the chunks lie in the staging buffer, which ranges of it are copied, the
walk along the block chains and the byte-offset frame table.  tests/encoded_plan_check.cc holds each against literals worked out by hand,
on heap blocks of exactly the chunks' sizes, in its own process under the address and undefined-behaviour sanitizers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-std=c++20", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
INCLUDES = ["-I", os.path.join(ROOT, "fast-feedback-service_amd", "csrc"), "-I", os.path.join(ROOT, "include")]


def test_decisions_match_the_formats_and_sanitizers_are_clean(tmp_path):
    exe = tmp_path / "encoded_plan_check"
    subprocess.run(["g++", *FLAGS, *INCLUDES, os.path.join(ROOT, "tests", "encoded_plan_check.cc"), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    failures = [line for line in run.stdout.splitlines() if line.startswith("FAIL")]
    assert not failures, failures[:10]
    assert run.returncode == 0 and run.stderr == "" and run.stdout.splitlines()[-1] == "OK", (run.returncode, run.stderr[-2000:])

"""CPU: a context's settings and the rules of its setters (csrc/context_settings.hpp) are plain arithmetic in a header without HIP:
which settings combine, each pair rule stated once for both of its setters, the setters' ranges, every refusal's text, and what a batch
takes of the settings at submit.  tests/context_settings_check.cc holds every text against a literal, both halves of every pair rule
against each other over a small state space, every state reachable by accepted calls against the rules, and the snapshot against its
source, in its own process under the address and undefined-behaviour sanitizers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-std=c++20", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
INCLUDES = ["-I", os.path.join(ROOT, "fast-feedback-service_amd", "csrc"), "-I", os.path.join(ROOT, "include")]


def test_rules_texts_reachable_states_and_snapshot(tmp_path):
    exe = tmp_path / "context_settings_check"
    subprocess.run(["g++", *FLAGS, *INCLUDES, os.path.join(ROOT, "tests", "context_settings_check.cc"), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    failures = [line for line in run.stdout.splitlines() if line.startswith("FAIL")]
    assert not failures, failures[:10]
    assert run.returncode == 0 and run.stderr == "" and run.stdout.splitlines()[-1] == "OK", (run.returncode, run.stderr[-2000:])

"""CPU: the driver's batch pipeline (host/batch_pipeline.cc: assemblies filled by several readers, one collector per GPU, the stop
watcher, the flush of half-filled batches) linked against a fake of the ffs_* calls it makes (tests/pipeline_cpu/fake_ffs.cc) and
driven by tests/pipeline_cpu/pipeline_check.cc, in a process of its own: once under ThreadSanitizer, once under the address and
undefined-behaviour sanitizers.  The program checks, in every case, that each expected image is reported exactly once with the
checksum of the bytes the reader produced for it, that a GPU's batches come out in ascending order, that global batch b went to GPU
b mod n_dev and that never more than K batches of a GPU are in flight; the cases are raw frames over readers x batch x K x GPUs,
chunks that land in their slot / the overflow area / the heap, a source that ends mid-batch, a stop while every assembly is in
flight and the readers are parked, a submit that fails, and --read-only."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "fast-feedback-service_amd", "host")
HERE = os.path.join(ROOT, "tests", "pipeline_cpu")
SOURCES = [os.path.join(HOST, "batch_pipeline.cc"), os.path.join(HERE, "fake_ffs.cc"), os.path.join(HERE, "pipeline_check.cc")]
COMMON = ["-std=c++20", "-Wall", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"), "-I", HOST, "-I", HERE]
BUILDS = {
    "thread": ["-fsanitize=thread", "-O1", "-g"],
    "address_undefined": ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-O1", "-g"],
}


@pytest.fixture(scope="module", params=sorted(BUILDS))
def run(request, tmp_path_factory):
    exe = tmp_path_factory.mktemp("pipeline_" + request.param) / "pipeline_check"
    subprocess.run(["g++", *COMMON, *BUILDS[request.param], *SOURCES, "-o", str(exe)], check=True)
    return subprocess.run(["timeout", "-k", "5", "120", str(exe)], capture_output=True, text=True)


def test_every_case_holds_and_the_sanitizer_is_silent(run):
    failures = [line for line in run.stdout.splitlines() if line.startswith("FAIL")]
    assert not failures, failures[:10]
    assert run.returncode == 0 and run.stderr == "" and run.stdout.splitlines()[-1] == "OK", (run.returncode, run.stderr[-3000:])


def test_what_the_moved_code_prints(run):
    lines = run.stdout.splitlines()
    assert "Error: injected device error" in lines                      # the failing submit: fail() names the context's error
    assert lines.count("Timeout waiting for image 14") >= 2             # the source that ends early, once per run at least
    assert not any(line.startswith("Thread") or line.startswith("GPU") for line in lines)   # nothing of -v without -v

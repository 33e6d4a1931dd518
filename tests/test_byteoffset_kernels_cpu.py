"""CPU: csrc/kernels_byteoffset.hpp compiled for the host (tests/byteoffset_cpu: a stand-in for ffs_device.h, 64 threads as the lanes
of a wave) and checked against the host decoder.  Finds index and boundary mistakes of the kernels without a GPU; the GPU suite
(test_gpu_byteoffset.py) checks the real thing."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "fast-feedback-service_amd")
HERE = os.path.join(ROOT, "tests", "byteoffset_cpu")


def test_kernels_on_host_threads(tmp_path):
    # (encoded_plan.hpp: the tile size, BoFrame and bo_tiles the kernels share with the host's planning; it includes the ABI's header)
    for src in (os.path.join(PKG, "csrc", "kernels_byteoffset.hpp"), os.path.join(PKG, "csrc", "encoded_plan.hpp"), os.path.join(HERE, "ffs_device.h"),
                os.path.join(HERE, "byteoffset_kernels_check.cc")):
        shutil.copy(src, tmp_path)
    exe = tmp_path / "check"
    subprocess.run(["g++", "-std=c++20", "-O1", "-fwrapv", "-pthread", "-I", os.path.join(PKG, "host"), "-I", os.path.join(ROOT, "include"),
                    str(tmp_path / "byteoffset_kernels_check.cc"), "-o", str(exe)], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "EMU OK" in p.stdout and "FAIL" not in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]
    assert p.stdout.count(": ok") == 25


def test_stand_in_has_the_librarys_flag_value():
    text = open(os.path.join(PKG, "csrc", "ffs_device.h")).read()
    assert re.search(r"kOvfCorruptByteOffset = 256u;", text)
    assert "kOvfCorruptByteOffset = 256u;" in open(os.path.join(HERE, "ffs_device.h")).read()

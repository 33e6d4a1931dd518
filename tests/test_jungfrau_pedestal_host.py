"""CPU: `ffs_hosttool jfrepedestal` -- the last step of a pedestal measurement, from the statistics files of spotfinder --jungfrau-pedestal
to a new calibration file, with no GPU -- against the NumPy truth (tests/jungfrau_pedestal_oracle.py), bit for bit; its refusals; the
synthetic dark sources through the tool (synth:tinydark is the Python mirror's function of index and seed, and has a calibration)."""
import os
import subprocess

import numpy as np
import pytest

import jungfrau_pedestal_oracle as P
from ffs_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "fast-feedback-service_amd", "bin", "ffs_hosttool")
W, H, SEED, N = 300, 200, 7, 24


def run(*args):
    return subprocess.run([TOOL, *map(str, args)], capture_output=True, text=True)


def tool(*args):
    p = run(*args)
    assert p.returncode == 0, (args, p.stdout, p.stderr)
    return p.stdout


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """A dark run folded by the oracle and written as the driver writes it, next to the calibration of the same seed."""
    d = tmp_path_factory.mktemp("jfped_host")
    ped, fac = synth.jungfrau_calibration(W, H, SEED)
    frames = synth.dark_frames(W, H, SEED, N)
    frames[:, 5, 5] = 0xFFFF                          # a pixel that never counts
    frames[::2, 9, 9] = (frames[::2, 9, 9] & 0xC000) | 100   # ... and a noisy one
    acc = P.fold(P.zeros(H, W), frames)
    prefix = str(d / "dark")
    acc[1].astype("<u4").tofile(prefix + ".count.u32")
    acc[2].astype("<u8").tofile(prefix + ".sum.u64")
    acc[3].astype("<u8").tofile(prefix + ".sum_sq.u64")
    np.concatenate([ped, fac]).astype("<f4").tofile(d / "old.f32")
    return d, prefix, ped, fac, acc


@pytest.mark.parametrize("extra,min_frames,max_rms", [((), 1, 0.0), ((N // 3,), N // 3, 0.0), ((2, 2.5), 2, 2.5), ((N // 3 + 1, 0), N // 3 + 1, 0.0)])
def test_jfrepedestal_equals_the_oracle(case, extra, min_frames, max_rms):
    d, prefix, ped, fac, acc = case
    out = d / f"new_{min_frames}_{max_rms}.f32"
    tool("jfrepedestal", d / "old.f32", prefix, out, *extra)
    got = np.fromfile(out, "<f4").reshape(6, H, W)
    new_ped, rms, ok = P.planes(*acc[1:], min_frames=min_frames, max_rms=max_rms)
    want_ped, want_fac = P.repedestal(ped, fac, new_ped, ok)
    assert np.array_equal(got[:3].view(np.uint32), want_ped.view(np.uint32))
    assert np.array_equal(got[3:].view(np.uint32), want_fac.view(np.uint32))
    assert (got[3:, 5, 5] == 0).all() and (got[:3, 5, 5] == 0).all()
    if max_rms:
        assert not ok[:, 9, 9].any() and ok[0].mean() > 0.99
    if min_frames > N // 3:
        assert (got[3:] == 0).mean() > 0.99     # no stage of a third of the run has that many frames (the stuck pixels' G0 has)
    else:
        assert (got[3:] != 0).mean() > 0.98


def test_jfrepedestal_refuses_files_of_the_wrong_size(case):
    d, prefix, ped, fac, acc = case
    out = d / "never.f32"

    def refused(*args, match):
        p = run("jfrepedestal", *args)
        assert p.returncode != 0 and match in p.stdout + p.stderr, (args, p.stdout, p.stderr)
        assert not out.exists()

    np.concatenate([ped, fac]).astype("<f4")[:, :-1].tofile(d / "short.f32")        # six planes of another detector
    refused(d / "short.f32", prefix, out, match="are not three planes")
    np.zeros(7, "<f4").tofile(d / "odd.f32")
    refused(d / "odd.f32", prefix, out, match="six planes")
    for suffix, dt in ((".count.u32", "<u4"), (".sum.u64", "<u8"), (".sum_sq.u64", "<u8")):
        bad = str(d / ("bad" + suffix.split(".")[1]))
        for s2, d2, a in ((".count.u32", "<u4", acc[1]), (".sum.u64", "<u8", acc[2]), (".sum_sq.u64", "<u8", acc[3])):
            (a.astype(d2).reshape(-1)[:-1] if s2 == suffix else a.astype(d2)).tofile(bad + s2)
        refused(d / "old.f32", bad, out, match="are not three planes")
    refused(d / "old.f32", str(d / "missing"), out, match="cannot open")
    refused(d / "old.f32", prefix, out, 0, match="min_frames")
    refused(d / "old.f32", prefix, out, -3, match="min_frames")
    refused(d / "old.f32", prefix, out, 1, -0.5, match="max_rms")
    refused(d / "old.f32", prefix, out, 1, "nan", match="max_rms")
    refused(d / "old.f32", prefix, out, 1, "inf", match="max_rms")
    refused(d / "old.f32", prefix, out, 1, "x", match="max_rms")


def test_tinydark_is_the_python_mirrors_function_and_has_a_calibration(tmp_path):
    tool("synthframes", f"synth:tinydark:{N}", tmp_path / "a")
    a = np.fromfile(tmp_path / "a", "<u2").reshape(-1, H, W)
    assert np.array_equal(a, synth.dark_frames(W, H, SEED, N))
    tool("synthframes", f"synth:tinydark:{N}:11", tmp_path / "b")
    assert np.array_equal(np.fromfile(tmp_path / "b", "<u2").reshape(-1, H, W), synth.dark_frames(W, H, 11, N))
    # the stage of a frame depends on the run's length: frame 5 of 6 is G2, frame 5 of 24 is G0
    tool("synthframes", "synth:tinydark:6", tmp_path / "c")
    c = np.fromfile(tmp_path / "c", "<u2").reshape(-1, H, W)
    assert np.median(c[5] >> 14) == 3 and np.median(a[5] >> 14) == 0
    tool("jfcal", "synth:tinydark", tmp_path / "cal.f32")
    ped, fac = synth.jungfrau_calibration(W, H, SEED)
    assert np.array_equal(np.fromfile(tmp_path / "cal.f32", "<f4").reshape(6, H, W), np.concatenate([ped, fac]))

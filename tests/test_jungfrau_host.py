"""CPU: the host's side of the raw Jungfrau input.  The host converter (host/codecs.hpp, jungfrau_convert: the text of csrc/jungfrau_model.hpp)
equals the NumPy truth bit for bit; the synthetic sources of raw words (synth:tinyraw) are a function of (index, seed), equal to the Python
mirror's, and their calibration file round-trips; the ABI declares the new entry and the binding lists it."""
import os
import re
import subprocess

import numpy as np
import pytest

import jungfrau_oracle as J
from ffs_amd import api, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "fast-feedback-service_amd", "bin")
TOOL = os.path.join(BIN, "ffs_hosttool")
SPOTFINDER = os.path.join(BIN, "spotfinder")


def tool(*args):
    p = subprocess.run([TOOL, *map(str, args)], capture_output=True, text=True)
    assert p.returncode == 0, (args, p.stdout, p.stderr)
    return p.stdout


def test_host_converter_equals_the_oracle(tmp_path):
    W, H = 67, 45
    ped, fac = J.calibration(W, H, seed=5)
    rng = np.random.default_rng(5)
    fac[rng.random(fac.shape) < 0.02] = 4096.0                      # (results beyond the clamp)
    ped[rng.random(ped.shape) < 0.05] = np.float32(1e-41)           # denormal pedestals
    ped[0, :, :8] = np.arange(8, dtype=np.float32)[None, :] + np.float32(0.5)   # ties
    fac[0, :, :8] = 1.0
    raw = np.concatenate([J.stage_mix_frames(3, H, W, ped, fac, seed=9, all_g0=(1,)), rng.integers(0, 1 << 16, (2, H, W)).astype(np.uint16)])
    raw[4, :, :8] = np.arange(1, 9, dtype=np.uint16)[None, :]       # G0, ADC 1..8 over pedestals k + 0.5
    raw.tofile(tmp_path / "raw.u16")
    np.concatenate([ped, fac]).astype("<f4").tofile(tmp_path / "cal.f32")
    tool("jfconvert", tmp_path / "raw.u16", tmp_path / "cal.f32", W, H, tmp_path / "out.u32")
    got = np.fromfile(tmp_path / "out.u32", "<u4").reshape(raw.shape)
    want = J.convert(raw, ped, fac)
    assert np.array_equal(got, want)
    assert (want == J.INVALID).sum() > 500 and (want == J.MAX_PHOTONS).sum() > 20 and (want == 0).sum() > 200
    assert want[4, 0, :8].tolist() == [0, 0, 0, 0, 0, 0, 0, 0]   # (ADC k + 1 over pedestal k + 0.5: the tie 0.5 -> 0)


def _frames_of(spec, tmp_path, name):
    tool("synthframes", spec, tmp_path / name)
    return np.fromfile(tmp_path / name, "<u2").reshape(-1, 200, 300)


def test_tinyraw_frames_are_a_function_of_index_and_seed(tmp_path):
    a = _frames_of("synth:tinyraw:3", tmp_path, "a")
    b = _frames_of("synth:tinyraw:2", tmp_path, "b")
    c = _frames_of("synth:tinyraw:3:11", tmp_path, "c")
    d = _frames_of("synth:tinyraw:3:11", tmp_path, "d")
    assert a.shape == (3, 200, 300) and np.array_equal(a[:2], b) and np.array_equal(c, d)
    assert not np.array_equal(a[0], a[1]) and not np.array_equal(a, c)
    # ... the function the Python mirror computes: the 32-bit twin of synth:tiny, encoded under the seed's calibration
    for seed, frames in ((7, a), (11, c)):
        assert np.array_equal(synth.raw_frames(synth.tiny_params(seed, np.uint32), range(3)), frames)
    # every stage, the three invalid words and the code 2 occur; the conversion gives the photons back within the ADC's resolution
    codes = np.bincount((a >> 14).reshape(-1), minlength=4)
    assert (codes > 0).all() and (a == 0xFFFF).any() and (a == 0xC000).any()
    ped, fac = synth.jungfrau_calibration(300, 200, 7)
    photons = synth.frames(synth.tiny_params(7, np.uint32), range(3), threads=2)
    conv = J.convert(a, ped, fac)
    ok = conv != J.INVALID
    assert 0.99 < ok.mean() < 1.0
    assert np.abs(conv[ok].astype(np.int64) - photons[ok].astype(np.int64)).max() <= 1
    # synth:tiny itself is untouched: 16-bit photon counts
    tool("synthframes", "synth:tiny:2", tmp_path / "t")
    assert np.array_equal(np.fromfile(tmp_path / "t", "<u2").reshape(2, 200, 300), synth.frames(synth.tiny_params(7), range(2), threads=2))


def test_calibration_file_round_trips(tmp_path):
    tool("jfcal", "synth:tinyraw:1:11", tmp_path / "cal.f32")
    planes = np.fromfile(tmp_path / "cal.f32", "<f4")
    assert planes.size == 6 * 200 * 300
    ped, fac = synth.jungfrau_calibration(300, 200, 11)
    assert np.array_equal(planes.reshape(6, 200, 300), np.concatenate([ped, fac]))
    assert not np.array_equal(ped, synth.jungfrau_calibration(300, 200, 7)[0])
    # inside the setter's ranges, a few entries without a calibration, inverted G1 and G2
    assert all(J.entry_ok(False, v) for v in (ped.min(), ped.max())) and all(J.entry_ok(True, v) for v in (fac.min(), fac.max(), np.abs(fac[fac != 0]).min()))
    assert 0 < (fac == 0).mean() < 0.01 and (fac[0][fac[0] != 0] > 0).all() and (fac[1] <= 0).all() and (fac[2] <= 0).all()
    # written by the mirror, read by the host converter: the file is the interface
    np.concatenate([ped, fac]).astype("<f4").tofile(tmp_path / "cal2.f32")
    tool("synthframes", "synth:tinyraw:2:11", tmp_path / "raw.u16")
    tool("jfconvert", tmp_path / "raw.u16", tmp_path / "cal2.f32", 300, 200, tmp_path / "out.u32")
    raw = np.fromfile(tmp_path / "raw.u16", "<u2").reshape(2, 200, 300)
    assert np.array_equal(np.fromfile(tmp_path / "out.u32", "<u4").reshape(2, 200, 300), J.convert(raw, ped, fac))
    p = subprocess.run([TOOL, "jfcal", "synth:tiny:1", str(tmp_path / "no.f32")], capture_output=True, text=True)
    assert p.returncode != 0 and "raw Jungfrau" in p.stdout


def test_abi_declares_the_entry_and_the_codec():
    text = open(os.path.join(ROOT, "include", "ffs_hip.h")).read()
    assert re.search(r"typedef struct \{ const float \*pedestal\[3\]; const float \*factor\[3\]; \} ffs_jungfrau_calibration;", text)
    assert re.search(r"int ffs_ctx_set_jungfrau_calibration\(ffs_ctx \*ctx, const ffs_jungfrau_calibration \*cal\);", text)
    assert re.search(r"#define FFS_CODEC_JUNGFRAU_RAW 2\b", text)
    assert "ffs_ctx_set_jungfrau_calibration" in api.EXPORTS and api.CODEC_JUNGFRAU_RAW == 2


@pytest.mark.parametrize("argv,text", [
    (["synth:tinyraw:2", "--jungfrau-calibration", "/nonexistent/cal.f32"], "--jungfrau-calibration: no such file"),
    (["synth:tinyraw:2", "--jungfrau-calibration"], "jungfrau-calibration"),
])
def test_driver_refuses_a_bad_flag_before_it_needs_a_gpu(argv, text):
    p = subprocess.run([SPOTFINDER, *argv], capture_output=True, text=True)
    assert p.returncode == 1 and text in p.stdout and "Usage:" in p.stdout


def test_driver_refuses_wrong_file_size_and_wrong_source(tmp_path):
    short = tmp_path / "short.f32"
    np.zeros(6 * 200 * 300 - 1, "<f4").tofile(short)
    p = subprocess.run([SPOTFINDER, "synth:tinyraw:2", "--jungfrau-calibration", str(short)], capture_output=True, text=True)
    assert p.returncode == 1 and "holds 1439996 bytes" in p.stdout and "1440000" in p.stdout
    good = tmp_path / "cal.f32"
    tool("jfcal", "synth:tinyraw:1", good)
    p = subprocess.run([SPOTFINDER, "synth:jungfrau9m:1", "--jungfrau-calibration", str(good)], capture_output=True, text=True)
    assert p.returncode == 1 and "uncompressed 16-bit frames" in p.stdout and "32 bits" in p.stdout

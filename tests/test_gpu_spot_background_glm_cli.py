"""GPU: the driver with --spot-background 3 --spot-background-model glm on synth: frames.  The JSON arrays must equal what the binding gives
for the same frames (Stream.spot_backgrounds_glm, spot_intensities_glm), number for number, and the model is named on standard output."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPOTFINDER = os.path.join(ROOT, "fast-feedback-service_amd", "bin", "spotfinder")


def _run(argv, cwd):
    r, w = os.pipe()
    proc = subprocess.Popen([SPOTFINDER, *argv, "--pipe_fd", str(w)], pass_fds=[w], cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    os.close(w)
    out, err = proc.communicate(timeout=300)
    with os.fdopen(r) as f:
        lines = [l for l in f.read().split("\n") if l]
    return proc.returncode, re.sub(r"\x1b\[[0-9;]*m", "", out), err, lines


def test_driver_glm_model(ffs, tmp_path):
    from ffs_amd import synth
    N = 4       # (two batches of two images)
    common = ["synth:tiny:%d" % N, "--threads", "1", "--batch", "2", "--single-buffer", "--max-valid", "none", "--spot-background", "3"]
    rc, out, err, lines = _run(common + ["--spot-background-model", "glm"], tmp_path)
    assert rc == 0 and not err, (out, err)
    assert "Spot background model: glm" in out
    got = {json.loads(l)["file-number"]: json.loads(l) for l in lines}
    assert sorted(got) == list(range(N))
    rc, out_c, err, lines_c = _run(common + ["--spot-background-model", "constant"], tmp_path)
    assert rc == 0 and not err and "Spot background model" not in out_c
    constant = {json.loads(l)["file-number"]: json.loads(l) for l in lines_c}
    p = synth.params(300, 200, np.uint16, seed=7, background=2.0, n_spots=40, sigma=(0.8, 1.6), peak=(30.0, 5000.0), max_value=65535)
    frames = synth.frames(p, range(N), threads=2)
    ctx = ffs.Context(300, 200, np.uint16, max_batch=2)
    ctx.set_params(want_reflections=1)
    st = ctx.stream()
    n_valid = n_differ = 0
    for first in (0, 2):
        res = st.process(frames[first:first + 2], first)
        bg = st.spot_backgrounds_glm(3)
        tukey = st.spot_backgrounds(3)
        intensity, variance = ffs.spot_intensities_glm(st.last_batch_reflections, bg)
        at = 0
        for k, fr in enumerate(res):
            line = got[first + k]
            n = len(fr.reflections)
            assert n > 0 and list(line) == sorted(line)          # keys in alphabetical order
            ok = bg["status"][at:at + n] == 0
            want_mean = [float(m) if o else None for m, o in zip(bg["mean"][at:at + n], ok)]
            want_int = [float(v) if o else None for v, o in zip(intensity[at:at + n], ok)]
            want_var = [float(v) if o else None for v, o in zip(variance[at:at + n], ok)]
            assert line["spot_background_mean"] == want_mean
            assert line["spot_intensity"] == want_int
            assert line["spot_variance"] == want_var
            assert line["total_intensity"] == sum(v for v in want_int if v is not None)
            # the default model's line for the same image is the Tukey call's
            t_ok = tukey["status"][at:at + n] == 0
            assert constant[first + k]["spot_background_mean"] == [float(m) if o else None for m, o in zip(tukey["mean"][at:at + n], t_ok)]
            n_differ += sum(1 for a, b in zip(line["spot_background_mean"], constant[first + k]["spot_background_mean"]) if a != b)
            n_valid += int(ok.sum())
            at += n
    assert n_valid > 10 and n_differ > 0

"""GPU: `spotfinder --kernel-size` end to end -- per-image counts equal the oracle's at that window, and `--validate` (the gather
path, k_exact_w) agrees with the general-window kernel image by image."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPOTFINDER = os.path.join(ROOT, "fast-feedback-service_amd", "bin", "spotfinder")


def _tiny_frames(n, seed=7):
    from ffs_amd import synth
    p = synth.params(300, 200, np.uint16, seed=seed, background=2.0, n_spots=40, sigma=(0.8, 1.6),
                     peak=(30.0, 5000.0), max_value=65535)
    return synth.frames(p, range(n), threads=2)


def _run(argv, cwd):
    r, w = os.pipe()
    proc = subprocess.Popen([SPOTFINDER, *argv, "--pipe_fd", str(w)], pass_fds=[w], cwd=cwd,
                            stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    os.close(w)
    out, err = proc.communicate(timeout=300)
    with os.fdopen(r) as f:
        lines = [l for l in f.read().split("\n") if l]
    return proc.returncode, re.sub(r"\x1b\[[0-9;]*m", "", out), err, lines


def test_kernel_size_json_counts_match_oracle(tmp_path):
    from oracle import oracle as O
    N = 5
    rc, out, err, lines = _run(["synth:tiny:%d" % N, "--threads", "2", "--batch", "2", "--kernel-size", "5,2"], tmp_path)
    assert rc == 0 and not err, (out, err)
    got = {json.loads(l)["file-number"]: json.loads(l) for l in lines}
    assert sorted(got) == list(range(N))
    mask = np.ones((200, 300), np.uint8)
    frames = _tiny_frames(N)
    for i, img in enumerate(frames):
        cc = O.cc2d(O.dispersion(img, mask, O.DispParams(5, 2, 2, 0.0, 6.0, 3.0)), img, 3)
        assert got[i]["num_strong_pixels"] == cc.num_strong_pixels
        assert got[i]["n_spots_total"] == len(cc.boxes)
    # (and the window made a difference: the 7x7 window gives other counts)
    cc7 = O.cc2d(O.dispersion(frames[0], mask), frames[0], 3)
    assert cc7.num_strong_pixels != got[0]["num_strong_pixels"]


def test_validate_with_kernel_size(tmp_path):
    N = 4
    rc, out, err, lines = _run(["synth:tiny:%d" % N, "--threads", "2", "--batch", "2", "--validate", "--kernel-size", "4"], tmp_path)
    assert rc == 0 and not err, (out, err)
    matches = re.findall(r"Image\s+(\d+): Compared: Match (\d+) px", out)
    assert sorted(int(a) for a, _ in matches) == list(range(N)) and "Mismatch" not in out

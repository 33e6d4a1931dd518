"""Access to the committed golden fixtures (tests/golden/*.npz, generated from the reference's
own standalone.cc by tests/golden/make_golden.py)."""
import hashlib
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def small_cases():
    z = np.load(os.path.join(GOLD, "dispersion_small.npz"))
    names = sorted({k.split("/")[0] for k in z.files})
    for n in names:
        img, mask = z[n + "/image"], z[n + "/mask"]
        strong = np.unpackbits(z[n + "/strong"])[: img.size].reshape(img.shape)
        yield n, img, mask, strong


def config1():
    from ffs_amd import synth
    z = np.load(os.path.join(GOLD, "dispersion_config1.npz"))
    p, mask = synth.config1_params(), synth.config1_mask()
    assert sha(mask) == str(z["mask_sha256"])
    for i in range(10):
        img = synth.frame(p, i)
        assert sha(img) == str(z[f"frame{i}/input_sha256"]), "synthetic generator drifted from the fixture"
        yield i, img, mask, z[f"frame{i}/strong_k"]


def samples(indices=range(6)):
    from ffs_amd import synth
    z = np.load(os.path.join(GOLD, "dispersion_samples.npz"))
    mask = synth.mask_eiger16m()
    assert sha(mask) == str(z["mask_sha256"])
    for i in indices:
        img = synth.reference_sample(i)
        assert sha(img) == str(z[f"sample{i}/input_sha256"])
        yield i, img, mask, z[f"sample{i}/strong_k"]


def random_input(seed):
    """The seeded frame and mask of test_oracle_golden.py::test_port_equals_compiled_reference (Poisson background at one of
    five levels, ten bright pixels, a pixel above 2^24 for odd seeds, 3 % of the pixels masked)."""
    rng = np.random.default_rng(seed)
    H, W = int(rng.integers(20, 200)), int(rng.integers(20, 300))
    lam = float(rng.choice([0.05, 1.0, 7.0, 200.0, 5000.0]))
    img = rng.poisson(lam, (H, W)).astype(np.uint32)
    for _ in range(10):
        y, x = rng.integers(0, H), rng.integers(0, W)
        img[y, x] += rng.integers(10, 60000)
    if seed % 2:
        img[rng.integers(0, H), rng.integers(0, W)] = (1 << 24) + 17
    mask = (rng.random((H, W)) > 0.03).astype(np.uint8)
    return img, mask


def random_case(seed):
    """random_input(seed) and the reference's strong mask for it (dispersion_random.npz)."""
    z = np.load(os.path.join(GOLD, "dispersion_random.npz"))
    img, mask = random_input(seed)
    assert sha(img) == str(z[f"seed{seed}/input_sha256"]) and sha(mask) == str(z[f"seed{seed}/mask_sha256"]), \
        "numpy's generator drifted from the fixture"
    return img, mask, np.unpackbits(z[f"seed{seed}/strong"])[: img.size].reshape(img.shape)

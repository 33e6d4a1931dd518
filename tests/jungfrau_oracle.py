"""The gain-stage conversion of raw Jungfrau words (csrc/jungfrau_model.hpp) restated in NumPy float32: the truth the kernel, the host
converter and the check program are held to, bit for bit.  Also the frames and calibrations the tests share."""
import numpy as np

INVALID = 0xFFFFFFFF
MAX_PHOTONS = (1 << 24) - 1
MAX_PEDESTAL = 65536.0
MIN_FACTOR, MAX_FACTOR = 2.0 ** -30, 2.0 ** 16


def convert(raw, pedestal, factor):
    """raw: (..., H, W) uint16 words; pedestal, factor: (3, H, W) float32.  -> uint32 of raw's shape."""
    raw = np.asarray(raw, np.uint16)
    p = np.asarray(pedestal, np.float32)
    f = np.asarray(factor, np.float32)
    assert p.dtype == np.float32 and f.dtype == np.float32 and p.shape == f.shape and p.shape[0] == 3 and raw.shape[-2:] == p.shape[1:]
    g = (raw >> 14).astype(np.intp)
    s = np.where(g == 3, 2, np.where(g == 2, 2, g))
    adc = (raw & 0x3FFF).astype(np.float32)
    ped = np.choose(s, [p[0], p[1], p[2]])
    fac = np.choose(s, [f[0], f[1], f[2]])
    with np.errstate(all="ignore"):
        d = adc - ped               # float32 - float32: one float32 operation
        v = d * fac                 # likewise
        q = np.rint(v)              # ties to even
    assert d.dtype == np.float32 and v.dtype == np.float32 and q.dtype == np.float32
    out = np.where(q <= 0, 0, np.where(q >= np.float32(MAX_PHOTONS), MAX_PHOTONS, q.astype(np.int64))).astype(np.uint32)
    invalid = (g == 2) | (raw == 0xFFFF) | (raw == 0xC000) | (fac == 0)
    out[invalid] = INVALID
    return out


def convert_loop(raw, pedestal, factor):
    """The same, a pixel at a time over np.float32 scalars."""
    raw = np.asarray(raw, np.uint16)
    flat = raw.reshape(-1, *raw.shape[-2:])
    out = np.zeros(flat.shape, np.uint32)
    for n in range(flat.shape[0]):
        for y in range(flat.shape[1]):
            for x in range(flat.shape[2]):
                r = int(flat[n, y, x])
                g, adc = r >> 14, r & 0x3FFF
                s = {0: 0, 1: 1, 2: 2, 3: 2}[g]
                ped, fac = np.float32(pedestal[s][y, x]), np.float32(factor[s][y, x])
                if g == 2 or r == 0xFFFF or r == 0xC000 or fac == np.float32(0):
                    out[n, y, x] = INVALID
                    continue
                with np.errstate(all="ignore"):
                    d = np.float32(adc) - ped
                    v = d * fac
                    q = np.rint(v)
                assert type(d) is np.float32 and type(v) is np.float32
                out[n, y, x] = 0 if q <= 0 else MAX_PHOTONS if q >= np.float32(MAX_PHOTONS) else int(q)
    return out.reshape(raw.shape)


def entry_ok(is_factor, v):
    """What ffs_ctx_set_jungfrau_calibration accepts for one entry."""
    v = np.float32(v)
    if not np.isfinite(v):
        return False
    if not is_factor:
        return bool(abs(v) <= np.float32(MAX_PEDESTAL))
    return bool(v == 0 or np.float32(MIN_FACTOR) <= abs(v) <= np.float32(MAX_FACTOR))


def calibration(W, H, seed):
    """A plausible calibration: pedestals near 2800 / 14600 / 15300 ADU, factors of a 12.4 keV beam (G0 positive, G1 and G2 inverted and
    ~30x / ~400x coarser), a few pixels without a calibration in one stage."""
    rng = np.random.default_rng(seed)
    ped = np.stack([rng.normal(m, sd, (H, W)) for m, sd in ((2800, 120), (14600, 90), (15300, 80))]).astype(np.float32)
    gain = np.stack([rng.normal(m, abs(m) * 0.03, (H, W)) for m in (41.0, -1.45, -0.105)])     # ADU per keV
    fac = (1.0 / (gain * 12.4)).astype(np.float32)
    dead = rng.random((3, H, W)) < 0.004
    fac[dead] = 0.0
    return ped, fac


def encode(photons, pedestal, factor, seed):
    """Raw words whose conversion gives `photons` back up to the ADC's resolution: the stage by magnitude (G0 below 25 photons, ~508 ADU
    each; G1 below 700, ~18 ADU each; else G2, ~1.3 ADU each), the ADC clipped to 14 bits -- beyond ~11000 photons G2 runs into ADC 0, the
    saturated word; pixels without a calibration in their stage stay there (invalid)."""
    ph = np.asarray(photons, np.float64)
    s = np.where(ph < 25, 0, np.where(ph < 700, 1, 2))
    ped = np.choose(s, list(np.asarray(pedestal, np.float64)))
    fac = np.choose(s, list(np.asarray(factor, np.float64)))
    with np.errstate(all="ignore"):
        adc = np.where(fac != 0, np.rint(ped + ph / np.where(fac != 0, fac, 1.0)), 0.0)
    adc = np.clip(adc, 0, 0x3FFF).astype(np.uint16)
    raw = (np.array([0, 1, 3], np.uint16)[s] << 14) | adc
    rng = np.random.default_rng(seed)
    u = rng.random(raw.shape)
    raw = np.where(u < 0.001, 0xC000, np.where(u < 0.002, 0xFFFF, np.where(u < 0.003, 0x8000 | (raw & 0x3FFF), raw)))
    return raw.astype(np.uint16)


def stage_mix_frames(n, H, W, pedestal, factor, seed, all_g0=()):
    """n frames of random words in which every run of eight consecutive pixels sees the three stages, the code 2 and the three invalid words
    (where W * H allows), with ADCs near the pedestal so that results spread over 0 .. a few thousand; frames in all_g0 are wholly in G0."""
    rng = np.random.default_rng(seed)
    k = np.arange(H * W)
    out = np.zeros((n, H * W), np.uint16)
    for i in range(n):
        code = np.array([0, 1, 3, 0, 2, 1, 3, 0], np.uint16)[(k + i) % 8]
        adc = rng.integers(0, 0x4000, H * W).astype(np.uint16)
        near = rng.random(H * W) < 0.7
        s = np.where(code == 3, 2, np.minimum(code, 2)).astype(np.intp)
        ped = np.choose(s, [np.asarray(pl).reshape(-1) for pl in pedestal])
        fac = np.choose(s, [np.asarray(pl).reshape(-1) for pl in factor])
        with np.errstate(all="ignore"):
            want = rng.integers(0, 3000, H * W) / np.where(fac != 0, fac.astype(np.float64), 1.0) + ped
        adc = np.where(near, np.clip(np.rint(want), 0, 0x3FFF).astype(np.uint16), adc)
        raw = (code << 14) | adc
        if i in all_g0:
            raw = adc.copy()
        else:
            raw[(k + 3 * i) % 8 == 3] = np.where(rng.random(((k + 3 * i) % 8 == 3).sum()) < 0.5, 0xC000, 0xFFFF)
        out[i] = raw
    return out.reshape(n, H, W)

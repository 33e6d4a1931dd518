"""Batch-to-batch transitions on one stream: the kinds of batch, and the walk through every ordered pair of them.

A stream carries state from one batch to the next (dirty plane / counts / occupancy flags, the extended planes that take turns, the
byte mask that is zero-filled only when asked for, `dense_batch`, the sticky decisions of ffs_wait, tables per mask and window).  A
KIND is everything that defines one batch on a 16-bit context of one shape: frames, mask, parameters, a tuning delta, the input form
and the batch length.  The WALK is a cyclic de Bruijn sequence of order 2 over the kinds: every ordered pair (previous kind, kind),
self-pairs included, exactly once.  Nothing here needs a GPU: tests/test_batch_walk.py holds the inputs to their conditions with the
oracle alone, tests/test_gpu_transitions.py runs the walks."""
from dataclasses import dataclass, field, replace

import numpy as np

from oracle import oracle as O
from util import make_frame

# The shape.  The default kind takes the hot path on it (wave logs + bands), and it is tall for the sake of the `dense` and `overflow`
# kinds: a wave of the streaming kernel owns 62 eight-pixel groups by 72-90 rows and its log holds 256 (row, group) entries, so a frame
# that arrives on the logs WITHOUT overflowing them (flag 32 switches a stream's logs off for good, and the walk would be over) can hold
# 2048 strong pixels per ~37 000 at the very most.  20 480 and 40 000 strong pixels in full groups need a frame of a million.
W, H = 640, 1800
BAND_ROWS = 75                # rows of a streaming band on this shape (24 bands): what the bright rows below are spaced by
MAX_BATCH = 3
MAX_STRONG = 40000            # the context's max_strong_per_frame: the `overflow` kind's big frame is beyond it
CHAIN_LDS_ENTRIES = 20480     # kChainLdsEntries: strong pixels of a frame the one launch's LDS forest holds
CHAIN_MAX_RUNS = 16384        # runs its run-based instantiation holds

ALGO_EXTENDED = 1

# ffs_default_params() with want_reflections on (what bench.py and the driver ask for), restored before every batch
DEFAULT_PARAMS = dict(min_count=2, nsig_b=6.0, nsig_s=3.0, threshold=0.0, max_valid=-1, min_spot_size=3, min_spot_size_3d=3,
                      max_peak_centroid_separation=2.0, want_reflections=1, want_strong_list=0, want_strong_mask=0,
                      algorithm=0, extended_flavour=0, kernel_half_x=3, kernel_half_y=3)
# the tuning keys the kinds change (all may change between batches of a context), at their defaults
DEFAULT_TUNING = dict(threshold_path=0, window_kernel=0, strong_log=1, sparse_stage=2, ext_first_pass=2, ext_e_sparse=0)


@dataclass(frozen=True)
class Kind:
    name: str
    frames: tuple                    # names of FRAMES entries, one per frame of the batch
    mask: int = 0                    # index into masks()
    params: dict = field(default_factory=dict)     # set_params keywords over DEFAULT_PARAMS
    tuning: dict = field(default_factory=dict)     # set_tuning keywords over DEFAULT_TUNING
    form: str = "host"               # host / device / compressed

    @property
    def all_params(self):
        return {**DEFAULT_PARAMS, **self.params}

    @property
    def all_tuning(self):
        return {**DEFAULT_TUNING, **self.tuning}

    @property
    def extended(self):
        return self.all_params["algorithm"] == ALGO_EXTENDED

    @property
    def window(self):
        p = self.all_params
        return not self.extended and self.all_tuning["threshold_path"] != 2 and (
            (p["kernel_half_x"], p["kernel_half_y"]) != (3, 3) or self.all_tuning["window_kernel"] == 1)

    @property
    def wants_lists_or_bytes(self):
        return bool(self.all_params["want_strong_list"] or self.all_params["want_strong_mask"])


def _sparse(seed):
    return lambda: make_frame(W=W, H=H, seed=seed, n_spots=40)[0]


def _flat():
    """Pixels of 3 and 4 everywhere: nothing is strong, and every word of the image is non-zero."""
    return np.random.default_rng(5).integers(3, 5, (H, W)).astype(np.uint16)


def _rows_frame(seed, period, bars=0):
    """Dense data the wave logs can carry: a sparse frame plus a full-width bright row every `period` rows (every pixel of such a row
    is strong, eight to a log entry: a wave finds 62 entries per row, and ceil(BAND_ROWS / period) rows at most), plus a few one-pixel
    columns that join two neighbouring rows into one component."""
    rng = np.random.default_rng(seed)
    img = make_frame(W=W, H=H, seed=seed, n_spots=40)[0].copy()
    ys = np.arange(int(rng.integers(2, period - 2)), H, period)
    for y in ys:
        img[y, :] = rng.integers(1500, 4000, W).astype(np.uint16)
    for _ in range(bars):
        i, x = int(rng.integers(0, len(ys) - 1)), int(rng.integers(0, W))
        img[ys[i]:ys[i + 1], x] = 3000
    return img


_SPARSE_KINDS = ["default", "lists", "bytemask", "ext0", "ext1", "ext_plain", "win52", "win_as_7x7", "path1", "path2", "plane", "grid",
                 "device_in", "compressed", "odd_params"]
_BUILDERS = {f"{k}{f}": _sparse(1000 + 10 * i + f) for i, k in enumerate(_SPARSE_KINDS) for f in range(3)}
_BUILDERS.update({
    "dense0": lambda: _rows_frame(60, 38, 2), "dense1": lambda: _rows_frame(61, 40, 2), "dense2": lambda: _rows_frame(62, 42, 1),
    "zeros": lambda: np.zeros((H, W), np.uint16), "flat": _flat, "sevens": lambda: np.full((H, W), 7, np.uint16),
    "short0": _sparse(1900),
    "overflow0": _sparse(1910), "big": lambda: _rows_frame(70, 25), "overflow2": _sparse(1912),
})
_frames = {}


def frame(name):
    """One frame of the fixed set, built on first use."""
    if name not in _frames:
        _frames[name] = _BUILDERS[name]()
        _frames[name].setflags(write=False)
    return _frames[name]


_masks = []


def masks():
    """Mask 0: every pixel valid.  Mask 1: module gaps, dead pixels and a rectangle."""
    if not _masks:
        _masks.extend([np.ones((H, W), np.uint8), make_frame(W=W, H=H, seed=7, n_spots=1, masked=True)[1]])
    return _masks


def _three(name):
    return tuple(f"{name}{f}" for f in range(3))


KINDS = [
    Kind("default", _three("default")),
    Kind("lists", _three("lists"), params=dict(want_strong_list=1, want_reflections=1)),
    Kind("bytemask", _three("bytemask"), params=dict(want_strong_mask=1)),         # (right after two kinds that do not ask for it)
    Kind("dense", _three("dense")),
    Kind("empty", ("zeros", "flat", "sevens")),
    Kind("short", ("short0",)),
    Kind("overflow", ("overflow0", "big", "overflow2")),
    Kind("ext0", _three("ext0"), params=dict(algorithm=ALGO_EXTENDED, extended_flavour=0)),
    Kind("ext1", _three("ext1"), mask=1, params=dict(algorithm=ALGO_EXTENDED, extended_flavour=1, want_strong_mask=1),
         tuning=dict(ext_e_sparse=1)),
    Kind("ext_plain", _three("ext_plain"), params=dict(algorithm=ALGO_EXTENDED), tuning=dict(ext_first_pass=0)),
    Kind("win52", _three("win52"), mask=1, params=dict(kernel_half_x=5, kernel_half_y=2)),
    Kind("win_as_7x7", _three("win_as_7x7"), tuning=dict(window_kernel=1)),
    Kind("path1", _three("path1"), tuning=dict(threshold_path=1)),
    Kind("path2", _three("path2"), tuning=dict(threshold_path=2)),
    Kind("plane", _three("plane"), tuning=dict(strong_log=0)),
    Kind("grid", _three("grid"), tuning=dict(sparse_stage=1)),
    Kind("device_in", _three("device_in"), form="device"),
    Kind("compressed", _three("compressed"), form="compressed"),
    Kind("odd_params", _three("odd_params"), params=dict(min_count=3, nsig_b=4.0, nsig_s=2.5, threshold=4.0, max_valid=1000, min_spot_size=1,
                                                         max_peak_centroid_separation=0.5)),
]
BY_NAME = {k.name: k for k in KINDS}
NOT_SPARSE = ("dense", "empty", "overflow")      # kinds whose frames are not "50 to 5000 strong pixels, 5 components"


def in_flight_kinds():
    """The kinds that differ by parameters, data, input form and batch length alone: what may change while other batches of the
    context are in flight (the header promises the parameter snapshot at submit; tuning and mask stay fixed).  The two kinds that
    carry a mask or a tuning delta besides take part without it, under a name of their own."""
    out = []
    for k in KINDS:
        if not k.tuning and k.mask == 0:
            out.append(k)
        elif k.name in ("ext1", "win52"):
            out.append(replace(k, name=k.name + "_m0", mask=0, tuning={}))
    return out


def de_bruijn(n):
    """The cyclic de Bruijn sequence B(n, 2) as the concatenation of the Lyndon words whose length divides 2, in lexicographic order
    (Fredricksen-Kessler-Maiorana): n * n symbols, every ordered pair of symbols once as (s[i - 1], s[i]), cyclically."""
    seq = []
    for a in range(n):
        seq.append(a)                        # the Lyndon word (a)
        for b in range(a + 1, n):
            seq.extend((a, b))               # the Lyndon words (a, b), a < b -- which sort between (a) and (a + 1)
    assert len(seq) == n * n
    return seq


def walk(kinds=KINDS, offset=0):
    """[(previous kind or None, kind)]: the de Bruijn sequence over `kinds` from `offset` on, plus its first batch once more at the end
    -- a stream has no batch before its first, so the wrap-around pair needs one batch of its own: n * n + 1 batches, n * n pairs."""
    seq = de_bruijn(len(kinds))
    seq = seq[offset:] + seq[:offset]
    seq = seq + seq[:1]
    return [(kinds[seq[i - 1]] if i else None, kinds[seq[i]]) for i in range(len(seq))]


# ---- the oracle's answer for a frame of a kind -----------------------------------------------------------------------------------
@dataclass
class Want:
    strong: np.ndarray
    cc: object
    refl: object
    first: np.ndarray = None         # extended kinds: the first-pass plane and the eroded signal region
    eroded: np.ndarray = None

    @property
    def precomputed(self):
        return self.strong, self.cc, self.refl


def disp_params(kind):
    p = kind.all_params
    return O.DispParams(p["kernel_half_x"], p["kernel_half_y"], p["min_count"], p["threshold"], p["nsig_b"], p["nsig_s"])


def strong_mask(kind, img, mask, debug=False):
    """The oracle's strong pixels of `img` under the kind's parameters (extended, debug: also its two intermediate planes)."""
    p = kind.all_params
    if kind.extended:
        return O.dispersion_extended(img, mask, disp_params(kind), flavour=p["extended_flavour"], max_valid=float(p["max_valid"]), debug=debug)
    strong = O.dispersion(img, mask, disp_params(kind))
    if p["max_valid"] >= 0:
        strong = strong & (img <= p["max_valid"]).astype(np.uint8)     # the device kernels' trusted-range rule on the centre pixel
    return strong


def oracle_kind_frame(kind, f):
    img, mask, p = frame(kind.frames[f]), masks()[kind.mask], kind.all_params
    first = eroded = None
    if kind.extended:
        strong, first, eroded = strong_mask(kind, img, mask, debug=True)
    else:
        strong = strong_mask(kind, img, mask)
    cc = O.cc2d(strong, img, p["min_spot_size"])
    refl = O.cc2d_reflections(cc.k, cc.intensity, W, H, p["min_spot_size"], p["max_peak_centroid_separation"])
    return Want(strong, cc, refl, first, eroded)


class OracleCache:
    """Oracle results once per (kind, frame)."""

    def __init__(self):
        self._want = {}

    def __call__(self, kind, f):
        key = (kind.name, f)
        if key not in self._want:
            self._want[key] = oracle_kind_frame(kind, f)
        return self._want[key]


def run_counts(strong):
    """(horizontal runs, runs cut at the 32-pixel words of the bit plane) of a strong mask."""
    s = strong.astype(bool)
    starts = s.copy()
    starts[:, 1:] &= ~s[:, :-1]
    word_starts = starts.copy()
    word_starts[:, 32::32] |= s[:, 32::32]
    return int(starts.sum()), int(word_starts.sum())


# ---- the walker: what is called on the context and the stream before and for each batch ------------------------------------------
class Walker:
    """Issues one batch of a kind on a stream.  Before each batch: the default tuning and parameters with the kind's over them (one call
    each, so that no combination in between is ever set), and set_mask only when the mask id changes.  `resident(ctx, frames)` puts
    frames into the library's device layout for the `device` form (util._resident on a GPU) and `compress(frame)` makes a chunk."""

    def __init__(self, ctx, resident=None, compress=None):
        self.ctx = ctx
        self.mask_id = None
        self._resident, self._compress = resident, compress
        self._dev, self._chunks = {}, {}

    def prepare(self, kind, tuning=True, mask=True):
        if tuning:
            self.ctx.set_tuning(**kind.all_tuning)
        self.ctx.set_params(**kind.all_params)
        if mask and kind.mask != self.mask_id:
            self.ctx.set_mask(masks()[kind.mask])
            self.mask_id = kind.mask

    def frames(self, kind):
        return np.stack([frame(n) for n in kind.frames])

    def submit(self, stream, kind, first_frame_id):
        if kind.form == "device":
            if kind.name not in self._dev:
                self._dev[kind.name] = self._resident(self.ctx, self.frames(kind))
            mem, pitch, fstride = self._dev[kind.name]
            stream.submit_device(mem.data_ptr(), pitch, fstride, len(kind.frames), first_frame_id=first_frame_id)
        elif kind.form == "compressed":
            if kind.name not in self._chunks:
                self._chunks[kind.name] = [self._compress(frame(n)) for n in kind.frames]
            stream.submit_compressed(self._chunks[kind.name], first_frame_id=first_frame_id)
        else:
            stream.submit(self.frames(kind), first_frame_id=first_frame_id)

    def run(self, stream, kind, first_frame_id):
        self.prepare(kind)
        self.submit(stream, kind, first_frame_id)
        return stream.wait()

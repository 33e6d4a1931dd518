"""GPU: the settings of a context through the library's setters (csrc/context_settings.hpp behind ffs_ctx_set_*): each of the six pairs of
settings that do not combine, in both call orders -- the first call is accepted, the second is refused with the text that
tests/context_settings_check.cc holds for that caller, and the first setting stays in force -- and the entry refusals of the gain map, the
bin map and the Jungfrau calibration.  No batch is submitted."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H = 16, 8
NO_GAIN = "the reference's device kernels, which that flavour copies, have no gain"
EROSION = "the device-flavour erosion skips masked neighbours by the static mask"
# per rule: the text for the first side's setter, the text for the second side's
TEXTS = {
    "no_map": ("ffs_ctx_set_params: the radial_profile algorithm needs a radial bin map (ffs_ctx_set_radial_bins) and the context has none",
               "ffs_ctx_set_radial_bins: the context's parameters say the radial_profile algorithm, which needs the map: set another algorithm first"),
    "wide_map": ("ffs_ctx_set_params: the radial_profile algorithm takes a radial bin map of at most 128 bins and the context's has 129",
                 "ffs_ctx_set_radial_bins: the context's parameters say the radial_profile algorithm, which takes at most 128 bins, got 129"),
    "flavour_scope": ("ffs_ctx_set_params: extended_flavour 1 cannot be combined with the window scope of max_valid (ffs_ctx_set_max_valid_scope): " + EROSION,
                      "ffs_ctx_set_max_valid_scope: the window scope cannot be combined with extended_flavour 1: " + EROSION),
    "flavour_gain": ("ffs_ctx_set_params: extended_flavour 1 cannot be combined with a detector gain (ffs_ctx_set_gain): " + NO_GAIN,
                     "ffs_ctx_set_gain: a detector gain cannot be combined with extended_flavour 1: " + NO_GAIN),
    "gain_and_map": ("ffs_ctx_set_gain: a gain map is set (ffs_ctx_set_gain_map): drop it with ffs_ctx_set_gain_map(ctx, NULL) first",
                     "ffs_ctx_set_gain_map: a scalar gain is set (ffs_ctx_set_gain): switch it off with ffs_ctx_set_gain(ctx, 0) first"),
    "flavour_map": ("ffs_ctx_set_params: extended_flavour 1 cannot be combined with a gain map (ffs_ctx_set_gain_map): " + NO_GAIN,
                    "ffs_ctx_set_gain_map: a gain map cannot be combined with extended_flavour 1: " + NO_GAIN),
}
BINS = (np.arange(W * H, dtype=np.uint16).reshape(H, W) % 100)
WIDE = (np.arange(W * H, dtype=np.uint16).reshape(H, W) % 129)
GAINS = np.full((H, W), 1.5, np.float32)


def _params(ctx, **kw):
    """set_params that leaves the binding's copy of the parameters as the library's when the call is refused"""
    before = {k: getattr(ctx.params, k) for k in kw}
    try:
        ctx.set_params(**kw)
    except Exception:
        for k, v in before.items():
            setattr(ctx.params, k, v)
        raise


def _sides(ffs):
    """per rule: (on, off) of its first side and (on, off) of its second -- `on` is the value the rule is about, `off` one it lets through"""
    radial = (lambda c: _params(c, algorithm=ffs.ALGO_RADIAL_PROFILE), lambda c: _params(c, algorithm=ffs.ALGO_DISPERSION))
    flavour = (lambda c: _params(c, extended_flavour=1), lambda c: _params(c, extended_flavour=0))
    gain = (lambda c: c.set_gain(2.5), lambda c: c.set_gain(0.0))
    gain_map = (lambda c: c.set_gain_map(GAINS), lambda c: c.set_gain_map(None))
    scope = (lambda c: c.set_max_valid_scope("window"), lambda c: c.set_max_valid_scope("centre"))
    a_map = lambda c: c.set_radial_bins(BINS, 100)
    return {
        "no_map": (radial, (lambda c: c.set_radial_bins(None), a_map)),
        "wide_map": (radial, (lambda c: c.set_radial_bins(WIDE, 129), a_map)),
        "flavour_scope": (flavour, scope),
        "flavour_gain": (flavour, gain),
        "gain_and_map": (gain, gain_map),
        "flavour_map": (flavour, gain_map),
    }


def _refused(ffs, call, ctx, text):
    with pytest.raises(ffs.FfsError) as e:
        call(ctx)
    assert str(e.value) == f"libffs_hip error -1: {text}"


@pytest.mark.parametrize("order", ["first_then_second", "second_then_first"])
@pytest.mark.parametrize("rule", list(TEXTS))
def test_whichever_call_comes_second_is_refused(ffs, rule, order):
    sides = _sides(ffs)[rule]
    i = 0 if order == "first_then_second" else 1
    (on_a, _), (on_b, off_b), text_b = sides[i], sides[1 - i], TEXTS[rule][1 - i]
    ctx = ffs.Context(W, H, np.uint16)
    if rule in ("no_map", "wide_map"):
        ctx.set_radial_bins(BINS, 100)      # the radial_profile algorithm can only be set over a map of at most 128 bins
    on_a(ctx)                               # the first call is accepted
    _refused(ffs, on_b, ctx, text_b)        # the second is refused, with its own text
    off_b(ctx)                              # its "off" value goes through, and so does the first call again ...
    on_a(ctx)
    _refused(ffs, on_b, ctx, text_b)        # ... which is still in force


def test_entry_refusals_name_index_position_and_value(ffs):
    ctx = ffs.Context(W, H, np.uint16)
    gains = GAINS.copy()
    gains[5, 7] = 0.0
    _refused(ffs, lambda c: c.set_gain_map(gains), ctx,
             "ffs_ctx_set_gain_map: entry 87 (x = 7, y = 5) is 0.000000: every entry must be finite and in [2^-60, 2^60], under masked pixels too")
    bins = BINS.copy()
    bins[5, 7] = 100
    _refused(ffs, lambda c: c.set_radial_bins(bins, 100), ctx,
             "ffs_ctx_set_radial_bins: entry 87 (x = 7, y = 5) is 100: every entry must be below n_bins = 100 or 0xFFFF (in no bin)")
    # neither left anything in force: what each would have stood against goes through
    ctx.set_gain(2.5)
    _refused(ffs, lambda c: _params(c, algorithm=ffs.ALGO_RADIAL_PROFILE), ctx, TEXTS["no_map"][0])


def test_calibration_refusals(ffs):
    pedestal, factor = np.zeros((3, H, W), np.float32), np.ones((3, H, W), np.float32)
    _refused(ffs, lambda c: c.set_jungfrau_calibration(pedestal, factor), ffs.Context(W, H, np.uint16),
             "ffs_ctx_set_jungfrau_calibration: raw Jungfrau words convert to 32-bit photon counts: the context must have pixel_bytes 4")
    ctx = ffs.Context(W, H, np.uint32)
    ctx.set_jungfrau_calibration(pedestal, factor)
    bad = pedestal.copy()
    bad[1, 5, 7] = 70000.0
    _refused(ffs, lambda c: c.set_jungfrau_calibration(bad, factor), ctx,
             "ffs_ctx_set_jungfrau_calibration: pedestal[1] entry 87 (x = 7, y = 5) is 70000.000000: a pedestal must be finite and in [-65536, 65536]")
    bad = factor.copy()
    bad[2, 5, 7] = 1e6
    _refused(ffs, lambda c: c.set_jungfrau_calibration(pedestal, bad), ctx,
             "ffs_ctx_set_jungfrau_calibration: factor[2] entry 87 (x = 7, y = 5) is 1000000.000000: a factor must be 0 (no calibration) or finite with a magnitude in "
             "[2^-30, 2^16]")
    ctx.set_jungfrau_calibration(None)

"""CPU only: the host arithmetic of the pixel histograms -- hist_quantiles and hist_exceedance on counters formed in numpy by the fp32 rule of the
device kernel (t = (v - lo) * scale, one subtraction then one multiplication; row 0: t < 0, row 1 + floor(t): 0 <= t < B, row B + 1: the rest) --
and the argument checks of the samplers and entry points, which must raise before any device call."""
import numpy as np
import pytest


def numpy_counts(x, B, lo, scale):
    """[C, H, W] fp32 samples -> [B + 2, H, W] int64 counters by the rule of csrc/lmc_pixel_hist.hip"""
    x = np.asarray(x)
    assert x.dtype == np.float32 and np.asarray(lo).dtype == np.float32 and np.asarray(scale).dtype == np.float32
    with np.errstate(invalid="ignore", over="ignore"):
        t = (x - lo) * scale
        assert t.dtype == np.float32
        row = np.where(t < 0, 0, np.where(t < np.float32(B), 1 + np.floor(t), B + 1)).astype(np.int64)
    counts = np.zeros((B + 2,) + x.shape[1:], dtype=np.int64)
    for r in range(B + 2):
        counts[r] = (row == r).sum(axis=0)
    return counts


def gaussian_case(width):
    """148 samples per pixel of 200 + N(0, 1) at 9 x 7; the range is the pixel's own mean -+ width std"""
    rng = np.random.default_rng(3)
    x = (200.0 + rng.standard_normal((148, 9, 7))).astype(np.float32)
    m, s = x.mean(0, dtype=np.float64), x.std(0, dtype=np.float64)
    lo, hi = (m - width * s).astype(np.float32), (m + width * s).astype(np.float32)
    scale = np.float32(62) / (hi - lo)
    return x, lo, scale


def test_hist_quantiles_lie_within_one_bin_of_the_sample_quantiles():
    """The estimate and np.quantile(method="inverted_cdf") -- the ceil(q n)-th order statistic -- lie in the same bin by construction, so they differ by
    at most one bin width; 1e-4 of a bin covers the fp32 rounding of t (at most 62 x 2 x 6e-8 of a bin).  Measured here: 0.72 bin widths at worst."""
    from lmc_atomi_amd import hist_quantiles
    x, lo, scale = gaussian_case(4.0)
    counts = numpy_counts(x, 62, lo, scale)
    assert counts[0].sum() == 0 and counts[-1].sum() == 0, "the case is built without tail mass"
    assert (counts.sum(0) == 148).all()
    qs = (0.05, 0.25, 0.5, 0.95)
    est = hist_quantiles(counts, lo, scale, qs)
    assert est.shape == (4, 9, 7) and est.dtype == np.float64
    ref = np.quantile(x.astype(np.float64), qs, axis=0, method="inverted_cdf")
    err_bins = np.abs(est - ref) * scale.astype(np.float64)
    print("worst error in bin widths:", err_bins.max())
    assert err_bins.max() <= 1 + 1e-4, err_bins.max()


def test_a_quantile_outside_the_range_is_infinite_not_clamped():
    from lmc_atomi_amd import hist_quantiles
    x, lo, scale = gaussian_case(0.5)            # mean -+ 0.5 std: some 31 % of the mass in either tail row
    counts = numpy_counts(x, 62, lo, scale)
    assert (counts[0] > 0.05 * 148).all() and (counts[-1] > 0.05 * 148).all()
    est = hist_quantiles(counts, lo, scale, (0.05, 0.5, 0.95))
    assert (est[0] == -np.inf).all() and (est[2] == np.inf).all()
    assert np.isfinite(est[1]).all() and (np.abs(est[1] - 200.0) < 1.0).all()


def test_torch_and_numpy_containers_agree():
    import torch
    from lmc_atomi_amd import hist_exceedance, hist_quantiles
    x, lo, scale = gaussian_case(2.0)
    counts = numpy_counts(x, 62, lo, scale)
    qs = (0.05, 0.5, 0.95)
    a = hist_quantiles(counts, lo, scale, qs)
    b = hist_quantiles(torch.from_numpy(counts), torch.from_numpy(lo), torch.from_numpy(scale), qs)
    assert isinstance(b, torch.Tensor) and b.dtype == torch.float64 and tuple(b.shape) == (3, 9, 7)
    np.testing.assert_array_equal(b.numpy(), a)
    e = hist_exceedance(torch.from_numpy(counts), torch.from_numpy(lo), torch.from_numpy(scale), 200.5)
    assert isinstance(e, torch.Tensor) and e.dtype == torch.float64
    np.testing.assert_array_equal(e.numpy(), hist_exceedance(counts, lo, scale, 200.5))


def test_hist_exceedance_equals_a_direct_count_on_bin_edges():
    """lo = 0, scale = 1: the edges are the integers, t = v exactly; for t on an edge the fraction is P(x >= t) of the samples themselves, for t between
    edges that of the next edge above."""
    from lmc_atomi_amd import hist_exceedance
    rng = np.random.default_rng(8)
    B = 7
    x = (rng.integers(-6, 2 * (B + 3) + 1, (41, 9, 7)) * 0.5).astype(np.float32)      # integers and half-integers in [-3, B + 3]
    lo, scale = np.zeros((9, 7), np.float32), np.ones((9, 7), np.float32)
    counts = numpy_counts(x, B, lo, scale)
    for t, edge in ((3.0, 3.0), (2.25, 3.0), (0.0, 0.0), (-2.0, 0.0), (float(B), float(B)), (B + 0.5, np.inf)):
        got = hist_exceedance(counts, lo, scale, t)
        np.testing.assert_array_equal(got, (x >= edge).mean(axis=0, dtype=np.float64), err_msg=f"t = {t}")
    np.testing.assert_array_equal(hist_exceedance(counts, lo, scale, np.inf), np.zeros((9, 7)))
    np.testing.assert_array_equal(hist_exceedance(counts, lo, scale, -np.inf), (x >= 0).mean(axis=0, dtype=np.float64))
    with pytest.raises(ValueError, match="NaN"):
        hist_exceedance(counts, lo, scale, np.nan)
    tmap = rng.integers(0, B + 1, (9, 7)).astype(np.float64)                             # a threshold per pixel
    np.testing.assert_array_equal(hist_exceedance(counts, lo, scale, tmap), (x >= tmap[None]).mean(axis=0, dtype=np.float64))


class _NoDevice:
    """stands where a prox would: a sampler that reached it has gone past the argument checks"""
    def __getattr__(self, name):
        raise AssertionError("the argument check must come before anything else")


@pytest.mark.parametrize("cls", ["MYULASampler", "MYMALASampler", "ULPDASampler"])
def test_histogram_arguments_raise_before_any_device_call(cls):
    import lmc_atomi_amd as la
    args = (_NoDevice(), _NoDevice(), (16, 16)) if cls != "ULPDASampler" else (_NoDevice(), _NoDevice(), _NoDevice(), (16, 16))
    make = getattr(la, cls)
    with pytest.raises(ValueError, match="moments=True"):
        make(*args, n_chains=2, tau=0.1, moments=False, hist_bins=16, hist_range=(0.0, 1.0))
    for bad in (0, 63):
        with pytest.raises(ValueError, match="hist_bins"):
            make(*args, n_chains=2, tau=0.1, moments=True, hist_bins=bad, hist_range=(0.0, 1.0))
    with pytest.raises(ValueError, match="go together"):
        make(*args, n_chains=2, tau=0.1, moments=True, hist_bins=16)
    with pytest.raises(ValueError, match="go together"):
        make(*args, n_chains=2, tau=0.1, moments=True, hist_range=(0.0, 1.0))
    lo, hi = np.zeros((16, 16)), np.ones((16, 16))
    hi[3, 5] = 0.0                                                 # hi <= lo at one pixel
    with pytest.raises(ValueError, match="hist_range"):
        make(*args, n_chains=2, tau=0.1, moments=True, hist_bins=16, hist_range=(lo, hi))
    lo[7, 1] = np.nan
    with pytest.raises(ValueError, match="finite"):
        make(*args, n_chains=2, tau=0.1, moments=True, hist_bins=16, hist_range=(lo, np.ones((16, 16))))
    with pytest.raises(ValueError, match="finite"):
        make(*args, n_chains=2, tau=0.1, moments=True, hist_bins=16, hist_range=(0.0, np.inf))


def test_entry_points_refuse_a_histogram_in_the_reference_form():
    import lmc_atomi_amd as la
    kw = dict(hist_bins=8, hist_range=(0.0, 1.0))
    with pytest.raises(ValueError, match="hist_bins"):
        la.MoreauYosidaUnadjustedLangevin(_NoDevice(), _NoDevice(), np.zeros(64), tau=0.1, gamma=0.5, niter=2, dims=(8, 8), **kw)
    with pytest.raises(ValueError, match="hist_bins"):
        la.UnadjustedLangevinPrimalDual(_NoDevice(), _NoDevice(), _NoDevice(), np.zeros(64), 0.1, 1.0, niter=2, dims=(8, 8), **kw)

"""Pixel-wise posterior histograms (lmc_pixel_histogram / lmc_sampler_set_histogram / lmc_sampler_get_histogram / lmc_allreduce_histogram): per pixel
B + 2 unsigned 64-bit counters over the kept samples, rows by the fp32 rule t = (v - lo) * scale (row 0: t < 0, row 1 + floor(t): 0 <= t < B, row
B + 1: everything else).

The reference is that rule in numpy fp32 (tests/test_pixel_hist_api.py: numpy_counts) on the fp32 states themselves.  The counters are integers added
by integer atomics, so every comparison is assert_array_equal: no launch shape, atomic order or stream may change a single count."""

import numpy as np
import pytest

from tests import test_gpu_block_moments as BM
from tests.test_pixel_hist_api import numpy_counts

pytestmark = pytest.mark.gpu

TAU, GAMMA = BM.TAU, BM.GAMMA


@pytest.fixture(scope="module")
def la():
    import torch
    assert torch.cuda.is_available()
    import lmc_atomi_amd as la
    return la


def crafted_states(rng, C_, shape, B):
    """integers and half-integers in [-3, B + 3] (every edge v = k is hit exactly), and a few pixels of -inf, +inf, NaN and -0.0"""
    x = (rng.integers(-6, 2 * (B + 3) + 1, (C_,) + shape) * 0.5).astype(np.float32)
    flat = x.reshape(-1)
    where = rng.choice(flat.size, size=min(16, flat.size // 4), replace=False)
    flat[where] = np.resize(np.array([-np.inf, np.inf, np.nan, -0.0], dtype=np.float32), where.size)
    return x


# The kernel gives a wave 128 consecutive pixels, a lane the pixels l and 64 + l of them, a workgroup 512.  (16, 64) = 1024 pixels: two full workgroups;
# (19, 203) = 3857: eight workgroups, the last with one full wave and one whose only pixel is in its first slot; (9, 7) = 63: less than one wave, second slot
# empty; (9, 11) = 99: the second slot of a wave partly inside the image (H W mod 128 in 65 .. 127); (33, 520): many workgroups, a partial last one.
# 3 chains: only the one-by-one tail of the chain loop; 37: groups of eight and a tail; 300: two chain segments.
CRAFTED = [(shape, C_) for shape in [(16, 64), (19, 203), (9, 7), (9, 11), (33, 520)] for C_ in (3, 37)] + [((9, 7), 300), ((16, 64), 300)]


@pytest.mark.parametrize("B", [1, 7, 62])
@pytest.mark.parametrize("shape,C_", CRAFTED)
def test_stateless_histogram_of_crafted_states_equals_the_rule(la, shape, C_, B):
    import torch
    rng = np.random.default_rng(1000 * B + shape[1] + C_)
    x = crafted_states(rng, C_, shape, B)
    lo, scale = np.zeros(shape, np.float32), np.ones(shape, np.float32)      # hi = B: scale = B / (B - 0) = 1 exactly, so t = v
    want = numpy_counts(x, B, lo, scale)
    assert (want.sum(0) == C_).all()
    neg_zero = np.argwhere((x == 0) & np.signbit(x))
    assert len(neg_zero), "the case holds a -0.0"
    c, i, j = neg_zero[0]
    assert want[1, i, j] >= 1                                                 # -0.0 belongs to row 1, not to row 0
    xd = torch.from_numpy(x).cuda()
    got = la.pixel_histogram(xd, B, 0.0, float(B))
    assert got.dtype == torch.int64 and tuple(got.shape) == (B + 2,) + shape and got.is_cuda
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    np.testing.assert_array_equal(got.sum(0).cpu().numpy(), np.full(shape, C_))
    again = la.pixel_histogram(xd, B, 0.0, float(B), out=got)
    assert again is got
    np.testing.assert_array_equal(got.cpu().numpy(), 2 * want)


# (chains, LMC_HIST_SEG): without the variable the launcher splits the chains of an image this small into segments of 129 .. 256 -- 248 chains in one
# segment, 300 in two of 150, 511 in two of 256 and 255.  With it the segments have the length it names, as they have on large images: 2040 chains in ONE
# segment (the most the eleven planes are sized for: 2040 = 0b11111111000, planes 3 .. 10), 2300 in two of 1150, 1100 in two of 550, 1024 in one.
LONG_SEGMENTS = [(248, None), (300, None), (511, None), (2040, "2040"), (2300, "2040"), (1100, "1024"), (1024, "1024")]


@pytest.mark.parametrize("shape", [(16, 64), (9, 11)])
@pytest.mark.parametrize("C_,seg", LONG_SEGMENTS)
def test_every_chain_in_one_bin_fills_the_high_bits_of_the_counters(la, shape, C_, seg, monkeypatch):
    """The same value in every chain: a whole chain segment lands in ONE row of a pixel, so the in-register counters hold the segment's length -- up to the
    2040 they are sized for, every plane in use."""
    import torch
    if seg is not None:
        monkeypatch.setenv("LMC_HIST_SEG", seg)      # read at every launch
    B = 7
    rng = np.random.default_rng(C_)
    img = (rng.integers(-2, 2 * (B + 1) + 1, shape) * 0.5).astype(np.float32)
    x = np.broadcast_to(img, (C_,) + shape).copy()
    want = numpy_counts(x, B, np.zeros(shape, np.float32), np.ones(shape, np.float32))
    assert want.max() == C_
    got = la.pixel_histogram(torch.from_numpy(x).cuda(), B, 0.0, float(B))
    np.testing.assert_array_equal(got.cpu().numpy(), want)


@pytest.mark.parametrize("shape", [(16, 64), (9, 11)])
@pytest.mark.parametrize("C_,seg", [(2040, "2040"), (2300, "2040"), (1100, "1024")])
def test_long_segments_of_crafted_states_equal_the_rule(la, shape, C_, seg, monkeypatch):
    """Segments of 2040, 1150 and 550 chains with every row of a pixel in use (B = 62, values on every edge): counts of all sizes in the planes at once."""
    import torch
    monkeypatch.setenv("LMC_HIST_SEG", seg)
    B = 62
    x = crafted_states(np.random.default_rng(C_ + shape[1]), C_, shape, B)
    want = numpy_counts(x, B, np.zeros(shape, np.float32), np.ones(shape, np.float32))
    got = la.pixel_histogram(torch.from_numpy(x).cuda(), B, 0.0, float(B))
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    np.testing.assert_array_equal(got.sum(0).cpu().numpy(), np.full(shape, C_))


@pytest.mark.parametrize("shape,C_", [((16, 64), 37), ((19, 203), 37), ((33, 520), 19)])
def test_stateless_histogram_of_realistic_states_equals_the_rule(la, shape, C_):
    """States 200 + N(0, 1) and a range of its own per pixel, mean -+ 2 std: neither lo nor scale is a round number, and both tails carry mass."""
    import torch
    rng = np.random.default_rng(shape[1])
    x = (200.0 + rng.standard_normal((C_,) + shape)).astype(np.float32)
    m, s = x.mean(0, dtype=np.float64), x.std(0, dtype=np.float64)
    lo, hi = (m - 2 * s).astype(np.float32), (m + 2 * s).astype(np.float32)
    scale = np.float32(62) / (hi - lo)
    want = numpy_counts(x, 62, lo, scale)
    assert want[0].sum() > 0 and want[-1].sum() > 0, "both tail rows carry mass"
    got = la.pixel_histogram(torch.from_numpy(x).cuda(), 62, lo, torch.from_numpy(hi))      # numpy and torch ranges alike
    np.testing.assert_array_equal(got.cpu().numpy(), want)


def pixel_range(y, half=2.0):
    return (y - half).astype(np.float32), (y + half).astype(np.float32)


def check_sampler_arrays(smp, B, lo, hi):
    assert smp.hist_bins == B
    np.testing.assert_array_equal(smp.hist_lo.cpu().numpy(), lo)
    np.testing.assert_array_equal(smp.hist_scale.cpu().numpy(), np.float32(B) / (hi - lo))
    return smp.hist_lo.cpu().numpy(), smp.hist_scale.cpu().numpy()


@pytest.mark.parametrize("burn,thin", [(2, 2), (1, 5)])
@pytest.mark.parametrize("tag", sorted(BM.GROUPINGS))
def test_histogram_over_every_launch_grouping(la, tag, burn, thin):
    """step(4); step(1); step(9) with the reductions in line (moments_overlap -1) and on the side stream (1): equal counts, equal to the rule applied to
    the states of a step(1) replay where the grouping can be replayed; final states bit-identical to a sampler without a histogram, s1 / s2 within the
    tolerance of the float64 atomics.  The groupings run on the sampler's own Philox noise, as in tests/test_gpu_block_moments.py: injected noise takes
    one iteration per launch whatever the policy, so it would never reach the pair launches; it gets a run of its own at the end."""
    shape, C_, problem, policy, kernel, replay = BM.GROUPINGS[tag]
    B = 62
    rng = np.random.default_rng(11)
    if problem == "mask_haar":
        y, pf, pg = BM.mask_haar_problem(la, shape, rng)
    else:
        y, pf, pg = BM.blur_problem(la, shape, rng, "tv" if problem == "blur_tv" else "l2")
    x0 = (200.0 + rng.normal(0, 1.0, (C_,) + shape)).astype(np.float32)
    noise = rng.standard_normal((14, C_) + shape).astype(np.float32)
    kw = dict(n_chains=C_, tau=TAU, gamma=GAMMA)
    lo = hi = None

    def run(overlap, hist, single=False, injected=False):
        pol = dict(policy or {}, moments_overlap=overlap)
        extra = dict(hist_bins=B, hist_range=(lo, hi)) if hist else {}
        extra.update(dict(noise="injected") if injected else dict(seed=5))
        given = (lambda a, b: dict(noise=noise[a:b])) if injected else (lambda a, b: {})
        smp = la.MYULASampler(pf, pg, shape, moments=True, burn_in=burn, thin=thin, policy=pol, **extra, **kw)
        kept = []
        try:
            smp.set_state(x0)
            if single:
                for it in range(14):
                    smp.step(1, **given(it, it + 1))
                    if it >= burn and (it - burn) % thin == 0:
                        kept.append(smp.get_state().cpu().numpy())
            else:
                smp.step(4, **given(0, 4))
                if not injected:
                    assert kernel in smp.kernel_name, smp.kernel_name
                smp.step(1, **given(4, 5))
                smp.step(9, **given(5, 14))
            s1, s2, n = smp.moments()
            out = dict(x=smp.get_state().cpu().numpy(), s1=s1.cpu().numpy(), s2=s2.cpu().numpy(), count=n, kept=kept)
            if hist:
                out["lo"], out["scale"] = check_sampler_arrays(smp, B, lo, hi)
                counts, nh = smp.histogram()
                assert nh == n
                out["hist"] = counts.cpu().numpy()
            return out
        finally:
            smp.close()

    plain = run(-1, False)
    mean = plain["s1"] / plain["count"]                               # the intended use: the range of a pixel from the moments of a run without a histogram
    std = np.sqrt(np.maximum(plain["s2"] / plain["count"] - mean * mean, 1e-6))
    lo, hi = (mean - 2 * std).astype(np.float32), (mean + 2 * std).astype(np.float32)
    inline, side = run(-1, True), run(1, True)
    assert inline["count"] > 0
    np.testing.assert_array_equal(side["hist"], inline["hist"])
    for r in (inline, side):
        np.testing.assert_array_equal(r["hist"].sum(0), np.full(shape, r["count"]))
        assert r["count"] == plain["count"]
        np.testing.assert_array_equal(r["x"], plain["x"])
        np.testing.assert_allclose(r["s1"], plain["s1"], **BM.TOL)
        np.testing.assert_allclose(r["s2"], plain["s2"], **BM.TOL)
    assert inline["hist"][1:-1].sum() > 0, "the range holds samples"
    if replay:
        one = run(-1, False, single=True)
        np.testing.assert_array_equal(one["x"], inline["x"])
        want = sum(numpy_counts(x, B, inline["lo"], inline["scale"]) for x in one["kept"])
        assert len(one["kept"]) * C_ == inline["count"]
        np.testing.assert_array_equal(inline["hist"], want)
        # injected noise (one iteration per launch whatever the policy), in line and on the side stream, against its own replay
        one = run(-1, False, single=True, injected=True)
        want = sum(numpy_counts(x, B, inline["lo"], inline["scale"]) for x in one["kept"])
        for overlap in (-1, 1):
            r = run(overlap, True, injected=True)
            np.testing.assert_array_equal(r["x"], one["x"])
            np.testing.assert_array_equal(r["hist"], want)


def test_mymala_counts_a_rejected_chain_again(la):
    """the construction of tests/test_gpu_block_moments.py::test_mymala_counts_a_rejected_chain_again_in_blocks_as_in_pixels"""
    shape, C_, nit, burn, B = (24, 96), 8, 16, 1, 32
    rng = np.random.default_rng(17)
    img = np.zeros(shape)
    img[6:12, 24:72] = 150.0
    img += np.linspace(0, 30, shape[1])[None, :]
    h = np.ones((5, 5)) / 25.0
    pf = la.L2(Op=la.Convolve2D(shape, h, offset=(2, 2)), b=img + rng.normal(0, BM.SIGMA, shape), sigma=1 / BM.SIGMA ** 2)
    pg = la.TV(shape, sigma=0.3, niter=5)
    x0 = np.broadcast_to(img.astype(np.float32), (C_,) + shape).copy()
    lo, hi = pixel_range(img, 1.0)
    kw = dict(n_chains=C_, tau=0.01 * GAMMA, gamma=GAMMA, seed=9)
    a = la.MYMALASampler(pf, pg, shape, moments=True, burn_in=burn, hist_bins=B, hist_range=(lo, hi), **kw)
    b = la.MYMALASampler(pf, pg, shape, **kw)
    try:
        lo32, sc32 = check_sampler_arrays(a, B, lo, hi)
        a.set_state(x0)
        b.set_state(x0)
        a.step(nit)
        stayed, prev = 0, x0
        want = np.zeros((B + 2,) + shape, dtype=np.int64)
        for it in range(nit):
            b.step(1)
            x = b.get_state().cpu().numpy()
            if it >= burn:
                stayed += int((x.reshape(C_, -1) == prev.reshape(C_, -1)).all(axis=1).sum())
                want += numpy_counts(x, B, lo32, sc32)
            prev = x
        np.testing.assert_array_equal(a.get_state().cpu().numpy(), prev)
        counts, n = a.histogram()
    finally:
        a.close()
        b.close()
    assert stayed > 0, "expected some rejections among the kept iterations at this step size"
    assert n == C_ * (nit - burn)
    np.testing.assert_array_equal(counts.cpu().numpy(), want)


def test_ulpda_histogram_matches_a_single_step_replay(la):
    shape, C_, nit, burn, thin, B = (16, 40), 5, 7, 1, 2, 62
    rng = np.random.default_rng(23)
    y, pf, _ = BM.blur_problem(la, shape, rng)
    lo, hi = pixel_range(y)
    x0 = (200.0 + rng.normal(0, 1.0, (C_,) + shape)).astype(np.float32)
    args = (pf, la.L21(sigma=0.3), la.Gradient(shape), shape)
    kw = dict(n_chains=C_, tau=0.95 * GAMMA, mu=1.0, theta=1.0, gfirst=False, seed=3)
    a = la.ULPDASampler(*args, moments=True, burn_in=burn, thin=thin, hist_bins=B, hist_range=(lo, hi), **kw)
    b = la.ULPDASampler(*args, **kw)
    try:
        lo32, sc32 = check_sampler_arrays(a, B, lo, hi)
        a.set_state(x0)
        b.set_state(x0)
        a.step(nit)
        want = np.zeros((B + 2,) + shape, dtype=np.int64)
        for it in range(nit):
            b.step(1)
            if it >= burn and (it - burn) % thin == 0:
                want += numpy_counts(b.get_state().cpu().numpy(), B, lo32, sc32)
        np.testing.assert_array_equal(a.get_state().cpu().numpy(), b.get_state().cpu().numpy())
        counts, n = a.histogram()
    finally:
        a.close()
        b.close()
    assert n == C_ * 3 and want[1:-1].sum() > 0
    np.testing.assert_array_equal(counts.cpu().numpy(), want)


def test_reset_and_refusals(la):
    import torch
    shape, B = (16, 32), 16
    rng = np.random.default_rng(41)
    y, pf, pg = BM.blur_problem(la, shape, rng)
    lo, hi = pixel_range(y, 4.0)
    lib = la._dev.lib()
    E_INVALID, E_STATE = -1, -5
    lo_d = torch.from_numpy(lo).cuda()
    sc_d = torch.from_numpy(np.float32(B) / (hi - lo)).cuda()

    def set_hist(smp, bins, lo_t=lo_d, sc_t=sc_d):
        return lib.lmc_sampler_set_histogram(smp._h, bins, la._dev.ptr(lo_t), la._dev.ptr(sc_t))

    def refused(rc, code):
        assert rc == code, (rc, code)
        assert lib.lmc_last_error(), "lmc_last_error() is empty"

    kw = dict(n_chains=3, tau=TAU, gamma=GAMMA, seed=1)
    smp = la.MYULASampler(pf, pg, shape, moments=True, **kw)
    off = la.MYULASampler(pf, pg, shape, **kw)
    try:
        smp.set_state(np.full(shape, 200.0, dtype=np.float32))
        refused(lib.lmc_sampler_get_histogram(smp._h, None, None, None), E_INVALID)        # get without set
        refused(lib.lmc_allreduce_histogram(smp._h, None, None, None, None), E_INVALID)
        with pytest.raises(ValueError):
            smp.histogram()
        refused(set_hist(smp, 63), E_INVALID)
        refused(set_hist(smp, -1), E_INVALID)
        refused(set_hist(smp, B, None, sc_d), E_INVALID)
        refused(set_hist(smp, B, lo_d, None), E_INVALID)
        refused(set_hist(off, B), E_STATE)                                                  # moments = 0
        assert set_hist(smp, B) == 0
        smp.hist_bins, smp.hist_lo, smp.hist_scale = B, lo_d, sc_d
        smp.step(2)
        counts, n = smp.histogram()
        assert n == 6
        np.testing.assert_array_equal(counts.sum(0).cpu().numpy(), np.full(shape, 6))
        refused(set_hist(smp, 8), E_STATE)                                                  # after a kept sample
        refused(set_hist(smp, 0), E_STATE)
        smp.reset_moments()
        counts, n = smp.histogram()
        assert n == 0 and int(counts.abs().sum()) == 0
        smp.step(1)
        counts, n = smp.histogram()
        assert n == 3
        want = numpy_counts(smp.get_state().cpu().numpy(), B, lo_d.cpu().numpy(), sc_d.cpu().numpy())
        np.testing.assert_array_equal(counts.cpu().numpy(), want)
        smp.reset_moments()
        assert set_hist(smp, 0, None, None) == 0                                            # off again
        refused(lib.lmc_sampler_get_histogram(smp._h, None, None, None), E_INVALID)
        smp.hist_bins = None
        smp.step(1)                                                                         # and the sampler goes on without one
        assert smp.moments()[2] == 3
    finally:
        smp.close()
        off.close()


def test_shards_sum_to_the_whole_and_the_one_rank_collective_is_a_copy(la):
    shape, B = (24, 136), 62
    rng = np.random.default_rng(31)
    y, pf, pg = BM.blur_problem(la, shape, rng)
    lo, hi = pixel_range(y)
    x0 = (200.0 + rng.normal(0, 1.0, (4,) + shape)).astype(np.float32)
    kw = dict(tau=TAU, gamma=GAMMA, seed=7, moments=True, burn_in=1, hist_bins=B, hist_range=(lo, hi))
    hists = []
    for off, n in ((0, 4), (0, 2), (2, 2)):
        smp = la.MYULASampler(pf, pg, shape, n_chains=n, chain_offset=off, **kw)
        try:
            smp.set_state(x0[off:off + n])
            smp.step(5)
            counts, cnt = smp.histogram()
            assert cnt == 4 * n
            for got, gcnt in (smp.allreduce_histogram(None), la.allreduce_sampler_histogram(smp)):      # NULL communicator / no process group
                assert gcnt == cnt
                np.testing.assert_array_equal(got.cpu().numpy(), counts.cpu().numpy())
            hists.append(counts.cpu().numpy())
        finally:
            smp.close()
    whole, first, second = hists
    assert whole[1:-1].sum() > 0
    np.testing.assert_array_equal(first + second, whole)


def test_entry_points_return_the_histogram_and_the_quantiles(la):
    shape = (32, 264)
    rng = np.random.default_rng(5)
    y, pf, pg = BM.blur_problem(la, shape, rng)
    lo, hi = pixel_range(y, 3.0)
    kw = dict(hist_bins=32, hist_range=(lo, hi), quantiles=(0.1, 0.9))

    def check(res, dims):
        assert tuple(res.hist.shape) == (34,) + dims and res.count > 0
        np.testing.assert_array_equal(res.hist.sum(0).cpu().numpy(), np.full(dims, res.count))
        assert sorted(res.quantiles) == [0.1, 0.9]
        want = la.hist_quantiles(res.hist, res.hist_lo, res.hist_scale, (0.1, 0.9))
        for i, q in enumerate((0.1, 0.9)):
            assert tuple(res.quantiles[q].shape) == dims
            np.testing.assert_array_equal(res.quantiles[q].cpu().numpy(), want[i].cpu().numpy())
        assert np.isfinite(res.quantiles[0.1].cpu().numpy()).any()

    res = la.MoreauYosidaUnadjustedLangevin(pf, pg, y.ravel(), tau=TAU, gamma=GAMMA, niter=6, seed=2, n_chains=5, burn_in=2, **kw)
    check(res, shape)
    np.testing.assert_array_equal(res.hist_lo.cpu().numpy(), lo)
    plain = la.MoreauYosidaUnadjustedLangevin(pf, pg, y.ravel(), tau=TAU, gamma=GAMMA, niter=2, seed=2, n_chains=2)
    assert plain.hist is None and plain.quantiles == {}
    out = la.sharded_myula(pf, pg, shape, 5, y, TAU, GAMMA, niter=6, seed=2, burn_in=2, hist_bins=32, hist_range=(lo, hi))
    assert len(out) == 5 and out.hist is out[4] and out.scales == {} and out.count == out[2] == res.count
    np.testing.assert_array_equal(out.hist.cpu().numpy(), res.hist.cpu().numpy())
    both = la.sharded_myula(pf, pg, shape, 5, y, TAU, GAMMA, niter=6, seed=2, burn_in=2, moment_scales=(4,), hist_bins=32, hist_range=(lo, hi))
    assert len(both) == 6 and both.scales is both[4] and sorted(both.scales) == [4] and both.hist is both[5]
    np.testing.assert_array_equal(both.hist.cpu().numpy(), res.hist.cpu().numpy())

    small = (16, 64)
    y2, pf2, pg2 = BM.blur_problem(la, small, rng)
    kw2 = dict(hist_bins=32, hist_range=pixel_range(y2, 3.0), quantiles=(0.1, 0.9))
    res = la.UnadjustedLangevinPrimalDual(pf2, la.L21(sigma=0.3), la.Gradient(small), y2.ravel(), 0.95 * GAMMA, 1.0, niter=5, seed=2, gfirst=False,
                                          n_chains=3, burn_in=1, **kw2)
    check(res, small)
    res = la.MoreauYosidaMetropolisAdjustedLangevin(pf2, pg2, y2.ravel(), tau=0.01 * GAMMA, gamma=GAMMA, niter=5, seed=2, n_chains=3, burn_in=1, **kw2)
    check(res, small)

"""All four optional accumulators of a sampler handle at once -- block moments, pixel histogram, chain-group moments, covariance sketch -- on every
sampler kind and through every driver: the path that one attach, one reduce, one reset and one epilogue form.

Shapes: a 20 x 27 image (rows of 27 floats are no multiple of 4, partial blocks at the scales 2 and 16, an odd width), 5 chains with chain_offset = 3 in
2 groups (unequal groups -- the global ids 3 .. 7 put 2 chains in group 0 and 3 in group 1 -- and the first chain not in group 0), scales (2, 16), 8 bins,
3 probes about a non-zero centre, burn_in = 1, thin = 2, 7 iterations: the iterations 1, 3 and 5 are kept, 15 samples.

Bounds, each the one its own file uses for "the sampler against the stateless pass over its kept states", none new:
  * histogram counters: equal bits (integers; tests/test_gpu_pixel_hist.py);
  * pixel and block moments: rtol 1e-12, atol 0 (tests/test_gpu_block_moments.py TOL: float64 atomics commute but arrive in any order);
  * chain-group moments: (n_g - 1) 2^-53 sum |term| per entry, n_g the samples of the group (tests/test_gpu_group_moments.py: the float64 summation
    bound for any order).  Here sum |term| is taken as |sum| of the sampler compared against, which is never larger, so the bound is never wider;
  * covariance sketch: equal bits (tests/test_gpu_cov_sketch.py: one owner per element, ordered launches)."""
import functools

import numpy as np
import pytest

from tests import test_gpu_block_moments as BM
from tests import test_gpu_group_moments as GM

pytestmark = pytest.mark.gpu

SHAPE, C_, OFFSET = (20, 27), 5, 3
BURN, THIN, NIT = 1, 2, 7
KEPT = 3                                  # the iterations 1, 3, 5
GROUP_COUNTS = [2 * KEPT, 3 * KEPT]       # the global chain ids 3 .. 7 mod 2
KINDS = ["myula", "mymala", "skrock", "ulpda"]
# The data are 100 + noise under a zero-padded 5 x 5 box blur, which sees as little as 9 / 25 of the neighbourhood of a corner pixel: the posterior pulls the
# border towards 100 * 25 / 9 = 278, so [0, 400) holds every sample and no quantile is infinite; the start, 100 + N(0, 1), straddles the bin edge at 100.
HIST_RANGE = (0.0, 400.0)

la = BM.la


def accumulator_keywords():
    rng = np.random.default_rng(11)
    P = rng.standard_normal((3,) + SHAPE).astype(np.float32)
    m = (100.0 + rng.normal(0, 0.5, SHAPE)).astype(np.float32)
    return {"scales": dict(moment_scales=(2, 16)), "hist": dict(hist_bins=8, hist_range=HIST_RANGE), "groups": dict(chain_groups=2),
            "cov": dict(cov_probes=P, cov_center=m)}


def problem(la, kind):
    """-> (proxf, proxg, x0 [C, H, W] fp32): blur 5 x 5 + TV(niter=10); for ULPDA blur (a cold implicit solve, so that a pass can be repeated) + L21"""
    rng = np.random.default_rng(7)
    y, pf, pg = BM.blur_problem(la, SHAPE, rng, "tv", level=100.0)
    if kind == "ulpda":
        pf = la.L2(Op=la.Convolve2D(SHAPE, np.ones((5, 5)) / 25.0, offset=(2, 2)), b=y, sigma=1 / BM.SIGMA ** 2, warm=False)
        pg = la.L21(sigma=0.3)
    return pf, pg, (100.0 + rng.normal(0, 1.0, (C_,) + SHAPE)).astype(np.float32)


def make_sampler(la, kind, pf, pg, **kw):
    common = dict(n_chains=C_, chain_offset=OFFSET, moments=True, burn_in=BURN, thin=THIN, **kw)
    if kind == "myula":
        return la.MYULASampler(pf, pg, SHAPE, tau=BM.TAU, gamma=BM.GAMMA, seed=5, **common)
    if kind == "mymala":
        return la.MYMALASampler(pf, pg, SHAPE, tau=0.0003 * BM.GAMMA, gamma=BM.GAMMA, seed=9, **common)
    if kind == "skrock":
        return la.SKROCKSampler(pf, pg, SHAPE, n_stages=3, tau=BM.TAU, gamma=BM.GAMMA, seed=5, **common)
    return la.ULPDASampler(pf, pg, la.Gradient(SHAPE), SHAPE, tau=0.95 * BM.GAMMA, mu=1.0, theta=1.0, gfirst=False, seed=3, **common)


def start(smp, kind, x0):
    smp.iteration = 0
    smp.set_state(x0)
    if kind == "ulpda":
        smp.set_dual(np.zeros(2 * SHAPE[0] * SHAPE[1], dtype=np.float32))


def snapshot(smp):
    """every accumulator the sampler keeps, as host arrays by name, with the final state"""
    out = BM.accumulators(smp)
    out["state"] = smp.get_state().cpu().numpy()
    if smp.hist_bins is not None:
        counts, n = smp.histogram()
        assert n == out["count"]
        out["hist"] = counts.cpu().numpy()
    if smp.chain_groups is not None:
        G1, G2, gn = smp.group_moments()
        out["G1"], out["G2"], out["group_counts"] = G1.cpu().numpy(), G2.cpu().numpy(), gn.tolist()
    if smp.cov_k is not None:
        Y, s, Q, n = smp.cov_sketch()
        assert n == out["count"]
        out["Y"], out["s"], out["Q"] = (t.cpu().numpy() for t in (Y, s, Q))
    return out


def assert_same(got, want, tag):
    """every accumulator of `want` is in `got`, within the bound of its kind (module docstring); the trajectories are the same"""
    np.testing.assert_array_equal(got["state"], want["state"], err_msg=f"{tag} final state")
    assert got["count"] == want["count"] == KEPT * C_, (tag, got["count"], want["count"])
    for key, w in want.items():
        g = got[key]
        if key in ("hist", "Y", "s", "Q"):
            np.testing.assert_array_equal(g, w, err_msg=f"{tag} {key}")
        elif key == "group_counts":
            assert g == w == GROUP_COUNTS, (tag, g, w)
        elif key in ("G1", "G2"):
            terms = (np.asarray(want["group_counts"], dtype=np.float64) - 1).reshape(-1, 1, 1)
            tol = terms * GM.U * np.abs(w)
            err = np.abs(g - w)
            print(f"{tag} {key}: worst error / tolerance {float((err / tol).max()):.3g}")
            assert (err <= tol).all(), (tag, key, float((err - tol).max()))
        elif key not in ("state", "count"):
            assert np.abs(w).max() > 0, (tag, key)
            print(f"{tag} {key}: worst relative difference {float((np.abs(g - w) / np.abs(w)).max()):.3g}")
            np.testing.assert_allclose(g, w, err_msg=f"{tag} {key}", **BM.TOL)


@functools.lru_cache(maxsize=None)
def passes(kind):
    """-> (first pass of the sampler with all four, its second pass after reset_moments(), {name: the sampler with that accumulator alone})"""
    import lmc_atomi_amd as la
    pf, pg, x0 = problem(la, kind)
    kws = accumulator_keywords()
    smp = make_sampler(la, kind, pf, pg, **{k: v for kw in kws.values() for k, v in kw.items()})
    try:
        assert smp.moment_scales == (2, 16) and smp.hist_bins == 8 and smp.chain_groups == 2 and smp.cov_k == 3
        start(smp, kind, x0)
        smp.step(NIT)
        first = snapshot(smp)
        smp.reset_moments()
        empty = snapshot(smp)
        assert empty["count"] == 0 and empty["group_counts"] == [0, 0]
        for key, v in empty.items():
            if key not in ("state", "count", "group_counts"):
                assert not np.asarray(v).any(), (kind, key, "not zero after reset_moments()")
        start(smp, kind, x0)
        smp.step(NIT)
        second = snapshot(smp)
    finally:
        smp.close()
    alone = {}
    for name, kw in kws.items():
        solo = make_sampler(la, kind, pf, pg, **kw)
        try:
            start(solo, kind, x0)
            solo.step(NIT)
            alone[name] = snapshot(solo)
        finally:
            solo.close()
    return first, second, alone


@pytest.mark.parametrize("kind", KINDS)
def test_all_four_together_equal_each_one_alone(la, kind):
    first, _, alone = passes(kind)
    assert sorted(first) == sorted(["state", "count", "s1", "s2", "S1_2", "S2_2", "S1_16", "S2_16", "hist", "G1", "G2", "group_counts", "Y", "s", "Q"])
    assert first["hist"].sum(axis=0).tolist() == np.full(SHAPE, KEPT * C_).tolist()
    for name, want in alone.items():
        assert len(want) > 4, (name, sorted(want))          # state, count, s1, s2 and its own accumulator
        assert_same(first, want, f"{kind}: all four against {name} alone")


@pytest.mark.parametrize("kind", KINDS)
def test_a_second_pass_after_reset_equals_the_first(la, kind):
    first, second, _ = passes(kind)
    assert_same(second, first, f"{kind}: the pass after reset_moments() against the first")


@pytest.mark.parametrize("kind", KINDS)
def test_every_driver_returns_all_four_summaries(la, kind):
    import torch
    pf, pg, x0 = problem(la, kind)
    kw = {k: v for kws in accumulator_keywords().values() for k, v in kws.items()}
    kw.update(niter=NIT, n_chains=C_, dims=SHAPE, chain_offset=OFFSET, burn_in=BURN, thin=THIN)
    if kind == "myula":
        res = la.MoreauYosidaUnadjustedLangevin(pf, pg, x0, tau=BM.TAU, gamma=BM.GAMMA, seed=5, **kw)
    elif kind == "mymala":
        res = la.MoreauYosidaMetropolisAdjustedLangevin(pf, pg, x0, tau=0.0003 * BM.GAMMA, gamma=BM.GAMMA, seed=9, **kw)
        assert tuple(res.accepted.shape) == (C_,) and tuple(res.acceptance_rate.shape) == (C_,)
    elif kind == "skrock":
        res = la.StabilisedLangevin(pf, pg, x0, BM.TAU, gamma=BM.GAMMA, n_stages=3, seed=5, **kw)
        assert res.n_stages == 3 and res.gradient_evaluations == 3 * NIT
    else:
        res = la.UnadjustedLangevinPrimalDual(pf, pg, la.Gradient(SHAPE), x0, 0.95 * BM.GAMMA, 1.0, gfirst=False, seed=3, **kw)
    assert isinstance(res, la.MYULAResult)
    assert res.count == KEPT * C_ and tuple(res.state.shape) == (C_,) + SHAPE
    finite = lambda t: bool(torch.isfinite(torch.as_tensor(t)).all())
    assert finite(res.mean) and finite(res.var)
    assert sorted(res.scale_mean) == sorted(res.scale_std) == [2, 16]
    for s, blocks in ((2, (10, 14)), (16, (2, 2))):
        assert tuple(res.scale_mean[s].shape) == blocks and finite(res.scale_mean[s]) and finite(res.scale_std[s])
    assert tuple(res.hist.shape) == (10,) + SHAPE and sorted(res.quantiles) == [0.05, 0.5, 0.95]
    for q, v in res.quantiles.items():
        assert tuple(v.shape) == SHAPE and finite(v), q
    assert tuple(res.mcse_mean.shape) == SHAPE and finite(res.mcse_mean) and finite(res.mcse_var)
    assert res.group_counts.tolist() == GROUP_COUNTS
    sk = res.cov_sketch
    assert sk is not None and sk.n == KEPT * C_ and sk.cov_xt.shape == (3,) + SHAPE and sk.cov_tt.shape == (3, 3)
    assert np.isfinite(sk.cov_xt).all() and np.isfinite(sk.cov_tt).all() and np.isfinite(sk.t_mean).all()
    assert np.abs(sk.cov_xt).max() > 0 and (np.diag(sk.cov_tt) > 0).all()

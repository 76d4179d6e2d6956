"""Multi-scale posterior moments (lmc_sampler_set_moment_scales / lmc_sampler_get_block_moments / lmc_allreduce_block_moments): for every enabled
scale s out of 2, 4, 8, 16 the sums over the kept samples of b and b^2, b = the sum of one chain's sample over an s x s block (edge blocks partial).

The reference is numpy float64 on the fp32 states of every kept iteration (get_state() after step(1)), block sums by np.add.reduceat.  Tolerance on
every accumulator: rtol 1e-12, atol 0 -- the figure of tests/test_gpu_overlap.py for float64 atomics that commute but arrive in any order.  The
reference's own error is far below it: a block sum has at most 256 terms and an accumulator at most 37 chains x 7 kept iterations, each
addition within 1.1e-16 relative of terms of one sign, so below 1e-13 in all."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SCALES = (2, 4, 8, 16)
TOL = dict(rtol=1e-12, atol=0)
SIGMA = 0.75
GAMMA, TAU = SIGMA ** 2, 0.2 * SIGMA ** 2


@pytest.fixture(scope="module")
def la():
    import torch
    assert torch.cuda.is_available()
    import lmc_atomi_amd as la
    return la


def block_sums(X, s):
    """[..., H, W] -> [..., ceil(H/s), ceil(W/s)]: sums over s x s blocks, partial at the bottom and right edges"""
    H, W = X.shape[-2:]
    return np.add.reduceat(np.add.reduceat(X, np.arange(0, H, s), axis=-2), np.arange(0, W, s), axis=-1)


class Reference:
    def __init__(self, shape):
        self.s1, self.s2, self.count = np.zeros(shape), np.zeros(shape), 0
        self.S1 = {s: 0.0 for s in SCALES}
        self.S2 = {s: 0.0 for s in SCALES}

    def keep(self, x):
        x = np.asarray(x)
        assert x.dtype == np.float32
        x = x.astype(np.float64)
        self.s1 += x.sum(0)
        self.s2 += (x * x).sum(0)
        self.count += x.shape[0]
        for s in SCALES:
            b = block_sums(x, s)
            self.S1[s] = self.S1[s] + b.sum(0)
            self.S2[s] = self.S2[s] + (b * b).sum(0)


def accumulators(smp):
    s1, s2, n = smp.moments()
    out = {"s1": s1.cpu().numpy(), "s2": s2.cpu().numpy(), "count": n}
    for s in smp.moment_scales:
        S1, S2, nb = smp.block_moments(s)
        assert nb == n
        out[f"S1_{s}"], out[f"S2_{s}"] = S1.cpu().numpy(), S2.cpu().numpy()
    return out


def check_against(acc, ref, tag=""):
    assert acc["count"] == ref.count and ref.count > 0, (tag, acc["count"], ref.count)
    np.testing.assert_allclose(acc["s1"], ref.s1, err_msg=f"{tag} s1", **TOL)
    np.testing.assert_allclose(acc["s2"], ref.s2, err_msg=f"{tag} s2", **TOL)
    for s in SCALES:
        assert acc[f"S2_{s}"].shape == ref.S2[s].shape, (tag, s)
        np.testing.assert_allclose(acc[f"S2_{s}"], ref.S2[s], err_msg=f"{tag} S2 scale {s}", **TOL)
        np.testing.assert_allclose(acc[f"S1_{s}"], ref.S1[s], err_msg=f"{tag} S1 scale {s}", **TOL)
        np.testing.assert_allclose(acc[f"S1_{s}"], block_sums(acc["s1"], s), err_msg=f"{tag} S1 scale {s} vs the block sum of s1", **TOL)


def blur_problem(la, shape, rng, prior="tv", level=200.0):
    y = level + rng.normal(0, 1.0, shape)
    h = np.ones((5, 5)) / 25.0
    pf = la.L2(Op=la.Convolve2D(shape, h, offset=(2, 2)), b=y, sigma=1 / SIGMA ** 2)
    pg = la.TV(shape, sigma=0.3, niter=10) if prior == "tv" else la.L2(sigma=0.05)
    return y, pf, pg


def mask_haar_problem(la, shape, rng, level=200.0):
    mask = (rng.uniform(size=shape) < 0.6).astype(np.float64)
    y = mask * (level + rng.normal(0, 1.0, shape))
    pf = la.L2(Op=la.Diagonal(mask, dims=shape), b=y, sigma=1 / SIGMA ** 2, dims=shape)
    return y, pf, la.WaveletL1(shape, sigma=2.0)


# (16, 64): exactly one tile row of the fused kernel; (32, 264): the pipe step kernel, partial last column of 16-blocks; (19, 203): W % 4 != 0, the generic
# kernel, partial blocks on both edges; (9, 7): smaller than one 16-block; (33, 520): several tiles and one extra row.  3 and 37 chains: the tails of the
# unrolled chain loops, and more than one chain segment.
@pytest.mark.parametrize("C_", [3, 37])
@pytest.mark.parametrize("shape", [(16, 64), (32, 264), (19, 203), (9, 7), (33, 520)])
def test_block_moments_match_the_float64_reference(la, shape, C_):
    """States near 200 with a spread near 1: a block sum formed in fp32 would miss the tolerance on S2."""
    rng = np.random.default_rng(shape[1] + C_)
    y, pf, pg = blur_problem(la, shape, rng)
    x0 = (200.0 + rng.normal(0, 1.0, (C_,) + shape)).astype(np.float32)
    noise = rng.standard_normal((4, C_) + shape).astype(np.float32)
    kw = dict(n_chains=C_, tau=TAU, gamma=GAMMA, noise="injected", moments=True)
    smp = la.MYULASampler(pf, pg, shape, moment_scales=SCALES, **kw)
    plain = la.MYULASampler(pf, pg, shape, **kw)
    ref = Reference(shape)
    try:
        assert smp.moment_scales == SCALES and plain.moment_scales == ()
        smp.set_state(x0)
        plain.set_state(x0)
        for k in range(4):
            smp.step(1, noise=noise[k:k + 1])
            plain.step(1, noise=noise[k:k + 1])
            ref.keep(smp.get_state().cpu().numpy())
        acc = accumulators(smp)
        p1, p2, pn = plain.moments()
        np.testing.assert_array_equal(smp.get_state().cpu().numpy(), plain.get_state().cpu().numpy())
    finally:
        smp.close()
        plain.close()
    assert abs(ref.s1.mean() / ref.count - 200.0) < 20.0          # the regime the test is about: a mean two orders above the spread
    check_against(acc, ref, f"{shape} x {C_}")
    assert pn == acc["count"]
    np.testing.assert_allclose(acc["s1"], p1.cpu().numpy(), err_msg="s1 vs a sampler without scales", **TOL)
    np.testing.assert_allclose(acc["s2"], p2.cpu().numpy(), err_msg="s2 vs a sampler without scales", **TOL)


GROUPINGS = {
    # tag: (shape, chains, problem, policy, kernel the sampler must report, replayable by step(1))
    "pipe": ((48, 264), 5, "blur_tv", None, "pipe", True),
    "rows": ((40, 64), 7, "blur_l2", None, "rows", True),
    # two iterations per launch on the rows kernel: its windows start at band boundaries, so its states equal those of single launches to fp32
    # rounding only (tests/test_gpu_rows_pair.py) and a kept iterate in between cannot be read back -- no step(1) replay reproduces them bit for bit.
    # This configuration is checked across the policies and against itself; "rows" above is the same problem with the replay.
    "rows_pair": ((40, 64), 7, "blur_l2", {"iterations_per_launch": 2}, "rows_pair", False),
    "block_pair": ((64, 64), 4, "mask_haar", None, "block", True),     # bit-identical to single launches (tests/test_gpu_block_pair.py)
    "tile": ((9, 7), 3, "blur_tv", None, "", True),
}


@pytest.mark.parametrize("burn,thin", [(2, 2), (1, 5)])
@pytest.mark.parametrize("tag", sorted(GROUPINGS))
def test_block_moments_over_every_launch_grouping(la, tag, burn, thin, monkeypatch):
    """step(4); step(1); step(9) with the reductions in line, and on the side stream with 1, 3 and the full-speed number of workgroups: bit-identical
    states, equal counts, accumulators equal to 1e-12 and equal to the reference built from a step(1) replay of the same seed."""
    shape, C_, problem, policy, kernel, replay = GROUPINGS[tag]
    rng = np.random.default_rng(11)
    if problem == "mask_haar":
        y, pf, pg = mask_haar_problem(la, shape, rng)
    else:
        y, pf, pg = blur_problem(la, shape, rng, "tv" if problem == "blur_tv" else "l2")
    x0 = (200.0 + rng.normal(0, 1.0, (C_,) + shape)).astype(np.float32)
    kw = dict(n_chains=C_, tau=TAU, gamma=GAMMA, seed=5, policy=policy)
    ref, final = None, None
    if replay:
        ref = Reference(shape)
        one = la.MYULASampler(pf, pg, shape, **kw)
        one.set_state(x0)
        for it in range(14):
            one.step(1)
            if it >= burn and (it - burn) % thin == 0:
                ref.keep(one.get_state().cpu().numpy())
        final = one.get_state().cpu().numpy()
        one.close()
    runs = []
    for overlap, wgs in (("0", "128"), ("1", "1"), ("1", "3"), ("1", "0")):
        monkeypatch.setenv("LMC_MOMENTS_OVERLAP", overlap)      # read once, when the sampler is created
        monkeypatch.setenv("LMC_MOMENTS_BG_WGS", wgs)
        smp = la.MYULASampler(pf, pg, shape, moments=True, burn_in=burn, thin=thin, moment_scales=SCALES, **kw)
        try:
            smp.set_state(x0)
            smp.step(4)
            name = smp.kernel_name
            smp.step(1)
            smp.step(9)
            runs.append((accumulators(smp), smp.get_state().cpu().numpy(), name))
        finally:
            smp.close()
    acc0, x_ref, name = runs[0]
    assert kernel in name, name
    assert acc0["count"] > 0
    if replay:
        np.testing.assert_array_equal(x_ref, final)
        check_against(acc0, ref, f"{tag} in line")
    for acc, x, _ in runs[1:]:
        np.testing.assert_array_equal(x, x_ref)
        assert acc["count"] == acc0["count"]
        for k in acc0:
            if k != "count":
                np.testing.assert_allclose(acc[k], acc0[k], err_msg=f"{tag} {k}", **TOL)
        if replay:
            check_against(acc, ref, f"{tag} side stream")
        else:
            for s in SCALES:
                np.testing.assert_allclose(acc[f"S1_{s}"], block_sums(acc["s1"], s), err_msg=f"{tag} S1 scale {s}", **TOL)


def test_mymala_counts_a_rejected_chain_again_in_blocks_as_in_pixels(la):
    shape, C_, nit, burn = (24, 96), 8, 16, 1
    rng = np.random.default_rng(17)
    img = np.zeros(shape)
    img[6:12, 24:72] = 150.0
    img += np.linspace(0, 30, shape[1])[None, :]
    h = np.ones((5, 5)) / 25.0
    pf = la.L2(Op=la.Convolve2D(shape, h, offset=(2, 2)), b=img + rng.normal(0, SIGMA, shape), sigma=1 / SIGMA ** 2)
    pg = la.TV(shape, sigma=0.3, niter=5)
    x0 = np.broadcast_to(img.astype(np.float32), (C_,) + shape).copy()      # from the image itself, as that run: from a start far off every early proposal is downhill and accepted
    kw = dict(n_chains=C_, tau=0.01 * GAMMA, gamma=GAMMA, seed=9)      # the step size of tests/test_gpu_mymala.py's Philox run: acceptance strictly between 0 and 1
    a = la.MYMALASampler(pf, pg, shape, moments=True, burn_in=burn, moment_scales=SCALES, **kw)
    b = la.MYMALASampler(pf, pg, shape, **kw)
    ref = Reference(shape)
    try:
        a.set_state(x0)
        b.set_state(x0)
        a.step(nit)
        stayed = 0
        prev = x0
        for it in range(nit):
            b.step(1)
            x = b.get_state().cpu().numpy()
            if it >= burn:
                stayed += int((x.reshape(C_, -1) == prev.reshape(C_, -1)).all(axis=1).sum())
                ref.keep(x)
            prev = x
        np.testing.assert_array_equal(a.get_state().cpu().numpy(), prev)
        acc = accumulators(a)
    finally:
        a.close()
        b.close()
    assert stayed > 0, "expected some rejections among the kept iterations at this step size"
    check_against(acc, ref, "mymala")


def test_ulpda_block_moments_match_a_single_step_replay(la):
    shape, C_, nit, burn, thin = (16, 40), 5, 7, 1, 2
    rng = np.random.default_rng(23)
    y, pf, _ = blur_problem(la, shape, rng)
    x0 = (200.0 + rng.normal(0, 1.0, (C_,) + shape)).astype(np.float32)
    args = (pf, la.L21(sigma=0.3), la.Gradient(shape), shape)
    kw = dict(n_chains=C_, tau=0.95 * GAMMA, mu=1.0, theta=1.0, gfirst=False, seed=3)
    a = la.ULPDASampler(*args, moments=True, burn_in=burn, thin=thin, moment_scales=SCALES, **kw)
    b = la.ULPDASampler(*args, **kw)
    ref = Reference(shape)
    try:
        a.set_state(x0)
        b.set_state(x0)
        a.step(nit)
        for it in range(nit):
            b.step(1)
            if it >= burn and (it - burn) % thin == 0:
                ref.keep(b.get_state().cpu().numpy())
        np.testing.assert_array_equal(a.get_state().cpu().numpy(), b.get_state().cpu().numpy())
        acc = accumulators(a)
    finally:
        a.close()
        b.close()
    check_against(acc, ref, "ulpda")


def test_shards_sum_to_the_whole_and_the_one_rank_collective_is_a_copy(la):
    shape = (24, 136)
    rng = np.random.default_rng(31)
    y, pf, pg = blur_problem(la, shape, rng)
    x0 = (200.0 + rng.normal(0, 1.0, (4,) + shape)).astype(np.float32)
    kw = dict(tau=TAU, gamma=GAMMA, seed=7, moments=True, burn_in=1, moment_scales=SCALES)
    accs = []
    for off, n in ((0, 4), (0, 2), (2, 2)):
        smp = la.MYULASampler(pf, pg, shape, n_chains=n, chain_offset=off, **kw)
        try:
            smp.set_state(x0[off:off + n])
            smp.step(5)
            acc = accumulators(smp)
            for s in SCALES:      # NULL communicator: a job of one rank returns the sampler's own accumulators
                S1, S2, cnt = smp.allreduce_block_moments(None, s)
                assert cnt == acc["count"]
                np.testing.assert_array_equal(S1.cpu().numpy(), acc[f"S1_{s}"])
                np.testing.assert_array_equal(S2.cpu().numpy(), acc[f"S2_{s}"])
                T1, T2, cnt = la.allreduce_sampler_block_moments(smp, s)
                assert cnt == acc["count"]
                np.testing.assert_array_equal(T2.cpu().numpy(), acc[f"S2_{s}"])
            accs.append(acc)
        finally:
            smp.close()
    whole, lo, hi = accs
    assert whole["count"] == lo["count"] + hi["count"] == 4 * 4
    for k in whole:
        if k != "count":
            np.testing.assert_allclose(lo[k] + hi[k], whole[k], err_msg=k, **TOL)


def test_reset_and_refusals(la):
    shape = (16, 32)
    rng = np.random.default_rng(41)
    y, pf, pg = blur_problem(la, shape, rng)
    lib = la._dev.lib()
    E_INVALID, E_STATE = -1, -5

    def set_scales(smp, scales):
        return lib.lmc_sampler_set_moment_scales(smp._h, len(scales), (C.c_int32 * max(len(scales), 1))(*scales))

    def refused(rc, code):
        assert rc == code, (rc, code)
        assert lib.lmc_last_error(), "lmc_last_error() is empty"

    smp = la.MYULASampler(pf, pg, shape, n_chains=3, tau=TAU, gamma=GAMMA, seed=1, moments=True, moment_scales=(4, 16))
    off = la.MYULASampler(pf, pg, shape, n_chains=3, tau=TAU, gamma=GAMMA, seed=1)
    try:
        smp.set_state(np.full(shape, 200.0, dtype=np.float32))
        for bad in ((3,), (32,), (2, 2), (2, 4, 8, 16, 2)):
            refused(set_scales(smp, bad), E_INVALID)
        refused(set_scales(off, (2, 4)), E_STATE)                # moments = 0
        smp.step(2)
        S1, S2, n = smp.block_moments(4)
        assert n == 6 and float(S2.abs().sum()) > 0 and S2.shape == (4, 8)
        refused(set_scales(smp, (2,)), E_STATE)                   # after a kept iterate
        for scale in (2, 8, 3, 0):                                # not enabled / not a scale
            refused(lib.lmc_sampler_get_block_moments(smp._h, scale, None, None, None, None), E_INVALID)
            refused(lib.lmc_allreduce_block_moments(smp._h, None, scale, None, None, None, None), E_INVALID)
        with pytest.raises(la.LMCError):
            smp.block_moments(2)
        smp.reset_moments()
        for s in (4, 16):
            S1, S2, n = smp.block_moments(s)
            assert n == 0 and float(S1.abs().sum()) == 0.0 and float(S2.abs().sum()) == 0.0
        assert set_scales(smp, (2, 8)) == 0                       # empty accumulators: the scales may change
        smp.moment_scales = (2, 8)
        smp.step(1)
        ref = Reference(shape)
        ref.keep(smp.get_state().cpu().numpy())
        for s in (2, 8):
            S1, S2, n = smp.block_moments(s)
            assert n == 3
            np.testing.assert_allclose(S2.cpu().numpy(), ref.S2[s], **TOL)
        refused(lib.lmc_sampler_get_block_moments(smp._h, 4, None, None, None, None), E_INVALID)
        smp.reset_moments()
        assert set_scales(smp, ()) == 0                           # off again
        refused(lib.lmc_sampler_get_block_moments(smp._h, 2, None, None, None, None), E_INVALID)
    finally:
        smp.close()
        off.close()


def test_entry_points_return_the_scale_summaries(la):
    shape = (20, 44)
    rng = np.random.default_rng(5)
    y, pf, pg = blur_problem(la, shape, rng)
    res = la.MoreauYosidaUnadjustedLangevin(pf, pg, y.ravel(), tau=TAU, gamma=GAMMA, niter=6, seed=2, n_chains=4, burn_in=2, moment_scales=(4, 16))
    assert sorted(res.scale_mean) == sorted(res.scale_std) == [4, 16]
    mean = res.mean.cpu().numpy()
    for s in (4, 16):
        npix = block_sums(np.ones(shape), s)
        assert res.scale_mean[s].shape == npix.shape
        np.testing.assert_allclose(res.scale_mean[s].cpu().numpy(), block_sums(mean, s) / npix, rtol=1e-10)
        std = res.scale_std[s].cpu().numpy()
        assert np.isfinite(std).all() and (std > 0).all()
    plain = la.MoreauYosidaUnadjustedLangevin(pf, pg, y.ravel(), tau=TAU, gamma=GAMMA, niter=2, seed=2, n_chains=2)
    assert plain.scale_mean == {} and plain.scale_std == {}
    out = la.sharded_myula(pf, pg, shape, 4, y, TAU, GAMMA, niter=6, seed=2, burn_in=2, moment_scales=(4, 16))
    assert len(out) == 5
    for s in (4, 16):
        np.testing.assert_allclose(out[4][s][0].cpu().numpy(), res.scale_mean[s].cpu().numpy(), rtol=1e-10)
        np.testing.assert_allclose(out[4][s][1].cpu().numpy(), res.scale_std[s].cpu().numpy(), rtol=1e-6)

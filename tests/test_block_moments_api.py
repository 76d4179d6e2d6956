"""CPU only: the host arithmetic of the multi-scale moments -- block_mean_var (mean and variance of a block MEAN from the block-sum accumulators, every
block divided by its own pixel count) -- and the argument checks that come before any device call."""
import numpy as np
import pytest


def direct(samples, s):
    """samples [N, H, W] -> mean and variance over N of the mean of every s x s block (partial at the edges), block by block"""
    N, H, W = samples.shape
    bh, bw = -(-H // s), -(-W // s)
    mean, var = np.zeros((bh, bw)), np.zeros((bh, bw))
    for i in range(bh):
        for j in range(bw):
            m = samples[:, i * s:(i + 1) * s, j * s:(j + 1) * s].reshape(N, -1).mean(axis=1)
            mean[i, j], var[i, j] = m.mean(), m.var()
    return mean, var


@pytest.mark.parametrize("shape", [(16, 32), (19, 203), (9, 7), (33, 40)])
@pytest.mark.parametrize("scale", [2, 4, 8, 16])
def test_block_mean_var_divides_by_each_blocks_own_pixel_count(shape, scale):
    from lmc_atomi_amd import block_mean_var
    rng = np.random.default_rng(shape[1] + scale)
    x = 200.0 + rng.normal(0, 1.0, (12,) + shape)
    H, W = shape
    b = np.add.reduceat(np.add.reduceat(x, np.arange(0, H, scale), axis=1), np.arange(0, W, scale), axis=2)
    mean, var = block_mean_var(b.sum(0), (b * b).sum(0), x.shape[0], scale, shape)
    ref_mean, ref_var = direct(x, scale)
    assert mean.shape == ref_mean.shape == (-(-H // scale), -(-W // scale))
    np.testing.assert_allclose(mean, ref_mean, rtol=1e-13)
    # var = E b^2 - (E b)^2 cancels about (200 / spread of a block mean)^2 of the 1.1e-16 precision
    np.testing.assert_allclose(var, ref_var, rtol=0, atol=200.0 ** 2 * 1e-14)


def test_block_mean_var_takes_torch_tensors():
    import torch
    from lmc_atomi_amd import block_mean_var
    rng = np.random.default_rng(0)
    x = rng.normal(5.0, 1.0, (6, 9, 7))
    b = np.add.reduceat(np.add.reduceat(x, np.arange(0, 9, 4), axis=1), np.arange(0, 7, 4), axis=2)
    m_np, v_np = block_mean_var(b.sum(0), (b * b).sum(0), 6, 4, (9, 7))
    m_t, v_t = block_mean_var(torch.from_numpy(b.sum(0)), torch.from_numpy((b * b).sum(0)), 6, 4, (9, 7))
    assert isinstance(m_t, torch.Tensor) and m_t.dtype == torch.float64
    np.testing.assert_allclose(m_t.numpy(), m_np, rtol=1e-15)
    np.testing.assert_allclose(v_t.numpy(), v_np, rtol=1e-12, atol=1e-15)


class _NoDevice:
    """stands where a prox would: a sampler that reached it has gone past the argument checks"""
    def __getattr__(self, name):
        raise AssertionError("the argument check must come before anything else")


@pytest.mark.parametrize("cls", ["MYULASampler", "MYMALASampler", "ULPDASampler"])
def test_moment_scales_without_moments_raise_before_any_device_call(cls):
    import lmc_atomi_amd as la
    args = (_NoDevice(), _NoDevice(), (16, 16)) if cls != "ULPDASampler" else (_NoDevice(), _NoDevice(), _NoDevice(), (16, 16))
    with pytest.raises(ValueError, match="moments=True"):
        getattr(la, cls)(*args, n_chains=2, tau=0.1, moments=False, moment_scales=(2, 4))
    for bad in ((3,), (32,), (2, 2)):
        with pytest.raises(ValueError, match="moment_scales"):
            getattr(la, cls)(*args, n_chains=2, tau=0.1, moments=True, moment_scales=bad)


def test_entry_points_refuse_moment_scales_in_the_reference_form():
    import lmc_atomi_amd as la
    with pytest.raises(ValueError, match="moment_scales"):
        la.MoreauYosidaUnadjustedLangevin(_NoDevice(), _NoDevice(), np.zeros(64), tau=0.1, gamma=0.5, niter=2, dims=(8, 8), moment_scales=(2,))

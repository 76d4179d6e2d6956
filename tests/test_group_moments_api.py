"""CPU only: the host arithmetic of the chain-group moments -- mcse_from_group_moments against a loop-by-loop restatement of its definition
(include/lmc_atomi.h, lmc_sampler_set_chain_groups), its container rule and refusals, its statistical validity on a process with a known answer --
and the argument checks of the samplers and entry points, which must raise before any device call."""
import numpy as np
import pytest


def group_sums(x, G, chain_offset=0, dtype=np.float64):
    """[C, H, W] (or [T, C, H, W]) samples -> (S1, S2 [G, H, W], counts [G]) with group = (chain_offset + c) mod G, summed in ``dtype``"""
    x = np.asarray(x)
    if x.ndim == 3:
        x = x[None]
    xs = x.astype(dtype)
    S1 = np.zeros((G,) + x.shape[2:], dtype=dtype)
    S2 = np.zeros_like(S1)
    counts = np.zeros(G, dtype=np.int64)
    for c in range(x.shape[1]):
        g = (chain_offset + c) % G
        S1[g] += xs[:, c].sum(axis=0)
        S2[g] += (xs[:, c] * xs[:, c]).sum(axis=0)
        counts[g] += x.shape[0]
    return S1, S2, counts


def definition(S1, S2, n):
    """the definition, pixel by pixel and group by group, in Python floats (float64)"""
    G = len(n)
    out = {k: np.empty(S1.shape[1:]) for k in ("mean", "var", "mcse_mean", "mcse_var", "ess")}
    for p in np.ndindex(*S1.shape[1:]):
        N = float(sum(int(v) for v in n))
        A = [float(S1[(g,) + p]) for g in range(G)]
        B = [float(S2[(g,) + p]) for g in range(G)]
        mg = [A[g] / n[g] for g in range(G)]
        vg = [B[g] / n[g] - mg[g] * mg[g] for g in range(G)]
        m = sum(A) / N
        v = sum(B) / N - m * m
        s = sum(n[g] * (mg[g] - m) ** 2 for g in range(G)) / (G - 1)
        vbar = sum(n[g] * vg[g] for g in range(G)) / N
        sv = sum(n[g] * (vg[g] - vbar) ** 2 for g in range(G)) / (G - 1)
        out["mean"][p], out["var"][p] = m, v
        out["mcse_mean"][p], out["mcse_var"][p] = np.sqrt(s / N), np.sqrt(sv / N)
        out["ess"][p] = N * v / s if s != 0 else np.inf
    return out


def random_case(seed=4, G=5, shape=(4, 3)):
    """groups of unequal size: sums of n_g draws of 3 + N(0, 1) per group and pixel"""
    rng = np.random.default_rng(seed)
    n = rng.integers(3, 40, G)
    assert len(set(n.tolist())) > 1
    S1, S2 = np.zeros((G,) + shape), np.zeros((G,) + shape)
    for g in range(G):
        x = 3.0 + rng.standard_normal((n[g],) + shape)
        S1[g], S2[g] = x.sum(0), (x * x).sum(0)
    return S1, S2, n.astype(np.int64)


def test_mcse_equals_the_definition_restated_loop_by_loop():
    from lmc_atomi_amd import mcse_from_group_moments
    S1, S2, n = random_case()
    want = definition(S1, S2, [int(v) for v in n])
    got = mcse_from_group_moments(S1, S2, n)
    for k, w in want.items():
        g = getattr(got, k)
        assert isinstance(g, np.ndarray) and g.dtype == np.float64 and g.shape == S1.shape[1:], k
        np.testing.assert_allclose(g, w, rtol=1e-12, atol=0, err_msg=k)
    assert np.isfinite(got.ess).all() and (got.mcse_mean > 0).all() and (got.mcse_var > 0).all()


def test_numpy_in_numpy_out_torch_in_torch_out():
    import torch
    from lmc_atomi_amd import mcse_from_group_moments
    S1, S2, n = random_case(seed=9)
    a = mcse_from_group_moments(S1, S2, n)
    b = mcse_from_group_moments(torch.from_numpy(S1), torch.from_numpy(S2), torch.from_numpy(n))
    c = mcse_from_group_moments(S1.astype(np.float32).astype(np.float64), S2, [int(v) for v in n])       # a list of counts
    assert isinstance(c.mean, np.ndarray)
    for k in ("mean", "var", "mcse_mean", "mcse_var", "ess"):
        t = getattr(b, k)
        assert isinstance(t, torch.Tensor) and t.dtype == torch.float64 and tuple(t.shape) == S1.shape[1:], k
        np.testing.assert_array_equal(t.numpy(), getattr(a, k), err_msg=k)


def test_one_group_and_an_empty_group_are_refused():
    from lmc_atomi_amd import mcse_from_group_moments
    S1, S2, n = random_case()
    with pytest.raises(ValueError, match="2 chain groups"):
        mcse_from_group_moments(S1[:1], S2[:1], n[:1])
    n0 = n.copy()
    n0[2] = 0
    with pytest.raises(ValueError, match="count of 0"):
        mcse_from_group_moments(S1, S2, n0)
    with pytest.raises(ValueError):
        mcse_from_group_moments(S1, S2, n[:-1])


def test_equal_group_means_give_an_infinite_ess_not_a_clamp():
    from lmc_atomi_amd import mcse_from_group_moments
    n = np.array([4, 4, 4])
    S1 = np.zeros((3, 2, 2))
    S2 = np.zeros((3, 2, 2))
    S1[:, 0, 0], S2[:, 0, 0] = 8.0, 24.0            # every group: mean 2, variance 2 -- s = 0 exactly
    S1[:, 0, 1], S2[:, 0, 1] = [4.0, 8.0, 12.0], [12.0, 24.0, 44.0]
    S1[:, 1, :], S2[:, 1, :] = S1[:, 0, :], S2[:, 0, :]
    r = mcse_from_group_moments(S1, S2, n)
    assert r.ess[0, 0] == np.inf and r.mcse_mean[0, 0] == 0.0 and r.var[0, 0] == 2.0
    assert np.isfinite(r.ess[0, 1]) and r.ess[0, 1] > 0


def test_mcse_of_stationary_ar1_chains_matches_the_known_asymptotic_variance():
    """x_{t+1} = rho x_t + sqrt(1 - rho^2) xi, rho = 0.5, started in stationarity: unit variance, the mean of N samples has variance
    (1 + rho) / (1 - rho) / N = 3 / N, and -- x^2 having autocorrelation rho^(2k) and variance 2 -- the variance estimate has variance
    2 (1 + rho^2) / (1 - rho^2) / N = 2 (5/3) / N.  64 chains, 400 kept iterations, 9 x 7 pixels, 32 groups: one pixel scatters by 1 / sqrt(2 x 31) = 13 %,
    the median of 63 pixels by about 2 %; over eight seeds the two ratios were 0.951 .. 1.011 and 0.952 .. 0.998."""
    from lmc_atomi_amd import mcse_from_group_moments
    rho, C_, T, shape, G = 0.5, 64, 400, (9, 7), 32
    rng = np.random.default_rng(12)
    x = np.empty((T, C_) + shape)
    x[0] = rng.standard_normal((C_,) + shape)
    for t in range(1, T):
        x[t] = rho * x[t - 1] + np.sqrt(1 - rho * rho) * rng.standard_normal((C_,) + shape)
    S1, S2, n = group_sums(x, G)
    assert (n == 2 * T).all()
    r = mcse_from_group_moments(S1, S2, n)
    N = C_ * T
    ratio_mean = np.median(r.mcse_mean) / np.sqrt(3.0 / N)
    ratio_var = np.median(r.mcse_var) / np.sqrt(2.0 * (5.0 / 3.0) / N)
    print("median mcse_mean / sqrt(3/N) =", ratio_mean, " median mcse_var / sqrt(2 (5/3) / N) =", ratio_var)
    assert 0.85 <= ratio_mean <= 1.15, ratio_mean
    assert 0.85 <= ratio_var <= 1.15, ratio_var
    np.testing.assert_allclose(r.mean, x.mean(axis=(0, 1)), rtol=0, atol=1e-12)
    np.testing.assert_allclose(r.var, x.var(axis=(0, 1)), rtol=1e-10, atol=0)


class _NoDevice:
    """stands where a prox would: a sampler that reached it has gone past the argument checks"""
    def __getattr__(self, name):
        raise AssertionError("the argument check must come before anything else")


@pytest.mark.parametrize("cls", ["MYULASampler", "MYMALASampler", "ULPDASampler", "SKROCKSampler"])
def test_chain_group_arguments_raise_before_any_device_call(cls):
    import lmc_atomi_amd as la
    args = (_NoDevice(), _NoDevice(), (16, 16)) if cls != "ULPDASampler" else (_NoDevice(), _NoDevice(), _NoDevice(), (16, 16))
    make = getattr(la, cls)
    with pytest.raises(ValueError, match="moments=True"):
        make(*args, n_chains=8, tau=0.1, moments=False, chain_groups=4)
    for bad in (0, 1, 65, -3):
        with pytest.raises(ValueError, match="chain_groups"):
            make(*args, n_chains=8, tau=0.1, moments=True, chain_groups=bad)


def test_entry_points_refuse_bad_chain_groups_before_any_device_call():
    import lmc_atomi_amd as la
    x0 = np.zeros(64)
    myula = lambda **kw: la.MoreauYosidaUnadjustedLangevin(_NoDevice(), _NoDevice(), x0, tau=0.1, gamma=0.5, niter=2, dims=(8, 8), **kw)
    ulpda = lambda **kw: la.UnadjustedLangevinPrimalDual(_NoDevice(), _NoDevice(), _NoDevice(), x0, 0.1, 1.0, niter=2, dims=(8, 8), **kw)
    mymala = lambda **kw: la.MoreauYosidaMetropolisAdjustedLangevin(_NoDevice(), _NoDevice(), x0, tau=0.1, gamma=0.5, niter=2, dims=(8, 8), **kw)
    skrock = lambda **kw: la.StabilisedLangevin(_NoDevice(), _NoDevice(), x0, tau=0.1, gamma=0.5, niter=2, dims=(8, 8), **kw)
    for fn in (myula, ulpda):
        with pytest.raises(ValueError, match="many-chain form"):
            fn(chain_groups=4)                                   # the reference form: n_chains=None
    for fn in (myula, ulpda, mymala, skrock):
        with pytest.raises(ValueError, match="exceeds n_chains"):
            fn(n_chains=3, chain_groups=4)
        for bad in (1, 65):
            with pytest.raises(ValueError, match="chain_groups must be"):
                fn(n_chains=100, chain_groups=bad)
    with pytest.raises(ValueError, match="exceeds n_chains"):
        la.sharded_myula(_NoDevice(), _NoDevice(), (8, 8), 3, x0, 0.1, 0.5, chain_groups=4)


def test_the_binding_names_the_cap_of_the_header():
    import os
    import re
    from lmc_atomi_amd import _capi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "lmc_atomi.h")) as f:
        m = re.search(r"#define\s+LMC_MAX_CHAIN_GROUPS\s+(\d+)", f.read())
    assert m and int(m.group(1)) == _capi.MAX_CHAIN_GROUPS == 64

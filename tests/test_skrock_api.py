"""CPU-only: the SK-ROCK coefficients of the library (`lmc_skrock_coefficients`, host code: the library loads without a device) against the
formulas of include/lmc_atomi.h evaluated with numpy.polynomial.chebyshev, the closed forms of the scheme for a linear drift, and the refusals that
are raised before any device handle exists.

For a linear drift -l x and z = -delta l one iteration is X+ = R_s(z) X + sqrt(2 delta) B_s(z) Z with
  R_s(z) = T_s(w0 + w1 z) / T_s(w0),     B_s(z) = U_{s-1}(w0 + w1 z) / U_{s-1}(w0) (1 + w1 z / 2),
U the Chebyshev polynomials of the second kind (U_{s-1} = T_s' / s).  The closed forms pin the coefficients: with nu_1 = s w0 / 2 in place of
s w1 / 2 the noise factor grows to 25 at s = 15.

Bounds: 1e-12 relative -- float64 three-term recurrences of at most 64 terms, all of one sign at w0 > 1, against numpy's Clenshaw sums."""
import ctypes as C

import numpy as np
import pytest
from numpy.polynomial import chebyshev as cheb

LMC_E_INVALID = -1
STAGES = (2, 3, 5, 10, 15, 64)


def T(j, x):
    return cheb.chebval(x, [0.0] * j + [1.0])


def dT(j, x):
    return cheb.chebval(x, cheb.chebder([0.0] * j + [1.0]))


def reference(s, eta):
    w0 = 1.0 + eta / s ** 2
    w1 = T(s, w0) / dT(s, w0)
    mu, nu, kappa = np.empty(s), np.empty(s), np.empty(s)
    mu[0], nu[0], kappa[0] = w1 / w0, s * w1 / 2, s * w1 / w0
    for j in range(2, s + 1):
        mu[j - 1] = 2 * w1 * T(j - 1, w0) / T(j, w0)
        nu[j - 1] = 2 * w0 * T(j - 1, w0) / T(j, w0)
        kappa[j - 1] = -T(j - 2, w0) / T(j, w0)
    return w0, w1, mu, nu, kappa


def step_factor(s, eta):
    return (s - 0.5) ** 2 * (2 - 4 * eta / 3) - 1.5


@pytest.fixture(scope="module")
def la():
    import lmc_atomi_amd as la
    return la


@pytest.mark.parametrize("s", STAGES)
def test_coefficients_match_the_chebyshev_formulas(la, s):
    eta = 0.05
    mu, nu, kappa = la.skrock_coefficients(s, eta)
    assert mu.dtype == nu.dtype == kappa.dtype == np.float64 and mu.shape == nu.shape == kappa.shape == (s,)
    _, _, rmu, rnu, rkappa = reference(s, eta)
    for name, got, ref in (("mu", mu, rmu), ("nu", nu, rnu), ("kappa", kappa, rkappa)):
        err = np.abs(got - ref) / np.abs(ref)
        print(f"s={s} {name}: max rel err {err.max():.2e}")
        assert err.max() <= 1e-12, (name, err.max())
    assert np.abs(nu[1:] + kappa[1:] - 1.0).max() <= 1e-12
    # the stability bound: through the C function and through skrock_step_bound
    from lmc_atomi_amd import _dev
    ls = C.c_double()
    assert _dev.lib().lmc_skrock_coefficients(s, eta, None, None, None, C.byref(ls)) == 0
    assert abs(ls.value - step_factor(s, eta)) <= 1e-12 * step_factor(s, eta)
    assert abs(la.skrock_step_bound(4.0, s, eta) - step_factor(s, eta) / 4.0) <= 1e-12 * step_factor(s, eta)


@pytest.mark.parametrize("s", (2, 3, 5, 10, 15))
@pytest.mark.parametrize("frac", (0.1, 0.5, 1.0))
def test_recursion_of_the_returned_coefficients_reproduces_the_closed_forms(la, s, frac):
    eta = 0.05
    mu, nu, kappa = la.skrock_coefficients(s, eta)
    w0, w1, _, _, _ = reference(s, eta)
    z = -frac * step_factor(s, eta)
    # K_j = r_j X + b_j q Z for the drift -l x, z = -delta l:  K_1 = X + mu_1 z (X + nu_1 q Z) + kappa_1 q Z,  K_j = (mu_j z + nu_j) K_{j-1} + kappa_j K_{j-2}
    r2, b2 = 1.0, 0.0
    r1, b1 = 1.0 + mu[0] * z, mu[0] * z * nu[0] + kappa[0]
    for j in range(2, s + 1):
        r1, r2 = (mu[j - 1] * z + nu[j - 1]) * r1 + kappa[j - 1] * r2, r1
        b1, b2 = (mu[j - 1] * z + nu[j - 1]) * b1 + kappa[j - 1] * b2, b1
    R = T(s, w0 + w1 * z) / T(s, w0)
    B = dT(s, w0 + w1 * z) / dT(s, w0) * (1 + w1 * z / 2)          # U_{s-1} = T_s' / s: the factor s cancels
    print(f"s={s} z={z:.4g}: R {r1:.15e} vs {R:.15e}, B {b1:.15e} vs {B:.15e}")
    assert abs(r1 - R) <= 1e-12 and abs(b1 - B) <= 1e-12
    assert abs(R) <= 1.0


@pytest.mark.parametrize("s,eta", [(1, 0.05), (65, 0.05), (10, 0.0), (10, -1.0), (10, float("nan"))])
def test_bad_stage_counts_and_dampings_are_refused(la, s, eta):
    from lmc_atomi_amd import _dev
    with pytest.raises(ValueError):
        la.skrock_coefficients(s, eta)
    with pytest.raises(ValueError):
        la.skrock_step_bound(1.0, s, eta)
    buf = (C.c_double * 64)()
    assert _dev.lib().lmc_skrock_coefficients(s, eta, buf, None, None, None) == LMC_E_INVALID
    assert _dev.lib().lmc_last_error()


def test_refusals_are_raised_before_any_device_handle(la):
    """TV(rtol > 0), a warm-started dual, array-valued epsg, a bad stage count and tau=None: all raised by the constructor's own checks, which come
    before the first device call -- so they raise with or without a GPU."""
    shape = (8, 8)
    pf = la.L2(Op=la.Convolve2D(shape, np.ones((5, 5)) / 25), b=np.zeros(64), sigma=1.0)
    kw = dict(n_chains=2, tau=0.1, gamma=0.5)
    with pytest.raises(NotImplementedError, match="rtol"):
        la.SKROCKSampler(pf, la.TV(shape, 0.3, rtol=1e-4), shape, **kw)
    with pytest.raises(NotImplementedError, match="warm"):
        la.SKROCKSampler(pf, la.TV(shape, 0.3, niter=3, warm=True), shape, **kw)
    with pytest.raises(NotImplementedError, match="warm"):
        la.SKROCKSampler(pf, la.TV(shape, 0.3, niter=3), shape, tv_warm=True, **kw)
    with pytest.raises(NotImplementedError, match="epsg"):
        la.SKROCKSampler(pf, la.L2(sigma=0.05), shape, epsg=np.full(64, 0.5), **kw)
    with pytest.raises(ValueError):
        la.SKROCKSampler(pf, la.TV(shape, 0.3), shape, n_stages=1, **kw)
    with pytest.raises(ValueError):
        la.SKROCKSampler(pf, la.TV(shape, 0.3), shape, eta=0.0, **kw)
    with pytest.raises(NotImplementedError, match="tau=None"):
        la.SKROCKSampler(pf, la.TV(shape, 0.3), shape, n_chains=2, gamma=0.5)
    with pytest.raises(NotImplementedError, match="rtol"):
        la.StabilisedLangevin(pf, la.TV(shape, 0.3, rtol=1e-4), np.zeros(64), tau=0.1, gamma=0.5, n_chains=2)
    with pytest.raises(NotImplementedError, match="tau=None"):
        la.StabilisedLangevin(pf, la.TV(shape, 0.3), np.zeros(64), None, gamma=0.5, n_chains=2)


def test_sampler_surface(la):
    import inspect
    sig = inspect.signature(la.SKROCKSampler.__init__)
    assert list(sig.parameters)[:6] == ["self", "proxf", "proxg", "dims", "n_stages", "eta"]
    assert sig.parameters["n_stages"].default == 10 and sig.parameters["eta"].default == 0.05
    assert issubclass(la.SKROCKSampler, la.MYULASampler)
    sl = inspect.signature(la.StabilisedLangevin)
    assert list(sl.parameters)[:11] == ["proxf", "proxg", "x0", "tau", "gamma", "epsg", "niter", "n_stages", "eta", "seed", "callback"]
    for name in ("n_chains", "dims", "chain_offset", "burn_in", "thin", "device", "moment_scales", "hist_bins", "hist_range", "quantiles"):
        assert sl.parameters[name].kind is inspect.Parameter.KEYWORD_ONLY
    from lmc_atomi_amd import _capi
    assert _capi.ABI_VERSION == 4 and _capi.MAX_SKROCK_STAGES == 64

"""CPU-only: the host side of the SAPG estimation of the prior weight (include/lmc_atomi.h): `lmc_sapg_update` against its definition in numpy
float64, `lmc_sapg_dimension`, the config check, the struct size, and the Python argument errors that are raised before any device handle exists.
The library loads without a device.

    delta_n     = step_scale (n + 1)^(-step_exponent) / d
    eta_{n+1}   = clamp(log(theta_n) + delta_n (d / k - theta_n gbar), log(theta_min), log(theta_max))
    theta_{n+1} = exp(eta_{n+1})

Bound on the update: 1e-14 relative -- four double operations, `exp` and `log`, each within an ulp (1.1e-16) of numpy's, and |eta| <= log(1e3) ~ 7
multiplies the error of eta by at most that in theta."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LMC_E_INVALID, LMC_E_UNSUPPORTED = -1, -2
PRIOR_NONE, PRIOR_L2, PRIOR_L1, PRIOR_TV_ISO, PRIOR_TV_ANISO, PRIOR_HAAR_L1, PRIOR_EPROX = range(7)


@pytest.fixture(scope="module")
def la():
    import lmc_atomi_amd as la
    return la


@pytest.fixture(scope="module")
def lib():
    from lmc_atomi_amd import _dev
    return _dev.lib()


def config(**kw):
    from lmc_atomi_amd import _capi
    c = _capi.lmc_sapg_config()
    c.struct_size = C.sizeof(_capi.lmc_sapg_config)
    c.theta0, c.theta_min, c.theta_max = 0.3, 1e-3, 1e2
    c.dim_eff = 1000.0
    c.step_scale, c.step_exponent = 10.0, 0.8
    c.warmup_iters, c.n_updates, c.iters_per_update, c.average_from = 0, 10, 1, 5
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def update(lib, cfg, n, theta, gbar):
    out = C.c_double(-1.0)
    rc = lib.lmc_sapg_update(C.byref(cfg), n, theta, gbar, C.byref(out))
    return rc, out.value


def reference(n, theta, gbar, d, k=1.0, c0=10.0, p=0.8, lo=1e-3, hi=1e2):
    delta = c0 * (n + 1.0) ** (-p) / d
    eta = np.log(theta) + delta * (d / k - theta * gbar)
    return np.exp(np.clip(eta, np.log(lo), np.log(hi)))


def test_update_matches_the_definition(lib):
    d = 1000.0
    worst, inside = 0.0, 0
    for n in (0, 1, 10, 10 ** 4):
        for theta in np.logspace(-3, 2, 11):
            for gbar in d * np.logspace(-3, 3, 13):          # six decades around d: theta gbar = d is the fixed point of theta = 1
                rc, got = update(lib, config(dim_eff=d), n, float(theta), float(gbar))
                assert rc == 0
                ref = reference(n, theta, gbar, d)
                err = abs(got - ref) / ref
                worst = max(worst, err)
                inside += 1e-3 < ref < 1e2
                assert err <= 1e-14, (n, theta, gbar, got, ref)
    print(f"lmc_sapg_update against numpy float64: max relative error {worst:.2e}; {inside} of {4 * 11 * 13} cases strictly inside the bounds")
    assert inside > 100


def test_python_update_of_degree_two_matches_the_definition(la):
    """`sapg_update(degree=k)` calls the degree-1 entry point with step_scale / k and k gbar: the same step in other roundings.  Where the step is not
    clamped both terms of delta (d / k - theta gbar) are below ~20 in magnitude and each carries about four roundings of 1.1e-16 relative: 4 x 20 x
    1.1e-16 ~ 1e-14 absolute in eta = relative in theta, on either side; bound 5e-14."""
    d = 256.0
    for n in (0, 3):
        for theta in (0.05, 1.0, 20.0):
            for gbar in (1.0, 128.0, 4000.0):
                got = la.sapg_update(theta, gbar, n, d, degree=2.0)
                ref = reference(n, theta, gbar, d, k=2.0)
                assert abs(got - ref) <= 5e-14 * ref, (n, theta, gbar, got, ref)


def test_a_step_that_leaves_the_bounds_returns_the_bound_bit_for_bit(lib):
    lo, hi = 0.0123456789, 7.654321      # log / exp do not round-trip every double: the bound itself must come back
    cfg = config(theta_min=lo, theta_max=hi, theta0=1.0, dim_eff=100.0)
    rc, got = update(lib, cfg, 0, 1.0, 1e9)          # a huge statistic: far below the lower bound
    assert rc == 0 and got == lo
    rc, got = update(lib, cfg, 0, 1.0, 0.0)          # eta = log(1) + 10 / 100 * 100 = 10 > log(hi)
    assert rc == 0 and got == hi
    rc, got = update(lib, cfg, 0, lo, 1e9)
    assert rc == 0 and got == lo
    rc, got = update(lib, cfg, 0, hi, 0.0)
    assert rc == 0 and got == hi


def problem(kind, H, W):
    from lmc_atomi_amd import _capi
    p = _capi.lmc_problem()
    p.struct_size = C.sizeof(_capi.lmc_problem)
    p.H, p.W, p.prior_kind = H, W, kind
    return p


def test_default_dimensions(lib, la):
    H, W = 16, 24
    want = {PRIOR_L1: (H * W, 1.0), PRIOR_L2: (H * W, 2.0), PRIOR_TV_ISO: (H * W - 1, 1.0), PRIOR_TV_ANISO: (H * W - 1, 1.0),
            PRIOR_HAAR_L1: (H * W - (H // 8) * (W // 8), 1.0)}
    for kind, (d_ref, k_ref) in want.items():
        d, k = C.c_double(), C.c_double()
        p = problem(kind, H, W)
        assert lib.lmc_sapg_dimension(C.byref(p), C.byref(d), C.byref(k)) == 0
        assert (d.value, k.value) == (float(d_ref), k_ref), kind
        assert lib.lmc_sapg_dimension(C.byref(p), None, None) == 0
    for kind in (PRIOR_NONE, PRIOR_EPROX):
        d = C.c_double()
        assert lib.lmc_sapg_dimension(C.byref(problem(kind, H, W)), C.byref(d), None) == LMC_E_UNSUPPORTED
        assert lib.lmc_last_error()
    assert lib.lmc_sapg_dimension(C.byref(problem(PRIOR_HAAR_L1, 12, 24)), None, None) == LMC_E_UNSUPPORTED
    assert lib.lmc_sapg_dimension(None, None, None) == LMC_E_INVALID
    bad = problem(PRIOR_L1, H, W)
    bad.struct_size -= 4
    assert lib.lmc_sapg_dimension(C.byref(bad), None, None) == LMC_E_INVALID
    # the Python form, without a device
    assert la.sapg_dimension(la.TV((H, W), 0.3)) == (H * W - 1.0, 1.0)
    assert la.sapg_dimension(la.L2(sigma=0.05), (H, W)) == (float(H * W), 2.0)
    assert la.sapg_dimension(la.L1(sigma=0.05), (H, W)) == (float(H * W), 1.0)
    assert la.sapg_dimension(la.WaveletL1((H, W), 2.0)) == (float(H * W - 6), 1.0)
    with pytest.raises(NotImplementedError):
        la.sapg_dimension(la.Laplace(0.1), (H, W))


NAN, INF = float("nan"), float("inf")
BAD_CONFIGS = [
    dict(struct_size=8), dict(theta_min=0.0), dict(theta_min=-1.0), dict(theta_min=NAN), dict(theta_max=INF), dict(theta_max=NAN),
    dict(theta0=1e-4), dict(theta0=1e3), dict(theta0=NAN), dict(theta_min=2.0, theta_max=1.0, theta0=1.5),
    dict(dim_eff=-1.0), dict(dim_eff=NAN), dict(dim_eff=INF), dict(dim_eff=0.0),     # 0 = "the default": lmc_sapg_update has no problem to take it from
    dict(step_scale=0.0), dict(step_scale=-1.0), dict(step_scale=NAN), dict(step_scale=INF),
    dict(step_exponent=0.5), dict(step_exponent=1.0001), dict(step_exponent=NAN),
    dict(warmup_iters=-1), dict(n_updates=0), dict(iters_per_update=0), dict(average_from=-1), dict(average_from=10),
]


@pytest.mark.parametrize("bad", BAD_CONFIGS, ids=lambda b: ",".join(f"{k}={v}" for k, v in b.items()))
def test_bad_configs_are_invalid(lib, bad):
    rc, _ = update(lib, config(**bad), 0, 0.3, 100.0)
    assert rc == LMC_E_INVALID
    assert lib.lmc_last_error()


def test_bad_update_arguments_are_invalid(lib):
    good = config()
    assert update(lib, good, 0, 0.3, 100.0)[0] == 0
    assert update(lib, config(theta_min=0.3, theta_max=0.3), 0, 0.3, 100.0) == (0, 0.3)     # min = theta0 = max is allowed
    assert update(lib, config(step_exponent=1.0), 0, 0.3, 100.0)[0] == 0
    for n, theta, gbar in ((-1, 0.3, 1.0), (0, 0.0, 1.0), (0, -0.3, 1.0), (0, NAN, 1.0), (0, INF, 1.0), (0, 0.3, NAN), (0, 0.3, INF)):
        assert update(lib, good, n, theta, gbar)[0] == LMC_E_INVALID, (n, theta, gbar)
    assert lib.lmc_sapg_update(None, 0, 0.3, 1.0, C.byref(C.c_double())) == LMC_E_INVALID
    assert lib.lmc_sapg_update(C.byref(good), 0, 0.3, 1.0, None) == LMC_E_INVALID


def test_config_layout_matches_the_header():
    from lmc_atomi_amd import _capi
    code = '#include <stdio.h>\n#include "lmc_atomi.h"\nint main(){printf("%zu\\n", sizeof(lmc_sapg_config));return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "s.c"), os.path.join(d, "s")
        open(src, "w").write(code)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        size = int(subprocess.run([exe], check=True, capture_output=True, text=True).stdout)
    assert C.sizeof(_capi.lmc_sapg_config) == size
    assert _capi.ABI_VERSION == 4


def test_argument_errors_are_raised_before_any_device_handle(la):
    """Bounds, theta0 outside them, the exponent, the counts: ValueError from the one-call form's own checks, which come before the sampler is
    created -- so they raise with or without a GPU.  Unsupported combinations: NotImplementedError, equally early."""
    shape = (8, 8)
    pf = la.L2(Op=la.Convolve2D(shape, np.ones((5, 5)) / 25), b=np.zeros(64), sigma=1.0)
    tv = la.TV(shape, 0.3)
    args = (pf, tv, np.zeros(64), 0.1, 0.5)
    for kw in (dict(theta_bounds=(0.0, 1.0)), dict(theta_bounds=(-1.0, 1.0)), dict(theta_bounds=(2.0, 1.0)), dict(theta_bounds=(1e-3, float("inf"))),
               dict(theta_bounds=(1e-3,)), dict(theta_bounds=None),
               dict(theta_bounds=(0.5, 1.0)),                       # theta0 = the weight of proxg = 0.3 lies outside
               dict(theta_bounds=(1e-3, 1e2), theta0=1e-4), dict(theta_bounds=(1e-3, 1e2), theta0=1e3),
               dict(theta_bounds=(1e-3, 1e2), step_exponent=0.5), dict(theta_bounds=(1e-3, 1e2), step_exponent=1.1),
               dict(theta_bounds=(1e-3, 1e2), step_scale=0.0), dict(theta_bounds=(1e-3, 1e2), warmup=-1),
               dict(theta_bounds=(1e-3, 1e2), iters_per_update=0), dict(theta_bounds=(1e-3, 1e2), average_from=20),
               dict(theta_bounds=(1e-3, 1e2), dim_eff=-1.0)):
        kw = dict(kw)
        bounds = kw.pop("theta_bounds")
        with pytest.raises(ValueError):
            la.EstimatePriorWeight(*args, 20, bounds, n_chains=2, **kw)
    with pytest.raises(ValueError):
        la.EstimatePriorWeight(*args, 0, (1e-3, 1e2), n_chains=2)
    ok = dict(n_chains=2)
    with pytest.raises(NotImplementedError):
        la.EstimatePriorWeight(pf, la.Laplace(0.1), np.zeros(64), 0.1, 0.5, 20, (1e-3, 1e2), theta0=0.1, dims=shape, **ok)
    with pytest.raises(NotImplementedError):
        la.EstimatePriorWeight(pf, None, np.zeros(64), 0.1, 0.5, 20, (1e-3, 1e2), theta0=0.1, **ok)
    with pytest.raises(NotImplementedError, match="warm"):
        la.EstimatePriorWeight(pf, la.TV(shape, 0.3, niter=3, warm=True), np.zeros(64), 0.1, 0.5, 20, (1e-3, 1e2), **ok)
    with pytest.raises(NotImplementedError, match="epsg"):
        la.EstimatePriorWeight(pf, la.L2(sigma=0.05), np.zeros(64), 0.1, 0.5, 20, (1e-3, 1e2), epsg=np.full(64, 0.5), **ok)
    with pytest.raises(NotImplementedError, match="mymala"):
        la.EstimatePriorWeight(*args, 20, (1e-3, 1e2), sampler="mymala", **ok)
    with pytest.raises(ValueError):
        la.sapg_update(0.3, 1.0, 0, 0.0)
    with pytest.raises(ValueError):
        la.sapg_update(0.3, 1.0, 0, 64.0, step_exponent=0.4)


def test_surface(la):
    import inspect
    sig = inspect.signature(la.MYULASampler.estimate_prior_weight)
    assert list(sig.parameters) == ["self", "n_updates", "theta_bounds", "theta0", "warmup", "iters_per_update", "step_scale", "step_exponent",
                                    "average_from", "dim_eff", "noise"]
    assert sig.parameters["step_scale"].default == 10.0 and sig.parameters["step_exponent"].default == 0.8
    assert la.SKROCKSampler.set_prior_weight is la.MYULASampler.set_prior_weight
    one = inspect.signature(la.EstimatePriorWeight)
    assert list(one.parameters)[:7] == ["proxf", "proxg", "x0", "tau", "gamma", "n_updates", "theta_bounds"]
    assert one.parameters["sampler"].default == "myula" and one.parameters["n_stages"].default == 10
    assert [f for f in ("theta", "theta_trace", "stat_trace", "dim_eff", "degree") if hasattr(la.SAPGResult(1, 2, 3, 4, 5), f)] == \
        ["theta", "theta_trace", "stat_trace", "dim_eff", "degree"]

"""CPU only: the host side of the covariance sketch -- the identities behind cov_from_sketch, the Nystrom modes, the argument checks, the header and
the signatures.  The device side is tests/test_gpu_cov_sketch.py."""
import ctypes as C
import inspect
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from tests import _cov_sketch_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def sums_of(X, P, m):
    """float64 sums of the samples X [n, N] the way the definition forms them, and s1"""
    Y, s, Q = R.sketch_ref(X, P, m)
    return Y, s, Q, X.astype(np.float32).astype(np.float64).sum(axis=0)


def low_rank_samples(rng, n, N, lam, noise=0.0, mean=100.0):
    U = np.linalg.qr(rng.standard_normal((N, len(lam))))[0]
    X = mean + 10 * rng.standard_normal(N) + (rng.standard_normal((n, len(lam))) * np.sqrt(lam)) @ U.T + noise * rng.standard_normal((n, N))
    return X.astype(np.float32)          # the samples ARE fp32 numbers; everything after is float64


def test_reference_and_restatement_agree_on_exact_data_and_split_their_runs():
    """integers: both yardsticks are exact, whatever the run lengths; 2 x 2500 pixels and 1100 chains cross both run boundaries"""
    rng = np.random.default_rng(0)
    x = rng.integers(-3, 4, size=(1100, 2, 2500)).astype(np.float32) + 7
    P = rng.integers(-1, 2, size=(3, 2, 2500)).astype(np.float32)
    m = np.full((2, 2500), 7, dtype=np.float32)
    assert 2 * 2500 > R.PIXEL_RUN and 1100 > R.CHAIN_RUN
    for a, b in zip(R.sketch_ref(x, P, m), R.sketch_fp32(x, P, m)):
        np.testing.assert_array_equal(a, b)
    # float data: the restatement rounds, and by about fp32
    xf = (100 + 5 * rng.standard_normal((8, 4, 600))).astype(np.float32)
    Pf = rng.standard_normal((3, 4, 600)).astype(np.float32)
    ref = R.sketch_ref(xf, Pf, None)
    e = R.max_abs_errors(R.sketch_fp32(xf, Pf, None), ref)
    assert all(0 < v <= 1e-4 * np.abs(r).max() for v, r in zip(e, ref)), e


@pytest.mark.parametrize("centre", ["mean", "none", "off"])
def test_cov_from_sketch_reproduces_the_sample_covariance(centre):
    from lmc_atomi_amd import cov_from_sketch
    rng = np.random.default_rng(1)
    H, W, n, k = 6, 9, 300, 5
    X = low_rank_samples(rng, n, H * W, np.array([9.0, 4.0, 1.0]), noise=0.3)
    P = rng.standard_normal((k, H, W)).astype(np.float32)
    m = {"mean": X.mean(axis=0).astype(np.float32).reshape(H, W), "none": None, "off": np.full((H, W), 37.0, dtype=np.float32)}[centre]
    Y, s, Q, s1 = sums_of(X, P, m)
    cs = cov_from_sketch(Y.reshape(k, H, W), s, Q, n, s1.reshape(H, W), m)
    assert cs.n == n and cs.cov_xt.shape == (k, H, W) and cs.cov_tt.shape == (k, k) and cs.t_mean.shape == (k,)
    X64, P64 = X.astype(np.float64), P.reshape(k, -1).astype(np.float64)
    S = np.cov(X64.T, bias=True)
    # The margin over float64 rounding comes from the identity check itself: the same covariances by a second float64 evaluation order (centred samples
    # first, then the products) differ from np.cov by rounding alone; the sketch, which subtracts terms of the size of centre offset^2, may be 4 times as
    # far plus the cancellation it documents: |tbar| |dbar| 2^-52 per entry.
    Xc = X64 - X64.mean(axis=0)
    alt_xt, alt_tt = (P64 @ Xc.T) @ Xc / n, (P64 @ Xc.T) @ (P64 @ Xc.T).T / n
    order_xt, order_tt = np.abs(alt_xt - P64 @ S).max(), np.abs(alt_tt - P64 @ S @ P64.T).max()
    dbar = s1 / n - (0 if m is None else m.reshape(-1).astype(np.float64))
    cancel_xt = 2.0 ** -52 * (np.abs(Y).max() / n + np.abs(s / n).max() * np.abs(dbar).max())
    cancel_tt = 2.0 ** -52 * (np.abs(Q).max() / n + np.abs(s / n).max() ** 2)
    e_xt, e_tt = np.abs(cs.cov_xt.reshape(k, -1) - P64 @ S).max(), np.abs(cs.cov_tt - P64 @ S @ P64.T).max()
    print(f"centre={centre}: cov_xt err {e_xt:.3e} (order {order_xt:.3e}, cancellation {cancel_xt:.3e})  cov_tt err {e_tt:.3e} (order {order_tt:.3e}, "
          f"cancellation {cancel_tt:.3e})")
    assert order_xt > 0 and order_tt > 0
    assert e_xt <= 4 * order_xt + n * cancel_xt
    assert e_tt <= 4 * order_tt + n * cancel_tt
    np.testing.assert_allclose(cs.t_mean, (P64 @ (X64 - (0 if m is None else m.reshape(-1).astype(np.float64))).T).mean(axis=1), rtol=1e-12, atol=1e-12)


def test_modes_recover_a_rank_3_covariance_from_8_gaussian_probes():
    from lmc_atomi_amd import cov_from_sketch, random_probes
    rng = np.random.default_rng(2)
    H, W, n, k = 12, 20, 400, 8
    lam = np.array([9.0, 4.0, 1.0])
    X = low_rank_samples(rng, n, H * W, lam)
    P = random_probes(k, (H, W), seed=5)
    assert P.dtype == np.float32 and P.shape == (k, H, W)
    np.testing.assert_array_equal(P, random_probes(k, (H, W), seed=5))
    np.testing.assert_array_equal(P, np.random.default_rng(5).standard_normal((k, H, W)).astype(np.float32))
    m = np.round(X.mean(axis=0)).astype(np.float32)
    Y, s, Q, s1 = sums_of(X, P, m)
    cs = cov_from_sketch(Y, s, Q, n, s1, m)
    S = np.cov(X.astype(np.float64).T, bias=True)
    w, V = np.linalg.eigh(S)
    # X is fp32: its covariance has rank 3 up to the fp32 rounding of the samples (1e-5 of values near 100, eigenvalues of order 1e-10): rcond above that
    vals, imgs = cs.modes(3, rcond=1e-6)
    assert vals.shape == (3,) and imgs.shape == (3, H * W)
    np.testing.assert_allclose(vals, w[::-1][:3], rtol=1e-6)
    for i in range(3):
        assert abs(abs(imgs[i] @ V[:, -1 - i]) - 1) <= 1e-6, i
    with pytest.raises(ValueError, match="rank"):
        cs.modes(4, rcond=1e-6)
    with pytest.raises(ValueError, match="rank"):
        cs.modes(0)
    with pytest.raises(ValueError):
        cs.modes(k + 1, rcond=0.0)
    # image-shaped sums give image-shaped modes
    cs2 = cov_from_sketch(Y.reshape(k, H, W), s, Q, n, s1.reshape(H, W), m.reshape(H, W))
    assert cs2.modes(2, rcond=1e-6)[1].shape == (2, H, W)


def test_modes_of_a_full_rank_covariance_are_lower_bounds():
    from lmc_atomi_amd import cov_from_sketch, random_probes
    rng = np.random.default_rng(3)
    H, W, n, k = 6, 10, 500, 8
    X = low_rank_samples(rng, n, H * W, np.array([9.0, 4.0, 1.0]), noise=0.5)
    Y, s, Q, s1 = sums_of(X, random_probes(k, (H, W), 1), None)
    vals, _ = cov_from_sketch(Y, s, Q, n, s1).modes(3)
    top = np.linalg.eigvalsh(np.cov(X.astype(np.float64).T, bias=True))[::-1][:3]
    assert (vals <= top * (1 + 1e-9)).all() and (vals > 0).all() and (np.diff(vals) <= 0).all(), (vals, top)


def test_corr_is_nan_where_a_variance_is_zero():
    from lmc_atomi_amd import CovSketch
    cs = CovSketch(np.array([[[0.5, 0.0], [0.2, 0.1]], [[0.0, 0.0], [0.0, 0.0]]]), np.array([[4.0, 0.0], [0.0, 0.0]]), np.zeros(2), 10)
    var = np.array([[1.0, 0.0], [0.25, 1.0]])
    c = cs.corr(var)
    assert c.shape == (2, 2, 2)
    np.testing.assert_array_equal(c[0], np.array([[0.25, np.nan], [0.2, 0.05]]))
    assert np.isnan(c[1]).all()            # a projection without variance


def test_cov_from_sketch_refuses_what_has_no_covariance():
    from lmc_atomi_amd import cov_from_sketch
    Y, s, Q = np.zeros((2, 3, 4)), np.zeros(2), np.zeros((2, 2))
    with pytest.raises(ValueError, match="no samples"):
        cov_from_sketch(Y, s, Q, 0, np.zeros((3, 4)))
    with pytest.raises(ValueError):
        cov_from_sketch(Y, np.zeros(3), Q, 5, np.zeros((3, 4)))


class _NoDevice:
    """stands where a prox would: a sampler that reached it has gone past the argument checks"""
    def __getattr__(self, name):
        raise AssertionError("the argument check must come before anything else")


def bad_arguments(shape):
    H, W = shape
    good = np.ones((2, H, W), dtype=np.float32)
    nan = good.copy()
    nan[1, 0, 0] = np.nan
    return [
        (dict(cov_probes=np.ones((2, H, W + 1))), "cov_probes must be"),
        (dict(cov_probes=np.ones((H, W))), "cov_probes must be"),
        (dict(cov_probes=np.ones((33, H * W))), "1 .. 32"),
        (dict(cov_probes=np.ones((0, H, W))), "1 .. 32"),
        (dict(cov_probes=nan), "finite"),
        (dict(cov_probes=good, cov_center=np.ones((H, W + 1))), "cov_center must be"),
        (dict(cov_probes=good, cov_center=np.full((H, W), np.inf)), "finite"),
        (dict(cov_center=np.ones((H, W))), "without cov_probes"),
    ]


@pytest.mark.parametrize("cls", ["MYULASampler", "MYMALASampler", "ULPDASampler", "SKROCKSampler"])
def test_sampler_arguments_raise_before_any_device_call(cls):
    import lmc_atomi_amd as la
    shape = (16, 12)
    args = (_NoDevice(), _NoDevice(), shape) if cls != "ULPDASampler" else (_NoDevice(), _NoDevice(), _NoDevice(), shape)
    make = getattr(la, cls)
    with pytest.raises(ValueError, match="moments=True"):
        make(*args, n_chains=8, tau=0.1, moments=False, cov_probes=np.ones((2,) + shape))
    for kw, msg in bad_arguments(shape):
        with pytest.raises(ValueError, match=msg):
            make(*args, n_chains=8, tau=0.1, moments=True, **kw)


def test_entry_points_refuse_bad_sketch_arguments_before_any_device_call():
    import lmc_atomi_amd as la
    shape = (8, 8)
    x0 = np.zeros(64)
    myula = lambda **kw: la.MoreauYosidaUnadjustedLangevin(_NoDevice(), _NoDevice(), x0, tau=0.1, gamma=0.5, niter=2, dims=shape, **kw)
    ulpda = lambda **kw: la.UnadjustedLangevinPrimalDual(_NoDevice(), _NoDevice(), _NoDevice(), x0, 0.1, 1.0, niter=2, dims=shape, **kw)
    mymala = lambda **kw: la.MoreauYosidaMetropolisAdjustedLangevin(_NoDevice(), _NoDevice(), x0, tau=0.1, gamma=0.5, niter=2, dims=shape, **kw)
    skrock = lambda **kw: la.StabilisedLangevin(_NoDevice(), _NoDevice(), x0, tau=0.1, gamma=0.5, niter=2, dims=shape, **kw)
    for fn in (myula, ulpda):
        with pytest.raises(ValueError, match="many-chain form"):
            fn(cov_probes=np.ones((2,) + shape))                 # the reference form: n_chains=None
    for fn in (myula, ulpda, mymala, skrock):
        for kw, msg in bad_arguments(shape):
            with pytest.raises(ValueError, match=msg):
                fn(n_chains=4, **kw)


def test_stateless_form_checks_its_arguments_first():
    import lmc_atomi_amd as la
    x = np.zeros((3, 4, 5), dtype=np.float32)
    with pytest.raises(ValueError, match="C, H, W"):
        la.cov_sketch(np.zeros((4, 5)), np.ones((1, 4, 5)))
    for kw, msg in bad_arguments((4, 5)):
        if "cov_probes" in kw:
            with pytest.raises(ValueError, match=msg):
                la.cov_sketch(x, kw["cov_probes"], kw.get("cov_center"))
    for bad in (0, 33):
        with pytest.raises(ValueError):
            la.random_probes(bad, (4, 5))


def test_no_gpu_means_loud_failure_not_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import lmc_atomi_amd as la
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        la.cov_sketch(np.zeros((3, 4, 5), dtype=np.float32), np.ones((2, 4, 5), dtype=np.float32))


@pytest.mark.parametrize("fn", ["MoreauYosidaUnadjustedLangevin", "StabilisedLangevin", "MoreauYosidaMetropolisAdjustedLangevin",
                                "UnadjustedLangevinPrimalDual"])
def test_new_keywords_are_keyword_only_and_last(fn):
    import lmc_atomi_amd as la
    params = inspect.signature(getattr(la, fn)).parameters
    names = list(params)
    assert names[-2:] == ["cov_probes", "cov_center"]
    for n in names[-2:]:
        assert params[n].kind is inspect.Parameter.KEYWORD_ONLY and params[n].default is None


@pytest.mark.parametrize("cls", ["MYULASampler", "MYMALASampler", "ULPDASampler", "SKROCKSampler"])
def test_sampler_classes_take_the_keywords(cls):
    import lmc_atomi_amd as la
    c = getattr(la, cls)
    params = inspect.signature(c.__init__ if cls != "SKROCKSampler" else la.MYULASampler.__init__).parameters
    assert params["cov_probes"].default is None and params["cov_center"].default is None
    assert c.cov_k is None and callable(c.cov_sketch)


def test_exports():
    import lmc_atomi_amd as la
    for name in ("cov_sketch", "cov_from_sketch", "CovSketch", "random_probes", "allreduce_cov_sketch"):
        assert name in la.__all__ and hasattr(la, name), name
    assert la.MYULAResult(None, None, None, 0, None, None, 0.0).cov_sketch is None


def test_header_constant_prototypes_and_the_unchanged_layout():
    from lmc_atomi_amd import _capi
    with open(os.path.join(ROOT, "include", "lmc_atomi.h")) as f:
        text = f.read()
    m = re.search(r"#define\s+LMC_MAX_COV_PROBES\s+(\d+)", text)
    assert m and int(m.group(1)) == _capi.MAX_COV_PROBES == 32
    flat = re.sub(r"\s+", " ", text)
    for proto in (
            "size_t lmc_cov_sketch_workspace_bytes(int64_t C, int32_t H, int32_t W, int32_t k);",
            "int lmc_cov_sketch(const float* x_dev, int64_t C, int32_t H, int32_t W, int32_t k, const float* probes_dev, const float* center_dev, "
            "double* y_dev, double* s_dev, double* q_dev, void* workspace_dev, void* stream);",
            "int lmc_sampler_set_cov_sketch(lmc_sampler* s, int32_t k, const float* probes_dev, const float* center_dev);",
            "int lmc_sampler_get_cov_sketch(lmc_sampler* s, double* y_dev, double* s_dev, double* q_dev, uint64_t* count, void* stream);"):
        assert proto in flat, proto
    for name in ("lmc_cov_sketch_workspace_bytes", "lmc_cov_sketch", "lmc_sampler_set_cov_sketch", "lmc_sampler_get_cov_sketch"):
        assert name in _capi.exported_symbols()
    assert _capi._SIGNATURES["lmc_cov_sketch_workspace_bytes"][0] is C.c_size_t
    code = ('#include <stdio.h>\n#include "lmc_atomi.h"\nint main(){printf("%zu %zu %zu %zu %d %d\\n", sizeof(lmc_problem), sizeof(lmc_myula_config), '
            'sizeof(lmc_ulpda_config), sizeof(lmc_sapg_config), LMC_ATOMI_ABI_VERSION, LMC_MAX_COV_PROBES);return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "s.c"), os.path.join(d, "s")
        with open(src, "w") as f:
            f.write(code)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        got = tuple(map(int, subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()))
    assert got == (200, C.sizeof(_capi.lmc_myula_config), C.sizeof(_capi.lmc_ulpda_config), C.sizeof(_capi.lmc_sapg_config), 4, 32), got
    assert C.sizeof(_capi.lmc_problem) == 200 and _capi.ABI_VERSION == 4


def test_the_library_exports_the_four_symbols_and_sizes_a_workspace():
    from lmc_atomi_amd import _capi
    lib = C.CDLL(_capi.LIB_PATH)
    fn = lib.lmc_cov_sketch_workspace_bytes
    fn.restype, fn.argtypes = _capi._SIGNATURES["lmc_cov_sketch_workspace_bytes"]
    for name in ("lmc_cov_sketch", "lmc_sampler_set_cov_sketch", "lmc_sampler_get_cov_sketch"):
        assert hasattr(lib, name)
    # T float64 and fp32 over the chains padded to 32, and one fp32 partial per slab of 2048 pixels
    assert fn(70, 72, 136, 32) == 96 * 32 * (8 + 4 + 4 * 5)
    assert fn(1, 1, 1, 1) == 32 * 32 * (8 + 4 + 4)
    for bad in ((0, 4, 4, 1), (3, 0, 4, 1), (3, 4, 4, 0), (3, 4, 4, 33)):
        assert fn(*bad) == 0

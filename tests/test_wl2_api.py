"""CPU only: the weighted Gaussian data term (LMC_DATA_WL2_* in include/lmc_atomi.h, `la.L2(weights=...)`) as far as it goes without a device -- the
constants, the unchanged layout of lmc_problem, the validation of `L2(weights=...)`, its descriptor and [2][H][W] host layout, `grad_lipschitz`, the
unweighted `L2` as it was, the refusals the C ABI makes before a device is touched, and the float64 reference of tests/_wl2_ref.py itself."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import _wl2_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LMC_E_INVALID, LMC_E_UNSUPPORTED = -1, -2
STEP_TOL = 1e-5


@pytest.fixture(scope="module")
def la():
    import lmc_atomi_amd as la
    return la


@pytest.fixture(scope="module")
def lib():
    from lmc_atomi_amd import _dev
    return _dev.lib()


# ------------------------------------------------------------------ the reference itself
def test_gradient_of_the_reference_is_the_gradient_of_its_value():
    shape = (9, 13)
    _, op, y, w, x0 = R.recipe(shape)
    ref = R.WL2Ref(op, y, w, sigma=0.7)
    x = x0[0]
    g = ref.grad(x)
    rng = np.random.default_rng(0)
    for _ in range(3):
        d = rng.standard_normal(shape)
        fd = (ref(x + 1e-4 * d) - ref(x - 1e-4 * d)) / 2e-4
        assert abs(fd - (g * d).sum()) < 1e-6 * abs(fd)        # f is quadratic: the central difference is exact up to rounding
    ones = R.WL2Ref(op, y, np.ones(shape), sigma=0.7)
    assert np.allclose(ones.grad(x), ones.grad_unweighted(x)) and np.isclose(ones(x), ones.unweighted_value(x))


@pytest.mark.parametrize("shape,data", [((20, 33), "blur5"), ((24, 150), "blur5"), ((24, 264), "blur7"), ((24, 136), "identity")])
def test_recipe_discriminates(shape, data):
    op = R.Op("identity") if data == "identity" else R.Op("blur", *R.box_kernel(int(data[4:])))
    _, op, y, w, x0 = R.recipe(shape, op=op)
    zero, d_unw, d_post, d_step, d_f = R.assert_discriminates(R.WL2Ref(op, y, w, R.SIGMA_F), x0, STEP_TOL)
    print(f"{shape} {data}: w = 0 on {zero:.2f}; gradients differ by {d_unw:.2f} / {d_post}; steps by {d_step:.2e}; energies by {d_f:.2e}")
    assert 0.15 <= zero <= 0.25 and w.max() <= 4.0 and w[w > 0].min() >= 0.25


def test_grad_lipschitz_bounds_the_difference_quotient():
    shape = (12, 17)
    _, op, y, w, x0 = R.recipe(shape)
    ref = R.WL2Ref(op, y, w, sigma=R.SIGMA_F)
    d = x0[1] - x0[0]
    assert np.linalg.norm(ref.grad(x0[1]) - ref.grad(x0[0])) <= ref.grad_lipschitz() * np.linalg.norm(d)


# ------------------------------------------------------------------ constants and layout
def header_values():
    code = ('#include <stdio.h>\n#include "lmc_atomi.h"\nint main(){printf("%d %d %zu %d\\n", LMC_DATA_WL2_IDENTITY, LMC_DATA_WL2_BLUR, sizeof(lmc_problem), '
            'LMC_ATOMI_ABI_VERSION);return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "s.c"), os.path.join(d, "s")
        open(src, "w").write(code)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        return tuple(map(int, subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()))


def test_constants_and_the_unchanged_layout():
    from lmc_atomi_amd import _capi
    assert (_capi.DATA_WL2_IDENTITY, _capi.DATA_WL2_BLUR) == (7, 8) and _capi.WL2_KINDS == (7, 8)
    assert C.sizeof(_capi.lmc_problem) == 200
    assert header_values() == (7, 8, 200, 4)
    assert _capi.ABI_VERSION == 4


# ------------------------------------------------------------------ the Python class
def test_weighted_l2_describes_itself(la):
    from lmc_atomi_amd import _capi
    shape = (8, 12)
    h, off = R.box_kernel(5)
    y = np.arange(96, dtype=np.float64).reshape(shape) % 7
    w = R.weights(shape)
    for Op, kind in [(la.Convolve2D(shape, h, offset=off), _capi.DATA_WL2_BLUR), (la.Identity(96), _capi.DATA_WL2_IDENTITY), (None, _capi.DATA_WL2_IDENTITY)]:
        for wt, b in [(w, y), (w.ravel(), y.ravel())]:
            pf = la.L2(Op=Op, b=b, sigma=2.0, weights=wt, dims=shape)
            d = pf.descriptor()
            assert d["data_kind"] == kind and d["sigma_f"] == 2.0
            yw = np.asarray(d["y"].cpu() if hasattr(d["y"], "cpu") else d["y"])
            assert yw.shape == (2,) + shape and yw.dtype == np.float32
            assert np.array_equal(yw[0], y.astype(np.float32)) and np.array_equal(yw[1], w.astype(np.float32))
            assert pf.hasgrad and tuple(pf.dims) == shape
            if kind == _capi.DATA_WL2_BLUR:
                assert d["h"] is Op.h and tuple(d["offset"]) == tuple(off)
    assert tuple(la.L2(Op=la.Identity(96), b=y.ravel(), weights=w).dims) == shape       # flat b: the shape comes from the weights
    with pytest.raises(ValueError):
        la.L2(Op=la.Identity(96), b=y.ravel(), weights=w.ravel())                          # no shape anywhere
    with pytest.raises(NotImplementedError):
        la.L2(Op=la.Identity(96), b=y, weights=w).prox(y, 1.0)


def test_weighted_l2_argument_errors(la):
    shape = (8, 12)
    y = np.ones(shape)
    Op = la.Identity(96)
    idx = np.arange(96).reshape(shape)
    for bad in (np.ones((3, 3)), np.ones(95), np.ones((12, 8)), np.where(idx == 5, -1e-3, 1.0), np.where(idx == 7, np.nan, 1.0), np.where(idx == 9, np.inf, 1.0)):
        with pytest.raises(ValueError):
            la.L2(Op=Op, b=y, weights=bad, dims=shape)
    with pytest.raises(ValueError):
        la.L2(Op=Op, b=np.where(idx == 3, np.nan, 1.0), weights=np.ones(shape), dims=shape)
    with pytest.raises(NotImplementedError):
        la.L2(Op=la.Diagonal(np.ones(shape), dims=shape), b=y, weights=np.ones(shape))
    with pytest.raises(NotImplementedError):
        la.L2(sigma=0.3, weights=np.ones(shape), dims=shape)                               # as a prior the weights have no meaning
    with pytest.raises(NotImplementedError):
        la.L2(Op=la.Gradient(shape), b=y, weights=np.ones(shape), dims=shape)
    la.L2(Op=Op, b=y, weights=np.zeros(shape), dims=shape)                                 # all pixels unobserved is a valid, if empty, term


def test_grad_lipschitz_values(la):
    shape = (8, 12)
    y = np.ones(shape)
    w = R.weights(shape)
    h = np.array([[0.5, -0.25], [0.125, 0.25]])
    blur = la.Convolve2D(shape, h, offset=(0, 0))
    assert la.L2(Op=blur, b=y, sigma=0.04, weights=w).grad_lipschitz() == pytest.approx(0.04 * w.max() * 1.125 ** 2, rel=1e-12)
    assert la.L2(Op=blur, b=y, sigma=0.04).grad_lipschitz() == pytest.approx(0.04 * 1.125 ** 2, rel=1e-12)
    assert la.L2(Op=la.Identity(96), b=y, sigma=3.0, weights=w, dims=shape).grad_lipschitz() == pytest.approx(3.0 * w.max(), rel=1e-12)
    assert la.L2(b=y.ravel(), sigma=3.0, dims=shape).grad_lipschitz() == 3.0
    ref = R.WL2Ref(R.Op("blur", h, (0, 0)), y, w, 0.04)
    assert ref.grad_lipschitz() == pytest.approx(la.L2(Op=blur, b=y, sigma=0.04, weights=w).grad_lipschitz(), rel=1e-12)


def test_l2_without_weights_is_the_object_it_was(la):
    from lmc_atomi_amd import _capi
    shape = (8, 12)
    h, off = R.box_kernel(5)
    y = np.arange(96, dtype=np.float64)
    pf = la.L2(Op=la.Convolve2D(shape, h, offset=off), b=y, sigma=2.0)
    d = pf.descriptor()
    assert set(d) == {"data_kind", "sigma_f", "y", "h", "offset"} and d["data_kind"] == _capi.DATA_BLUR and d["y"] is y and d["sigma_f"] == 2.0
    d = la.L2(Op=la.Identity(96), b=y, sigma=2.0, dims=shape).descriptor()
    assert d == {"data_kind": _capi.DATA_IDENTITY, "sigma_f": 2.0, "y": y}
    m = np.ones(shape)
    d = la.L2(Op=la.Diagonal(m, dims=shape), b=y).descriptor()
    assert set(d) == {"data_kind", "sigma_f", "y", "mask"} and d["data_kind"] == _capi.DATA_MASK
    assert la.L2(sigma=0.3).prior_descriptor() == {"prior_kind": _capi.PRIOR_L2, "prior_sigma": 0.3}
    assert la.L2(Op=la.Identity(96), b=y, weights=None, dims=shape).weights is None


# ------------------------------------------------------------------ refusals made before a device is touched
def problem(data_kind, prior_kind=3, H=16, W=24, **kw):
    from lmc_atomi_amd import _capi
    p = _capi.lmc_problem()
    p.struct_size = C.sizeof(_capi.lmc_problem)
    p.H, p.W, p.data_kind, p.sigma_f = H, W, data_kind, 1.0
    p.y_dev = 0x1000                               # never dereferenced: every call below fails before a launch
    p.prior_kind, p.prior_sigma = prior_kind, 0.3
    if prior_kind in (3, 4):
        p.tv_niter = 10
    keep = None
    if data_kind == 8:
        keep = (C.c_float * 25)(*([0.04] * 25))
        p.kh = p.kw = 5
        p.oy = p.ox = 2
        p.h_host = C.cast(keep, C.POINTER(C.c_float))
    for k, v in kw.items():
        setattr(p, k, v)
    return p, keep


def myula_config(p):
    from lmc_atomi_amd import _capi
    cfg = _capi.lmc_myula_config()
    cfg.struct_size = C.sizeof(_capi.lmc_myula_config)
    cfg.problem = p
    cfg.n_chains, cfg.tau, cfg.gamma, cfg.epsg, cfg.thin = 2, 0.1, 0.5, 1.0, 1
    return cfg


REFUSED = [dict(ncvx_kind=1, ncvx_gamma=1.0), dict(ncvx_kind=2, ncvx_gamma=1.0, ncvx_niter=5), dict(tv_rtol=1e-4), dict(tv_warm=1, tv_niter=3),
           dict(prior_kind=5), dict(step_variant=3), dict(step_variant=4), dict(step_variant=5), dict(step_variant=6), dict(step_variant=8)]


@pytest.mark.parametrize("kind", [7, 8])
@pytest.mark.parametrize("fields", REFUSED, ids=lambda f: ",".join(f"{k}={v}" for k, v in f.items()))
def test_c_abi_refuses_what_has_no_weighted_form(lib, kind, fields):
    p, keep = problem(kind, **fields)
    hnd = C.c_void_p()
    for create in (lib.lmc_myula_create, lib.lmc_mymala_create):
        rc = create(C.byref(myula_config(p)), C.byref(hnd))
        msg = lib.lmc_last_error().decode()
        assert rc == LMC_E_UNSUPPORTED and not hnd.value and "weighted" in msg, (rc, msg)
    rc = lib.lmc_skrock_create(C.byref(myula_config(p)), 3, C.c_float(0.05), C.byref(hnd))
    assert rc == LMC_E_UNSUPPORTED and not hnd.value and lib.lmc_last_error().decode(), (rc, lib.lmc_last_error().decode())
    buf = (C.c_float * (16 * 24))()
    out = (C.c_float * (16 * 24))()
    rc = lib.lmc_fused_eval(C.byref(p), buf, out, 1, C.c_float(0.0), C.c_float(-1.0), C.c_float(0.0), C.c_float(1.0), None)
    assert rc == LMC_E_UNSUPPORTED and "weighted" in lib.lmc_last_error().decode(), (rc, lib.lmc_last_error().decode())


@pytest.mark.parametrize("kind", [7, 8])
def test_c_abi_entry_points_without_a_weighted_form(lib, kind):
    from lmc_atomi_amd import _capi
    p, keep = problem(kind)
    buf = (C.c_float * (16 * 24))()
    out = (C.c_float * (16 * 24))()
    rc = lib.lmc_l2_prox(C.byref(p), buf, out, 1, C.c_float(0.5), 5, 0, None, None)
    assert rc == LMC_E_UNSUPPORTED and "weighted" in lib.lmc_last_error().decode(), (rc, lib.lmc_last_error().decode())
    u = _capi.lmc_ulpda_config()
    u.struct_size = C.sizeof(_capi.lmc_ulpda_config)
    u.problem = p
    u.n_chains, u.tau, u.mu, u.theta, u.cg_niter, u.thin = 2, 0.1, 0.1, 1.0, 5, 1
    hnd = C.c_void_p()
    rc = lib.lmc_ulpda_create(C.byref(u), C.byref(hnd))
    assert rc == LMC_E_UNSUPPORTED and not hnd.value and "weighted" in lib.lmc_last_error().decode(), (rc, lib.lmc_last_error().decode())


def test_c_abi_checks_the_weighted_problem_like_the_unweighted_one(lib):
    """The operator fields are read as for kinds 1 and 2: a missing observation or kernel is LMC_E_INVALID, and so is kind 9."""
    for kind, fields in [(7, dict(y_dev=None)), (8, dict(y_dev=None)), (9, {}), (7, dict(mask_dev=0x1000)), (8, dict(mask_dev=0x1000))]:      # (no weighted mask kind)
        p, keep = problem(kind, **fields)
        hnd = C.c_void_p()
        rc = lib.lmc_myula_create(C.byref(myula_config(p)), C.byref(hnd))
        assert rc == LMC_E_INVALID and not hnd.value, (kind, fields, rc)
    p, keep = problem(8)
    p.h_host = None
    assert lib.lmc_myula_create(C.byref(myula_config(p)), C.byref(C.c_void_p())) == LMC_E_INVALID


def test_python_refusals_before_a_device(la):
    shape = (24, 96)
    _, op, y, w, x0 = R.recipe(shape)
    pf = la.L2(Op=la.Convolve2D(shape, op.args[0], offset=op.args[1]), b=y, sigma=R.SIGMA_F, weights=w)
    with pytest.raises(NotImplementedError, match="ULPDA"):
        la.ULPDASampler(pf, la.L21(ndim=2, sigma=0.3), la.Gradient(shape), shape, n_chains=2, tau=0.1, mu=0.1)
    with pytest.raises(NotImplementedError):
        pf.prox(x0[0], 1.0)

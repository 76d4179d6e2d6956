"""CPU only: the host side of the Poisson data term (LMC_DATA_POISSON_* in include/lmc_atomi.h, `la.Poisson`): the float64 reference of the definition
(tests/_poisson_ref.py) against finite differences, the Lipschitz constant, the argument errors of the Python class, the enum values of the header
against the ctypes mirror, the unchanged layout of `lmc_problem`, and the refusals of the C ABI that are made before a device is touched.  The library
loads without a device."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import _poisson_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LMC_E_INVALID, LMC_E_UNSUPPORTED = -1, -2
SIZEOF_LMC_PROBLEM = 200          # of the commit before the Poisson term: the values are additive, the layout does not move


@pytest.fixture(scope="module")
def la():
    import lmc_atomi_amd as la
    return la


@pytest.fixture(scope="module")
def lib():
    from lmc_atomi_amd import _dev
    return _dev.lib()


# ------------------------------------------------------------------ the reference itself
def test_dphi_is_the_derivative_of_phi():
    rng = np.random.default_rng(0)
    u = np.concatenate([rng.uniform(-6, -0.05, 400), rng.uniform(0.05, 40, 400)])
    y = np.where(rng.uniform(size=u.size) < 0.25, 0.0, rng.poisson(8.0, u.size).astype(np.float64))
    beta = rng.uniform(0.3, 1.0, u.size)
    e = 1e-6
    fd = (R.phi(u + e, y, beta) - R.phi(u - e, y, beta)) / (2 * e)
    # central difference: truncation e^2 phi''' / 6 with |phi'''| <= 2 y / beta^3 (< 2e3 here) plus rounding ~ eps |phi| / e ~ 1e-8 ... 1e-7
    assert np.max(np.abs(fd - R.dphi(u, y, beta))) < 5e-7


def test_phi_is_c1_at_zero_and_zero_log_zero_is_zero():
    y = np.array([0.0, 1.0, 7.0, 30.0])
    beta = np.array([0.5, 0.3, 1.0, 0.5])
    for e in (1e-9, 1e-12):
        # across 0 the value moves by 2 e |phi'(0)| and the derivative by 2 e phi''(0) = 2 e y / beta^2 (+ rounding of values up to ~100), no jump
        assert np.all(np.abs(R.phi(-e, y, beta) - R.phi(e, y, beta)) <= 2 * e * np.abs(1 - y / beta) * 1.01 + 1e-13)
        assert np.all(np.abs(R.dphi(-e, y, beta) - R.dphi(e, y, beta)) <= 2 * e * y / beta ** 2 * 1.01 + 1e-13)
    assert np.array_equal(R.dphi(0.0, y, beta), 1.0 - y / beta)
    # y = 0: phi(u) = u + beta on both sides (linear, unbounded below), no NaN from 0 log 0
    u = np.array([-3.0, 0.0, 2.0])
    assert np.array_equal(R.phi(u, 0.0, 0.5), u + 0.5) and np.array_equal(R.dphi(u, 0.0, 0.5), np.ones(3))
    # the minimum of phi is 0 at u = y - beta
    assert abs(float(R.phi(6.5, 7.0, 0.5))) < 1e-15 and float(R.dphi(6.5, 7.0, 0.5)) == 0.0
    # convex: phi' is non-decreasing through 0
    uu = np.linspace(-5, 5, 2001)
    assert np.all(np.diff(R.dphi(uu, 7.0, 0.5)) >= 0)


@pytest.mark.parametrize("which", ["blur", "mask", "identity"])
def test_grad_lipschitz_bounds_the_difference_quotient(la, which):
    shape = (20, 33)
    h, off = R.box_kernel(5)
    if which == "blur":
        op, Op = R.Op("blur", h, off), la.Convolve2D(shape, h, offset=off)
    elif which == "mask":
        m = R.random_mask(shape)
        op, Op = R.Op("mask", m), la.Diagonal(m, dims=shape)
    else:
        op, Op = R.Op("identity"), la.Identity(shape[0] * shape[1])
    _, _, y, beta, _ = R.recipe(shape, op=op, beta=R.ramp_background(shape))
    pf_ref = R.PoissonRef(op, y, beta, sigma=1.3)
    pf = la.Poisson(Op, y, beta, sigma=1.3)
    L = pf.grad_lipschitz()
    # (the device's taps are the fp32 roundings of h: 1e-7 of the sum)
    assert L == pytest.approx(1.3 * np.max(y / beta ** 2) * (np.abs(h).sum() ** 2 if which == "blur" else 1.0), rel=1e-6)
    assert L == pytest.approx(pf_ref.grad_lipschitz(), rel=1e-6)
    L = pf_ref.grad_lipschitz()
    rng = np.random.default_rng(1)
    worst = 0.0
    for _ in range(40):
        a = rng.normal(0, 6, shape)
        b = a + rng.normal(0, rng.choice([1e-3, 0.1, 5.0]), shape)
        worst = max(worst, np.linalg.norm(pf_ref.grad(a) - pf_ref.grad(b)) / np.linalg.norm(a - b))
    assert 0 < worst <= L * (1 + 1e-12), (worst, L)


def test_gradient_of_the_reference_is_the_gradient_of_its_value():
    shape = (9, 11)
    _, op, y, beta, x0 = R.recipe(shape, n_chains=1)
    pf = R.PoissonRef(op, y, beta, sigma=0.7)
    x = x0[0]
    g = pf.grad(x)
    rng = np.random.default_rng(2)
    for _ in range(5):
        d = rng.normal(size=shape)
        e = 1e-6
        fd = (pf(x + e * d) - pf(x - e * d)) / (2 * e)
        assert abs(fd - float((g * d).sum())) <= 1e-6 * max(1.0, abs(fd))
    assert pf.grad(x.ravel()).shape == (shape[0] * shape[1],)


def test_recipe_reaches_both_branches():
    for shape in [(20, 33), (24, 264)]:
        _, op, y, beta, x0 = R.recipe(shape)
        y0, neg, pos, cond, d_unext, d_gauss = R.assert_discriminates(R.PoissonRef(op, y, beta), x0, 1e-5)
        assert 0.15 <= y0 <= 0.40 and 0.30 <= neg <= 0.60 and cond < 1.5


# ------------------------------------------------------------------ the Python class
def test_poisson_is_exported_and_describes_itself(la):
    from lmc_atomi_amd import _capi
    shape = (8, 12)
    h, off = R.box_kernel(5)
    y = np.arange(96, dtype=np.float64).reshape(shape) % 7
    for Op, kind in [(la.Convolve2D(shape, h, offset=off), _capi.DATA_POISSON_BLUR), (la.Diagonal(np.ones(shape), dims=shape), _capi.DATA_POISSON_MASK),
                     (la.Identity(96), _capi.DATA_POISSON_IDENTITY)]:
        pf = la.Poisson(Op, y, 0.5, sigma=2.0)
        d = pf.descriptor()
        assert d["data_kind"] == kind and d["sigma_f"] == 2.0
        yb = np.asarray(d["y"].cpu() if hasattr(d["y"], "cpu") else d["y"])
        assert yb.shape == (2,) + shape and yb.dtype == np.float32
        assert np.array_equal(yb[0], y.astype(np.float32)) and np.all(yb[1] == np.float32(0.5))
        assert pf.hasgrad and pf.dims == shape
    ramp = R.ramp_background(shape)
    pf = la.Poisson(la.Identity(96), y.ravel(), ramp)            # flat counts: the shape comes from the background
    assert np.array_equal(pf.background, ramp) and pf.sigma == 1.0 and pf.dims == shape
    assert la.Poisson(la.Identity(96), y.ravel(), 0.5, dims=shape).dims == shape
    with pytest.raises(ValueError):
        la.Poisson(la.Identity(96), y.ravel(), 0.5)              # no shape anywhere
    assert "Poisson" in la.__all__
    with pytest.raises(NotImplementedError):
        pf.prox(y, 1.0)


def test_poisson_argument_errors(la):
    shape = (8, 12)
    Op = la.Identity(96)
    y = np.ones(shape)
    bad_counts = [np.where(np.arange(96).reshape(shape) == 5, -1.0, 1.0), np.full(shape, np.nan), np.full(shape, np.inf)]
    for b in bad_counts:
        with pytest.raises(ValueError):
            la.Poisson(Op, b, 0.5)
    for bg in (0.0, -1.0, float("nan"), float("inf"), np.zeros(shape), np.where(np.arange(96).reshape(shape) == 7, 0.0, 0.5)):
        with pytest.raises(ValueError):
            la.Poisson(Op, y, bg)
    with pytest.raises(ValueError):
        la.Poisson(Op, y, np.ones((3, 3)))         # neither a scalar nor [H, W]
    with pytest.raises(NotImplementedError):
        la.Poisson(la.Gradient(shape), y, 0.5)
    la.Poisson(Op, np.zeros(shape), 0.5)            # all-zero counts are counts
    la.Poisson(Op, y * 0.25, 1e-3)                  # the counts need not be integers


# ------------------------------------------------------------------ header, ctypes mirror, layout
def header_values():
    code = ('#include <stdio.h>\n#include "lmc_atomi.h"\nint main(){printf("%d %d %d %d %d %d %d %zu %d\\n", LMC_DATA_NONE, LMC_DATA_IDENTITY, LMC_DATA_BLUR, '
            'LMC_DATA_MASK, LMC_DATA_POISSON_IDENTITY, LMC_DATA_POISSON_BLUR, LMC_DATA_POISSON_MASK, sizeof(lmc_problem), LMC_ATOMI_ABI_VERSION);return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "s.c"), os.path.join(d, "s")
        open(src, "w").write(code)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        return tuple(map(int, subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()))


def test_enum_values_and_the_unchanged_layout():
    from lmc_atomi_amd import _capi
    *kinds, size, abi = header_values()
    assert tuple(kinds) == (0, 1, 2, 3, 4, 5, 6)
    assert (_capi.DATA_NONE, _capi.DATA_IDENTITY, _capi.DATA_BLUR, _capi.DATA_MASK, _capi.DATA_POISSON_IDENTITY, _capi.DATA_POISSON_BLUR,
            _capi.DATA_POISSON_MASK) == tuple(kinds)
    assert _capi.POISSON_KINDS == (4, 5, 6)
    assert size == SIZEOF_LMC_PROBLEM == C.sizeof(_capi.lmc_problem)
    assert abi == 4 == _capi.ABI_VERSION
    assert [f[0] for f in _capi.lmc_problem._fields_][-3:] == ["box_enable", "box_lo", "box_hi"]


# ------------------------------------------------------------------ refusals made before a device is touched
def problem(data_kind, prior_kind=3, H=16, W=24, **kw):
    from lmc_atomi_amd import _capi
    p = _capi.lmc_problem()
    p.struct_size = C.sizeof(_capi.lmc_problem)
    p.H, p.W, p.data_kind, p.sigma_f = H, W, data_kind, 1.0
    p.y_dev = 0x1000                               # never dereferenced: every call below fails before a launch
    p.mask_dev = 0x1000
    p.prior_kind, p.prior_sigma = prior_kind, 0.3
    if prior_kind in (3, 4):
        p.tv_niter = 10
    keep = None
    if data_kind in (2, 5):
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


@pytest.mark.parametrize("kind", [4, 5, 6])
@pytest.mark.parametrize("fields", REFUSED, ids=lambda f: ",".join(f"{k}={v}" for k, v in f.items()))
def test_c_abi_refuses_what_has_no_poisson_form(lib, kind, fields):
    p, keep = problem(kind, **fields)
    hnd = C.c_void_p()
    rc = lib.lmc_myula_create(C.byref(myula_config(p)), C.byref(hnd))
    msg = lib.lmc_last_error().decode()
    assert rc == LMC_E_UNSUPPORTED and not hnd.value and "Poisson" in msg, (rc, msg)
    rc = lib.lmc_skrock_create(C.byref(myula_config(p)), 3, C.c_float(0.05), C.byref(hnd))
    assert rc == LMC_E_UNSUPPORTED and not hnd.value, (rc, lib.lmc_last_error().decode())
    buf = (C.c_float * (16 * 24))()
    out = (C.c_float * (16 * 24))()
    rc = lib.lmc_fused_eval(C.byref(p), buf, out, 1, C.c_float(0.0), C.c_float(-1.0), C.c_float(0.0), C.c_float(1.0), None)
    assert rc == LMC_E_UNSUPPORTED and "Poisson" in lib.lmc_last_error().decode(), (rc, lib.lmc_last_error().decode())


@pytest.mark.parametrize("kind", [4, 5, 6])
def test_c_abi_entry_points_without_a_poisson_form(lib, kind):
    from lmc_atomi_amd import _capi
    p, keep = problem(kind)
    buf = (C.c_float * (16 * 24))()
    out = (C.c_float * (16 * 24))()
    rc = lib.lmc_l2_prox(C.byref(p), buf, out, 1, C.c_float(0.5), 5, 0, None, None)
    assert rc == LMC_E_UNSUPPORTED and "Poisson" in lib.lmc_last_error().decode(), (rc, lib.lmc_last_error().decode())
    u = _capi.lmc_ulpda_config()
    u.struct_size = C.sizeof(_capi.lmc_ulpda_config)
    u.problem = p
    u.n_chains, u.tau, u.mu, u.theta, u.cg_niter, u.thin = 2, 0.1, 0.1, 1.0, 5, 1
    hnd = C.c_void_p()
    rc = lib.lmc_ulpda_create(C.byref(u), C.byref(hnd))
    assert rc == LMC_E_UNSUPPORTED and not hnd.value and "Poisson" in lib.lmc_last_error().decode(), (rc, lib.lmc_last_error().decode())


def test_c_abi_checks_the_poisson_problem_like_the_gaussian_one(lib):
    """The operator fields are read as for kinds 1 to 3: a missing observation, mask or kernel is LMC_E_INVALID, an unknown kind too."""
    for kind, fields in [(4, dict(y_dev=None)), (5, dict(y_dev=None)), (6, dict(mask_dev=None)), (7, {}), (-1, {})]:
        p, keep = problem(kind, **fields)
        hnd = C.c_void_p()
        rc = lib.lmc_myula_create(C.byref(myula_config(p)), C.byref(hnd))
        assert rc == LMC_E_INVALID and not hnd.value, (kind, fields, rc)
    p, keep = problem(5)
    p.h_host = None
    assert lib.lmc_myula_create(C.byref(myula_config(p)), C.byref(C.c_void_p())) == LMC_E_INVALID

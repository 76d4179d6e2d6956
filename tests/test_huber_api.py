"""CPU only: the Huber data term (LMC_DATA_HUBER_* in include/lmc_atomi.h, `la.HuberLoss`) as far as it goes without a device -- the constants and the
tables of `_capi`, the unchanged layout of lmc_problem, the validation of `HuberLoss`, its descriptors and [2][H][W] host layout, `grad_lipschitz`, and
the refusals that the C ABI and the Python surface make before a device is touched."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import _huber_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LMC_E_INVALID, LMC_E_UNSUPPORTED = -1, -2
INF = float("inf")


@pytest.fixture(scope="module")
def la():
    import lmc_atomi_amd as la
    return la


@pytest.fixture(scope="module")
def lib():
    from lmc_atomi_amd import _dev
    return _dev.lib()


# ------------------------------------------------------------------ constants and layout
def header_values():
    code = ('#include <stdio.h>\n#include "lmc_atomi.h"\nint main(){printf("%d %d %d %zu %d\\n", LMC_DATA_HUBER_IDENTITY, LMC_DATA_HUBER_BLUR, '
            'LMC_DATA_HUBER_PSF, sizeof(lmc_problem), LMC_ATOMI_ABI_VERSION);return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "s.c"), os.path.join(d, "s")
        open(src, "w").write(code)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        return tuple(map(int, subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()))


def test_constants_tables_and_the_unchanged_layout():
    from lmc_atomi_amd import _capi
    assert (_capi.DATA_HUBER_IDENTITY, _capi.DATA_HUBER_BLUR, _capi.DATA_HUBER_PSF) == (13, 14, 15) and _capi.HUBER_KINDS == (13, 14, 15)
    assert all(k in _capi.TWO_PLANE_KINDS for k in (13, 14, 15))                        # y_dev is [2][H][W] for all three
    assert 15 in _capi.PSF_KINDS and 13 not in _capi.PSF_KINDS and 14 not in _capi.PSF_KINDS
    assert not set(_capi.HUBER_KINDS) & set(_capi.WL2_KINDS + _capi.POISSON_KINDS + (_capi.DATA_SPECTRAL,))
    assert _capi.PSF_KINDS[:3] == (9, 10, 11) and _capi.WL2_KINDS == (7, 8)             # the tables of before keep their entries
    assert C.sizeof(_capi.lmc_problem) == 200
    assert header_values() == (13, 14, 15, 200, 4)
    assert _capi.ABI_VERSION == 4


# ------------------------------------------------------------------ the Python class
def test_huber_loss_describes_itself(la):
    from lmc_atomi_amd import _capi
    shape = (8, 12)
    h, off = R.box_kernel(5)
    y = np.arange(96, dtype=np.float64).reshape(shape) % 7
    d_ = R.thresholds(shape)
    assert (d_ == 0).any() and np.isinf(d_).any()
    big = np.outer(np.hanning(13), np.hanning(11)) + 0.01
    ops = [(la.Convolve2D(shape, h, offset=off), _capi.DATA_HUBER_BLUR), (la.Identity(96), _capi.DATA_HUBER_IDENTITY),
           (la.PSF(shape, big, offset=(6, 5)), _capi.DATA_HUBER_PSF)]
    for Op, kind in ops:
        for dl, b in [(d_, y), (d_.ravel(), y.ravel())]:
            pf = la.HuberLoss(Op, b, dl, sigma=2.0, dims=shape)
            d = pf.descriptor()
            assert d["data_kind"] == kind and d["sigma_f"] == 2.0
            yd = np.asarray(d["y"].cpu() if hasattr(d["y"], "cpu") else d["y"])
            assert yd.shape == (2,) + shape and yd.dtype == np.float32
            assert np.array_equal(yd[0], y.astype(np.float32)) and np.array_equal(yd[1], d_.astype(np.float32))       # (+inf and 0 as they are)
            assert pf.hasgrad and tuple(pf.dims) == shape
            if kind == _capi.DATA_HUBER_BLUR:
                assert d["h"] is Op.h and tuple(d["offset"]) == tuple(off)
            if kind == _capi.DATA_HUBER_PSF:
                assert set(Op.descriptor()) <= set(d)
    pf = la.HuberLoss(la.Identity(96), y, 4.0)                                           # a scalar threshold; the shape from b
    assert tuple(pf.dims) == shape and np.array_equal(pf.delta, np.full(shape, 4.0))
    assert np.isinf(la.HuberLoss(la.Identity(96), y, INF).delta).all()                  # the plain Gaussian term everywhere
    assert tuple(la.HuberLoss(la.Identity(96), y.ravel(), d_).dims) == shape            # flat b: the shape comes from delta
    with pytest.raises(ValueError):
        la.HuberLoss(la.Identity(96), y.ravel(), d_.ravel())                             # no shape anywhere
    assert la.HuberLoss is not la.Huber and "HuberLoss" in la.__all__


def test_huber_loss_argument_errors(la):
    shape = (8, 12)
    y = np.ones(shape)
    Op = la.Identity(96)
    idx = np.arange(96).reshape(shape)
    for bad in (np.ones((3, 3)), np.ones(95), np.ones((12, 8)), np.where(idx == 5, -1e-3, 1.0), np.where(idx == 7, np.nan, 1.0), -1.0, float("nan"),
                np.where(idx == 9, -INF, 1.0)):
        with pytest.raises(ValueError):
            la.HuberLoss(Op, y, bad, dims=shape)
    for bad_b in (np.where(idx == 3, np.nan, 1.0), np.where(idx == 3, INF, 1.0), np.ones(95)):
        with pytest.raises(ValueError):
            la.HuberLoss(Op, bad_b, 4.0, dims=shape)
    with pytest.raises(NotImplementedError, match="delta = 0"):
        la.HuberLoss(la.Diagonal(np.ones(shape), dims=shape), y, 4.0)
    with pytest.raises(NotImplementedError):
        la.HuberLoss(la.Gradient(shape), y, 4.0, dims=shape)
    with pytest.raises(NotImplementedError):
        la.HuberLoss(None, y, 4.0, dims=shape)
    with pytest.raises(NotImplementedError):
        la.HuberLoss(la.FourierSampling((8, 16), np.ones((8, 16))), np.ones((8, 16)), 4.0)
    with pytest.raises(NotImplementedError):
        la.HuberLoss(la.PeriodicConvolve2D((8, 16), np.ones((3, 3)) / 9.0), np.ones((8, 16)), 4.0)
    with pytest.raises(NotImplementedError):
        la.HuberLoss(Op, y, 4.0).prox(y, 1.0)
    la.HuberLoss(Op, y, np.zeros(shape), dims=shape)                                     # all pixels unobserved is a valid, if empty, term


def test_grad_lipschitz_values(la):
    shape = (8, 12)
    y = np.ones(shape)
    d = R.thresholds(shape)
    h = np.array([[0.5, -0.25], [0.125, 0.25]])
    blur = la.Convolve2D(shape, h, offset=(0, 0))
    assert la.HuberLoss(blur, y, d, sigma=0.04).grad_lipschitz() == pytest.approx(0.04 * 1.125 ** 2, rel=1e-12)      # no factor of delta
    assert la.HuberLoss(blur, y, d, sigma=0.04).grad_lipschitz() == la.L2(Op=blur, b=y, sigma=0.04).grad_lipschitz()
    assert la.HuberLoss(la.Identity(96), y, d, sigma=3.0).grad_lipschitz() == 3.0
    assert la.HuberLoss(la.PSF(shape, np.full((11, 11), 0.01), offset=(5, 5)), y, d, sigma=2.0).grad_lipschitz() == pytest.approx(2.0 * 1.21 ** 2, rel=1e-6)
    ref = R.HuberRef(R.Op("blur", h, (0, 0)), y, d, 0.04)
    assert ref.grad_lipschitz() == pytest.approx(la.HuberLoss(blur, y, d, sigma=0.04).grad_lipschitz(), rel=1e-12)
    # the bound holds on the reference: psi is 1-Lipschitz
    _, op, yy, dd, x0 = R.recipe((12, 17))
    r = R.HuberRef(op, yy, dd, R.SIGMA_F)
    assert np.linalg.norm(r.grad(x0[1]) - r.grad(x0[0])) <= r.grad_lipschitz() * np.linalg.norm(x0[1] - x0[0])


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
    if data_kind == 14:
        keep = (C.c_float * 25)(*([0.04] * 25))
        p.kh = p.kw = 5
        p.oy = p.ox = 2
        p.h_host = C.cast(keep, C.POINTER(C.c_float))
    if data_kind == 15:
        keep = (C.c_float * 121)(*([1.0 / 121] * 121))
        p.psf_kh = p.psf_kw = 11
        p.psf_oy = p.psf_ox = 5
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


@pytest.mark.parametrize("kind", [13, 14])
@pytest.mark.parametrize("fields", REFUSED, ids=lambda f: ",".join(f"{k}={v}" for k, v in f.items()))
def test_c_abi_refuses_what_has_no_huber_form(lib, kind, fields):
    p, keep = problem(kind, **fields)
    hnd = C.c_void_p()
    for create in (lib.lmc_myula_create, lib.lmc_mymala_create):
        rc = create(C.byref(myula_config(p)), C.byref(hnd))
        msg = lib.lmc_last_error().decode()
        assert rc == LMC_E_UNSUPPORTED and not hnd.value and "Huber" in msg, (rc, msg)
    rc = lib.lmc_skrock_create(C.byref(myula_config(p)), 3, C.c_float(0.05), C.byref(hnd))
    assert rc == LMC_E_UNSUPPORTED and not hnd.value and lib.lmc_last_error().decode(), (rc, lib.lmc_last_error().decode())
    buf = (C.c_float * (16 * 24))()
    out = (C.c_float * (16 * 24))()
    rc = lib.lmc_fused_eval(C.byref(p), buf, out, 1, C.c_float(0.0), C.c_float(-1.0), C.c_float(0.0), C.c_float(1.0), None)
    assert rc == LMC_E_UNSUPPORTED and "Huber" in lib.lmc_last_error().decode(), (rc, lib.lmc_last_error().decode())


@pytest.mark.parametrize("fields", [dict(ncvx_kind=1, ncvx_gamma=1.0), dict(tv_rtol=1e-4), dict(tv_warm=1, tv_niter=3)],
                         ids=lambda f: ",".join(f"{k}={v}" for k, v in f.items()))
def test_c_abi_refuses_on_a_large_psf_what_the_psf_refuses(lib, fields):
    p, keep = problem(15, **fields)
    hnd = C.c_void_p()
    rc = lib.lmc_myula_create(C.byref(myula_config(p)), C.byref(hnd))
    assert rc == LMC_E_UNSUPPORTED and not hnd.value and "PSF" in lib.lmc_last_error().decode(), (rc, lib.lmc_last_error().decode())


@pytest.mark.parametrize("kind", [13, 14, 15])
def test_c_abi_entry_points_without_a_huber_form(lib, kind):
    from lmc_atomi_amd import _capi
    p, keep = problem(kind)
    buf = (C.c_float * (16 * 24))()
    out = (C.c_float * (16 * 24))()
    rc = lib.lmc_l2_prox(C.byref(p), buf, out, 1, C.c_float(0.5), 5, 0, None, None)
    assert rc == LMC_E_UNSUPPORTED and "Huber" in lib.lmc_last_error().decode(), (rc, lib.lmc_last_error().decode())
    u = _capi.lmc_ulpda_config()
    u.struct_size = C.sizeof(_capi.lmc_ulpda_config)
    u.problem = p
    u.n_chains, u.tau, u.mu, u.theta, u.cg_niter, u.thin = 2, 0.1, 0.1, 1.0, 5, 1
    hnd = C.c_void_p()
    rc = lib.lmc_ulpda_create(C.byref(u), C.byref(hnd))
    assert rc == LMC_E_UNSUPPORTED and not hnd.value and "Huber" in lib.lmc_last_error().decode(), (rc, lib.lmc_last_error().decode())


def test_c_abi_checks_the_huber_problem_like_the_plain_one(lib):
    """The operator fields are read as for kinds 1, 2 and 9: a missing observation or kernel is LMC_E_INVALID, so is a mask (there is no Huber mask
    kind), and 16 is no kind."""
    cases = [(13, dict(y_dev=None)), (14, dict(y_dev=None)), (15, dict(y_dev=None)), (16, {}), (13, dict(mask_dev=0x1000)), (14, dict(mask_dev=0x1000)),
             (15, dict(mask_dev=0x1000)), (15, dict(kh=5, kw=5)), (15, dict(psf_kh=0)), (14, dict(oy=7))]
    for kind, fields in cases:
        p, keep = problem(kind, **fields)
        hnd = C.c_void_p()
        rc = lib.lmc_myula_create(C.byref(myula_config(p)), C.byref(hnd))
        assert rc == LMC_E_INVALID and not hnd.value, (kind, fields, rc, lib.lmc_last_error().decode())
    for kind in (14, 15):
        p, keep = problem(kind)
        p.h_host = None
        assert lib.lmc_myula_create(C.byref(myula_config(p)), C.byref(C.c_void_p())) == LMC_E_INVALID


def test_python_refusals_before_a_device(la):
    shape = (24, 96)
    _, op, y, d, x0 = R.recipe(shape)
    pf = la.HuberLoss(la.Convolve2D(shape, op.args[0], offset=op.args[1]), y, d, sigma=R.SIGMA_F)
    with pytest.raises(NotImplementedError, match="ULPDA"):
        la.ULPDASampler(pf, la.L21(ndim=2, sigma=0.3), la.Gradient(shape), shape, n_chains=2, tau=0.1, mu=0.1)
    pp = la.HuberLoss(la.PSF(shape, np.full((11, 11), 1.0 / 121), offset=(5, 5)), y, d, sigma=R.SIGMA_F)
    with pytest.raises(NotImplementedError, match="ULPDA"):
        la.ULPDASampler(pp, la.L21(ndim=2, sigma=0.3), la.Gradient(shape), shape, n_chains=2, tau=0.1, mu=0.1)
    with pytest.raises(NotImplementedError):
        pf.prox(x0[0], 1.0)

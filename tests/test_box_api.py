"""CPU-only: the host side of the box constraint (`lmc_problem.box_enable / box_lo / box_hi`, include/lmc_atomi.h): the three declarations of the struct
-- the header, the ctypes mirror and the stub of INTEGRATION.md -- agree in size and in the place of the new fields, no box is the default, and whatever
of the validation runs before a device is touched: the checks of `load_problem` through `lmc_fused_eval` and `lmc_myula_create`, and the Python
argument errors that are raised before a handle exists.  The library loads without a device."""
import ctypes as C
import os
import re
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


def header_layout():
    """(sizeof(lmc_problem), offsets of box_enable, box_lo, box_hi, LMC_ATOMI_ABI_VERSION) as the C compiler sees include/lmc_atomi.h"""
    code = ('#include <stdio.h>\n#include <stddef.h>\n#include "lmc_atomi.h"\nint main(){printf("%zu %zu %zu %zu %d\\n", sizeof(lmc_problem), '
            'offsetof(lmc_problem, box_enable), offsetof(lmc_problem, box_lo), offsetof(lmc_problem, box_hi), LMC_ATOMI_ABI_VERSION);return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "s.c"), os.path.join(d, "s")
        open(src, "w").write(code)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        return tuple(map(int, subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()))


def integration_stub():
    """The lmc_problem class of the binding printed in INTEGRATION.md, executed."""
    txt = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    m = re.search(r"class lmc_problem\(C\.Structure\):\n(?:    .*\n|\n)+?(?=\nclass )", txt)
    assert m, "INTEGRATION.md no longer holds the lmc_problem stub"
    ns = {"C": C}
    exec(m.group(0), ns)
    return ns["lmc_problem"]


def test_header_ctypes_and_integration_stub_agree():
    from lmc_atomi_amd import _capi
    size, o_en, o_lo, o_hi, abi = header_layout()
    assert abi == 4 == _capi.ABI_VERSION                 # the fields are appended: struct_size tells the layouts apart, the version stays
    stub = integration_stub()
    for cls in (_capi.lmc_problem, stub):
        assert C.sizeof(cls) == size, (cls, C.sizeof(cls), size)
        assert (cls.box_enable.offset, cls.box_lo.offset, cls.box_hi.offset) == (o_en, o_lo, o_hi)
        assert [f[0] for f in cls._fields_][-3:] == ["box_enable", "box_lo", "box_hi"]
    assert [f[0] for f in stub._fields_] == [f[0] for f in _capi.lmc_problem._fields_]
    # appended: every earlier field is where it was (prox_scale_pixel_stride is the last of them)
    assert o_en == _capi.lmc_problem.prox_scale_pixel_stride.offset + 4


def test_no_box_is_the_default(la):
    from lmc_atomi_amd import _capi
    assert _capi.lmc_problem().box_enable == 0
    for pg in (la.TV((8, 8)), la.TV((8, 8), isotropic=False), la.L1(), la.L2(sigma=1.0), la.Laplace(1.0), la.Huber(1.0, 1.0), la.WaveletL1((8, 8))):
        assert pg.bounds is None if hasattr(pg, "bounds") else True
        assert "box" not in pg.prior_descriptor()
    d = la.TV((8, 8), bounds=(0, 255)).prior_descriptor()
    assert d["box"] == (0.0, 255.0) and d["prior_kind"] == PRIOR_TV_ISO
    assert la.TV((8, 8), isotropic=False, bounds=(0, float("inf"))).prior_descriptor()["box"] == (0.0, float("inf"))
    assert la.Box(-1, 1).prior_descriptor() == {"prior_kind": PRIOR_NONE, "box": (-1.0, 1.0)}
    assert la.Box(-1, 1)(np.zeros(4)) == 0.0
    for pg in (la.L1(bounds=(0, 1)), la.L2(sigma=2.0, bounds=(0, 1)), la.Laplace(1.0, bounds=(0, 1)), la.Huber(1.0, 1.0, bounds=(0, 1)),
               la.Gaussian(1.0, bounds=(0, 1)), la.GenGaussian(3, 1.0, bounds=(0, 1)), la.SmoothedLaplace(1.0, bounds=(0, 1)),
               la.UncenteredLaplace(1.0, 0.5, bounds=(0, 1)), la.ElementwiseProx("chi", 1.0, bounds=(0, 1))):
        assert pg.prior_descriptor()["box"] == (0.0, 1.0)


def problem(kind, H=16, W=24, **kw):
    from lmc_atomi_amd import _capi
    p = _capi.lmc_problem()
    p.struct_size = C.sizeof(_capi.lmc_problem)
    p.H, p.W, p.prior_kind, p.prior_sigma = H, W, kind, 0.3
    if kind in (PRIOR_TV_ISO, PRIOR_TV_ANISO):
        p.tv_niter = 10
    p.box_enable, p.box_lo, p.box_hi = 1, 0.0, 255.0
    for k, v in kw.items():
        setattr(p, k, v)
    return p


NAN, INF = float("nan"), float("inf")
CASES = [
    (PRIOR_TV_ISO, dict(box_lo=5.0, box_hi=5.0), LMC_E_INVALID, "box_lo < box_hi"),
    (PRIOR_TV_ISO, dict(box_lo=7.0, box_hi=-7.0), LMC_E_INVALID, "box_lo < box_hi"),
    (PRIOR_L1, dict(box_lo=INF, box_hi=INF), LMC_E_INVALID, "box_lo < box_hi"),
    (PRIOR_L2, dict(box_lo=NAN), LMC_E_INVALID, "NaN"),
    (PRIOR_NONE, dict(box_hi=NAN), LMC_E_INVALID, "NaN"),
    (PRIOR_TV_ISO, dict(box_enable=2), LMC_E_INVALID, "box_enable"),
    (PRIOR_TV_ISO, dict(tv_niter=0), LMC_E_INVALID, "tv_niter"),
    (PRIOR_TV_ANISO, dict(tv_niter=0), LMC_E_INVALID, "tv_niter"),
    (PRIOR_HAAR_L1, dict(), LMC_E_UNSUPPORTED, "separable"),
    (PRIOR_TV_ISO, dict(tv_rtol=1e-4), LMC_E_UNSUPPORTED, "tv_rtol"),
    (PRIOR_TV_ANISO, dict(tv_rtol=1e-4), LMC_E_UNSUPPORTED, "tv_rtol"),
    (PRIOR_TV_ISO, dict(tv_warm=1, tv_niter=3), LMC_E_UNSUPPORTED, "tv_warm"),
]


@pytest.mark.parametrize("kind,fields,status,word", CASES)
def test_load_problem_checks_the_box_before_any_device_call(lib, kind, fields, status, word):
    """Through `lmc_fused_eval` (the problem is loaded before the pointers are looked at) and `lmc_myula_create` (before the device is asked for)."""
    from lmc_atomi_amd import _capi
    p = problem(kind, **fields)
    rc = lib.lmc_fused_eval(C.byref(p), None, None, 1, 0.0, 0.0, 1.0, 1.0, None)
    msg = lib.lmc_last_error().decode()
    assert rc == status and word in msg, (rc, msg)
    cfg = _capi.lmc_myula_config()
    cfg.struct_size = C.sizeof(_capi.lmc_myula_config)
    cfg.problem = p
    cfg.n_chains, cfg.tau, cfg.gamma, cfg.epsg, cfg.thin = 2, 0.1, 0.5, 1.0, 1
    hnd = C.c_void_p()
    for create in (lib.lmc_myula_create, lib.lmc_mymala_create):
        rc = create(C.byref(cfg), C.byref(hnd))
        msg = lib.lmc_last_error().decode()
        assert rc == status and word in msg and not hnd.value, (rc, msg)


@pytest.mark.parametrize("kind", [PRIOR_NONE, PRIOR_L2, PRIOR_L1, PRIOR_TV_ISO, PRIOR_TV_ANISO])
@pytest.mark.parametrize("lo,hi", [(0.0, 255.0), (0.0, INF), (-INF, 0.0), (-INF, INF)])
def test_valid_boxes_pass_the_problem_check(lib, kind, lo, hi):
    """A good box gets past `load_problem`: the call then fails on its NULL image pointers, not on the box."""
    p = problem(kind, box_lo=lo, box_hi=hi)
    rc = lib.lmc_fused_eval(C.byref(p), None, None, 1, 0.0, 0.0, 1.0, 1.0, None)
    msg = lib.lmc_last_error().decode()
    assert rc == LMC_E_INVALID and "pointers" in msg, (rc, msg)


def test_box_disabled_ignores_the_bounds(lib):
    p = problem(PRIOR_TV_ISO, box_enable=0, box_lo=NAN, box_hi=-1.0, tv_rtol=1e-4)
    rc = lib.lmc_fused_eval(C.byref(p), None, None, 1, 0.0, 0.0, 1.0, 1.0, None)
    assert rc == LMC_E_INVALID and "pointers" in lib.lmc_last_error().decode()


def test_python_argument_errors_before_a_handle_exists(la):
    shape = (16, 24)
    for bad in [(5, 5), (7, -7), (NAN, 1), (0, NAN), (1,), (1, 2, 3), "ab", 3.0]:
        for make in (lambda b: la.TV(shape, bounds=b), lambda b: la.TV(shape, isotropic=False, bounds=b), lambda b: la.L1(bounds=b),
                     lambda b: la.L2(sigma=1.0, bounds=b), lambda b: la.Laplace(1.0, bounds=b), lambda b: la.Huber(1.0, 1.0, bounds=b)):
            with pytest.raises(ValueError):
                make(bad)
    with pytest.raises(ValueError):
        la.Box(3, 1)
    with pytest.raises(ValueError):
        la.TV(shape, niter=0, bounds=(0, 1))
    for iso in (True, False):
        with pytest.raises(NotImplementedError):
            la.TV(shape, niter=10, rtol=1e-4, isotropic=iso, bounds=(0, 255))
    with pytest.raises(NotImplementedError):
        la.TV(shape, niter=3, warm=True, bounds=(0, 255))
    with pytest.raises(NotImplementedError):
        la.WaveletL1(shape, sigma=0.3, bounds=(0, 255))
    with pytest.raises(NotImplementedError):
        la.L2(b=np.zeros(shape), bounds=(0, 255))            # bounds belong to the prior
    assert la.WaveletL1(shape, sigma=0.3, bounds=None).sigma == 0.3
    # the samplers without a box form say so before they build a problem (no device here: anything later would raise RuntimeError)
    pf = la.L2(b=np.zeros(shape), sigma=1.0, dims=shape)
    pg = la.TV(shape, sigma=0.3, niter=10, bounds=(0, 255))
    kw = dict(n_chains=2, tau=0.1, gamma=0.5)
    with pytest.raises(NotImplementedError, match="MYMALA"):
        la.MYMALASampler(pf, pg, shape, **kw)
    with pytest.raises(NotImplementedError, match="SK-ROCK"):
        la.SKROCKSampler(pf, pg, shape, n_stages=5, **kw)
    with pytest.raises(NotImplementedError, match="ULPDA"):
        la.ULPDASampler(pf, la.L1(sigma=0.3, bounds=(0, 255)), la.Gradient(shape), shape, n_chains=2, tau=0.1, mu=0.1)
    with pytest.raises(NotImplementedError, match="EstimatePriorWeight"):
        la.EstimatePriorWeight(pf, pg, np.zeros(shape), 0.1, 0.5, 4, (1e-3, 1e2), dims=shape)
    with pytest.raises(NotImplementedError, match="tv_warm"):
        la.MYULASampler(pf, la.TV(shape, sigma=0.3, niter=3, bounds=(0, 255)), shape, tv_warm=True, **kw)

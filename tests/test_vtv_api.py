"""CPU only, no device: the argument checks of the vectorial TV prior and of the multi-channel sampler that precede any device call, the prior's
descriptor, the size of lmc_mch_config against the C compiler's, and the launch plan of the prox kernel (lmc_vtv_plan is host code)."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

import lmc_atomi_amd as la
from lmc_atomi_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS = (8, 12)


def test_vectorial_tv_refuses_bad_arguments():
    for nch in (0, 5, -1):
        with pytest.raises(ValueError, match="n_channels"):
            la.VectorialTV(DIMS, nch)
    for niter in (0, 65):
        with pytest.raises(ValueError, match="niter"):
            la.VectorialTV(DIMS, 3, niter=niter)
    for bounds in ((1.0, 1.0), (2.0, 1.0), (float("nan"), 1.0), (0.0,), "ab"):
        with pytest.raises(ValueError, match="bounds"):
            la.VectorialTV(DIMS, 3, bounds=bounds)
    with pytest.raises(ValueError, match="momentum"):
        la.VectorialTV(DIMS, 3, momentum="nesterov")
    pg = la.VectorialTV(DIMS, 3)
    for shape in ((2,) + DIMS, (3, 8, 11), (4, 3) + DIMS, (3 * 8 * 12 + 1,), (3, 2, 8, 11), DIMS):
        with pytest.raises(ValueError, match="operand of shape"):
            pg.prox(np.zeros(shape), 1.0)
        with pytest.raises(ValueError, match="operand of shape"):
            pg(np.zeros(shape))


def test_descriptor():
    pg = la.VectorialTV(DIMS, 3, sigma=0.3, niter=7, bounds=(0, np.inf))
    d = pg.prior_descriptor()
    assert d["prior_kind"] == _capi.PRIOR_VTV == 8
    assert d["prior_sigma"] == 0.3 and d["tv_niter"] == 7 and d["tv_step"] == 0.125 and d["n_channels"] == 3
    assert np.array_equal(d["tv_betas"], la.fgp_betas(7)) and d["box"] == (0.0, np.inf)
    assert "box" not in la.VectorialTV(DIMS, 2).prior_descriptor()
    assert _capi.MAX_CHANNELS == 4


def _terms(n, op=None, sigma=2.0, **kw):
    return [la.L2(Op=op() if op else None, b=np.full(DIMS, 10.0 * ch), sigma=sigma, dims=DIMS, **kw) for ch in range(n)]


def test_sampler_checks_its_terms_before_any_device_call():
    pg = la.VectorialTV(DIMS, 3)
    h = np.ones((3, 3)) / 9.0
    blur = lambda: la.Convolve2D(DIMS, h, offset=(1, 1))
    new = lambda pf, g=pg, **kw: la.MultichannelMYULASampler(pf, g, DIMS, tau=0.1, gamma=0.5, **kw)
    with pytest.raises(ValueError, match="2 terms for 3 channels"):
        new(_terms(2))
    with pytest.raises(ValueError, match="sequence"):
        new(la.L2(b=np.zeros(DIMS), dims=DIMS))
    with pytest.raises(ValueError, match="same operator kind"):
        new(_terms(2, blur) + _terms(1))
    with pytest.raises(ValueError, match="same sigma"):
        new(_terms(2) + _terms(1, sigma=3.0))
    other = la.L2(Op=la.Convolve2D(DIMS, np.ones((3, 3)) / 8.0, offset=(1, 1)), b=np.zeros(DIMS), sigma=2.0)
    with pytest.raises(ValueError, match="same taps and offset"):
        new(_terms(2, blur) + [other])
    shifted = la.L2(Op=la.Convolve2D(DIMS, h, offset=(0, 1)), b=np.zeros(DIMS), sigma=2.0)
    with pytest.raises(ValueError, match="same taps and offset"):
        new(_terms(2, blur) + [shifted])
    with pytest.raises(ValueError, match="weights"):
        new(_terms(2) + _terms(1, weights=np.ones(DIMS)))
    with pytest.raises(ValueError, match="observation"):
        new(_terms(2) + [la.L2(sigma=2.0, dims=DIMS)])
    pois = la.Poisson(la.Identity(DIMS[0] * DIMS[1]), np.ones(DIMS), np.ones(DIMS), dims=DIMS)
    with pytest.raises(NotImplementedError, match="Poisson"):
        new(_terms(2) + [pois])
    with pytest.raises(NotImplementedError, match="VectorialTV"):
        new(_terms(3), la.TV(DIMS))
    with pytest.raises(ValueError, match="dims"):
        la.MultichannelMYULASampler(_terms(3), la.VectorialTV((8, 16), 3), DIMS, tau=0.1, gamma=0.5)
    with pytest.raises(NotImplementedError, match="tau"):
        la.MultichannelMYULASampler(_terms(3), pg, DIMS)
    with pytest.raises(NotImplementedError, match="epsg"):
        new(_terms(3), epsg=np.ones(3))


def test_other_samplers_refuse_the_prior_before_any_device_call():
    pg = la.VectorialTV(DIMS, 1)
    pf = la.L2(b=np.zeros(DIMS), dims=DIMS)
    for make in (lambda: la.MYULASampler(pf, pg, DIMS, tau=0.1, gamma=0.5), lambda: la.MYMALASampler(pf, pg, DIMS, tau=0.1, gamma=0.5),
                 lambda: la.SKROCKSampler(pf, pg, DIMS, tau=0.1, gamma=0.5)):
        with pytest.raises(NotImplementedError, match="VectorialTV"):
            make()


def test_driver_names_what_is_not_built():
    pg = la.VectorialTV(DIMS, 3)
    run = lambda **kw: la.MoreauYosidaUnadjustedLangevin(_terms(3), pg, np.zeros((3,) + DIMS), tau=0.1, gamma=0.5, n_chains=2, **kw)
    for kw in ({"moment_scales": (2,)}, {"hist_bins": 8}, {"hist_range": (0, 1)}, {"chain_groups": 2}, {"cov_probes": np.zeros((1,) + DIMS)},
               {"cov_center": np.zeros(DIMS)}, {"quantiles": (0.5,)}, {"callback": lambda x: None}, {"diagnostics": True}):
        with pytest.raises(NotImplementedError, match=next(iter(kw))):
            run(**kw)


def test_config_size_matches_the_header():
    code = '#include <stdio.h>\n#include "lmc_atomi.h"\nint main(){printf("%zu %d %d\\n", sizeof(lmc_mch_config), LMC_MAX_CHANNELS, (int)LMC_PRIOR_VTV);return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "s.c"), os.path.join(d, "s")
        open(src, "w").write(code)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        size, nch, kind = map(int, subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split())
    assert ctypes.sizeof(_capi.lmc_mch_config) == size
    assert (_capi.MAX_CHANNELS, _capi.PRIOR_VTV) == (nch, kind)


def test_plan():
    for nch in (1, 2, 3, 4):
        for K in range(1, _capi.MAX_TV_ITERS + 1):
            th, tw, ipl, nl = _capi.vtv_plan((97, 261), nch, K)
            assert th >= 1 and tw >= 1 and ipl >= 1 and nl >= 1
            assert ipl * nl >= K and ipl * (nl - 1) < K
            assert ipl <= 10
            if K <= 10:
                assert nl == 1 and ipl == K
            assert _capi.vtv_plan((4, 4), nch, K) == (th, tw, ipl, nl)      # the image does not change the plan
    assert _capi.vtv_plan((97, 261), 3, 23)[3] > 1
    lib = _capi.load()
    null = ctypes.POINTER(ctypes.c_int32)()
    assert lib.lmc_vtv_plan(8, 8, 3, 10, null, null, null, null) == 0
    for bad in ((0, 8, 3, 10), (8, 0, 3, 10), (8, 8, 0, 10), (8, 8, 5, 10), (8, 8, 3, 0), (8, 8, 3, 65)):
        assert lib.lmc_vtv_plan(*bad, null, null, null, null) == -1, bad
        assert lib.lmc_last_error()
        with pytest.raises(_capi.LMCError):
            _capi.vtv_plan(bad[:2], bad[2], bad[3])

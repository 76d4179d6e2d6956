"""CPU-only: the surface of the split Gibbs sampler -- the header's struct size compiled from C against the binding, the exported symbols, the refusals of
lmc_sgs_create / lmc_sgs_xstep (they are decided on the host before any device call, so the library answers without a device; the pointers of the
problems below are never read) and the errors the Python classes raise before a handle exists, and the resources of the new kernels."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from _sgs_cases import FAKE, INVALID, LMC_E_INVALID, LMC_E_UNSUPPORTED, UNSUPPORTED, create, sgs_config


@pytest.fixture(scope="module")
def la():
    import lmc_atomi_amd as la
    return la


def test_config_size_symbols_and_constants():
    from lmc_atomi_amd import _capi
    code = ('#include <stdio.h>\n#include "lmc_atomi.h"\nint main(void){printf("%zu %zu %d\\n", sizeof(lmc_sgs_config), sizeof(lmc_problem), '
            'LMC_MAX_SGS_INNER);return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "s.c"), os.path.join(d, "s")
        open(src, "w").write(code)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        size, psize, inner = map(int, subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split())
    assert C.sizeof(_capi.lmc_sgs_config) == size and psize == 200 == C.sizeof(_capi.lmc_problem)
    assert inner == _capi.MAX_SGS_INNER == 16
    for name in ("create", "destroy", "set_state", "get_state", "step", "iteration", "set_iteration", "get_moments", "reset_moments", "set_chain_groups",
                 "get_group_moments", "energies", "noise", "kernel_name", "xstep"):
        assert f"lmc_sgs_{name}" in _capi.exported_symbols()


@pytest.mark.parametrize("fields,word", UNSUPPORTED, ids=[str(i) for i in range(len(UNSUPPORTED))])
def test_create_refuses_what_has_no_gaussian_conditional(la, fields, word):
    rc, msg = create(sgs_config(**fields))
    assert rc == LMC_E_UNSUPPORTED and word in msg, (rc, msg)


@pytest.mark.parametrize("fields", INVALID, ids=[str(i) for i in range(len(INVALID))])
def test_create_rejects_bad_values(la, fields):
    rc, msg = create(sgs_config(**fields))
    assert rc == LMC_E_INVALID and msg, (rc, msg)


def test_xstep_refusals(la):
    from lmc_atomi_amd import _dev
    lib = _dev.lib()
    call = lambda cfg, rho=1.0, z=FAKE, out=2 * FAKE, n=1: lib.lmc_sgs_xstep(C.byref(cfg.problem), z, None, out, n, rho, None)
    for fields, word in UNSUPPORTED[:7] + UNSUPPORTED[11:]:
        assert call(sgs_config(**fields)) == LMC_E_UNSUPPORTED and word in lib.lmc_last_error().decode()
    assert call(sgs_config(), rho=0.0) == LMC_E_INVALID
    assert call(sgs_config(), rho=float("nan")) == LMC_E_INVALID
    assert call(sgs_config(), out=FAKE) == LMC_E_INVALID          # in place
    assert call(sgs_config(), n=0) == LMC_E_INVALID
    assert call(sgs_config(data_kind=12, H=12, W=16)) == LMC_E_INVALID


def test_python_refusals_come_before_any_handle(la):
    shape = (16, 16)
    ones, img = np.ones(shape), np.zeros(shape)
    kw = dict(n_chains=2, rho=1.0, tau=0.1, gamma=0.5)
    tv = la.TV(shape, sigma=0.3, niter=10)
    refused = [
        (la.L2(Op=la.Convolve2D(shape, np.ones((5, 5)) / 25, offset=(2, 2)), b=img, sigma=1.0), tv),
        (la.L2(Op=la.PSF(shape, np.ones((9, 9)) / 81), b=img, sigma=1.0), tv),
        (la.Poisson(la.Identity(256), ones, 1.0), tv),
        (la.HuberLoss(la.Identity(256), img, 1.0, dims=shape), tv),
        (la.L2(b=img, sigma=1.0, dims=shape), la.TV(shape, sigma=0.3, niter=10, rtol=1e-4)),
        (la.L2(b=img, sigma=1.0, dims=shape), la.TV(shape, sigma=0.3, niter=3, warm=True)),
        (la.L2(b=img, sigma=1.0, dims=shape), la.VectorialTV(shape, 3, sigma=0.3, niter=10)),
    ]
    for pf, pg in refused:
        with pytest.raises(NotImplementedError):
            la.SplitGibbsSampler(pf, pg, shape, **kw)
    with pytest.raises(NotImplementedError, match="PeriodicConvolve2D"):
        la.SplitGibbsSampler(refused[0][0], tv, shape, **kw)
    with pytest.raises(NotImplementedError):
        la.SplitGibbsSampler(la.L2(b=img, sigma=1.0, dims=shape), la.L1(sigma=0.5), shape, epsg=np.ones(2), **kw)
    pf = la.L2(b=img, sigma=1.0, dims=shape)
    for bad in (dict(rho=0.0), dict(rho=float("nan")), dict(tau=-1.0), dict(tau=float("inf")), dict(gamma=0.0), dict(n_inner=0), dict(n_inner=17),
                dict(noise="dice"), dict(chain_groups=1), dict(chain_groups=65), dict(epsg=-1.0)):
        with pytest.raises(ValueError):
            la.SplitGibbsSampler(pf, tv, shape, **{**kw, **bad})
    with pytest.raises(ValueError):
        la.SplitGibbs(pf, tv, img, 1.0, 0.1, 0.5, 3, n_chains=2, chain_groups=4)      # more groups than chains


def test_step_bound(la):
    assert la.sgs_step_bound(2.0, 0.5) == pytest.approx(1.0 / (0.25 + 2.0), rel=1e-15)
    for rho, gamma in ((0.0, 1.0), (1.0, -1.0), (float("nan"), 1.0), (1.0, float("inf"))):
        with pytest.raises(ValueError):
            la.sgs_step_bound(rho, gamma)


def test_sgs_kernels_use_no_scratch():
    import kernel_resources
    from lmc_atomi_amd import _capi
    res = [r for r in kernel_resources.kernel_resources(_capi.LIB_PATH) if "sgs_" in r["demangled"]]
    import re
    names = sorted({re.search(r"(sgs_\w+(?:<[^>]*>)?)\(", r["demangled"]).group(1) for r in res})
    assert names == sorted(["sgs_cols_gibbs_kernel", "sgs_couple1_kernel", "sgs_couple4_kernel", "sgs_coupling_energy_kernel", "sgs_xdiag1_kernel<0>",
                            "sgs_xdiag1_kernel<1>", "sgs_xdiag4_kernel<0>", "sgs_xdiag4_kernel<1>", "sgs_xdiag_philox1_kernel",
                            "sgs_xdiag_philox4_kernel"]), names
    for r in res:
        print(f"{r['demangled'][:60]}: vgpr {r['vgpr']} sgpr {r['sgpr']} lds {r['lds']} scratch {r['scratch']}")
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, r
    gibbs = next(r for r in res if "sgs_cols_gibbs_kernel" in r["demangled"])
    assert gibbs["vgpr"] <= 128, gibbs     # two workgroups of 8 waves per CU are four waves per SIMD: 512 / 4 registers each, as the other FFT kernels

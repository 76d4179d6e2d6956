"""CPU only, no device: the second-order TGV prior (LMC_PRIOR_TGV) as the header, the binding and the shipped library state it -- the enum value, the
unchanged size of lmc_problem, the argument checks of `TGV` that precede any device call, the refusals the samplers make before a handle exists, and
the kernels of lmc_tgv.hip in the SHIPPED library: their names, no scratch and no spilled register, the LDS of a workgroup (read from the code-object
notes through scripts/kernel_resources.py like tests/test_radon_resources.py)."""
import ctypes
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import lmc_atomi_amd as la
from lmc_atomi_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
DIMS = (8, 12)

KERNELS = ["tgv_prox_kernel<false>", "tgv_prox_kernel<true>"]
LDS_LIMIT = 160 * 1024          # gfx950: the LDS of a CU, all of which one workgroup may take
THREADS = 1024                  # of a prox workgroup: four waves per SIMD, so at most 128 registers per lane
PATCH = 64                      # the patch is 64 x 64: eight planes of (64 + 2) x 64 floats


def test_enum_limits_and_struct_size_match_the_header():
    code = ('#include <stdio.h>\n#include "lmc_atomi.h"\nint main(){printf("%zu %d %d %d\\n", sizeof(lmc_problem), (int)LMC_PRIOR_TGV, LMC_MAX_TGV_ITERS, '
            'LMC_ATOMI_ABI_VERSION);return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "s.c"), os.path.join(d, "s")
        open(src, "w").write(code)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        size, kind, iters, abi = map(int, subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split())
    assert size == 200 == ctypes.sizeof(_capi.lmc_problem)
    assert kind == 9 == _capi.PRIOR_TGV
    assert iters == 256 == _capi.MAX_TGV_ITERS
    assert abi == 4 == _capi.ABI_VERSION


def test_launch_iters_is_host_code_and_leaves_a_tile():
    L = _capi.tgv_launch_iters()
    assert L == _capi.load().lmc_tgv_launch_iters()
    assert 1 <= L and 2 * L < PATCH, "a halo of L on both sides leaves a tile"
    assert "lmc_tgv_prox" in _capi.exported_symbols() and "lmc_tgv_launch_iters" in _capi.exported_symbols()


def test_tgv_refuses_bad_arguments():
    for alpha0 in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="alpha0"):
            la.TGV(DIMS, 1.0, alpha0=alpha0)
    for niter in (0, -3, 257):
        with pytest.raises(ValueError, match="niter"):
            la.TGV(DIMS, 1.0, niter=niter)
    for step in (0.0, -0.1, 0.3, 1.0, float("nan")):          # 12 * 0.3^2 = 1.08 > 1
        with pytest.raises(ValueError, match="step"):
            la.TGV(DIMS, 1.0, step=step)
    for bounds in ((1.0, 1.0), (2.0, 1.0), (float("nan"), 1.0), (0.0,), "ab"):
        with pytest.raises(ValueError, match="bounds"):
            la.TGV(DIMS, 1.0, bounds=bounds)
    for sigma in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="sigma"):
            la.TGV(DIMS, sigma)
    with pytest.raises(ValueError, match="dims"):
        la.TGV((0, 4), 1.0)
    la.TGV(DIMS, 1.0, step=1 / np.sqrt(12.0))          # the default, spelled out
    la.TGV(DIMS, 1.0, step=0.25, niter=256, bounds=(0, np.inf))


def test_descriptor_and_the_missing_value():
    pg = la.TGV(DIMS, sigma=0.3, alpha0=0.5, niter=17, bounds=(0, np.inf))
    d = pg.prior_descriptor()
    assert d == {"prior_kind": 9, "prior_sigma": 0.3, "tgv_niter": 17, "tgv_alpha0": 0.5, "tgv_step": 0.0, "box": (0.0, np.inf)}
    assert "box" not in la.TGV(DIMS, 1.0).prior_descriptor()
    d = la.TGV(DIMS, 1.0)
    assert (d.alpha0, d.niter, d.bounds, d.step) == (2.0, 40, None, 0.0)
    assert la.TGV(DIMS, 1.0, step=0.25).prior_descriptor()["tgv_step"] == 0.25
    with pytest.raises(NotImplementedError, match="minimisation"):
        pg(np.zeros(DIMS))
    assert "TGV" in la.__all__


def test_samplers_refuse_before_any_device_call():
    pg = la.TGV(DIMS, 1.0)
    pf = la.L2(b=np.zeros(DIMS), dims=DIMS)
    with pytest.raises(NotImplementedError, match="TGV"):
        la.MYMALASampler(pf, pg, DIMS, tau=0.1, gamma=0.5)
    with pytest.raises(NotImplementedError, match="TGV"):
        la.MoreauYosidaMetropolisAdjustedLangevin(pf, pg, np.zeros(DIMS), tau=0.1, gamma=0.5, niter=2, n_chains=2)
    with pytest.raises(NotImplementedError, match="TGV"):
        la.MYULASampler(pf, pg, DIMS, tau=0.1, gamma=0.5, epsg=np.ones(DIMS))
    with pytest.raises(NotImplementedError, match="TGV"):
        la.ULPDASampler(pf, pg, la.Gradient(DIMS), DIMS, tau=0.1, mu=0.1)
    with pytest.raises(NotImplementedError, match="TGV"):
        la.EstimatePriorWeight(pf, pg, np.zeros(DIMS), tau=0.1, gamma=0.5, n_updates=2, theta_bounds=(0.01, 10.0))
    with pytest.raises(NotImplementedError, match="bounds"):
        la.SKROCKSampler(pf, la.TGV(DIMS, 1.0, bounds=(0, 1)), DIMS, tau=0.1, gamma=0.5)
    with pytest.raises(NotImplementedError, match="LMC_PRIOR_TGV"):
        la.sapg_dimension(pg, DIMS)


def test_statistic_dimension_is_refused_with_a_reason():
    lib = _capi.load()
    p = _capi.lmc_problem()
    p.struct_size = ctypes.sizeof(_capi.lmc_problem)
    p.H, p.W, p.prior_kind = 8, 12, _capi.PRIOR_TGV
    assert lib.lmc_sapg_dimension(ctypes.byref(p), None, None) == -2
    assert b"LMC_PRIOR_TGV" in lib.lmc_last_error()
    p.prior_kind = _capi.PRIOR_VTV          # what kind 8 answers has not moved: the range check
    assert lib.lmc_sapg_dimension(ctypes.byref(p), None, None) == -1


# ------------------------------------------------------------------ the kernels in the shipped library
@pytest.fixture(scope="module")
def resources():
    import kernel_resources
    return kernel_resources.kernel_resources(_capi.LIB_PATH)


def tgv_kernels(resources):
    names = {}
    for r in resources:
        m = re.search(r"(tgv_\w+(?:<[^>]*>)?)\(", r["demangled"])
        if m:
            assert m.group(1) not in names, m.group(1)
            names[m.group(1)] = r
    return names


def test_the_kernels_are_these_two(resources):
    assert sorted(tgv_kernels(resources)) == sorted(KERNELS)


@pytest.mark.parametrize("name", KERNELS)
def test_no_scratch_no_spilled_register_and_the_lds_of_one_workgroup(resources, name):
    r = tgv_kernels(resources)[name]
    print(f"{name}: vgpr {r['vgpr']} agpr {r['agpr']} sgpr {r['sgpr']} lds {r['lds']} scratch {r['scratch']}")
    assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (name, r)
    assert r["vgpr"] + r["agpr"] <= 128, "a workgroup of 1024 lanes is four waves per SIMD"
    dynamic = 8 * (PATCH + 2) * PATCH * 4          # eight planes between two pad rows each
    print(f"{name}: static {r['lds']} + dynamic {dynamic} of {LDS_LIMIT} bytes")
    assert r["lds"] + dynamic <= LDS_LIMIT

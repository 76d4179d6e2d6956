"""CPU only: the kernels of the vectorial TV prior (lmc_vtv.hip) exist in the SHIPPED library, once each, need no scratch and no spilled register --
x and the projected dual of a lane's pixels in registers, the extrapolated dual and the primal iterate in LDS (DESIGN 3.0p "Vectorial TV") -- and the
patch the launch plan asks for fits the LDS one workgroup may have.  Read from the code-object notes of liblmc_atomi.so like tests/test_radon_resources.py."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

# template arguments: the channels, then the box
PROX = [f"vtv_prox_kernel<{n}, {b}>" for n in (1, 2, 3, 4) for b in ("false", "true")]
KERNELS = PROX + ["vtv_value_kernel", "vtv_value_sum_kernel"]
LDS_LIMIT = 160 * 1024          # gfx950: the LDS of a CU, all of which one workgroup may take
THREADS = 1024                  # of a prox workgroup: four waves per SIMD, so at most 128 registers per lane


@pytest.fixture(scope="module")
def resources():
    import kernel_resources
    from lmc_atomi_amd import _capi
    return kernel_resources.kernel_resources(_capi.LIB_PATH)


def vtv_kernels(resources):
    names = {}
    for r in resources:
        m = re.search(r"(vtv_\w+(?:<[^>]*>)?)\(", r["demangled"])
        if m:
            assert m.group(1) not in names, m.group(1)
            names[m.group(1)] = r
    return names


def test_the_kernels_are_these_ten(resources):
    assert sorted(vtv_kernels(resources)) == sorted(KERNELS)


@pytest.mark.parametrize("name", KERNELS)
def test_no_scratch_and_no_spilled_register(resources, name):
    r = vtv_kernels(resources)[name]
    print(f"{name}: vgpr {r['vgpr']} agpr {r['agpr']} sgpr {r['sgpr']} lds {r['lds']} scratch {r['scratch']}")
    assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (name, r)
    if name in PROX:
        assert r["vgpr"] + r["agpr"] <= 128, "a workgroup of 1024 lanes is four waves per SIMD"


@pytest.mark.parametrize("nch", [1, 2, 3, 4])
def test_the_planned_patch_fits_the_lds_of_a_workgroup(resources, nch):
    """Per channel three arrays (primal iterate, two dual components) of the patch between two pad rows; the patch is the tile plus the halo of the
    plan: the iterations of a launch, one more where launches are chained (a resumed launch first forms x - gamma div(state))."""
    from lmc_atomi_amd import _capi
    worst = 0
    for K in range(1, _capi.MAX_TV_ITERS + 1):
        th, tw, ipl, nl = _capi.vtv_plan((97, 261), nch, K)
        halo = ipl if nl == 1 else ipl + 1
        ph, pw = th + 2 * halo, tw + 2 * halo
        assert ph * pw % THREADS == 0, "every lane owns the same number of pixels"
        worst = max(worst, 3 * nch * (ph + 2) * pw * 4)
    for box in ("false", "true"):
        static = vtv_kernels(resources)[f"vtv_prox_kernel<{nch}, {box}>"]["lds"]
        print(f"{nch} channels, box {box}: static {static} + dynamic {worst} of {LDS_LIMIT} bytes")
        assert static + worst <= LDS_LIMIT

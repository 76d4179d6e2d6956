"""CPU only: the weighted-Gaussian instantiations of the step kernels and the energy kernel exist in the SHIPPED library, once each, with no scratch and
no spilled register.  Read from the code-object notes of liblmc_atomi.so like tests/test_poisson_resources.py."""
import itertools
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

# template arguments: <K, PXL, KT, AL>
PIPE_KERNELS = [f"myula_step_pipe_wl2{box}_kernel<10, {pxl}, {kt}, {al}>"
                for box, pxl, kt, al in itertools.product(("", "_box"), (4, 8), (0, 5, 7), ("true", "false"))]
# <NP, TV, ANISO> and <NP, ANISO>
TILE_KERNELS = [f"myula_step_tile_wl2_kernel<{np_}, {tv}>" for np_ in range(1, 9) for tv in ("false, false", "true, false", "true, true")] + \
               [f"myula_step_tile_wl2_box_kernel<{np_}, {an}>" for np_ in range(1, 9) for an in ("false", "true")]


@pytest.fixture(scope="module")
def resources():
    import kernel_resources
    from lmc_atomi_amd import _capi
    return kernel_resources.kernel_resources(_capi.LIB_PATH)


def test_there_are_twenty_four_pipe_and_forty_tile_kernels():
    assert len(set(PIPE_KERNELS)) == 24 and len(set(TILE_KERNELS)) == 40


@pytest.mark.parametrize("name", PIPE_KERNELS + TILE_KERNELS + ["energy_wl2_kernel("])
def test_weighted_kernels_exist_once_without_scratch(resources, name):
    hits = [r for r in resources if r["demangled"].startswith(name)]
    assert len(hits) == 1, f"{name}: {len(hits)} kernels in the library"
    r = hits[0]
    assert r["scratch"] == 0 and r["vgpr_spill"] == 0, (name, r["scratch"], r["vgpr_spill"])


@pytest.mark.parametrize("name", PIPE_KERNELS)
def test_pipe_kernels_keep_the_one_team_budget(resources, name):
    """eight waves per workgroup, two per SIMD: at most 256 VGPRs + AGPRs"""
    (r,) = [r for r in resources if r["demangled"].startswith(name)]
    assert r["vgpr"] + r["agpr"] <= 256, r


def test_no_other_weighted_kernel(resources):
    names = [r["demangled"] for r in resources]
    assert len([n for n in names if n.startswith("myula_step_pipe_wl2_kernel<")]) == 12
    assert len([n for n in names if n.startswith("myula_step_pipe_wl2_box_kernel<")]) == 12
    assert len([n for n in names if n.startswith("myula_step_tile_wl2_kernel<")]) == 24
    assert len([n for n in names if n.startswith("myula_step_tile_wl2_box_kernel<")]) == 16
    for r in resources:
        if "wl2" in r["demangled"].split("(")[0]:
            assert r["scratch"] == 0 and r["vgpr_spill"] == 0, r

"""CPU only: the Huber instantiations of the step kernels and the energy kernel exist in the SHIPPED library, once each, with no scratch and no spilled
register.  Read from the code-object notes of liblmc_atomi.so like tests/test_wl2_resources.py: it counts kernels and reads their resources."""
import itertools
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

# template arguments: <K, PXL, KT, AL>
PIPE_KERNELS = [f"myula_step_pipe_hub{box}_kernel<10, {pxl}, {kt}, {al}>"
                for box, pxl, kt, al in itertools.product(("", "_box"), (4, 8), (0, 5, 7), ("true", "false"))]
# <NP, TV, ANISO> and <NP, ANISO>
TILE_KERNELS = [f"myula_step_tile_hub_kernel<{np_}, {tv}>" for np_ in range(1, 9) for tv in ("false, false", "true, false", "true, true")] + \
               [f"myula_step_tile_hub_box_kernel<{np_}, {an}>" for np_ in range(1, 9) for an in ("false", "true")]


@pytest.fixture(scope="module")
def resources():
    import kernel_resources
    from lmc_atomi_amd import _capi
    return kernel_resources.kernel_resources(_capi.LIB_PATH)


def test_there_are_twenty_four_pipe_and_forty_tile_kernels():
    assert len(set(PIPE_KERNELS)) == 24 and len(set(TILE_KERNELS)) == 40


@pytest.mark.parametrize("name", PIPE_KERNELS + TILE_KERNELS + ["energy_hub_kernel("])
def test_huber_kernels_exist_once_without_scratch(resources, name):
    hits = [r for r in resources if r["demangled"].startswith(name)]
    assert len(hits) == 1, f"{name}: {len(hits)} kernels in the library"
    r = hits[0]
    assert r["scratch"] == 0 and r["vgpr_spill"] == 0, (name, r["scratch"], r["vgpr_spill"])


@pytest.mark.parametrize("name", PIPE_KERNELS)
def test_pipe_kernels_keep_the_one_team_budget(resources, name):
    """eight waves per workgroup, two per SIMD: at most 256 VGPRs + AGPRs"""
    (r,) = [r for r in resources if r["demangled"].startswith(name)]
    assert r["vgpr"] + r["agpr"] <= 256, r


def test_no_other_huber_kernel_and_the_names_stay_clear_of_the_families_of_before(resources):
    names = [r["demangled"] for r in resources]
    assert len([n for n in names if n.startswith("myula_step_pipe_hub_kernel<")]) == 12
    assert len([n for n in names if n.startswith("myula_step_pipe_hub_box_kernel<")]) == 12
    assert len([n for n in names if n.startswith("myula_step_tile_hub_kernel<")]) == 24
    assert len([n for n in names if n.startswith("myula_step_tile_hub_box_kernel<")]) == 16
    hub = [r for r in resources if "_hub_" in r["demangled"].split("(")[0].split("<")[0]]
    assert len(hub) == 69, len(hub)      # 24 + 40 + the energy kernel + the four psf_hub_kernel instantiations
    for r in hub:
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, r
        assert "aniso" not in r["demangled"].split("<")[0]
    # the families the tests of before count by prefix keep their sizes: none of them is a prefix of a Huber name
    for prefix in ("myula_step_pipe_kernel<", "myula_step_pipe_box_kernel<", "myula_step_pipe_wl2_kernel<", "myula_step_pipe_pois_kernel<",
                   "myula_step_tile_kernel<", "myula_step_tile_box_kernel<", "myula_step_tile_wl2_kernel<", "myula_step_tile_pois_kernel<", "energy_wl2_kernel("):
        assert not [r for r in hub if r["demangled"].startswith(prefix)], prefix


def test_the_large_psf_epilogues_are_a_kernel_of_their_own_name(resources):
    """psf_hub_kernel<EPI, SEP>: the residual and the energy epilogue of the Huber term, general and separable; psf_conv_kernel keeps its eighteen."""
    hub = [r for r in resources if r["demangled"].startswith("psf_hub_kernel<")]
    assert len(hub) == 4, sorted(r["demangled"] for r in hub)
    for r in hub:
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["lds"] <= 48 * 1024, r
    assert len([r for r in resources if r["demangled"].startswith("psf_conv_kernel<")]) == 18

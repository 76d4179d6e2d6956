"""CPU only: the anisotropic-prior instantiations of the pipe kernel (lmc_step_pipe_aniso.hip) exist in the SHIPPED library, once each, and need no
scratch.  They run the isotropic stage with a clamp in place of the norm, so the stages need fewer registers than their isotropic twins; the four
whose isotropic twins spill (<10, 8, 5 | 7, true, AL>: the link of a chain that carries the blur, 76-236 B per lane) hand the dual state over in the
N wave instead of the L wave (DESIGN 3.0p "Anisotropic prior").  Read from the code-object notes of liblmc_atomi.so like tests/test_rtol_wide_resources.py."""
import itertools
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

# template arguments: <K, PXL, KT, CHAIN, AL>
ANISO_KERNELS = [f"myula_step_pipe_aniso_kernel<10, {pxl}, {kt}, {chain}, {al}>"
                 for pxl, kt, chain, al in itertools.product((4, 8), (0, 5, 7), ("false", "true"), ("true", "false"))]


@pytest.fixture(scope="module")
def resources():
    import kernel_resources
    from lmc_atomi_amd import _capi
    return kernel_resources.kernel_resources(_capi.LIB_PATH)


def test_there_are_twenty_four():
    assert len(set(ANISO_KERNELS)) == 24


@pytest.mark.parametrize("name", ANISO_KERNELS)
def test_anisotropic_pipe_kernels_exist_once_without_scratch(resources, name):
    hits = [r for r in resources if r["demangled"].startswith(name)]
    assert len(hits) == 1, f"{name}: {len(hits)} kernels in the library"
    r = hits[0]
    assert r["scratch"] == 0 and r["vgpr_spill"] == 0, (name, r["scratch"], r["vgpr_spill"])


def test_two_team_form_fits_four_waves_per_simd(resources):
    """myula_step_pipe2_aniso_kernel<10, 5>: sixteen waves per workgroup, four per SIMD -- at most 128 VGPRs, no scratch"""
    hits = [r for r in resources if r["demangled"].startswith("myula_step_pipe2_aniso_kernel<10, 5>")]
    assert len(hits) == 1, hits
    r = hits[0]
    assert r["vgpr"] + r["agpr"] <= 128 and r["scratch"] == 0 and r["vgpr_spill"] == 0, r


def test_no_other_anisotropic_pipe_kernel(resources):
    names = [r["demangled"] for r in resources if r["demangled"].startswith("myula_step_pipe_aniso_kernel<")]
    assert len(names) == 24, names

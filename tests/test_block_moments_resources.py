"""CPU only: the kernels of the multi-scale moment reduction (lmc_moments_ms.hip) are in the SHIPPED library by name and need neither scratch nor LDS --
the background form has to share a compute unit with the step kernel, whose LDS is full.  Read from the code-object notes of liblmc_atomi.so like
tests/test_rtol_wide_resources.py."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

KERNELS = ["moments_ms_kernel", "moments_ms_bg_kernel", "moments_ms_generic_kernel", "block_sums_kernel"]


@pytest.fixture(scope="module")
def resources():
    import kernel_resources
    from lmc_atomi_amd import _capi
    return kernel_resources.kernel_resources(_capi.LIB_PATH)


@pytest.mark.parametrize("name", KERNELS)
def test_multi_scale_moment_kernels_exist_without_scratch_or_lds(resources, name):
    hits = [r for r in resources if r["demangled"].split("(")[0].split("::")[-1] == name]
    assert len(hits) == 1, f"{name}: {len(hits)} kernels in the library"
    r = hits[0]
    assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["lds"] == 0, (name, r["scratch"], r["vgpr_spill"], r["lds"])


def test_the_background_form_fits_beside_the_one_team_pipe_kernel(resources):
    """two 188-register waves of the one-team pipe kernel leave a SIMD's 512 registers room for a wave of at most 136"""
    r = [r for r in resources if r["demangled"].split("(")[0].split("::")[-1] == "moments_ms_bg_kernel"][0]
    assert r["vgpr"] <= 136, r["vgpr"]

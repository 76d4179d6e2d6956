"""CPU only: the kernels of the chain-group moments (lmc_group_moments.hip) are in the SHIPPED library by name, once each, and need no scratch, spill no
register and allocate no LDS -- the eight float64 sums of a thread live in registers, and the launch on the side stream has to share a compute unit with
the step kernel, whose LDS is full.  Read from the code-object notes of liblmc_atomi.so like tests/test_pixel_hist_resources.py; no instruction stream is
looked at."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

KERNELS = ["group_moments4_kernel", "group_moments1_kernel"]


@pytest.fixture(scope="module")
def resources():
    import kernel_resources
    from lmc_atomi_amd import _capi
    return kernel_resources.kernel_resources(_capi.LIB_PATH)


@pytest.mark.parametrize("name", KERNELS)
def test_group_moment_kernels_exist_without_scratch_or_lds(resources, name):
    hits = [r for r in resources if r["demangled"].split("(")[0].split("::")[-1] == name]
    assert len(hits) == 1, f"{name}: {len(hits)} kernels in the library"
    r = hits[0]
    assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["lds"] == 0, (name, r["scratch"], r["vgpr_spill"], r["lds"])


def test_the_library_holds_no_other_group_moment_kernel(resources):
    names = sorted(r["demangled"].split("(")[0].split("::")[-1] for r in resources if "group_moments" in r["demangled"])
    assert names == sorted(KERNELS), names

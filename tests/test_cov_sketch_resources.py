"""CPU only: the kernels of the covariance sketch (lmc_cov_sketch.hip) are in the SHIPPED library by name, once each -- the projection and the update in their float4 and
their scalar-load instantiations -- and need no scratch, spill no register and allocate no LDS: the MFMA operands go from global memory into the lanes and
the accumulator tiles live in registers, and the launches on the side stream have to share a compute unit with the step kernel, whose LDS is full.  Read
from the code-object notes of liblmc_atomi.so like tests/test_group_moments_resources.py; no instruction stream is looked at."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

KERNELS = ["cov_sketch_project_kernel<true>", "cov_sketch_project_kernel<false>", "cov_sketch_finish_kernel", "cov_sketch_update_kernel<true>",
           "cov_sketch_update_kernel<false>"]


def short(r):
    """`void lmc::name<args>(parameters)` -> `name<args>`"""
    return r["demangled"].split("(")[0].split("::")[-1].split(" ")[-1]


@pytest.fixture(scope="module")
def resources():
    import kernel_resources
    from lmc_atomi_amd import _capi
    return kernel_resources.kernel_resources(_capi.LIB_PATH)


@pytest.mark.parametrize("name", KERNELS)
def test_cov_sketch_kernels_exist_without_scratch_or_lds(resources, name):
    hits = [r for r in resources if short(r) == name]
    assert len(hits) == 1, f"{name}: {len(hits)} kernels in the library"
    r = hits[0]
    assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["lds"] == 0, (name, r["scratch"], r["vgpr_spill"], r["sgpr_spill"], r["lds"])


def test_the_library_holds_no_other_cov_sketch_kernel(resources):
    names = sorted(short(r) for r in resources if "cov_sketch" in r["demangled"])
    assert names == sorted(KERNELS), names


def test_the_names_stay_clear_of_the_kernel_counts_of_other_tests():
    for name in KERNELS:
        assert not any(word in name for word in ("group_moments", "pixel_hist", "box", "wl2", "pois")) and not name.startswith("myula_step"), name

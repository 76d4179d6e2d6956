"""CPU only: the instantiations of the pipe kernel that carry the per-chain early exit of the TV prox to unaligned rows and column strips (AL = false,
RT = true; lmc_step_pipe_rt.hip) exist in the SHIPPED library and need what DESIGN 3.0r records: no scratch.  Read from the code-object notes of
liblmc_atomi.so like tests/test_kernel_resources.py."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

# template arguments: <K, PXL, KT, CHAIN, WARM, AL, RT>; scratch bytes per lane as recorded in DESIGN 3.0r
NEW_KERNELS = {
    "myula_step_pipe_kernel<10, 8, 5, false, false, false, true>": 0,      # 5 x 5 blur + TV(rtol > 0), W > 256 (667 x 877: two strips)
    "myula_step_pipe_kernel<10, 8, 7, false, false, false, true>": 0,      # 6 x 6 / 7 x 7 blur
    "myula_step_pipe_kernel<10, 8, 0, false, false, false, true>": 0,      # the prox alone, up to 10 passes
    "myula_step_pipe_kernel<10, 8, 0, true, false, false, true>": 0,       # links of a chained prox (ME-TV inner prox, TV(niter > 10))
    "myula_step_pipe_kernel<10, 4, 5, false, false, false, true>": 0,      # 129 .. 255 columns, W % 4 != 0
    "myula_step_pipe_kernel<10, 4, 7, false, false, false, true>": 0,
    "myula_step_pipe_kernel<10, 4, 0, false, false, false, true>": 0,
    "myula_step_pipe_kernel<10, 4, 0, true, false, false, true>": 0,
}


@pytest.fixture(scope="module")
def resources():
    import kernel_resources
    from lmc_atomi_amd import _capi
    return kernel_resources.kernel_resources(_capi.LIB_PATH)


@pytest.mark.parametrize("name", sorted(NEW_KERNELS))
def test_unaligned_exit_kernels_exist_and_use_the_recorded_scratch(resources, name):
    hits = [r for r in resources if r["demangled"].startswith(name)]
    assert len(hits) == 1, f"{name}: {len(hits)} kernels in the library"
    r = hits[0]
    assert r["scratch"] == NEW_KERNELS[name] and r["vgpr_spill"] == 0, (name, r["scratch"], r["vgpr_spill"])


def test_every_per_chain_exit_kernel_is_one_of_the_sixteen(resources):
    """aligned one-strip kernels (round 3) + the any-width ones: nothing else carries RT = true"""
    rt = [r["demangled"] for r in resources if r["demangled"].startswith("myula_step_pipe_kernel<") and r["demangled"].split(">")[0].endswith(", true")]
    assert len(rt) == 16, rt

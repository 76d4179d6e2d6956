"""CPU only: the register budget that lets the side-stream moment reduction share a SIMD with the two-team pipe kernel.

A workgroup of `myula_step_pipe2_kernel` / `myula_step_pipe2_aniso_kernel` puts four waves on every SIMD, and the reduction that runs under it
on the side stream (`moments4_bg_kernel`) gets a wave in only where its registers fit beside those four: a SIMD of gfx950 has 512 VGPRs per lane
(accumulation registers included), handed out in blocks of 8.  So 4 x VGPRs(two-team kernel) + VGPRs(moments4_bg_kernel) <= 512, and neither may
use scratch.  At 120 VGPRs per wave the reduction waited for whole CUs and the step went from 1.80 to 2.08 ms.
Read from the code-object notes of liblmc_atomi.so (scripts/kernel_resources.py), like tests/test_kernel_resources.py."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

SIMD_VGPRS = 512      # per lane
GRANULE = 8           # allocation block


@pytest.fixture(scope="module")
def resources():
    import kernel_resources
    from lmc_atomi_amd import _capi
    return kernel_resources.kernel_resources(_capi.LIB_PATH)


def regs(r):
    n = r["vgpr"] + r["agpr"]
    return (n + GRANULE - 1) // GRANULE * GRANULE


def one(resources, prefix):
    hits = [r for r in resources if r["demangled"].startswith(prefix)]
    assert len(hits) == 1, (prefix, [r["demangled"] for r in hits])
    return hits[0]


def two_team_kernels(resources):
    return [r for r in resources if r["demangled"].startswith("myula_step_pipe2")]


def test_both_two_team_kernels_are_in_the_library(resources):
    names = sorted(r["demangled"].split("(")[0] for r in two_team_kernels(resources))
    assert names == ["myula_step_pipe2_aniso_kernel<10, 5>", "myula_step_pipe2_kernel<10, 5>"], names


def test_reduction_wave_fits_beside_four_two_team_waves(resources):
    bg = one(resources, "moments4_bg_kernel(")
    for r in two_team_kernels(resources):
        total = 4 * regs(r) + regs(bg)
        print(f"{r['demangled'].split('(')[0]}: 4 x {regs(r)} + {regs(bg)} = {total} of {SIMD_VGPRS}")
        assert total <= SIMD_VGPRS, (r["demangled"], regs(r), regs(bg), total)


def test_register_budgets(resources):
    """the budgets the sum above is made of: 112 per two-team wave, 64 for the reduction"""
    bg = one(resources, "moments4_bg_kernel(")
    assert regs(bg) <= 64, bg
    for r in two_team_kernels(resources):
        assert regs(r) <= 112, r


def test_no_scratch(resources):
    for r in two_team_kernels(resources) + [one(resources, "moments4_bg_kernel(")]:
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, r

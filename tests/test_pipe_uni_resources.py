"""CPU only: the uniform-box instantiations of the pipe step kernel (lmc_step_pipe_uni.hip) exist in the SHIPPED library, once each, and the two-team
one keeps the register budget of `myula_step_pipe2_kernel` beside the side-stream moment reduction (tests/test_pipe2_budget.py): at most 112 VGPRs per
wave in allocation blocks of 8, no scratch, no spilled register, 4 x its registers + those of `moments4_bg_kernel` <= 512 per lane of a SIMD.  Read from
the code-object notes of liblmc_atomi.so (scripts/kernel_resources.py)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

SIMD_VGPRS = 512      # per lane
GRANULE = 8           # allocation block
TWO_TEAM = "myula_step_pipe_uni2_kernel<10, 5>"
ONE_TEAM = ["myula_step_pipe_uni_kernel<10, 8, 5>", "myula_step_pipe_uni_kernel<10, 4, 5>"]


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


def test_the_uniform_kernels_are_in_the_library_once_each(resources):
    names = sorted(r["demangled"].split("(")[0] for r in resources if r["demangled"].startswith("myula_step_pipe_uni"))
    assert names == sorted(ONE_TEAM + [TWO_TEAM]), names


def test_two_team_kernel_keeps_the_budget(resources):
    r = one(resources, TWO_TEAM)
    bg = one(resources, "moments4_bg_kernel(")
    total = 4 * regs(r) + regs(bg)
    print(f"{TWO_TEAM}: {r['vgpr']} + {r['agpr']} registers, 4 x {regs(r)} + {regs(bg)} = {total} of {SIMD_VGPRS}")
    assert regs(r) <= 112, r
    assert r["scratch"] == 0 and r["vgpr_spill"] == 0, r
    assert total <= SIMD_VGPRS, (regs(r), regs(bg), total)


@pytest.mark.parametrize("name", ONE_TEAM)
def test_one_team_twins_have_no_scratch(resources, name):
    r = one(resources, name)
    assert r["scratch"] == 0 and r["vgpr_spill"] == 0, r

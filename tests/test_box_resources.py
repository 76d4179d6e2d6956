"""CPU only: the box-constrained instantiations of the pipe kernel (lmc_step_pipe_box.hip) exist in the SHIPPED library, once each, and need no scratch:
the clamp of the primal iterate is one instruction per pixel and stage on a value the stage holds anyway.  The four whose unconstrained twins spill
(<10, 8, 5 | 7, true, AL>: the link of a chain that carries the blur) hand the dual state over in the N wave instead of the L wave, as the anisotropic
kernels do (DESIGN 3.0p "Box constraint", which records 0 B of scratch and no spilled register for all 25).  Read from the code-object notes of
liblmc_atomi.so like tests/test_rtol_wide_resources.py."""
import itertools
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

SCRATCH_LIMIT = 256          # bytes per lane: the library's fence (tests/test_kernel_resources.py)
RECORDED_SCRATCH = 0         # DESIGN 3.0p "Box constraint": every instantiation

# template arguments: <K, PXL, KT, CHAIN, AL>
BOX_KERNELS = [f"myula_step_pipe_box_kernel<10, {pxl}, {kt}, {chain}, {al}>"
               for pxl, kt, chain, al in itertools.product((4, 8), (0, 5, 7), ("false", "true"), ("true", "false"))] + ["myula_step_pipe_box2_kernel<10, 5>"]


@pytest.fixture(scope="module")
def resources():
    import kernel_resources
    from lmc_atomi_amd import _capi
    return kernel_resources.kernel_resources(_capi.LIB_PATH)


def test_there_are_twenty_five():
    assert len(set(BOX_KERNELS)) == 25 and RECORDED_SCRATCH <= SCRATCH_LIMIT


@pytest.mark.parametrize("name", BOX_KERNELS)
def test_box_pipe_kernels_exist_once_with_the_recorded_scratch(resources, name):
    hits = [r for r in resources if r["demangled"].startswith(name)]
    assert len(hits) == 1, f"{name}: {len(hits)} kernels in the library"
    r = hits[0]
    assert r["vgpr_spill"] == 0 and r["scratch"] == RECORDED_SCRATCH, (name, r["scratch"], r["vgpr_spill"])


def test_two_team_form_fits_four_waves_per_simd(resources):
    """myula_step_pipe_box2_kernel<10, 5>: sixteen waves per workgroup, four per SIMD -- at most 128 VGPRs"""
    (r,) = [r for r in resources if r["demangled"].startswith("myula_step_pipe_box2_kernel<10, 5>")]
    assert r["vgpr"] + r["agpr"] <= 128, r
    # ... and, like the other two-team kernels (tests/test_pipe2_budget.py), leaves room for a wave of the side-stream moment reduction on the SIMD:
    # registers come in blocks of 8, a SIMD has 512 per lane
    (bg,) = [q for q in resources if q["demangled"].startswith("moments4_bg_kernel(")]
    regs = lambda q: (q["vgpr"] + q["agpr"] + 7) // 8 * 8
    assert regs(r) <= 112 and 4 * regs(r) + regs(bg) <= 512, (regs(r), regs(bg))


def test_no_other_box_pipe_kernel_and_the_tile_and_elementwise_forms(resources):
    names = [r["demangled"] for r in resources]
    assert len([n for n in names if n.startswith("myula_step_pipe_box_kernel<")]) == 24
    assert len([n for n in names if n.startswith("myula_step_pipe_box2_kernel<")]) == 1
    # the tile kernel's box forms: NP = 1 .. 8, either form of the prior, beside the sixteen (+ eight anisotropic) kernels of before under their old names
    assert sorted(n.split("(")[0] for n in names if n.startswith("myula_step_tile_box_kernel<")) == \
        sorted(f"myula_step_tile_box_kernel<{np_}, {an}>" for np_ in range(1, 9) for an in ("false", "true"))
    assert len([n for n in names if n.startswith("myula_step_tile_kernel<")]) == 24
    assert len([n for n in names if n.startswith("box_prior_prox_kernel(")]) == 1
    for r in resources:
        if "box" in r["demangled"].split("(")[0]:
            assert r["scratch"] == 0 and r["vgpr_spill"] == 0, r

"""CPU only: what the use-once cache policy and the role priorities of the two-team step kernels must keep, read from
the shipped library (scripts/kernel_resources.py), as tests/test_pipe2_budget.py does.

* The side-stream moment reduction `moments4_bg_kernel` and every two-team kernel have no scratch and no spill.
* The headline's budget: four waves of `myula_step_pipe_uni2_kernel<10, 5>` (VGPRs in blocks of 8) and one of the reduction fit the 512 VGPRs per lane of
  a SIMD, so that a reduction wave gets in beside a workgroup's four.
* The gate.  The change reaches `myula_step_pipe2_kernel<10, 5>`, `myula_step_pipe_box2_kernel<10, 5>`, `myula_step_pipe_uni2_kernel<10, 5>` and
  `moments4_bg_kernel`.  Every other pipe kernel -- all one-team kernels and the anisotropic two-team kernel, whose code is pinned by
  tests/test_pipe_fold_resources.py -- and the in-line reductions `moments4_kernel` and `moments_kernel` keep the instruction streams of the commit before
  (78c8cda): tests/golden/stream_policy_gated_code_hashes.txt is `scripts/kernel_resources.py --code-hash` of that commit for those 213 functions, built
  with ROCm 7.2.0 (hashes of the compiler's output: a new compiler moves all of them, and the list is then made again from the commit before)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
GATED = os.path.join(ROOT, "tests", "golden", "stream_policy_gated_code_hashes.txt")

SIMD_VGPRS = 512      # per lane
GRANULE = 8           # allocation block
REACHED = ("myula_step_pipe2_kernel<", "myula_step_pipe_box2_kernel<", "myula_step_pipe_uni2_kernel<")
TWO_TEAM = REACHED + ("myula_step_pipe2_aniso_kernel<",)


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


def test_no_scratch_and_no_spill(resources):
    for prefix in TWO_TEAM + ("moments4_bg_kernel(",):
        r = one(resources, prefix)
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, r


def test_reduction_wave_fits_beside_four_waves_of_the_headline_kernel(resources):
    step, bg = one(resources, "myula_step_pipe_uni2_kernel<10, 5>("), one(resources, "moments4_bg_kernel(")
    total = 4 * regs(step) + regs(bg)
    print(f"4 x {regs(step)} + {regs(bg)} = {total} of {SIMD_VGPRS}")
    assert total <= SIMD_VGPRS, (regs(step), regs(bg))


def test_gated_kernels_keep_the_parents_code():
    import kernel_resources
    from lmc_atomi_amd import _capi
    now = dict(kernel_resources.code_hashes(_capi.LIB_PATH))
    want = dict(reversed(line.rstrip("\n").split(" ", 1)) for line in open(GATED))
    assert len(want) == 213
    assert not [n for n in want if n.startswith(REACHED) or n.startswith("moments4_bg_kernel(")]
    assert "myula_step_pipe2_aniso_kernel<10, 5>(StepArgs)" in want and "moments4_kernel(float const*, int, unsigned long, int, double*, double*)" in want
    pipe_now = sorted(n for n in now if n.startswith("myula_step_pipe") and not n.startswith(REACHED))
    assert pipe_now == sorted(n for n in want if n.startswith("myula_step_pipe")), sorted(set(pipe_now) ^ set(n for n in want if n.startswith("myula_step_pipe")))
    moved = sorted(n for n in want if now.get(n) != want[n])
    assert not moved, moved

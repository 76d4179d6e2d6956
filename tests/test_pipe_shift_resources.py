"""CPU only: what folding the wave shifts into the differences that use them (pipe_shift, sub_left_pair / right_pair_sub / pipe_cdown;
lmc_step_pipe_kernel.h) must keep, read from the shipped library (scripts/kernel_resources.py) and from the assembly of lmc_step_pipe_uni.hip.

* Budgets.  tests/golden/pipe_shift_parent_resources.txt lists every pipe kernel the change reaches (the 67 kernels with the folded momentum -- fixed
  count, cold start, isotropic -- that pipe_shift lets through) with the commit before's (df46979) VGPR block of 8, scratch bytes and spilled VGPRs: none may gain a block, scratch or a spill.
  The two-team kernels keep 112 VGPRs in blocks of 8 with no scratch and no spill, the side-stream moment reduction its 64 (tests/test_pipe2_budget.py),
  and no kernel whose name starts with myula_step_pipe_uni or myula_step_pipe2 is new.
* The gate.  The 34 folded kernels pipe_shift keeps out -- the 32 seven-tap ones and myula_step_pipe_kernel<2, {4, 8}, 0, false, false, true, false> --
  keep the instruction streams of the commit before: tests/golden/pipe_shift_gated_code_hashes.txt is `scripts/kernel_resources.py --code-hash` of
  that commit for them (ROCm 7.2.0; hashes of the compiler's output, as in tests/test_pipe_fold_resources.py).
* Static T-role bound.  `hipcc -S` of lmc_step_pipe_uni.hip with the Makefile's flags for that file, counted by scripts/isa_loops.py on
  myula_step_pipe_uni2_kernel<10, 5>: the TV roles are the loops with 8 transcendental instructions per tick (two stages of 4 pixels).  VALU
  instructions per tick and wave, commit before (same script, ROCm 7.2.0), left team / right team:
      general TV wave  82.7 / 85.7      first-stage wave T1  68.4 / 71.2
  The bound: every general TV role at least 4 VALU instructions per tick below the commit before, T1 at least 3 below.  Measured with the change: 76.7 / 76.7 and 62.7 / 63.7.
  The figures are of the compiler's output, like the code hashes of tests/test_pipe_fold_resources.py: a new compiler needs the parent counted again.
  Skipped where hipcc is absent."""
import ast
import os
import re
import shutil
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
GOLDEN = os.path.join(ROOT, "tests", "golden", "pipe_shift_parent_resources.txt")
GATED = os.path.join(ROOT, "tests", "golden", "pipe_shift_gated_code_hashes.txt")
GRANULE = 8
TWO_TEAM = ["myula_step_pipe2_kernel<10, 5>", "myula_step_pipe_box2_kernel<10, 5>", "myula_step_pipe_uni2_kernel<10, 5>"]
PINNED_NAMES = ["myula_step_pipe2_aniso_kernel<10, 5>", "myula_step_pipe2_kernel<10, 5>", "myula_step_pipe_uni2_kernel<10, 5>",
                "myula_step_pipe_uni_kernel<10, 4, 5>", "myula_step_pipe_uni_kernel<10, 8, 5>"]
# VALU per tick of the commit before, in the order the roles appear in the kernel: (general, T1) of one team, then of the other
PARENT_T_VALU = [82.7, 68.4, 85.7, 71.2]
MARGIN = [4.0, 3.0, 4.0, 3.0]
VALU = ("valu_pk", "valu_trans", "valu_dpp", "valu_mov", "valu_plain", "valu_int64")


def blocks(r):
    return (r["vgpr"] + r["agpr"] + GRANULE - 1) // GRANULE * GRANULE


@pytest.fixture(scope="module")
def resources():
    import kernel_resources
    from lmc_atomi_amd import _capi
    return {r["demangled"].split("(")[0]: r for r in kernel_resources.kernel_resources(_capi.LIB_PATH)}


def golden():
    rows = {}
    for line in open(GOLDEN):
        if line.strip() and not line.startswith("#"):
            b, s, sp, name = line.rstrip("\n").split(" ", 3)
            rows[name] = (int(b), int(s), int(sp))
    return rows


def test_no_reached_kernel_gains_a_register_block_scratch_or_a_spill(resources):
    want = golden()
    assert len(want) == 67
    worse = []
    for name, (b, s, sp) in sorted(want.items()):
        r = resources[name]
        if blocks(r) > b or r["scratch"] > s or r["vgpr_spill"] > sp:
            worse.append((name, (b, s, sp), (blocks(r), r["scratch"], r["vgpr_spill"])))
    assert not worse, worse


def test_gated_kernels_keep_the_parents_code():
    import kernel_resources
    from lmc_atomi_amd import _capi
    now = dict(kernel_resources.code_hashes(_capi.LIB_PATH))
    want = dict(reversed(line.rstrip("\n").split(" ", 1)) for line in open(GATED))
    assert len(want) == 34
    assert sum(", 7" in n for n in want) == 32
    moved = sorted(n for n in want if now.get(n) != want[n])
    assert not moved, moved


@pytest.mark.parametrize("name", TWO_TEAM)
def test_two_team_kernels_keep_112_registers_and_no_scratch(resources, name):
    r = resources[name]
    print(f"{name}: {r['vgpr']} + {r['agpr']} registers -> {blocks(r)}")
    assert blocks(r) <= 112, r
    assert r["scratch"] == 0 and r["vgpr_spill"] == 0, r


def test_moment_reduction_keeps_64_registers(resources):
    hits = [r for n, r in resources.items() if n.startswith("moments4_bg_kernel")]
    assert hits
    for r in hits:
        assert blocks(r) <= 64 and r["scratch"] == 0, r


def test_no_new_pinned_kernel_name(resources):
    now = sorted(n for n in resources if n.startswith("myula_step_pipe_uni") or n.startswith("myula_step_pipe2"))
    assert now == PINNED_NAMES, now


def t_roles(listing):
    """VALU per tick of the TV roles of an isa_loops.py listing, in order of appearance: per loop start the shortest loop, 8 transcendentals per tick."""
    first = {}
    for line in listing.splitlines():
        m = re.match(r"loop \[(\d+),(\d+)\].*per tick: (\{.*\})", line)
        if m:
            first.setdefault(int(m.group(1)), ast.literal_eval(m.group(3)))
    return [round(sum(c.get(k, 0.0) for k in VALU), 1) for _, c in sorted(first.items()) if c.get("valu_trans") == 8.0 and "valu_int64" not in c]


def test_tv_roles_are_below_the_parent():
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    csrc = os.path.join(ROOT, "lmc_atomi_amd", "csrc")
    with tempfile.TemporaryDirectory() as d:
        asm = os.path.join(d, "uni.s")
        subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-munsafe-fp-atomics", "-I" + os.path.join(ROOT, "include"), "-I" + csrc,
                        "-S", "--cuda-device-only", os.path.join(csrc, "lmc_step_pipe_uni.hip"), "-o", asm], check=True, capture_output=True)
        listing = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "isa_loops.py"), asm, "myula_step_pipe_uni2_kernel"],
                                 check=True, capture_output=True, text=True).stdout
    got = t_roles(listing)
    print("TV roles, VALU per tick:", got, "parent:", PARENT_T_VALU)
    assert len(got) == 4, listing
    for g, p, m in zip(got, PARENT_T_VALU, MARGIN):
        assert g <= p - m + 1e-9, (got, PARENT_T_VALU)

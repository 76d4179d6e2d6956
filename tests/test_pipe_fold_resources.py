"""CPU only: what folding the FGP momentum into the projection scale (pipe_stage<..., FOLD>, lmc_step_pipe_kernel.h) must leave alone, read from the
code objects of the shipped library (scripts/kernel_resources.py), and the host table the folded kernels read (lmc_tv_fold.h).

* The two two-team kernels that run folded stages, `myula_step_pipe2_kernel<10, 5>` and `myula_step_pipe_uni2_kernel<10, 5>`, keep the budget that lets a
  wave of the side-stream moment reduction in beside four of theirs (tests/test_pipe2_budget.py): at most 112 VGPRs in blocks of 8, no scratch, no spill.
* The pipe kernels WITHOUT the fold -- links of a chained prox and the warm dual (CHAIN, WARM), the per-chain early exit (RT), the anisotropic prior --
  keep the instruction streams of the commit before the fold (932ab8f): tests/golden/pipe_unfolded_code_hashes.txt is
  `scripts/kernel_resources.py --code-hash` of that commit for those 89 kernels, built with ROCm 7.2.0 (the hashes are of the compiler's output: a new
  compiler moves all of them, and the list is then made again from a build without `FOLD`).
* The table (1 + beta_k, c_k = beta_k / (1 + beta_{k-1}), c_1 = 0) for K = 10 against the same numbers formed in float64 from the checker's momentum
  sequence.  Tolerance: the table is formed in double from the float32 beta_k the kernels would read and rounded once, so 1 + beta_k is off by at most
  half an ulp of beta_k (< 2^-25) plus half an ulp of the result (2^-24 relative): 2^-23 relative covers it; c_k carries the relative errors of both
  beta_k and 1 + beta_{k-1} (2^-24 and 2^-25) and its own rounding (2^-24): 2^-22 relative covers it.  With the momentum off the factors are exactly 1 and 0."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from oracle import lmc_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
GOLDEN = os.path.join(ROOT, "tests", "golden", "pipe_unfolded_code_hashes.txt")

GRANULE = 8
TWO_TEAM_FOLDED = ["myula_step_pipe2_kernel<10, 5>", "myula_step_pipe_uni2_kernel<10, 5>"]


@pytest.fixture(scope="module")
def resources():
    import kernel_resources
    from lmc_atomi_amd import _capi
    return kernel_resources.kernel_resources(_capi.LIB_PATH)


@pytest.fixture(scope="module")
def hashes():
    import kernel_resources
    from lmc_atomi_amd import _capi
    return dict(kernel_resources.code_hashes(_capi.LIB_PATH))


@pytest.mark.parametrize("name", TWO_TEAM_FOLDED)
def test_two_team_kernels_keep_112_registers_and_no_scratch(resources, name):
    hits = [r for r in resources if r["demangled"].startswith(name + "(")]
    assert len(hits) == 1, (name, [r["demangled"] for r in hits])
    r = hits[0]
    n = (r["vgpr"] + r["agpr"] + GRANULE - 1) // GRANULE * GRANULE
    print(f"{name}: {r['vgpr']} + {r['agpr']} registers -> {n}")
    assert n <= 112, r
    assert r["scratch"] == 0 and r["vgpr_spill"] == 0, r


def unfolded(name):
    """CHAIN, WARM, RT or ANISO, from a pipe kernel's demangled name."""
    base, args = name.split("<")[0], [a.strip() for a in name.split("<")[1].split(">")[0].split(",")]
    if "aniso" in base:
        return True
    if base == "myula_step_pipe_kernel":        # <K, PXL, KT, CHAIN, WARM, AL, RT>
        return args[3] == "true" or args[4] == "true" or args[6] == "true"
    if base == "myula_step_pipe_box_kernel":    # <K, PXL, KT, CHAIN, AL>
        return args[3] == "true"
    return False


def test_unfolded_kernels_keep_the_parents_code(hashes):
    golden = dict(reversed(line.rstrip("\n").split(" ", 1)) for line in open(GOLDEN))
    assert len(golden) == 89
    now = {n: h for n, h in hashes.items() if n.startswith("myula_step_pipe") and unfolded(n)}
    assert sorted(now) == sorted(golden), sorted(set(now) ^ set(golden))
    moved = sorted(n for n in golden if now[n] != golden[n])
    assert not moved, moved


def host_table(betas):
    """lmc::tv_fold_table of the float32 `betas`, through a small program (the header is plain C++)."""
    b = np.asarray(betas, dtype=np.float32)
    code = ('#include <cstdio>\n#include "lmc_tv_fold.h"\nint main() {\n  const float b[] = {%s};\n  float t[2 * %d];\n'
            '  const bool ok = lmc::tv_fold_table(b, %d, t);\n  std::printf("%%d\\n", (int)ok);\n'
            '  for (int i = 0; i < 2 * %d; ++i) std::printf("%%.9g\\n", (double)t[i]);\n  return 0;\n}\n'
            % (", ".join("(float)%.17g" % v for v in b), len(b), len(b), len(b)))      # (a float32 prints exactly in 17 digits)
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "t.cpp"), os.path.join(d, "t")
        open(src, "w").write(code)
        subprocess.run(["g++", "-std=c++17", "-I", os.path.join(ROOT, "lmc_atomi_amd", "csrc"), src, "-o", exe], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
    return bool(int(out[0])), np.array(out[1:], dtype=np.float64).reshape(len(b), 2)


@pytest.mark.parametrize("momentum", ["unlocbox", "fista"])
def test_host_table_against_the_checkers_sequence(momentum):
    K = 10
    beta = np.asarray(O.fgp_betas(K, momentum), dtype=np.float64)
    ok, tab = host_table(beta)
    assert ok
    want_s = 1.0 + beta
    want_c = np.concatenate([[0.0], beta[1:] / (1.0 + beta[:-1])])
    es, ec = np.abs(tab[:, 0] - want_s) / want_s, np.abs(tab[:, 1] - want_c) / np.maximum(want_c, 1e-300)
    print(f"{momentum}: 1 + beta max rel {es.max():.2e} (2^-23 = {2.0 ** -23:.2e}); c max rel {ec.max():.2e} (2^-22 = {2.0 ** -22:.2e})")
    assert np.all(es <= 2.0 ** -23), es
    assert tab[0, 1] == 0.0
    assert np.all(ec[want_c > 0] <= 2.0 ** -22), ec
    assert np.all(tab[want_c == 0, 1] == 0.0)


def test_host_table_with_the_momentum_off():
    ok, tab = host_table(O.fgp_betas(10, "none"))
    assert ok
    assert np.all(tab[:, 0] == 1.0) and np.all(tab[:, 1] == 0.0), tab


def test_host_table_refuses_a_factor_of_zero():
    ok, _ = host_table([0.0, 0.25, -1.0, 0.5])
    assert not ok

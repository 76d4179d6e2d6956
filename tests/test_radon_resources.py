"""CPU only: the kernels of the Radon operator (lmc_radon.hip) exist in the SHIPPED library, once each, and need no scratch and no spilled register:
the forward kernel holds its eight partial sums and the per-angle constants in registers and sends out-of-tile candidates to a sentinel instead of
keeping a predicate per candidate (DESIGN 3.0p "Radon operator").  Read from the code-object notes of liblmc_atomi.so like tests/test_box_resources.py."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

# template argument: RadonEpi (lmc_launch.h) -- forward: raw, four residuals, four energies; adjoint: raw, subtract, overwrite
KERNELS = [f"radon_fwd_kernel<{e}>" for e in range(9)] + [f"radon_adj_kernel<{e}>" for e in (0, 9, 10)] + ["radon_energy_finish_kernel"]
LDS_LIMIT = 64 * 1024


@pytest.fixture(scope="module")
def resources():
    import kernel_resources
    from lmc_atomi_amd import _capi
    return kernel_resources.kernel_resources(_capi.LIB_PATH)


def radon_kernels(resources):
    names = {}
    for r in resources:
        m = re.search(r"(radon_\w+(?:<[^>]*>)?)\(", r["demangled"])
        if m:
            assert m.group(1) not in names, m.group(1)
            names[m.group(1)] = r
    return names


def test_the_kernels_are_these_thirteen(resources):
    assert sorted(radon_kernels(resources)) == sorted(KERNELS)


@pytest.mark.parametrize("name", KERNELS)
def test_no_scratch_and_no_spilled_register(resources, name):
    r = radon_kernels(resources)[name]
    print(f"{name}: vgpr {r['vgpr']} sgpr {r['sgpr']} lds {r['lds']} scratch {r['scratch']}")
    assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (name, r)
    assert r["lds"] == 0, "all LDS of the forward kernel is dynamic (its base stays 16-byte aligned)"


def test_forward_kernel_fits_two_workgroups_per_cu(resources):
    """Two workgroups of four waves share a CU's LDS (62 KiB each): two waves per SIMD, at most 256 registers per lane."""
    for name, r in radon_kernels(resources).items():
        if name.startswith("radon_fwd_kernel"):
            assert r["vgpr"] + r["agpr"] <= 256, (name, r)

"""CPU-only: the surface of the Daubechies wavelet-l1 prior -- descriptors, the SAPG dimension, the argument errors raised before any device handle
exists, the unchanged layout of lmc_problem, and the resources of the new kernels.  The library loads without a device."""
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

LMC_E_INVALID, LMC_E_UNSUPPORTED = -1, -2


@pytest.fixture(scope="module")
def la():
    import lmc_atomi_amd as la
    return la


def test_default_still_describes_the_block_haar_prior(la):
    from lmc_atomi_amd import _capi
    w = la.WaveletL1((16, 24), 0.4)
    assert w.prior_descriptor() == {"prior_kind": _capi.PRIOR_HAAR_L1, "prior_sigma": 0.4}
    assert la.WaveletL1((16, 24), 0.4, levels=3, wavelet="haar").prior_descriptor() == w.prior_descriptor()


def test_new_descriptors_carry_p_and_levels(la):
    from lmc_atomi_amd import _capi
    assert _capi.PRIOR_WAVELET_L1 == 7
    for name, p in (("db1", 1), ("db2", 2), ("db3", 3), ("db4", 4)):
        for L in (1, 2):
            d = la.WaveletL1((16, 24), 0.7, levels=L, wavelet=name).prior_descriptor()
            assert d == {"prior_kind": 7, "prior_sigma": 0.7, "wavelet_p": p, "wavelet_levels": L}
    assert la.WaveletL1((16, 24), 1.0, levels=2, wavelet="haar").prior_descriptor()["prior_kind"] == 7         # haar at another depth: the general transform
    assert la.WaveletL1((16, 24), 1.0, levels=3, wavelet="db1").prior_descriptor()["prior_kind"] == 7          # db1 always takes it
    # the two parameters ride in tv_niter and eprox_kind of the structure (the part of it that needs no device: the SAPG dimension's problem)
    from lmc_atomi_amd import algs
    c = algs._stat_problem(la.WaveletL1((16, 24), 0.7, levels=2, wavelet="db3"), (16, 24))
    assert (c.prior_kind, c.tv_niter, c.eprox_kind) == (7, 2, 3)


def test_sapg_dimension(la):
    assert la.sapg_dimension(la.WaveletL1((16, 24), levels=2, wavelet="db2")) == (384 - 24, 1.0)
    assert la.sapg_dimension(la.WaveletL1((16, 24), levels=1, wavelet="db4")) == (384 - 96, 1.0)
    assert la.sapg_dimension(la.WaveletL1((16, 24))) == (384 - 6, 1.0)              # the block-Haar prior, as before


def test_value_errors(la):
    for kw in (dict(wavelet="db5"), dict(wavelet="sym4"), dict(levels=0), dict(levels=9), dict(wavelet="db2", levels=4),      # 24 % 16
               dict(wavelet="db4", levels=3)):                                                                                     # 16 >> 2 = 4 < 8
        with pytest.raises(ValueError):
            la.WaveletL1((16, 24), **kw)
    with pytest.raises(ValueError):
        la.WaveletL1((6, 8), wavelet="db4", levels=1)           # 6 < 2p
    with pytest.raises(ValueError):
        la.WaveletL1((12, 16))                                  # the default needs multiples of 8, as before
    with pytest.raises(ValueError):
        la.Wavelet2D((16, 24), "db2", 4)
    with pytest.raises(ValueError):
        la.Wavelet2D((16, 24), "coif1", 1)
    la.WaveletL1((8, 8), wavelet="db4", levels=1)               # the smallest legal shape for db4
    la.WaveletL1((32, 40), wavelet="db4", levels=3)             # the coarsest input is exactly 2p


def test_not_implemented_errors(la):
    with pytest.raises(NotImplementedError):
        la.WaveletL1((16, 24), bounds=(0.0, 1.0))
    with pytest.raises(NotImplementedError):
        la.WaveletL1((16, 24), wavelet="db2", bounds=(0.0, 1.0))
    pg = la.WaveletL1((16, 24), wavelet="db2", levels=2)
    pf = la.L2(b=np.zeros((16, 24)), sigma=1.0, dims=(16, 24))
    with pytest.raises(NotImplementedError):
        la.UnadjustedLangevinPrimalDual(np.zeros(384), pf, pg, la.Gradient((16, 24)), 2, 0.1, 0.1, dims=(16, 24))
    with pytest.raises(NotImplementedError):
        la.MYULASampler(pf, pg, (16, 24), n_chains=2, tau=0.1, epsg=np.ones(384))


def test_refusals_keep_to_the_block_haar_kind(la):
    """`_refuse_term` goes on refusing LMC_PRIOR_HAAR_L1 and lets the new kind through."""
    from lmc_atomi_amd import _capi, algs
    haar = la.WaveletL1((16, 24)).prior_descriptor()
    db2 = la.WaveletL1((16, 24), wavelet="db2", levels=2).prior_descriptor()
    for kind in (_capi.DATA_POISSON_IDENTITY, _capi.DATA_WL2_IDENTITY, _capi.DATA_HUBER_IDENTITY):
        with pytest.raises(NotImplementedError):
            algs._refuse_term({"data_kind": kind}, haar, {})
        algs._refuse_term({"data_kind": kind}, db2, {})


def header_values():
    code = ('#include <stdio.h>\n#include "lmc_atomi.h"\nint main(){printf("%d %zu %d %d %d\\n", LMC_PRIOR_WAVELET_L1, sizeof(lmc_problem), '
            'LMC_ATOMI_ABI_VERSION, LMC_MAX_WAVELET_LEVELS, LMC_PRIOR_EPROX);return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "s.c"), os.path.join(d, "s")
        open(src, "w").write(code)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        return tuple(map(int, subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()))


def test_constants_and_the_unchanged_layout():
    from lmc_atomi_amd import _capi
    assert header_values() == (7, 200, 4, 8, 6)
    assert C.sizeof(_capi.lmc_problem) == 200 and _capi.ABI_VERSION == 4 and _capi.MAX_WAVELET_LEVELS == 8
    assert _capi.PRIOR_WAVELET_L1 == 7
    assert _capi.WAVELETS == {"haar": 1, "db1": 1, "db2": 2, "db3": 3, "db4": 4}


def test_library_refuses_bad_wavelet_problems_on_the_host(la):
    """lmc_sapg_dimension is host code: the range check of prior_kind and the preconditions of the new kind, without a device."""
    from lmc_atomi_amd import _capi, _dev
    lib = _dev.lib()

    def dim(kind, H, W, levels, p):
        q = _capi.lmc_problem()
        q.struct_size = C.sizeof(_capi.lmc_problem)
        q.H, q.W, q.prior_kind, q.tv_niter, q.eprox_kind = H, W, kind, levels, p
        d, k = C.c_double(), C.c_double()
        return lib.lmc_sapg_dimension(C.byref(q), C.byref(d), C.byref(k)), d.value, k.value

    assert dim(7, 16, 24, 2, 2) == (0, 360.0, 1.0)
    assert dim(7, 256, 256, 5, 4) == (0, 65536.0 - 64.0, 1.0)
    assert dim(8, 16, 24, 2, 2)[0] == LMC_E_INVALID                 # past the last kind
    for levels, p in ((0, 2), (9, 1), (2, 0), (2, 5), (4, 2), (3, 4)):
        assert dim(7, 16, 24, levels, p)[0] == LMC_E_INVALID, (levels, p)


def test_wavelet_kernels_use_no_scratch():
    import kernel_resources
    from lmc_atomi_amd import _capi
    res = kernel_resources.kernel_resources(_capi.LIB_PATH)
    names = {}
    for r in res:
        m = re.search(r"(wav_\w+(?:<[^>]*>)?)\(", r["demangled"])
        if m:
            names[m.group(1)] = r
    want = [f"wav_fwd_kernel<{p}, {m}>" for p in (1, 2, 3, 4) for m in (0, 1, 2)] + [f"wav_inv_kernel<{p}>" for p in (1, 2, 3, 4)] + ["wav_value_sum_kernel"]
    assert sorted(names) == sorted(want), sorted(names)
    for n, r in names.items():
        print(f"{n}: vgpr {r['vgpr']} sgpr {r['sgpr']} lds {r['lds']} scratch {r['scratch']}")
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (n, r)
        assert r["lds"] <= 40960, (n, r["lds"])          # four workgroups per CU (160 KiB): 16 waves, four per SIMD

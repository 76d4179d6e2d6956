"""CPU-only: the surface of the Fourier-domain data term -- the header constants compiled from C and the unchanged layout of lmc_problem, the folded
planes of lmc_spectral_tables (host code) against the numpy fold, the descriptors, the argument errors raised before any device handle exists, and the
resources of the new kernels.  The library loads without a device."""
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import _fourier_ref as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

LMC_E_INVALID, LMC_E_UNSUPPORTED = -1, -2


@pytest.fixture(scope="module")
def la():
    import lmc_atomi_amd as la
    return la


def header_values():
    code = ('#include <stdio.h>\n#include "lmc_atomi.h"\nint main(void){printf("%d %zu %d %d\\n", (int)LMC_DATA_SPECTRAL, sizeof(lmc_problem), '
            'LMC_ATOMI_ABI_VERSION, (int)LMC_DATA_WL2_PSF);return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "s.c"), os.path.join(d, "s")
        open(src, "w").write(code)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        return tuple(map(int, subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()))


def test_constants_and_the_unchanged_layout():
    from lmc_atomi_amd import _capi
    assert header_values() == (12, 200, 4, 11)
    assert C.sizeof(_capi.lmc_problem) == 200 and _capi.ABI_VERSION == 4
    assert _capi.DATA_SPECTRAL == 12 and _capi.SPECTRAL_PLANES == 11 and (_capi.FFT_MIN, _capi.FFT_MAX) == (8, 1024)
    for name in ("lmc_rfft2", "lmc_irfft2", "lmc_spectral_filter", "lmc_spectral_tables"):
        assert name in _capi.exported_symbols()


@pytest.mark.parametrize("shape", [(8, 8), (16, 64), (64, 16)], ids=["8x8", "16x64", "64x16"])
def test_spectral_tables_match_the_numpy_fold(la, shape):
    from lmc_atomi_amd.operators import spectral_tables
    rng = np.random.default_rng(shape[1])
    G = rng.normal(size=shape) + 1j * rng.normal(size=shape)
    b = 30 * (rng.normal(size=shape) + 1j * rng.normal(size=shape))
    got = spectral_tables(G, b)
    want = F.tables(G, b)
    assert got.shape == want.shape == (11, shape[0], shape[1] // 2 + 1) and got.dtype == np.float32
    for p in range(11):
        scale = np.max(np.abs(want[p]))
        assert np.max(np.abs(got[p] - want[p])) <= 1e-6 * scale, p
    for j in (0, shape[1] // 2):      # the self-conjugate columns: the second residual is zeroed, exactly
        assert not got[7:, :, j].any()
    assert got[7:, :, 1:shape[1] // 2].any()


def test_spectral_tables_refuse_bad_arguments(la):
    from lmc_atomi_amd import _dev
    lib = _dev.lib()
    z = np.zeros(2 * 16 * 16)
    out = np.zeros(11 * 16 * 9, dtype=np.float32)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    assert lib.lmc_spectral_tables(dp(z), dp(z), 16, 16, _dev.fptr(out)) == 0
    assert lib.lmc_spectral_tables(None, dp(z), 16, 16, _dev.fptr(out)) == LMC_E_INVALID
    assert lib.lmc_spectral_tables(dp(z), dp(z), 0, 16, _dev.fptr(out)) == LMC_E_INVALID
    for H, W in ((12, 16), (16, 4), (2048, 16)):
        assert lib.lmc_spectral_tables(dp(z), dp(z), H, W, _dev.fptr(out)) == LMC_E_UNSUPPORTED
        assert lib.lmc_last_error()


def test_descriptors_and_lipschitz_constant(la):
    from lmc_atomi_amd import _capi
    m = F.step_problem("wmask-l1")
    pf = la.L2(Op=la.FourierSampling((16, 64), m.mask), b=m.y, sigma=m.sigma_f, weights=m.weights)
    assert pf.grad_lipschitz() == pytest.approx(F.SpectralRef(m.G, m.b, m.sigma_f).grad_lipschitz(), rel=1e-12)
    assert pf.dims == (16, 64) and pf._spectral["tab"].shape == (11, 16, 33)
    assert np.max(np.abs(pf._spectral["tab"] - F.tables(m.G, m.b))) <= 1e-6 * np.max(np.abs(F.tables(m.G, m.b)))
    # a periodic blur makes the same descriptor: G the DFT of the wrapped kernel, b = F(observation)
    p = F.step_problem("periodic15-aniso")
    pc = la.L2(Op=la.PeriodicConvolve2D((64, 64), p.h, offset=p.offset), b=p.y, sigma=p.sigma_f)
    t = F.tables(p.G, p.b)
    assert np.max(np.abs(pc._spectral["tab"] - t)) <= 1e-6 * np.max(np.abs(t))
    assert pc.grad_lipschitz() == pytest.approx(p.sigma_f * np.max(np.abs(p.G)) ** 2, rel=1e-9)
    assert _capi.DATA_SPECTRAL not in _capi.PSF_KINDS + _capi.TWO_PLANE_KINDS


def test_value_errors(la):
    ones = np.ones((16, 32))
    for dims in ((12, 16), (16, 4), (2048, 16), (16, 24)):
        with pytest.raises(ValueError):
            la.FourierSampling(dims, np.ones(dims))
        with pytest.raises(ValueError):
            la.PeriodicConvolve2D(dims, np.ones((3, 3)))
        with pytest.raises(ValueError):
            la.rfft2(np.zeros(dims, dtype=np.float32))
        with pytest.raises(ValueError):
            la.irfft2(np.zeros((dims[0], dims[1] // 2 + 1), dtype=np.complex64), dims)
    with pytest.raises(ValueError):
        la.FourierSampling((16, 32), np.ones((16, 17)))                 # the half plane is not the full plane
    with pytest.raises(ValueError):
        la.FourierSampling((16, 32), -ones)
    with pytest.raises(ValueError):
        la.FourierSampling((16, 32), np.where(np.eye(16, 32) > 0, np.nan, 1.0))
    with pytest.raises(ValueError):
        la.FourierSampling((16, 32), ones * (1 + 0j))
    with pytest.raises(ValueError):
        la.FourierSampling((16, 32), ones, transfer=np.ones((16, 17)))
    with pytest.raises(ValueError):
        la.L2(Op=la.FourierSampling((16, 32), ones), b=np.zeros((16, 32)), sigma=1.0)              # a real b
    with pytest.raises(ValueError):
        la.L2(Op=la.FourierSampling((16, 32), ones), b=np.zeros((16, 17), dtype=complex), sigma=1.0)
    with pytest.raises(ValueError):
        la.L2(Op=la.FourierSampling((16, 32), ones), b=np.zeros((16, 32), dtype=complex), sigma=1.0, weights=-ones)
    with pytest.raises(ValueError):
        la.L2(Op=la.FourierSampling((16, 32), ones), b=np.zeros((16, 32), dtype=complex), sigma=1.0, weights=np.ones((16, 17)))
    with pytest.raises(ValueError):
        la.PeriodicConvolve2D((16, 32), np.ones((17, 3)))               # larger than the image
    with pytest.raises(ValueError):
        la.PeriodicConvolve2D((16, 32), np.ones((3, 3)), offset=(3, 0))
    with pytest.raises(ValueError):
        la.L2(Op=la.PeriodicConvolve2D((16, 32), np.ones((3, 3))), b=np.zeros((16, 32), dtype=complex), sigma=1.0)
    with pytest.raises(ValueError):
        la.irfft2(np.zeros((16, 32), dtype=np.complex64), (16, 32))
    la.PeriodicConvolve2D((16, 32), np.ones((16, 32)))                  # as large as the image


def test_not_implemented_errors(la):
    ones = np.ones((16, 32))
    fs = la.FourierSampling((16, 32), ones)
    pc = la.PeriodicConvolve2D((16, 32), np.ones((3, 3)) / 9)
    with pytest.raises(NotImplementedError):
        la.Poisson(fs, ones, 1.0)
    with pytest.raises(NotImplementedError):
        la.Poisson(pc, ones, 1.0)
    for op in (fs, pc):
        with pytest.raises(NotImplementedError):
            la.L2_ncvx_tv((16, 32), Op=op, Op2=la.Gradient((16, 32)), b=ones)
    from lmc_atomi_amd import _capi, algs
    d = {"data_kind": _capi.DATA_SPECTRAL}
    algs._refuse_spectral(d, {"prior_kind": _capi.PRIOR_TV_ISO}, {})
    algs._refuse_spectral({"data_kind": _capi.DATA_PSF}, {"tv_rtol": 1e-4}, {}, ("X", "y"))
    for prior, opts, who in (({"tv_rtol": 1e-4}, {}, None), ({"tv_warm": True}, {}, None), ({}, {"tv_warm": True}, None), ({}, {}, ("MYMALA", "why"))):
        with pytest.raises(NotImplementedError):
            algs._refuse_spectral(d, prior, opts, who)


def test_fft_kernels_use_no_scratch():
    import kernel_resources
    from lmc_atomi_amd import _capi
    res = kernel_resources.kernel_resources(_capi.LIB_PATH)
    names = {}
    for r in res:
        m = re.search(r"(fft_\w+(?:<[^>]*>)?)\(", r["demangled"])
        if m:
            names[m.group(1)] = r
    want = (["fft_rows_fwd_kernel", "fft_value_finish_kernel"] + [f"fft_rows_inv_kernel<{e}>" for e in range(3)]
            + [f"fft_cols_spectral_kernel<{m}>" for m in range(6)])
    assert sorted(names) == sorted(want), sorted(names)
    for n, r in names.items():
        print(f"{n}: vgpr {r['vgpr']} sgpr {r['sgpr']} lds {r['lds']} scratch {r['scratch']}")
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (n, r)

"""CPU-only: the surface of the multi-coil SENSE data term -- the header constants compiled from C and the unchanged layout of lmc_problem, the two new
symbols, the descriptor planes, lmc_sense_lipschitz (host code) against the numpy bound, the argument errors raised before any device handle exists,
the loud failure without a device, and the resources of the new kernels.  The library loads without a device."""
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import _sense_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

LMC_E_INVALID, LMC_E_UNSUPPORTED = -1, -2
DIMS, NC = (16, 32), 3


@pytest.fixture(scope="module")
def la():
    import lmc_atomi_amd as la
    return la


def op_and_data(la, dims=DIMS, n_coils=NC, wkind="weighted"):
    m = S.problem(dims, n_coils, wkind)
    return la.MultiCoilFourierSampling(dims, m.S, m.M), m


def header_values():
    code = ('#include <stdio.h>\n#include "lmc_atomi.h"\nint main(void){printf("%d %d %zu %d %d\\n", (int)LMC_DATA_SENSE, LMC_MAX_COILS, sizeof(lmc_problem), '
            'LMC_ATOMI_ABI_VERSION, (int)LMC_DATA_HUBER_RADON);return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "s.c"), os.path.join(d, "s")
        open(src, "w").write(code)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        return tuple(map(int, subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()))


def test_constants_and_the_unchanged_layout():
    from lmc_atomi_amd import _capi
    assert header_values() == (20, 32, 200, 4, 19)
    assert C.sizeof(_capi.lmc_problem) == 200 and _capi.ABI_VERSION == 4
    assert _capi.DATA_SENSE == 20 and _capi.MAX_COILS == 32
    assert _capi.DATA_SENSE not in _capi.PSF_KINDS + _capi.TWO_PLANE_KINDS + _capi.RADON_KINDS


def test_new_symbols_are_declared_exported_and_bound():
    from lmc_atomi_amd import _capi
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lmc_atomi.h")).read(), flags=re.S)
    raw = C.CDLL(_capi.LIB_PATH)
    for name in ("lmc_sense_apply", "lmc_sense_lipschitz"):
        assert re.search(rf"\b{name}\s*\(", header), name
        assert hasattr(raw, name), name
        assert name in _capi.exported_symbols()


def test_descriptor_planes(la):
    op, m = op_and_data(la)
    assert op.n_coils == NC and op.kspace_shape == (NC,) + DIMS and op.shape == (NC * 16 * 32, 16 * 32) and op.dims == DIMS
    head = op.descriptor()
    assert head.shape == (1 + 2 * NC,) + DIMS and head.dtype == np.float32
    np.testing.assert_array_equal(head[0], m.M)
    full = op.descriptor(m.b)
    assert full.shape == (1 + 4 * NC,) + DIMS and full.dtype == np.float32
    for c in range(NC):
        np.testing.assert_array_equal(full[1 + 2 * c], m.S[c].real)
        np.testing.assert_array_equal(full[2 + 2 * c], m.S[c].imag)
        np.testing.assert_array_equal(full[1 + 2 * NC + 2 * c], m.b[c].real)
        np.testing.assert_array_equal(full[2 + 2 * NC + 2 * c], m.b[c].imag)
    np.testing.assert_array_equal(op.descriptor(m.b.ravel()), full)      # a flat b
    pf = la.L2(Op=op, b=m.b, sigma=m.sigma_f)
    d = pf.descriptor()
    from lmc_atomi_amd import _capi
    assert d["data_kind"] == _capi.DATA_SENSE and d["n_coils"] == NC and d["sigma_f"] == m.sigma_f and pf.dims == DIMS
    ones = la.MultiCoilFourierSampling(DIMS, m.S)                        # the default mask
    assert np.array_equal(ones.mask, np.ones(DIMS, dtype=np.float32))


@pytest.mark.parametrize("name", S.IDS[:5])
def test_lipschitz_matches_the_numpy_bound(la, name):
    c = S.case(name)
    op, m = op_and_data(la, c.shape, c.n_coils)
    want = S.term(m).norm_bound()
    assert op.norm_bound() == pytest.approx(want, rel=1e-12)
    assert la.L2(Op=op, b=m.b, sigma=m.sigma_f).grad_lipschitz() == pytest.approx(m.sigma_f * want, rel=1e-12)


def test_lipschitz_refuses_bad_arguments(la):
    from lmc_atomi_amd import _dev
    lib = _dev.lib()
    d = np.ones((3, 8, 8), dtype=np.float32)
    assert lib.lmc_sense_lipschitz(_dev.fptr(d), 8, 8, 1) == 2.0                      # M = 1, S = 1 + i
    assert lib.lmc_sense_lipschitz(None, 8, 8, 1) == LMC_E_INVALID and lib.lmc_last_error()
    assert lib.lmc_sense_lipschitz(_dev.fptr(d), 0, 8, 1) == LMC_E_INVALID
    assert lib.lmc_sense_lipschitz(_dev.fptr(d), 8, 8, 0) == LMC_E_INVALID
    assert lib.lmc_sense_lipschitz(_dev.fptr(d), 8, 8, 33) == LMC_E_INVALID


def test_value_errors(la):
    m = S.problem(DIMS, NC, "weighted")
    for dims in ((12, 16), (16, 4), (2048, 16), (16, 24)):
        with pytest.raises(ValueError):
            la.MultiCoilFourierSampling(dims, np.ones((2,) + dims, dtype=complex))
    with pytest.raises(ValueError):
        la.MultiCoilFourierSampling(DIMS, np.ones((0,) + DIMS, dtype=complex))                   # no coil
    with pytest.raises(ValueError):
        la.MultiCoilFourierSampling(DIMS, np.ones((33,) + DIMS, dtype=complex))
    la.MultiCoilFourierSampling(DIMS, np.ones((32,) + DIMS, dtype=complex))
    with pytest.raises(ValueError):
        la.MultiCoilFourierSampling(DIMS, np.ones(DIMS, dtype=complex))                          # one map without the coil axis
    with pytest.raises(ValueError):
        la.MultiCoilFourierSampling(DIMS, np.ones((2, 16, 17), dtype=complex))
    with pytest.raises(ValueError):
        la.MultiCoilFourierSampling(DIMS, np.where(np.arange(2)[:, None, None] == 1, np.nan, np.ones((2,) + DIMS)) + 0j)
    with pytest.raises(ValueError):
        la.MultiCoilFourierSampling(DIMS, m.S, mask=-np.ones(DIMS))
    with pytest.raises(ValueError):
        la.MultiCoilFourierSampling(DIMS, m.S, mask=np.where(np.eye(*DIMS) > 0, np.inf, 1.0))
    with pytest.raises(ValueError):
        la.MultiCoilFourierSampling(DIMS, m.S, mask=np.ones((16, 17)))
    with pytest.raises(ValueError):
        la.MultiCoilFourierSampling(DIMS, m.S, mask=np.ones(DIMS) * (1 + 0j))
    op = la.MultiCoilFourierSampling(DIMS, m.S, m.M)
    with pytest.raises(ValueError):
        la.L2(Op=op, b=np.zeros((NC,) + DIMS), sigma=1.0)                                        # a real b
    with pytest.raises(ValueError):
        la.L2(Op=op, b=np.zeros((NC - 1,) + DIMS, dtype=complex), sigma=1.0)
    with pytest.raises(ValueError):
        la.L2(Op=op, b=np.zeros(DIMS + (NC,), dtype=complex), sigma=1.0)                         # the coil axis last
    with pytest.raises(ValueError):
        la.L2(Op=op, b=np.full((NC,) + DIMS, np.nan + 0j), sigma=1.0)
    with pytest.raises(ValueError):
        la.L2(Op=op, sigma=1.0)                                                                  # no b


def test_not_implemented_errors(la):
    from lmc_atomi_amd import _capi, algs
    op, m = op_and_data(la)
    pf = la.L2(Op=op, b=m.b, sigma=m.sigma_f)
    ones = np.ones(DIMS)
    with pytest.raises(NotImplementedError):
        pf.prox(np.zeros(DIMS, dtype=np.float32), 0.5)
    with pytest.raises(NotImplementedError):
        la.L2(Op=op, b=m.b, sigma=1.0, weights=ones)
    with pytest.raises(NotImplementedError):
        la.Poisson(op, ones, 1.0)
    with pytest.raises(NotImplementedError):
        la.HuberLoss(op, ones, 1.0)
    with pytest.raises(NotImplementedError):
        la.L2_ncvx_tv(DIMS, Op=op, Op2=la.Gradient(DIMS), b=ones)
    # what the samplers call before they touch a device
    d = pf.descriptor()
    assert d["data_kind"] == _capi.DATA_SENSE
    algs._refuse_sense(d, {"prior_kind": _capi.PRIOR_TV_ISO}, {})
    algs._refuse_sense({"data_kind": _capi.DATA_SPECTRAL}, {"tv_rtol": 1e-4}, {}, ("X", "y"))
    for prior, opts, who in (({"tv_rtol": 1e-4}, {}, None), ({"tv_warm": True}, {}, None), ({}, {"tv_warm": True}, None), ({}, {}, ("ULPDA", "why"))):
        with pytest.raises(NotImplementedError):
            algs._refuse_sense(d, prior, opts, who)
    assert la.MYMALASampler._sense_refusal is not None and la.MYULASampler._sense_refusal is None and la.SKROCKSampler._sense_refusal is None
    with pytest.raises(NotImplementedError, match="SENSE"):
        algs._refuse_sense(d, {}, {}, la.MYMALASampler._sense_refusal)
    with pytest.raises(NotImplementedError, match="SENSE"):
        algs._refuse_sgs(d, {}, None, 1.0)
    with pytest.raises(NotImplementedError):
        la.sgs_xstep(pf, np.zeros(DIMS, dtype=np.float32), 1.0)
    with pytest.raises(NotImplementedError):
        la.MultichannelMYULASampler([pf, pf], la.VectorialTV(DIMS, 2, sigma=0.3), DIMS, tau=0.1, gamma=0.5)


def test_no_gpu_means_loud_failure_not_fallback(la):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    op, m = op_and_data(la)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        op.matvec(np.zeros(DIMS, dtype=np.float32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        op.rmatvec(m.b)
    pf = la.L2(Op=op, b=m.b, sigma=m.sigma_f)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pf.grad(np.zeros(DIMS, dtype=np.float32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        la.MoreauYosidaUnadjustedLangevin(pf, la.TV(DIMS, 0.3), np.zeros(16 * 32), tau=0.1, gamma=0.5, niter=2)


def test_sense_kernels_use_no_scratch():
    import kernel_resources
    from lmc_atomi_amd import _capi
    res = kernel_resources.kernel_resources(_capi.LIB_PATH)
    names = {}
    for r in res:
        m = re.search(r"(sense_\w+(?:<[^>]*>)?)\(", r["demangled"])
        if m:
            names[m.group(1)] = r
    want = (["sense_rows_fwd_kernel"] + [f"sense_rows_inv_kernel<{e}>" for e in range(2)] + [f"sense_cols_kernel<{m}>" for m in range(4)]
            + ["sense_axpy_kernel<true>", "sense_axpy_kernel<false>"])
    assert sorted(names) == sorted(want), sorted(names)
    for n, r in names.items():
        print(f"{n}: vgpr {r['vgpr']} sgpr {r['sgpr']} lds {r['lds']} scratch {r['scratch']}")
        assert r["scratch"] == 0, (n, r)
        if "axpy" not in n:      # 512 threads, two workgroups per CU: at most 128 registers per lane
            assert r["vgpr"] <= 128, (n, r)

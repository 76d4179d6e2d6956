"""CPU-only: the surface of the Radon operator -- the header constants compiled from C and the unchanged layout of lmc_problem, the tables of
lmc_radon_tables (host code) against the numpy tables bit for bit, the descriptors, the Lipschitz bound, and the argument errors raised before any
device handle exists.  The library loads without a device."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import _radon_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LMC_E_INVALID, LMC_E_UNSUPPORTED = -1, -2


@pytest.fixture(scope="module")
def la():
    import lmc_atomi_amd as la
    return la


def header_values():
    code = ('#include <stdio.h>\n#include "lmc_atomi.h"\nint main(void){printf("%d %d %d %d %zu %d %d %d %d\\n", (int)LMC_DATA_RADON, '
            '(int)LMC_DATA_POISSON_RADON, (int)LMC_DATA_WL2_RADON, (int)LMC_DATA_HUBER_RADON, sizeof(lmc_problem), LMC_ATOMI_ABI_VERSION, '
            'LMC_MAX_RADON_ANGLES, LMC_MAX_RADON_DET, (int)LMC_DATA_HUBER_PSF);return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "s.c"), os.path.join(d, "s")
        open(src, "w").write(code)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        return tuple(map(int, subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()))


def test_constants_and_the_unchanged_layout():
    from lmc_atomi_amd import _capi
    assert header_values() == (16, 17, 18, 19, 200, 4, 1024, 4096, 15)
    assert C.sizeof(_capi.lmc_problem) == 200 and _capi.ABI_VERSION == 4
    assert (_capi.DATA_RADON, _capi.DATA_POISSON_RADON, _capi.DATA_WL2_RADON, _capi.DATA_HUBER_RADON) == (16, 17, 18, 19) == _capi.RADON_KINDS
    assert (_capi.MAX_RADON_ANGLES, _capi.MAX_RADON_DET) == (1024, 4096)
    assert not set(_capi.RADON_KINDS) & set(_capi.PSF_KINDS + _capi.TWO_PLANE_KINDS + (_capi.DATA_SPECTRAL,))
    for name in ("lmc_radon_apply", "lmc_radon_tables"):
        assert name in _capi.exported_symbols()


@pytest.mark.parametrize("name", [c.name for c in R.OP_CASES])
def test_tables_match_numpy_bit_for_bit(la, name):
    c = R.OP_CASES[R.OP_IDS.index(name)]
    op = la.Radon(c.shape, c.angles, c.n_det)
    ax, by = op.tables()
    want_ax, want_by = R.tables(c.shape, c.angles, R.case_n_det(c))
    assert ax.dtype == by.dtype == np.float32
    assert np.array_equal(ax, want_ax) and np.array_equal(by, want_by)


def test_tables_refuse_bad_arguments(la):
    from lmc_atomi_amd import _dev
    lib = _dev.lib()
    ang = np.array([0.1, 1.0], dtype=np.float32)
    ax, by = np.zeros((2, 8), dtype=np.float32), np.zeros((2, 6), dtype=np.float32)
    call = lambda a, na, nd, H, W: lib.lmc_radon_tables(a, na, nd, H, W, _dev.fptr(ax), _dev.fptr(by))
    assert call(_dev.fptr(ang), 2, 12, 6, 8) == 0
    assert lib.lmc_radon_tables(_dev.fptr(ang), 2, 12, 6, 8, None, None) == 0
    for args in ((None, 2, 12, 6, 8), (_dev.fptr(ang), 0, 12, 6, 8), (_dev.fptr(ang), 1025, 12, 6, 8), (_dev.fptr(ang), 2, 0, 6, 8),
                 (_dev.fptr(ang), 2, 4097, 6, 8), (_dev.fptr(ang), 2, 12, 0, 8), (_dev.fptr(ang), 2, 12, 6, 0)):
        assert call(*args) == LMC_E_INVALID and lib.lmc_last_error()
    bad = np.array([0.1, np.inf], dtype=np.float32)
    assert call(_dev.fptr(bad), 2, 12, 6, 8) == LMC_E_INVALID


def test_operator_fields_and_descriptors(la):
    from lmc_atomi_amd import _capi
    op = la.Radon((12, 20), R.SEVEN)
    assert op.dims == (12, 20) and op.n_det == R.default_n_det((12, 20)) == 26 and op.sino_shape == (7, 26) and op.shape == (7 * 26, 240)
    assert op.angles.dtype == np.float32 and np.array_equal(op.angles, R.angles32(R.SEVEN))
    assert op.H.shape == (240, 7 * 26)
    assert la.Radon((16, 16), [0.3], n_det=9).sino_shape == (1, 9)
    assert la.Radon((16, 16), 0.3).n_angles == 1                        # a scalar angle
    d = op.descriptor()
    assert np.array_equal(d["angles"], op.angles) and d["n_det"] == 26
    ref = R.RadonRef((12, 20), R.SEVEN)
    assert op.norm_bound() == pytest.approx(ref.norm2_bound(), rel=1e-12) and op.norm_bound() is not None and op._bound == op.norm_bound()
    assert la.Radon((16, 16), R._spread(5), 9).norm_bound() == pytest.approx(R.RadonRef((16, 16), R._spread(5), 9).norm2_bound(), rel=1e-12)
    ss = op.sino_shape
    rng = np.random.default_rng(0)
    y = rng.uniform(0, 20, ss)
    w = rng.uniform(0, 2, ss)
    beta = rng.uniform(0.5, 1.5, ss)
    delta = rng.uniform(1, 5, ss)
    cases = [(la.L2(Op=op, b=y, sigma=0.5), _capi.DATA_RADON, (7, 26), 1.0),
             (la.L2(Op=op, b=y.ravel(), sigma=0.5, weights=w), _capi.DATA_WL2_RADON, (2, 7, 26), float(w.max())),
             (la.Poisson(op, y, beta, sigma=0.5), _capi.DATA_POISSON_RADON, (2, 7, 26), float(np.max(y / beta ** 2))),
             (la.Poisson(op, y, 0.7, sigma=0.5), _capi.DATA_POISSON_RADON, (2, 7, 26), float(np.max(y / 0.7 ** 2))),
             (la.HuberLoss(op, y, delta.ravel(), sigma=0.5), _capi.DATA_HUBER_RADON, (2, 7, 26), 1.0),
             (la.HuberLoss(op, y, 3.0, sigma=0.5), _capi.DATA_HUBER_RADON, (2, 7, 26), 1.0)]
    for pf, kind, yshape, factor in cases:
        d = pf.descriptor()
        assert d["data_kind"] == kind and d["sigma_f"] == 0.5 and d["n_det"] == 26 and np.array_equal(d["angles"], op.angles)
        assert np.shape(d["y"]) == yshape and pf.dims == (12, 20)
        assert pf.grad_lipschitz() == pytest.approx(0.5 * factor * op.norm_bound(), rel=1e-12)
    yw = cases[1][0].descriptor()["y"]
    assert np.array_equal(np.asarray(yw[0]), y.astype(np.float32)) and np.array_equal(np.asarray(yw[1]), w.astype(np.float32))


def test_value_errors(la):
    shape = (12, 20)
    for angles in ([], np.zeros(1025), [0.1, np.nan], [np.inf], np.zeros((2, 2)), [1e39]):
        with pytest.raises(ValueError):
            la.Radon(shape, angles)
    for n_det in (0, -3, 4097):
        with pytest.raises(ValueError):
            la.Radon(shape, [0.1], n_det=n_det)
    with pytest.raises(ValueError):
        la.Radon((0, 4), [0.1])
    la.Radon(shape, np.zeros(1024), n_det=4096)
    op = la.Radon(shape, [0.1, 1.2, 2.0])
    ss = op.sino_shape
    good = np.ones(ss)
    img = np.ones(shape)                       # the image's size is not the sinogram's
    for bad in (img, np.ones(ss[0] * ss[1] + 1), np.ones((ss[1], ss[0]))):
        with pytest.raises(ValueError):
            la.L2(Op=op, b=bad)
        with pytest.raises(ValueError):
            la.L2(Op=op, b=good, weights=bad)
        with pytest.raises(ValueError):
            la.Poisson(op, bad, 1.0)
        with pytest.raises(ValueError):
            la.Poisson(op, good, bad)
        with pytest.raises(ValueError):
            la.HuberLoss(op, bad, 1.0)
        with pytest.raises(ValueError):
            la.HuberLoss(op, good, bad)
    with pytest.raises(ValueError):
        la.L2(Op=op)                           # no sinogram
    with pytest.raises(ValueError):
        la.L2(Op=op, b=good, weights=-good)
    with pytest.raises(ValueError):
        la.Poisson(op, -good, 1.0)
    with pytest.raises(ValueError):
        la.Poisson(op, good, 0.0)
    with pytest.raises(ValueError):
        la.HuberLoss(op, good, -1.0)
    with pytest.raises(ValueError):
        la.HuberLoss(op, np.where(np.eye(*ss) > 0, np.nan, 1.0), 1.0)


def test_not_implemented_errors(la):
    from lmc_atomi_amd import _capi, algs
    shape = (12, 20)
    op = la.Radon(shape, [0.1, 1.2, 2.0])
    good = np.ones(op.sino_shape)
    terms = [la.L2(Op=op, b=good), la.L2(Op=op, b=good, weights=good), la.Poisson(op, good, 1.0), la.HuberLoss(op, good, 2.0)]
    for pf in terms:
        with pytest.raises(NotImplementedError):
            pf.prox(np.zeros(shape), 1.0)
        d = pf.descriptor()
        algs._refuse_radon(d, {"prior_kind": _capi.PRIOR_TV_ISO}, {})                  # what is taken
        algs._refuse_term(d, {"prior_kind": _capi.PRIOR_HAAR_L1}, {"step_variant": "rows"})      # the operator's rules, not the fused terms'
        algs._refuse_psf(d, {"tv_rtol": 1e-4}, {}, ("X", "y"))
        algs._refuse_spectral(d, {"tv_rtol": 1e-4}, {}, ("X", "y"))
        for prior, opts, who in (({"tv_rtol": 1e-4}, {}, None), ({"tv_warm": True}, {}, None), ({}, {"tv_warm": True}, None), ({}, {}, ("MYMALA", "why")),
                                 ({}, {}, ("ULPDA", "why"))):
            with pytest.raises(NotImplementedError):
                algs._refuse_radon(d, prior, opts, who)
        with pytest.raises(NotImplementedError):
            algs._refuse_radon({**d, "ncvx_kind": _capi.NCVX_MC_TV}, {}, {})
    algs._refuse_radon({"data_kind": _capi.DATA_PSF}, {"tv_rtol": 1e-4}, {}, ("X", "y"))
    assert la.MYMALASampler._radon_refusal is not None and la.MYULASampler._radon_refusal is None and la.SKROCKSampler._radon_refusal is None
    with pytest.raises(NotImplementedError):
        la.L2_ncvx_tv(shape, Op=op, Op2=la.Gradient(shape), b=good)
    with pytest.raises(NotImplementedError):
        la.L2_ncvx_tv(shape, Op=op, b=good)

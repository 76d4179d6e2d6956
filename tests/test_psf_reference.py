"""CPU checks of the large-PSF harness (tests/_psf_ref.py) and of what the feature has without a device: the reference tells a wrong kernel from a right
one by three orders of magnitude, the float32 two-pass form stays inside the bound, the library's separability test, `la.PSF`'s validation, the
descriptors and the scratch fence of the psf_ kernels."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import _psf_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
X_ULP1 = float(np.spacing(np.float32(0.25)))


@pytest.fixture(scope="module")
def la():
    import lmc_atomi_amd as la
    return la


@pytest.mark.parametrize("name", R.IDS)
def test_planted_faults_exceed_the_bound_a_thousandfold(name):
    c = R.CASES[R.IDS.index(name)]
    ref = R.op_reference(name, False)
    x64, h64 = ref.x.astype(np.float64), c.h.astype(np.float64)
    assert 2 * X_ULP1 <= ref.bound < 1e-5, ref.bound      # operands of order 1: a few ulps of 1
    applied = 0
    for fault in R.FAULTS:
        if not R.fault_applies(fault, c):
            continue
        applied += 1
        err = float(np.max(np.abs(fault(x64, h64, c.offset) - ref.ref64)))
        print(f"{name} {fault.__name__}: err {err:.3e}, bound {ref.bound:.3e}, ratio {err / ref.bound:.1e}")
        assert err >= 1000 * ref.bound, (fault.__name__, err, ref.bound)
    assert applied >= 1


def test_every_fault_is_seen_by_some_case():
    for fault in R.FAULTS:
        assert sum(R.fault_applies(fault, c) for c in R.CASES) >= 4, fault.__name__
    small = R.CASES[R.IDS.index("gen-5x7-13x11")]
    assert not R.fault_applies(R.fault_last_row_dropped, small)      # the image is too small to see the last tap row


@pytest.mark.parametrize("adjoint", [False, True], ids=["H", "Ht"])
@pytest.mark.parametrize("name", [c.name for c in R.SEP_CASES])
def test_float32_two_pass_form_stays_inside_the_bound(name, adjoint):
    c = R.CASES[R.IDS.index(name)]
    ref = R.op_reference(name, adjoint)
    err, where = R.worst(R.two_pass_f32(c, ref.x, adjoint), ref.ref64)
    print(f"{name} adjoint={adjoint}: two-pass err {err:.3e} = {err / ref.bound:.2f} of the bound {ref.bound:.3e}")
    assert err <= ref.bound, (err, ref.bound, where)


def test_library_separability_test_accepts_the_separable_and_rejects_the_general(la):
    from lmc_atomi_amd import _capi, _dev
    lib = _capi.load()
    for c in R.CASES:
        kh, kw = c.h.shape
        u, v = np.zeros(kh, dtype=np.float32), np.zeros(kw, dtype=np.float32)
        rc = lib.lmc_psf_separable(_dev.fptr(c.h), kh, kw, _dev.fptr(u), _dev.fptr(v))
        ru, rv, worst = R.separable_factors(c.h)
        print(f"{c.name}: library says {rc}, worst deviation {worst:.3e} against 2^-22 = {R.SEP_RTOL:.3e}")
        assert rc == (1 if c.separable else 0), (c.name, rc, worst)
        assert (worst <= R.SEP_RTOL) == c.separable
        if c.separable:
            np.testing.assert_array_equal(u, ru.astype(np.float32))
            np.testing.assert_array_equal(v, rv.astype(np.float32))
    # a zero tap must be reproduced as zero: an outer product with one tap knocked out is rejected, a zero row is fine
    h = np.outer([1.0, 2.0, 3.0], [1.0, 0.5, 0.25]).astype(np.float32)
    assert lib.lmc_psf_separable(_dev.fptr(h), 3, 3, None, None) == 1
    g = h.copy()
    g[0, 2] = 0.0
    assert lib.lmc_psf_separable(_dev.fptr(g), 3, 3, None, None) == 0
    z = h.copy()
    z[1, :] = 0.0
    assert lib.lmc_psf_separable(_dev.fptr(z), 3, 3, None, None) == 1
    assert lib.lmc_psf_separable(_dev.fptr(h), 34, 3, None, None) == -1 and lib.lmc_psf_separable(None, 3, 3, None, None) == -1


def test_psf_validation(la):
    dims = (20, 24)
    ok = R.random_taps(13, 11, 1)
    op = la.PSF(dims, ok, offset=(4, 7))
    assert op.shape == (480, 480) and op.offset == (4, 7) and op.factors is None and op.h.dtype == np.float32
    assert la.PSF(dims, ok).offset == (6, 5)
    with pytest.raises(ValueError):
        la.PSF(dims, np.ones(5))                      # not 2-D
    with pytest.raises(ValueError):
        la.PSF(dims, np.ones((34, 3)) / 102)          # outside 1 .. 33
    with pytest.raises(ValueError):
        la.PSF(dims, np.ones((3, 35)) / 105)
    with pytest.raises(ValueError):
        la.PSF(dims, np.ones((0, 3)))
    for off in [(13, 0), (0, 11), (-1, 0)]:
        with pytest.raises(ValueError):
            la.PSF(dims, ok, offset=off)
    bad = ok.copy()
    bad[3, 3] = np.nan
    with pytest.raises(ValueError):
        la.PSF(dims, bad)
    bad[3, 3] = np.inf
    with pytest.raises(ValueError):
        la.PSF(dims, bad)
    with pytest.raises(ValueError):
        la.PSF(dims, ok, separable=True)              # not an outer product
    g = R.SEP_CASES[0]
    sep = la.PSF(g.shape, g.h, offset=g.offset)
    u, v = sep.factors
    assert u.shape == (21,) and v.shape == (21,) and np.allclose(np.outer(u, v), g.h, rtol=1e-6, atol=0)
    assert la.PSF(g.shape, g.h, offset=g.offset, separable=True).factors is not None
    assert la.PSF(g.shape, g.h, offset=g.offset, separable=False).factors is None
    assert la.PSF((8, 8), np.ones((33, 33)) / 1089).h.shape == (33, 33)


def test_convolve2d_still_refuses_eleven_by_eleven(la):
    with pytest.raises(ValueError):
        la.Convolve2D((16, 16), np.ones((11, 11)) / 121.0)
    la.Convolve2D((16, 16), np.ones((9, 9)) / 81.0)


def test_descriptors_carry_the_new_kinds_and_the_lipschitz_bound(la):
    from lmc_atomi_amd import _capi
    from lmc_atomi_amd.proximal import _Problem
    dims = (20, 24)
    h = R.random_taps(13, 11, 2) * 1.7
    op = la.PSF(dims, h, offset=(4, 7))
    y = np.ones(dims)
    norm2 = float(np.abs(op.h.astype(np.float64)).sum()) ** 2
    pf = la.L2(Op=op, b=y, sigma=2.0)
    d = pf.descriptor()
    assert d["data_kind"] == _capi.DATA_PSF == 9 and d["offset"] == (4, 7) and d["psf_separable"] == 0 and d["h"] is op.h
    assert pf.grad_lipschitz() == pytest.approx(2.0 * norm2, rel=1e-12)
    w = np.full(dims, 0.5)
    w[0, 0] = 3.0
    pw = la.L2(Op=op, b=y, sigma=2.0, weights=w)
    assert pw.descriptor()["data_kind"] == _capi.DATA_WL2_PSF == 11
    assert pw.grad_lipschitz() == pytest.approx(2.0 * 3.0 * norm2, rel=1e-12)
    pp = la.Poisson(op, np.full(dims, 4.0), 0.5, sigma=1.5)
    assert pp.descriptor()["data_kind"] == _capi.DATA_POISSON_PSF == 10
    assert pp.grad_lipschitz() == pytest.approx(1.5 * 16.0 * norm2, rel=1e-12)
    assert la.L2(Op=la.PSF(dims, h, separable=False), b=y).descriptor()["psf_separable"] == 2
    # what the C structure gets: the PSF in fields of its own, the blur fields empty
    for term, y_planes in ((pf, 1), (pw, 2), (pp, 2)):
        desc = dict(term.descriptor())
        desc["y"] = np.zeros((y_planes,) + dims, dtype=np.float32)      # (a host array: only the description is read here)
        try:
            p = _Problem(dims, desc).c
        except (RuntimeError, AssertionError):       # no device to put y on
            continue
        assert (p.psf_kh, p.psf_kw, p.psf_oy, p.psf_ox) == (13, 11, 4, 7) and (p.kh, p.kw, p.oy, p.ox) == (0, 0, 0, 0) and p.h_host
    # Convolve2D keeps its kinds
    assert la.L2(Op=la.Convolve2D(dims, np.ones((5, 5)) / 25), b=y).descriptor()["data_kind"] == _capi.DATA_BLUR
    with pytest.raises(NotImplementedError):
        pf.prox(np.zeros(dims), 1.0)
    with pytest.raises(NotImplementedError):
        la.L2_ncvx_tv(dims=dims, Op=op, b=y, sigma=1.0)


def test_the_psf_fields_fill_the_holes_of_the_structure(la):
    """No field moves and the structure keeps its size: the geometry sits in the four bytes in front of y_dev, the mode in the four in front of prox_scale."""
    from lmc_atomi_amd import _capi
    p = _capi.lmc_problem
    assert C.sizeof(p) == 200
    assert [getattr(p, n).offset for n in ("psf_kh", "psf_kw", "psf_oy", "psf_ox")] == [20, 21, 22, 23]
    assert (p.sigma_f.offset, p.y_dev.offset) == (16, 24)
    assert (p.eprox_scale_mask.offset, p.psf_separable.offset, p.prox_scale.offset) == (160, 164, 168)
    assert _capi.MAX_PSF == R.MAX_PSF == 33 and _capi.MAX_BLUR == 9
    assert _capi.ABI_VERSION == 4


def test_psf_kernels_are_in_the_library_without_scratch():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import kernel_resources as K
    finally:
        sys.path.pop(0)
    rs = [r for r in K.kernel_resources() if r["demangled"].startswith("psf_")]
    names = {r["demangled"] for r in rs}
    # the nine epilogues in both forms, and the second stage of the energies
    assert len([n for n in names if n.startswith("psf_conv_kernel<")]) == 18, sorted(names)
    assert any(n.startswith("psf_energy_finish_kernel") for n in names)
    for r in rs:
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, r
        assert r["lds"] <= 48 * 1024, r

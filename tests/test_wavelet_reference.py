"""CPU-only: the float64 checker of the Daubechies wavelet-l1 prior (tests/_wavelet.py) checks itself, and pins the taps compiled into the library
(`lmc_wavelet_filter` is host code; the library loads without a device).

Bounds.  W W^T = I to 1e-14: the taps come from a root finder and a handful of convolutions, each within a few ulp (1.1e-16) of exact, and a row of W
has at most 8 entries below 1.  Vanishing moments sum_k k^m g[k] = 0 to 1e-12: k^m <= 7^3 = 343 multiplies those few ulp.  Reconstruction and the
equalities with the block-Haar oracle to 1e-11 on data of size ~100: three levels, two directions, at most 16 multiply-adds each per pixel."""
import ctypes as C

import numpy as np
import pytest

import _wavelet as Wv
from oracle import lmc_oracle as O

PS = (1, 2, 3, 4)


def sizes(p):
    return sorted({2 * p, 16, 24})


@pytest.mark.parametrize("p", PS)
def test_filter_is_the_documented_one(p):
    h = Wv.scaling_filter(p)
    assert h.size == 2 * p and abs(h.sum() - np.sqrt(2.0)) < 1e-15 and abs(np.dot(h, h) - 1.0) < 1e-14
    if p == 2:
        assert np.allclose(h, [0.48296291, 0.83651630, 0.22414387, -0.12940952], atol=5e-9, rtol=0)
        s3 = np.sqrt(3.0)
        assert np.allclose(h, np.array([1 + s3, 3 + s3, 3 - s3, 1 - s3]) / (4 * np.sqrt(2.0)), atol=1e-15, rtol=0)      # the closed form of db2
    if p == 4:
        assert abs(h[0] - 0.23037781) < 5e-9
    if p == 1:
        assert np.allclose(h, np.sqrt(0.5), atol=1e-15, rtol=0)


@pytest.mark.parametrize("p", PS)
def test_analysis_matrix_is_orthonormal_and_the_wavelet_has_p_vanishing_moments(p):
    g = Wv.wavelet_filter(p)
    k = np.arange(2 * p, dtype=np.float64)
    for m in range(p):
        assert abs(np.sum(k ** m * g)) < 1e-12, (p, m)
    assert abs(np.sum(k ** p * g)) > 1e-3       # and no more than p
    for n in sizes(p):
        A = Wv.analysis_matrix(p, n)
        err = np.abs(A @ A.T - np.eye(n)).max()
        print(f"db{p} n={n}: |W W^T - I|_inf = {err:.2e}")
        assert err <= 1e-14
        assert np.abs(A.T @ A - np.eye(n)).max() <= 1e-14


@pytest.mark.parametrize("p", PS)
def test_perfect_reconstruction_and_the_two_forms_agree(p):
    rng = np.random.default_rng(p)
    for n in sizes(p):
        for m in sizes(p):
            x = rng.normal(0, 100, (2, n, m))
            for L in (1, 2, 3):
                if not Wv.legal((n, m), p, L):
                    continue
                c = Wv.dwt2(x, p, L)
                assert np.abs(Wv.idwt2(c, p, L) - x).max() < 1e-11
                assert np.abs(Wv.dwt2_taps(x, p, L) - c).max() < 1e-11
                assert np.abs(Wv.idwt2_taps(c, p, L) - x).max() < 1e-11
                assert abs(np.sum(c * c) - np.sum(x * x)) < 1e-11 * np.sum(x * x)        # Parseval
                assert np.abs(Wv.prox(x, p, L, 0.0) - x).max() < 1e-11
                assert np.abs(Wv.prox_taps(x, p, L, 7.0) - Wv.prox(x, p, L, 7.0)).max() < 1e-11
                assert np.allclose(Wv.value_taps(x, p, L), Wv.value(x, p, L), rtol=1e-13)
                # float32 replays stay float32
                assert Wv.prox(x.astype(np.float32), p, L, 7.0).dtype == np.float32 and Wv.prox_taps(x.astype(np.float32), p, L, 7.0).dtype == np.float32


def test_a_huge_threshold_projects_onto_the_approximation_space():
    rng = np.random.default_rng(0)
    x = rng.normal(0, 10, (16, 24))
    for p, L in ((1, 2), (2, 2), (3, 2)):
        z = Wv.prox(x, p, L, 1e9)
        c = Wv.dwt2(z, p, L)
        assert np.abs(c[Wv.detail_mask(c.shape, L)]).max() < 1e-12
        assert np.abs(c[:16 >> L, :24 >> L] - Wv.dwt2(x, p, L)[:16 >> L, :24 >> L]).max() < 1e-12
        assert np.abs(Wv.prox(z, p, L, 1e9) - z).max() < 1e-12      # idempotent


def test_p1_three_levels_is_the_block_haar_prior(golden):
    rng = np.random.default_rng(1)
    x = rng.normal(0, 30, (3, 16, 24))
    for thr in (0.0, 1.5, 40.0):
        assert np.abs(Wv.prox(x, 1, 3, thr) - O.haar_l1_prox(x, thr)).max() < 1e-11
    for i in range(3):
        assert abs(Wv.value(x, 1, 3)[i] - O.haar_l1_value(x[i])) < 1e-11 * O.haar_l1_value(x[i])
    g = golden("haar_pywt.npz")
    gx = np.asarray(g["x"], dtype=np.float64)
    for thr in (0.1, 2.0):
        assert np.abs(Wv.prox(gx, 1, 3, thr) - g["thr_%g" % thr]).max() < 1e-9 * np.abs(gx).max()
    assert abs(float(Wv.value(gx, 1, 3)) - float(g["val"])) < 1e-9 * float(g["val"])


@pytest.mark.parametrize("p", PS)
def test_prox_minimises_its_objective(p):
    rng = np.random.default_rng(10 + p)
    L = 2
    shape = (16, 24)
    x = rng.normal(0, 5, shape)
    t, sigma = 0.7, 1.3

    def objective(z):
        return 0.5 * np.sum((z - x) ** 2) + t * float(Wv.value(z, p, L, sigma))

    z0 = Wv.prox(x, p, L, t * sigma)
    f0 = objective(z0)
    for k in range(20):
        d = rng.normal(0, 10.0 ** -(k % 5), shape)
        assert f0 <= objective(z0 + d)


@pytest.mark.parametrize("p", PS)
def test_compiled_in_taps_equal_the_checker(p):
    from lmc_atomi_amd import _dev
    lib = _dev.lib()
    h = (C.c_double * 8)()
    n = C.c_int32(-1)
    assert lib.lmc_wavelet_filter(p, h, C.byref(n)) == 0
    assert n.value == 2 * p
    err = np.abs(np.array(h[:2 * p]) - Wv.scaling_filter(p)).max()
    print(f"db{p}: compiled-in taps against the factorisation: {err:.2e}")
    assert err <= 1e-15


def test_filter_entry_point_refuses_bad_arguments():
    from lmc_atomi_amd import _dev
    lib = _dev.lib()
    h = (C.c_double * 8)()
    for p in (0, 5, -1):
        assert lib.lmc_wavelet_filter(p, h, None) == -1
    assert lib.lmc_wavelet_filter(2, None, None) == -1
    assert lib.lmc_wavelet_filter(2, h, None) == 0

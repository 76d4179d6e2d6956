"""CPU only: the reference of the Radon operator (tests/_radon_ref.py) checked against the properties of the definition that need no kernel -- mass
conservation and unit column sums on the default detector, the exact projection at theta = 0, the Lipschitz bound against an SVD, the derived operator
bound against float32 replays in several summation orders -- and the planted faults that the bound has to tell from the definition."""
import numpy as np
import pytest

import _radon_ref as R


SMALL = [((5, 3), 4), ((12, 20), 7), ((33, 17), 9), ((16, 16), 5)]


@pytest.mark.parametrize("shape,na", SMALL, ids=[f"{s[0]}x{s[1]}" for s, _ in SMALL])
def test_mass_and_column_sums_on_the_default_detector(shape, na):
    ref = R.RadonRef(shape, R._spread(na))
    x = np.random.default_rng(3).uniform(0.0, 5.0, shape)
    sino = ref.apply(x)
    mass = sino.sum(axis=1)
    print(f"{shape}: sum_d (A x)[a][d] - sum x: worst {np.max(np.abs(mass - x.sum())):.2e}")
    assert np.max(np.abs(mass - x.sum())) <= 64 * np.spacing(x.sum())
    cols = ref.A.sum(0)
    assert np.max(np.abs(cols - na)) <= 8 * np.spacing(float(na)), (cols.min(), cols.max())


@pytest.mark.parametrize("shape,n_det", [((6, 8), 12), ((7, 9), 15), ((5, 4), 4), ((9, 8), 6)])
def test_theta_zero_is_the_column_sum(shape, n_det):
    """n_det = W (mod 2): t is an integer, every pixel falls into one bin whole."""
    H, W = shape
    assert (n_det - W) % 2 == 0
    ref = R.RadonRef(shape, [0.0], n_det)
    x = np.random.default_rng(4).integers(0, 9, shape).astype(np.float64)
    sino = ref.apply(x)[0]
    off = (n_det - W) // 2
    want = np.zeros(n_det)
    for j in range(W):
        if 0 <= j + off < n_det:
            want[j + off] = x[:, j].sum()
    assert np.array_equal(sino, want)


@pytest.mark.parametrize("shape,na,n_det", [((5, 3), 4, None), ((12, 20), 7, None), ((33, 17), 9, None), ((16, 16), 5, 9)])
def test_norm_bound_dominates_the_largest_singular_value(shape, na, n_det):
    ref = R.RadonRef(shape, R._spread(na), n_det)
    s2 = float(np.linalg.svd(ref.A, compute_uv=False)[0]) ** 2
    bound = ref.norm2_bound()
    print(f"{shape} n_det {ref.n_det}: bound {bound:.4f}, sigma_max^2 {s2:.4f}, ratio {bound / s2:.3f}")      # (an observation: 1.4 .. 1.6)
    assert bound >= s2
    assert ref.A.sum(0).max() <= na + 1e-9


@pytest.mark.parametrize("case", R.BOUND_CASES, ids=[c.name for c in R.BOUND_CASES])
def test_float32_replays_stay_inside_the_derived_bound(case):
    nd = R.case_n_det(case)
    A = R.dense(case.shape, case.angles, nd)
    A32 = R.dense(case.shape, case.angles, nd, np.float32)
    print(f"{case.name}: max |w32 - w64| / 2^-24 = {np.abs(A32.astype(np.float64) - A).max() / R.U:.2f}")
    assert np.abs(A32.astype(np.float64) - A).max() <= 2 * R.U      # what the bound's second part allows for
    rng = np.random.default_rng(1)
    for adjoint, M64, M32 in ((False, A, A32), (True, A.T, A32.T)):
        x = R.operand(1, M64.shape[1], 5 + adjoint)
        ref64 = x.astype(np.float64) @ M64.T
        bound = R.operator_bound(A, x, adjoint)[0]
        worst = 0.0
        n_in = M64.shape[1]
        for order in (np.arange(n_in), np.arange(n_in)[::-1], rng.permutation(n_in)):
            acc = np.zeros(M64.shape[0], np.float32)
            for k in order:
                acc += M32[:, k] * x[0, k]
            err = np.abs(acc.astype(np.float64) - ref64[0])
            pos = bound > 0
            assert np.all(err[~pos] == 0)
            worst = max(worst, float(np.max(err[pos] / bound[pos])))
        print(f"{case.name} adjoint={adjoint}: worst err / bound over three orders {worst:.3f}")
        assert worst <= 1.0


FAULT_SHAPES = [c for c in R.OP_CASES if c.name in ("12x20-seven", "33x17-9", "5x3-4", "9x11-70")]


@pytest.mark.parametrize("fault", sorted(R.FAULTS) + ["tables-swapped"])
def test_planted_faults_exceed_the_operator_bound(fault):
    """Each wrong operator, applied in float64, misses the derived bound of the right one on every case of the list (in one direction at least)."""
    for c in FAULT_SHAPES:
        nd = R.case_n_det(c)
        A = R.dense(c.shape, c.angles, nd)
        B = R.dense_swapped(c.shape, c.angles, nd) if fault == "tables-swapped" else R.dense(c.shape, c.angles, nd, **R.FAULTS[fault])
        x = R.operand(R.N_IMG, A.shape[1], 11)
        err = np.abs(x.astype(np.float64) @ (B - A).T)
        bound = R.operator_bound(A, x, False)
        ratio = float(np.max(err / np.maximum(bound, 1e-300)))
        print(f"{fault} on {c.name}: worst err / bound {ratio:.3g}")
        assert ratio > 1.0, (fault, c.name, ratio)

"""The high-precision reference of the closed-form proxes (tests/_eprox_ref.py) checked on the CPU: against its own stationarity equations, against
an independent 40-digit evaluation, against the values the reference's prox.py returned (tests/golden/prox.npz) and against the checker's float64
restatements; and the fp32 floor of the expressions eprox() commits to, from which the tolerance of tests/test_gpu_eprox_accuracy.py is taken.

Observed on the whole sweep (15 forms, 8 decades 1e-5 .. 1e2 of the scaled parameter, ~130 points each):

  stationarity residual / max(|x|, |p|), longdouble:   gaussian 8.4e-20, p=4/3 2.7e-19, p=3/2 1.1e-19, p=3 1.4e-19, p=4 2.5e-19,
                                                        smoothed_laplace 1.1e-19, gamma 7.6e-17, chi 3.8e-17                (bound 1e-15)
  reference against mpmath at 40 digits, relative to |p|:  <= 4.5e-19 (huber; the smooth forms <= 2.6e-19)                  (bound 1e-17)
  reference against prox.npz at the golden parameters:     <= 2.9e-15 absolute (p=4)                                         (bound 1e-12)
  checker (float64, the textbook formulas of prox.py) against the reference, relative to max(|x|, |p|):                      (bound 1e-7)
      smoothed_laplace 5.0e-8, p=3/2 1.3e-8, p=3 1.2e-8, gamma 1.9e-9, p=4/3 4.3e-10, p=4 3.2e-11, the others <= 6e-16.
  Relative to |p| alone the textbook formulas lose everything in float64 as well where p << |x|: p=4/3 7.7e4 and p=3/2 2.8 (g = 100,
  |x| = 1e-4), gamma 1.9e-6, chi 8.8e-7, smoothed_laplace 2.2e-7.  That is why the GPU tests take the reference of _eprox_ref.py and not the
  checker, and why the 1e-7 here is relative to max(|x|, |p|).
"""
import numpy as np
import pytest

import _eprox_ref as R
from oracle import lmc_oracle as O

GOLDEN = [("laplace_0.5", "laplace", (0.5,)), ("uncentered_laplace_0.7_1.5", "uncentered_laplace", (0.7, 1.5)), ("gaussian_0.3", "gaussian", (0.3,)),
          ("gen_gaussian_0.6_4_3", "gen_gaussian_4_3", (0.6,)), ("gen_gaussian_0.6_3_2", "gen_gaussian_3_2", (0.6,)),
          ("gen_gaussian_0.6_3", "gen_gaussian_3", (0.6,)), ("gen_gaussian_0.6_4", "gen_gaussian_4", (0.6,)), ("huber_0.5_0.4", "huber", (0.5, 0.4)),
          ("smoothed_laplace_0.9", "smoothed_laplace", (0.9,)), ("exp_0.5", "exp", (0.5,)), ("gamma_0.4_1.3", "gamma", (0.4, 1.3)),
          ("chi_0.7", "chi", (0.7,)), ("uniform_1.2", "uniform", (1.2,)), ("triangular_-0.5_0.8", "triangular", (-0.5, 0.8)),
          ("conjugate_laplace_0.8", "laplace_conj", (0.8,))]


def oracle_prox(kind, x, *q):
    x = np.asarray(x, dtype=np.float64)
    if kind.startswith("gen_gaussian"):
        return O.prox_gen_gaussian(x, q[0], {"4_3": 4 / 3, "3_2": 3 / 2, "3": 3, "4": 4}[kind[len("gen_gaussian_"):]])
    if kind == "laplace_conj":
        return O.prox_conjugate(x, q[0], O.prox_laplace)
    return getattr(O, "prox_" + kind)(x, *q)


def test_the_platform_has_an_extended_long_double_or_the_reference_goes_through_mpmath():
    import mpmath
    assert np.finfo(np.longdouble).eps < 1e-18 or R.USE_MPMATH
    assert mpmath.mp is not None


@pytest.mark.parametrize("kind", R.SMOOTH)
def test_reference_satisfies_its_stationarity_equation(kind):
    worst = 0.0
    for q in R.CASES[kind][0]:
        x, _ = R.sweep(kind, *q)
        p = np.asarray(R.ref(kind, x, *q), dtype=R.L)
        res = R.residual(kind, x, p, *q)
        scale = np.maximum(np.abs(x.astype(R.L)), np.abs(p))
        assert np.all(res <= 1e-15 * scale), (kind, q, float(np.max(res / np.maximum(scale, R.L(1e-300)))))
        worst = max(worst, float(np.max(res / np.maximum(scale, R.L(1e-300)))))
        if kind in ("gamma", "chi"):
            assert np.all(p > 0)
    print(f"{kind}: worst stationarity residual / max(|x|, |p|) = {worst:.2e}")


@pytest.mark.parametrize("kind", R.KINDS)
def test_reference_against_forty_digits(kind):
    """Every third point of the sweep through mpmath at 40 digits with the TEXTBOOK formulas (their cancellation costs at most ~15 of the 40 digits):
    an evaluation that shares neither the arithmetic nor the algebra of the reference."""
    import mpmath as mp
    mp.mp.dps = 40
    worst = 0.0
    for q in R.CASES[kind][0]:
        x, mask = R.sweep(kind, *q)
        sel = np.nonzero(~mask)[0][::3]
        p = np.asarray(R.ref(kind, x[sel], *q), dtype=R.L)
        for xv, pv, m in zip(x[sel], p, R._ref_mp(kind, x[sel], q)):
            d = abs(mp.mpf(float(pv)) + mp.mpf(float(pv - R.L(float(pv)))) - m)          # the longdouble as the sum of two doubles: exact
            assert d <= mp.mpf("1e-17") * abs(m), (kind, q, float(xv), float(pv), float(m))
            if m != 0:
                worst = max(worst, float(d / abs(m)))
    print(f"{kind}: worst |longdouble - 40 digits| / |p| = {worst:.2e}")


def test_reference_equals_the_golden_values_of_the_reference_implementation(golden):
    g = golden("prox.npz")
    for key, kind, q in GOLDEN:
        x = g["x"]
        k = R.kinks(kind, *q, dtype=np.float64)       # a grid point on a kink (1.25 = 1/0.8 of triangular, a jump): either side, as float64 decided it
        on_kink = np.isclose(x[:, None], k[None], rtol=1e-12, atol=0).any(axis=1) if k.size else np.zeros(x.size, bool)
        d = np.abs(R.nearest_reference(kind, x, g[key], on_kink, *q) - g[key])
        assert np.all(d <= 1e-12), (key, float(d.max()))
        print(f"{key}: {d.max():.2e}")


@pytest.mark.parametrize("kind", R.KINDS)
def test_the_checker_in_float64_agrees_with_the_reference(kind):
    """1e-7 relative to max(|x|, |p|).  The checker keeps the reference's textbook formulas on purpose (it restates prox.py); what they lose in float64
    relative to |p| alone is printed and recorded in the module docstring."""
    worst, worst_p = 0.0, 0.0
    for q in R.CASES[kind][0]:
        x, mask = R.sweep(kind, *q)
        got = np.asarray(oracle_prox(kind, x.astype(np.float64), *q), dtype=np.float64)
        want = R.nearest_reference(kind, x, got, mask, *q)
        d = np.abs(got - want)
        scale = np.maximum(np.abs(x.astype(np.float64)), np.abs(want))
        assert np.all(d <= 1e-7 * scale), (kind, q, float(np.max(d / np.maximum(scale, 1e-300))))
        worst = max(worst, float(np.max(d / np.maximum(scale, 1e-300))))
        worst_p = max(worst_p, float(np.max(np.where(want != 0, d / np.where(want != 0, np.abs(want), 1), 0))))
    print(f"{kind}: checker vs reference: {worst:.2e} of max(|x|, |p|), {worst_p:.2e} of |p|")


@pytest.mark.parametrize("kind", R.KINDS)
def test_fp32_floor_of_the_committed_expressions_and_the_tolerance_taken_from_it(kind):
    """FLOOR[kind] is the worst pointwise error of model32 (numpy float32, one rounding per operation) over the sweep, rounded up to one decimal;
    K = max(4, 4 FLOOR) and no form needs more than 16."""
    worst = 0.0
    for q in R.CASES[kind][0]:
        x, mask = R.sweep(kind, *q)
        e, msgs, nbad = R.check(kind, x, R.model32(kind, x, *q), mask, *q)
        assert nbad == 0, msgs
        worst = max(worst, e)
    print(f"{kind}: fp32 floor {worst:.3f} eps, table {R.FLOOR[kind]}, K {R.K[kind]}")
    assert worst <= R.FLOOR[kind] and (R.FLOOR[kind] - worst < 0.1 + 1e-9), (worst, R.FLOOR[kind])
    assert R.K[kind] == max(4.0, 4.0 * R.FLOOR[kind]) and R.K[kind] <= 16.0


@pytest.mark.parametrize("kind", R.WEIGHT_IS_IDENTITY_AT_ZERO)
def test_the_committed_expressions_are_the_identity_at_weight_zero(kind):
    params, scaled = R.CASES[kind]
    for q in {tuple(0.0 if i in scaled else v for i, v in enumerate(p)) for p in params}:
        x, _ = R.sweep(kind, *params[0])
        got = R.model32(kind, x, *q)
        assert np.array_equal(got.view(np.int32), x.view(np.int32)), (kind, q)


def _textbook32(kind, x, g):
    """The expressions of prox.py as they stood in eprox(), in float32."""
    c, ax, s = np.float32, np.abs(x), np.sign(x)
    if kind == "gen_gaussian_3":
        return s * (np.sqrt(c(1) + c(12) * g * ax) - c(1)) / (c(6) * g)
    if kind == "smoothed_laplace":
        u = g * ax - g * g - c(1)
        return s * (u + np.sqrt(u * u + c(4) * g * ax)) / (c(2) * g)
    if kind == "chi":
        return (x + np.sqrt(x * x + c(8) * g)) * c(0.25)


@pytest.mark.parametrize("kind", ["gen_gaussian_3", "smoothed_laplace", "chi"])
def test_the_metric_sees_the_cancellation_of_the_textbook_formulas(kind):
    """The acceptance of the GPU tests applied to the textbook expressions in float32: thousands of eps at g = 1e-4, exact zeros on dark pixels."""
    g = np.float32(1e-4)
    x, mask = R.sweep(kind, float(g))
    e, msgs, nbad = R.check(kind, x, _textbook32(kind, x, g), mask, float(g))
    assert e > 1000 and nbad > 10, (kind, e, nbad)

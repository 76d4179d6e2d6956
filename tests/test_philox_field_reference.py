"""The oracle's float32 noise field (`O.philox_normals`: Philox4x32-10, u01, Box-Muller) as a sample of N(0, 1), on the CPU: the reference that
tests/test_gpu_philox_field.py and the Philox cases of tests/_pixel.py hold the device to must itself be a unit normal field without structure along the
axes of its counter -- the four lanes of a quad, the column, the iteration, the chain, the key.

N = 2^22 deviates: 2 seeds (s, s ^ 1) x 16 iterations x 32 chains x 64 x 64 pixels.  Every bound below is a formula of N: a sample moment within 5 of
its standard error under N(0, 1) (mean 1 / sqrt N, variance sqrt(2 / N), skewness sqrt(6 / N), excess kurtosis sqrt(24 / N)), a sample correlation of M
pairs within 5 / sqrt M, the Kolmogorov-Smirnov distance to Phi below 1.95 / sqrt N (the 0.1 % point of its limit law).  None is fitted to what the
field gives."""
import math

import numpy as np
import pytest

import _pixel as X
from oracle import lmc_oracle as O

SEEDS = (X.SEED_P, X.SEED_P ^ 1)
N_IT, N_CH, H, W = 16, 32, 64, 64
CHAIN0 = 5


@pytest.fixture(scope="module")
def field():
    """[seed, iteration, chain, H, W], float32."""
    f = np.stack([np.stack([O.philox_normals(s, it, CHAIN0 + np.arange(N_CH), H, W) for it in range(N_IT)]) for s in SEEDS])
    assert f.dtype == np.float32 and f.size >= 2 ** 22
    f.setflags(write=False)
    return f


def corr(a, b):
    a, b = np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
    a, b = a - a.mean(), b - b.mean()
    return float(a @ b / np.sqrt((a @ a) * (b @ b))), a.size


def test_every_deviate_is_finite_and_inside_the_box_muller_radius(field):
    assert np.isfinite(field).all()
    # u_a >= 2^-33, so r = sqrt(-2 ln u_a) <= sqrt(66 ln 2) = 6.76
    assert np.abs(field).max() <= math.sqrt(66 * math.log(2)), np.abs(field).max()


def test_moments_within_five_standard_errors(field):
    x = field.astype(np.float64).ravel()
    n = x.size
    m = x.mean()
    d = x - m
    var = (d @ d) / n
    skew = np.mean(d ** 3) / var ** 1.5
    kurt = np.mean(d ** 4) / var ** 2 - 3.0
    print(f"N {n}: mean {m:.2e} (se {1 / math.sqrt(n):.1e}), var - 1 {var - 1:.2e} (se {math.sqrt(2 / n):.1e}), skewness {skew:.2e} (se {math.sqrt(6 / n):.1e}), "
          f"excess kurtosis {kurt:.2e} (se {math.sqrt(24 / n):.1e})")
    assert abs(m) <= 5 / math.sqrt(n)
    assert abs(var - 1) <= 5 * math.sqrt(2 / n)
    assert abs(skew) <= 5 * math.sqrt(6 / n)
    assert abs(kurt) <= 5 * math.sqrt(24 / n)


def test_no_correlation_along_any_axis_of_the_counter(field):
    q = field.reshape(field.shape[:3] + (H // 4, 4, W))       # [..., quad row-group, lane, column]
    pairs = {f"lanes {a}, {b} of a quad": (q[..., a, :], q[..., b, :]) for a in range(4) for b in range(a + 1, 4)}
    pairs["horizontally adjacent pixels"] = (field[..., :-1], field[..., 1:])
    pairs["vertically adjacent quads"] = (field[..., :-4, :], field[..., 4:, :])
    pairs["consecutive iterations"] = (field[:, :-1], field[:, 1:])
    pairs["consecutive chains"] = (field[:, :, :-1], field[:, :, 1:])
    pairs["seeds s and s ^ 1"] = (field[0], field[1])
    for name, (a, b) in pairs.items():
        r, m = corr(a, b)
        print(f"{name}: correlation {r:.2e} over {m} pairs (5 / sqrt M = {5 / math.sqrt(m):.1e})")
        assert abs(r) <= 5 / math.sqrt(m), name


def test_kolmogorov_smirnov_distance_to_the_normal_law(field):
    x = np.sort(field.astype(np.float64).ravel())
    n = x.size
    cdf = 0.5 * (1.0 + np.frompyfunc(math.erf, 1, 1)(x / math.sqrt(2.0)).astype(np.float64))
    i = np.arange(1, n + 1)
    dist = max(float(np.max(i / n - cdf)), float(np.max(cdf - (i - 1) / n)))
    print(f"KS distance {dist:.2e} over {n} deviates (1.95 / sqrt N = {1.95 / math.sqrt(n):.2e})")
    assert dist < 1.95 / math.sqrt(n)


def test_the_ends_of_the_integer_range_give_finite_deviates():
    """Philox outputs 0 and 0xFFFFFFFF: u01 is in (0, 1] -- 2^-33 at one end, 1.0 (rounded) at the other -- so the logarithm is finite, the radius of
    u_a = 1.0 is zero, and the angle of u_b = 1.0 is a full turn."""
    ends = np.array([0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF], dtype=np.uint32)
    u = O._u01(ends)
    assert u.dtype == np.float32 and u[0] == np.float32(2.0 ** -33) and u[-1] == np.float32(1.0) and (u > 0).all() and (u <= 1).all()
    ua, ub = np.meshgrid(ends, ends, indexing="ij")
    n0, n1 = O.box_muller(ua, ub)
    assert n0.dtype == np.float32 and np.isfinite(n0).all() and np.isfinite(n1).all()
    assert np.abs(np.stack([n0, n1])).max() <= math.sqrt(66 * math.log(2))
    assert (n0[-1] == 0).all() and (n1[-1] == 0).all()                                  # u_a = 1.0: r = 0
    assert abs(n1[0, 0] - math.sqrt(66 * math.log(2))) < 1e-5 and abs(n0[0, -1]) < 1e-6    # u_a = 2^-33: the largest radius, on the cosine at angle ~0

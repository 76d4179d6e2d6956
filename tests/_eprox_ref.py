"""High-precision reference of the fifteen closed-form elementwise proxes (``eprox()`` in csrc/lmc_device.h; prox.py:9-85 of the reference) and the
sweep the accuracy tests share.  Nothing here imports the package or the checker.

The reference is written cancellation-free in ``np.longdouble`` (80-bit) and, for the smooth families, polished by Newton steps on the stationarity
equation  p + t phi'(p) = x  of  prox_{t phi}(x) = argmin_p  (p - x)^2 / 2 + t phi(p),  so that it is pinned by that equation and not by a formula the
kernel shares.  The equations (g = the scaled parameter):

  gen_gaussian p=3      phi = |p|^3          p + 3 g p |p| = x
  gen_gaussian p=4      phi = p^4            p + 4 g p^3 = x
  gen_gaussian p=4/3    phi = |p|^(4/3)      p + (4 g / 3) sgn(p) |p|^(1/3) = x
  gen_gaussian p=3/2    phi = |p|^(3/2)      p + (3 g / 2) sgn(p) |p|^(1/2) = x
  gaussian              phi = p^2            p (1 + 2 g) = x
  smoothed_laplace      phi = |p| - ln(1 + g|p|)/g, t = g:  phi' = g|p| / (1 + g|p|) sgn(p), so with p >= 0 the modulus of the prox,
                        p + g^2 p / (1 + g p) = |x|   <=>   g p^2 + (1 + g^2 - g|x|) p - |x| = 0;   prox = sgn(x) p
  gamma                 phi = omega p - kappa ln p (p > 0):   p + omega - kappa / p = x   <=>   p^2 - (x - omega) p - kappa = 0
  chi                   phi = p^2 / 2 - kappa ln p (p > 0):   2 p - kappa / p = x         <=>   2 p^2 - x p - kappa = 0

The piecewise forms (laplace, uncentered_laplace, huber, exp, uniform, triangular, laplace_conj) are their case analysis; ``branches`` returns every
piece continued to the whole line, for the points within one fp32 step of a kink where either side is a correct answer.  laplace_conj is
x - g prox_laplace(x / g, 1 / g) = clip(x, -1, 1) for every g.

``model32`` evaluates in numpy float32, operation by operation, the expressions that ``eprox()`` commits to: its worst error against the reference
is the floor from which the tests' tolerance K = max(4, 4 floor) is taken (FLOOR, K below; tests/test_eprox_reference.py keeps them honest).
"""
import numpy as np

L = np.longdouble
F = np.float32
EPS32 = float(np.finfo(F).eps)
USE_MPMATH = not (np.finfo(L).eps < 1e-18)     # no 80-bit long double on this platform: every reference value through mpmath at 40 digits

KINDS = ("laplace", "uncentered_laplace", "gaussian", "gen_gaussian_4_3", "gen_gaussian_3_2", "gen_gaussian_3", "gen_gaussian_4", "huber",
         "smoothed_laplace", "exp", "gamma", "chi", "uniform", "triangular", "laplace_conj")
SMOOTH = ("gaussian", "gen_gaussian_4_3", "gen_gaussian_3_2", "gen_gaussian_3", "gen_gaussian_4", "smoothed_laplace", "gamma", "chi")
DECADES = tuple(float(F(10.0 ** e)) for e in range(-5, 3))          # 1e-5 ... 1e2 as the fp32 numbers the kernel receives


def f32(v):
    """The value as the fp32 number the device receives, held in a Python float."""
    return float(F(v))


# kind -> (tuples of parameters in the order of prox.py, indices that ElementwiseProx scales by the prox parameter)
def _cases():
    D = DECADES
    c = {k: ([(g,) for g in D], (0,)) for k in ("laplace", "gaussian", "gen_gaussian_4_3", "gen_gaussian_3_2", "gen_gaussian_3", "gen_gaussian_4",
                                                  "smoothed_laplace", "exp")}
    c["uncentered_laplace"] = ([(g, mu) for mu in (-0.5, 1.5) for g in D], (0,))
    c["huber"] = ([(f32(gam), t) for gam in (0.05, 0.5) for t in D], (1,))
    c["gamma"] = ([(f32(om), kap) for om in (1e-3, 1.0, 30.0) for kap in D], (1,))
    c["chi"] = ([(kap,) for kap in D], ())
    c["uniform"] = ([(om,) for om in D], ())
    c["triangular"] = ([(-0.5, f32(0.8)), (-4.0, f32(0.1))], ())
    c["laplace_conj"] = ([(g,) for g in D], ())
    return c


CASES = _cases()
WEIGHT_IS_IDENTITY_AT_ZERO = ("laplace", "uncentered_laplace", "gaussian", "gen_gaussian_4_3", "gen_gaussian_3_2", "gen_gaussian_3", "gen_gaussian_4",
                              "huber", "smoothed_laplace")

# floor: worst |model32 - ref| / |ref| over the sweep in units of fp32 eps (measured by tests/test_eprox_reference.py, rounded up to one decimal);
# K = max(4, 4 floor): two libm calls of <= 2 ulp composed (device cbrtf) and fma contraction on top of the floor
FLOOR = {"laplace": 0.5, "uncentered_laplace": 0.5, "gaussian": 0.8, "gen_gaussian_4_3": 3.9, "gen_gaussian_3_2": 2.1, "gen_gaussian_3": 1.2,
         "gen_gaussian_4": 1.4, "huber": 0.8, "smoothed_laplace": 1.3, "exp": 0.5, "gamma": 1.3, "chi": 1.1, "uniform": 0.0, "triangular": 0.8,
         "laplace_conj": 0.0}
K = {k: max(4.0, 4.0 * v) for k, v in FLOOR.items()}


# ------------------------------------------------------------------------------------------------------------------------------------------
# the reference
# ------------------------------------------------------------------------------------------------------------------------------------------
def _sgn(x):
    return np.sign(x)


def _smooth_closed(kind, x, q):
    """Cancellation-free closed forms (every sum is of terms of one sign), on |x| for the odd families."""
    g = q[0]
    ax = np.abs(x)
    if kind == "gaussian":
        return x / (1 + 2 * g)
    if kind == "gen_gaussian_3":
        return _sgn(x) * 2 * ax / (np.sqrt(1 + 12 * g * ax) + 1)
    if kind == "gen_gaussian_4":           # Cardano with the product of the two cube roots known: (a - b)(a^2 + a b + b^2) = a^3 - b^3
        s = np.sqrt(27 * g) * ax
        m = np.cbrt((np.sqrt(s * s + 1) + s) ** 2)
        return 3 * x / (1 + m + 1 / m)
    if kind == "gen_gaussian_4_3":         # q = |p|^(1/3):  q^3 + (4g/3) q = |x|
        xi = np.sqrt(ax * ax + 256 * g ** 3 / 729)
        a = np.cbrt((xi + ax) / 2)
        b = np.where(a > 0, (4 * g / 9) / np.where(a > 0, a, 1), 0)
        den = a * a + b * b + 4 * g / 9
        r = np.where(den > 0, ax / np.where(den > 0, den, 1), 0)
        return _sgn(x) * r ** 3
    if kind == "gen_gaussian_3_2":         # q = |p|^(1/2):  q^2 + (3g/2) q = |x|
        den = 3 * g + np.sqrt(9 * g * g + 16 * ax)
        r = np.where(den > 0, 4 * ax / np.where(den > 0, den, 1), 0)
        return _sgn(x) * r * r
    if kind == "smoothed_laplace":
        u = g * (ax - g) - 1
        r = np.sqrt(u * u + 4 * g * ax)
        return _sgn(x) * np.where(u < 0, 2 * ax / (r - u), (u + r) / np.where(g > 0, 2 * g, 1))
    if kind == "gamma":
        d, kap = x - q[0], q[1]
        r = np.sqrt(d * d + 4 * kap)
        return np.where(d < 0, 2 * kap / (r - d), (d + r) / 2)
    if kind == "chi":
        r = np.sqrt(x * x + 8 * q[0])
        return np.where(x < 0, 2 * q[0] / (r - x), (x + r) / 4)
    raise KeyError(kind)


def _newton_terms(kind, x, p, q):
    """f(p) and f'(p) of the stationarity equation in a form whose root is simple and whose evaluation near the root is benign: the symmetric
    families on moduli, the roots of p^(1/3), p^(1/2) substituted."""
    g = q[0]
    ax, ap = np.abs(x), np.abs(p)
    if kind == "gaussian":
        return ap * (1 + 2 * g) - ax, 1 + 2 * g + 0 * ap
    if kind == "gen_gaussian_3":
        return ap + 3 * g * ap * ap - ax, 1 + 6 * g * ap
    if kind == "gen_gaussian_4":
        return ap + 4 * g * ap ** 3 - ax, 1 + 12 * g * ap * ap
    if kind == "smoothed_laplace":
        return ap + g * g * ap / (1 + g * ap) - ax, 1 + (g / (1 + g * ap)) ** 2         # the equation before it is multiplied by 1 + g p
    if kind == "gamma":
        d = x - q[0]
        return p * p - d * p - q[1], 2 * p - d
    if kind == "chi":
        return 2 * p * p - x * p - q[0], 4 * p - x
    raise KeyError(kind)


def _ref_ld(kind, x, q):
    """The longdouble reference.  _smooth_closed is, term for term, the algebra that eprox() commits to (and model32 mirrors it), so on its own this
    would be a reference that agrees with the kernel by construction.  What makes it independent is (a) the Newton polish on the stationarity
    equation and (b) tests/test_eprox_reference.py::test_reference_against_forty_digits, which evaluates the TEXTBOOK formulas of prox.py in mpmath
    at 40 digits and holds this function to them at 1e-17: that test is part of the reference and must stay with it."""
    x = np.asarray(x, dtype=L)
    q = tuple(np.asarray(v, dtype=L) for v in q)
    if kind in SMOOTH:
        p = _smooth_closed(kind, x, q)
        if kind in ("gen_gaussian_4_3", "gen_gaussian_3_2"):
            # Newton on the substituted unknown r = |p|^(1/n):  r^n + c r - |x| = 0
            n, c = (3, 4 * q[0] / 3) if kind == "gen_gaussian_4_3" else (2, 3 * q[0] / 2)
            ax = np.abs(x)
            r = np.cbrt(np.abs(p)) if n == 3 else np.sqrt(np.abs(p))
            for _ in range(2):
                fp = n * r ** (n - 1) + c
                r = r - np.where(fp > 0, (r ** n + c * r - ax) / np.where(fp > 0, fp, 1), 0)
            return _sgn(x) * r ** n
        for _ in range(2):
            f, fp = _newton_terms(kind, x, p, q)
            step = f / fp
            p = p - (step if kind in ("gamma", "chi") else _sgn(x) * step)
        return p
    return _select(kind, x, q)


def branches(kind, x, *q):
    """Every piece of a piecewise form, continued to all x (longdouble)."""
    x = np.asarray(x, dtype=L)
    q = tuple(np.asarray(v, dtype=L) for v in q)
    z = np.zeros_like(x)
    if kind == "laplace":
        return [x - q[0], x + q[0], z]
    if kind == "exp":
        return [x - q[0], z]
    if kind == "uncentered_laplace":
        return [x - q[0], x + q[0], z + q[1]]
    if kind == "huber":
        gam, t = q
        return [x / (2 * t + 1), x - gam * np.sqrt(2 * t) * _sgn(x)]
    if kind == "uniform":
        return [x, z + q[0], z - q[0]]
    if kind == "laplace_conj":
        return [x, z + 1, z - 1]
    if kind == "triangular":
        o1, o2 = q
        # the root of p^2 - (x + o) p + (x o - 1) = 0 nearer to zero; below 1/o1 both roots are negative and the sum x + o1 + sqrt cancels
        r1, r2 = np.sqrt((x - o1) ** 2 + 4), np.sqrt((x - o2) ** 2 + 4)
        lo = np.where(x + o1 < 0, 2 * (x * o1 - 1) / (x + o1 - r1), (x + o1 + r1) / 2)
        hi = np.where(x + o2 < 0, 2 * (x * o2 - 1) / (x + o2 - r2), (x + o2 + r2) / 2)
        return [lo, hi, z]
    raise KeyError(kind)


def _select(kind, x, q):
    b = branches(kind, x, *q)
    if kind == "laplace":
        return np.where(x > q[0], b[0], np.where(x < -q[0], b[1], b[2]))
    if kind == "exp":
        return np.where(x >= q[0], b[0], b[1])
    if kind == "uncentered_laplace":
        return np.where(x - q[1] > q[0], b[0], np.where(x - q[1] < -q[0], b[1], b[2]))
    if kind == "huber":
        gam, t = q
        return np.where(np.abs(x) * np.sqrt(2 * t) <= gam * (2 * t + 1), b[0], b[1])
    if kind in ("uniform", "laplace_conj"):
        w = q[0] if kind == "uniform" else L(1)
        return np.where(x > w, b[1], np.where(x < -w, b[2], b[0]))
    if kind == "triangular":
        return np.where(x * q[0] > 1, b[0], np.where(x * q[1] > 1, b[1], b[2]))      # x < 1/o1 (o1 < 0), x > 1/o2 (o2 > 0)
    raise KeyError(kind)


def _ref_mp(kind, x, q):
    """The same through mpmath at 40 digits: the textbook formulas, whose cancellation costs at most ~15 of the 40 digits."""
    import mpmath as mp
    mp.mp.dps = 40
    out = []
    for v in zip(*(a.ravel() for a in np.broadcast_arrays(np.asarray(x, dtype=np.float64), *(np.asarray(v, dtype=np.float64) for v in q)))):
        out.append(_mp_one(mp, kind, mp.mpf(float(v[0])), [mp.mpf(float(w)) for w in v[1:]]))
    return out


def _mp_one(mp, kind, x, q):
    g = q[0]
    ax, s = abs(x), mp.sign(x)
    if kind == "laplace":
        return s * max(ax - g, 0)
    if kind == "uncentered_laplace":
        d = x - q[1]
        return q[1] + mp.sign(d) * max(abs(d) - g, 0)
    if kind == "gaussian":
        return x / (2 * g + 1)
    if kind == "gen_gaussian_4_3":
        xi = mp.sqrt(x * x + 256 * g ** 3 / 729)
        return x + 4 * g / (3 * mp.cbrt(2)) * (mp.cbrt(xi - x) - mp.cbrt(xi + x))
    if kind == "gen_gaussian_3_2":
        return x + 9 * g * g * s * (1 - mp.sqrt(1 + 16 * ax / (9 * g * g))) / 8
    if kind == "gen_gaussian_3":
        return s * (mp.sqrt(1 + 12 * g * ax) - 1) / (6 * g)
    if kind == "gen_gaussian_4":
        xi = mp.sqrt(x * x + 1 / (27 * g))
        return mp.cbrt((xi + x) / (8 * g)) - mp.cbrt((xi - x) / (8 * g))
    if kind == "huber":
        gam, t = q
        return x / (2 * t + 1) if ax * mp.sqrt(2 * t) <= gam * (2 * t + 1) else x - gam * mp.sqrt(2 * t) * s
    if kind == "smoothed_laplace":
        u = g * ax - g * g - 1
        return s * (u + mp.sqrt(u * u + 4 * g * ax)) / (2 * g)
    if kind == "exp":
        return x - g if x >= g else mp.mpf(0)
    if kind == "gamma":
        d = x - q[0]
        return (d + mp.sqrt(d * d + 4 * q[1])) / 2
    if kind == "chi":
        return (x + mp.sqrt(x * x + 8 * g)) / 4
    if kind == "uniform":
        return min(max(x, -g), g)
    if kind == "triangular":
        o1, o2 = q
        if x * o1 > 1:
            return (x + o1 + mp.sqrt((x - o1) ** 2 + 4)) / 2
        if x * o2 > 1:
            return (x + o2 + mp.sqrt((x - o2) ** 2 + 4)) / 2
        return mp.mpf(0)
    if kind == "laplace_conj":
        return min(max(x, -1), 1)
    raise KeyError(kind)


def ref(kind, x, *q):
    """prox_<kind>(x; q) for fp32-representable x and q, as float64 values of a longdouble (or 40-digit) evaluation: the error of the returned
    numbers is the final rounding to float64, 1.1e-16 relative."""
    if USE_MPMATH:
        return np.array([float(v) for v in _ref_mp(kind, x, q)]).reshape(np.shape(x))
    return np.asarray(_ref_ld(kind, x, q), dtype=L)


def ref64(kind, x, *q):
    return np.asarray(ref(kind, x, *q), dtype=np.float64)


def residual(kind, x, p, *q):
    """Stationarity residual of the smooth families, |f(p)| as in the module docstring, longdouble."""
    x, p = np.asarray(x, dtype=L), np.asarray(p, dtype=L)
    q = tuple(np.asarray(v, dtype=L) for v in q)
    g = q[0]
    ap, s = np.abs(p), _sgn(p)
    if kind == "gaussian":
        return np.abs(p * (1 + 2 * g) - x)
    if kind == "gen_gaussian_3":
        return np.abs(p + 3 * g * p * ap - x)
    if kind == "gen_gaussian_4":
        return np.abs(p + 4 * g * p ** 3 - x)
    if kind == "gen_gaussian_4_3":
        return np.abs(p + (4 * g / 3) * s * np.cbrt(ap) - x)
    if kind == "gen_gaussian_3_2":
        return np.abs(p + (3 * g / 2) * s * np.sqrt(ap) - x)
    if kind == "smoothed_laplace":
        return np.abs(ap + g * g * ap / (1 + g * ap) - np.abs(x))       # the quadratic divided by 1 + g|p|: terms of the size of |x|, not g p^2
    if kind == "gamma":
        return np.abs(p * p - (x - q[0]) * p - q[1])
    if kind == "chi":
        return np.abs(2 * p * p - x * p - q[0])
    raise KeyError(kind)


# ------------------------------------------------------------------------------------------------------------------------------------------
# the sweep
# ------------------------------------------------------------------------------------------------------------------------------------------
def kinks(kind, *q, dtype=F):
    """The kinks of a form as fp32 numbers (the fp32 nearest to the exact kink)."""
    q = tuple(np.asarray(v, dtype=L) for v in q)
    if kind in ("laplace", "exp"):
        k = [q[0], -q[0]]
    elif kind == "uncentered_laplace":
        k = [q[1] + q[0], q[1] - q[0]]
    elif kind == "huber":
        t = q[0] * (2 * q[1] + 1) / np.sqrt(2 * q[1])
        k = [t, -t]
    elif kind == "uniform":
        k = [q[0], -q[0]]
    elif kind == "triangular":
        k = [1 / q[0], 1 / q[1]]
    elif kind == "laplace_conj":
        k = [L(1), L(-1)]
    else:
        k = []
    return np.array([dtype(v) for v in k], dtype=dtype)


_ORDINARY = np.concatenate([np.logspace(-4, 3, 57), -np.logspace(-4, 3, 57), [0.0, -0.0, 255.0, -255.0]]).astype(F)


def sweep(kind, *q):
    """(x as float32, mask of the points within one fp32 step of a kink)."""
    k = kinks(kind, *q)
    near = np.concatenate([k, np.nextafter(k, F(np.inf)), np.nextafter(k, F(-np.inf))]).astype(F) if k.size else np.zeros(0, F)
    x = np.concatenate([_ORDINARY, near])
    return x, np.isin(x, near)               # an ordinary point that falls on a kink (x = 10 = 1/omega2) counts as one


def nearest_reference(kind, x, got, kink_mask, *q):
    """The reference at every point, float64; at the points within one fp32 step of a kink the branch value nearer to ``got``."""
    got = np.asarray(got, dtype=np.float64).ravel()
    want = ref64(kind, x, *q).ravel().copy()
    if kink_mask.any():
        idx = np.nonzero(kink_mask)[0]
        br = np.stack([np.asarray(b, dtype=np.float64).ravel()[idx] for b in branches(kind, x, *q)])
        want[idx] = br[np.argmin(np.abs(br - got[idx][None]), axis=0), np.arange(idx.size)]
    return want


def check(kind, x, got, kink_mask, *q, k=None):
    """Pointwise acceptance: |got - ref| <= K eps |ref|; ref == 0 -> got == 0; gamma and chi > 0; at kink neighbours the nearer branch is the
    reference.  Returns (worst error in eps over the points with a nonzero reference, the first failures as text, their number)."""
    k = K[kind] if k is None else k
    got = np.asarray(got, dtype=np.float64).ravel()
    want = nearest_reference(kind, x, got, kink_mask, *q)
    nz = want != 0
    with np.errstate(invalid="ignore", divide="ignore"):
        e = np.where(nz, np.abs(got - want) / (EPS32 * np.where(nz, np.abs(want), 1)), 0.0)
    e = np.where(np.isfinite(got), e, np.inf)
    bad = (e > k) | (~nz & (got != 0))
    if kind in ("gamma", "chi"):
        bad |= ~(got > 0)
    xs = np.asarray(x).ravel()
    msgs = [f"{kind}{tuple(float(v) for v in q)} x={float(xs[i])!r}: got {got[i]!r} want {want[i]!r} ({e[i]:.3g} eps, K={k:g})" for i in np.nonzero(bad)[0][:4]]
    return float(e.max()), msgs, int(bad.sum())


# ------------------------------------------------------------------------------------------------------------------------------------------
# the kernel's expressions in numpy float32 (one rounding per operation; fmaf where the kernel says fmaf)
# ------------------------------------------------------------------------------------------------------------------------------------------
def _fma(a, b, c):
    return (a.astype(np.float64) * np.float64(b) + np.float64(c)).astype(F) if isinstance(a, np.ndarray) else F(np.float64(a) * np.float64(b) + np.float64(c))


def model32(kind, x, *q):
    x = np.asarray(x, dtype=F)
    q = tuple(F(v) for v in q)
    g = q[0]
    ax = np.abs(x)
    c = lambda v: F(v)                                                       # noqa: E731
    cs = lambda v: np.copysign(v, x).astype(F)                               # noqa: E731
    with np.errstate(all="ignore"):
        if kind == "laplace":
            return cs(np.maximum(ax - g, c(0)))
        if kind == "uncentered_laplace":
            mu = q[1]
            return np.where(x < mu - g, -((-x) - g), np.where(x > mu + g, x - g, mu)).astype(F)      # -((-x) - g): x + g that keeps -0 at g = 0
        if kind == "gaussian":
            return x / (c(2) * g + c(1))
        if kind == "gen_gaussian_4_3":
            xi = np.sqrt(x * x + g * g * g * c(256 / 729))
            a = np.cbrt((xi + ax) * c(0.5)).astype(F)
            g49 = g * c(4 / 9)
            b = np.where(a > 0, g49 / a, c(0)).astype(F)
            den = a * a + b * b + g49
            r = np.where(den > 0, ax / den, c(0)).astype(F)
            w = g * c(4 / 3) * r
            return cs(np.where(w < c(0.5) * ax, ax - w, r * r * r))
        if kind == "gen_gaussian_3_2":
            den = c(3) * g + np.sqrt(c(9) * g * g + c(16) * ax)
            r = np.where(den > 0, c(4) * ax / den, c(0)).astype(F)
            w = c(1.5) * g * r
            return cs(np.where(w < c(0.5) * ax, ax - w, r * r))
        if kind == "gen_gaussian_3":
            return cs(c(2) * ax / (np.sqrt(c(1) + c(12) * g * ax) + c(1)))
        if kind == "gen_gaussian_4":
            s = np.sqrt(c(27) * g) * ax
            m = np.cbrt(np.square(np.sqrt(s * s + c(1)) + s)).astype(F)
            return x * (c(3) / (c(1) + m + c(1) / m))
        if kind == "huber":
            gam, t = q
            t2 = c(2) * t
            s = np.sqrt(t2)
            s_lo = _fma(-s, s, t2) * (c(0.5) / s) if s > 0 else c(0)           # sqrt(2t) = s + s_lo to twice the precision
            inner = x / (t2 + c(1))
            outer = cs(_fma(ax * 0 - gam, s, ax) - gam * s_lo)                  # fmaf(-g, s, |x|): one rounding of |x| - g s
            return np.where(ax * s <= gam * (t2 + c(1)), inner, outer).astype(F)
        if kind == "smoothed_laplace":
            u = g * (ax - g) - c(1)
            r = np.sqrt(u * u + c(4) * g * ax)
            return cs(np.where(u < 0, c(2) * ax / (r - u), (u + r) / (c(2) * g)))
        if kind == "exp":
            return np.where(x >= g, x - g, c(0)).astype(F)
        if kind == "gamma":
            d = x - q[0]
            r = np.sqrt(d * d + c(4) * q[1])
            return np.where(d < 0, c(2) * q[1] / (r - d), (d + r) * c(0.5)).astype(F)
        if kind == "chi":
            r = np.sqrt(x * x + c(8) * g)
            return np.where(x < 0, c(2) * g / (r - x), (x + r) * c(0.25)).astype(F)
        if kind == "uniform":
            return np.minimum(np.maximum(x, -g), g)
        if kind == "triangular":
            o1, o2 = q
            d1, d2 = x - o1, x - o2
            lo = c(2) * _fma(x, o1, c(-1)) / ((x + o1) - np.sqrt(d1 * d1 + c(4)))      # below 1/o1 < 0 the textbook sum x + o1 + sqrt cancels
            hi = ((x + o2) + np.sqrt(d2 * d2 + c(4))) * c(0.5)
            return np.where(x < c(1) / o1, lo, np.where(x > c(1) / o2, hi, c(0))).astype(F)
        if kind == "laplace_conj":
            return np.minimum(np.maximum(x, c(-1)), c(1))
    raise KeyError(kind)

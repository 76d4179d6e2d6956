"""Reference of the parallel-beam Radon operator (`la.Radon`, LMC_DATA_RADON .. LMC_DATA_HUBER_RADON in include/lmc_atomi.h), numpy only: the two tables,
t as their float32 sum, the dense float64 matrix of the definition with its `apply` / `apply_adjoint`, the four data terms on it (the term classes of
tests/_poisson_ref.py, _wl2_ref.py, _huber_ref.py and _pixel.py take any operator with `fwd` / `adj`), the case lists and the bounds.

Operator bound, derived and not measured; it holds for any summation order.  For one output with n non-zero weights, S_w = sum w |operand| and
S_1 = sum_{w > 0} |operand|:   |got - ref64| <= 2^-24 ((n + 2) S_w + 2 S_1).   The first part is the gamma_n bound of an n-term fp32 dot product with
rounded products, the second allows an absolute error of 2 * 2^-24 in a weight.  An output with n = 0 must be exactly 0.
Whole steps and trajectories: the project's rules of tests/_pixel.py -- per pixel max(3 e32, 2 ulp32), e32 from the float32 replay here."""
import functools
import math
from collections import namedtuple

import numpy as np

import _huber_ref as HU
import _pixel as X
import _poisson_ref as P
import _psf_ref as PR
import _wl2_ref as W

N_IMG = 3
U = 2.0 ** -24
MAX_ANGLES, MAX_DET = 1024, 4096
f32 = X.f32


# ------------------------------------------------------------------ the definition
def default_n_det(shape):
    return int(math.ceil(math.hypot(*shape))) + 2


def angles32(angles):
    """The float32 values ARE the angles."""
    return np.atleast_1d(np.asarray(angles, dtype=np.float64)).astype(np.float32)


def tables(shape, angles, n_det, sin_sign=1.0, centre_shift=0.0, origin_shift=0.0):
    """ax[a][j] = X_j cos, by[a][i] = Y_i sin + (n_det - 1) / 2: float64 products (libm's cos and sin of the float32 angle widened), rounded once.  The
    keyword arguments plant faults."""
    H, W = shape
    th = [float(a) for a in angles32(angles)]
    c = np.array([math.cos(t) for t in th])
    s = np.array([math.sin(t) for t in th]) * sin_sign
    Xc = np.arange(W, dtype=np.float64) - (W - 1) / 2.0 + centre_shift
    Yc = np.arange(H, dtype=np.float64) - (H - 1) / 2.0 + centre_shift
    ax = (Xc[None, :] * c[:, None]).astype(np.float32)
    by = (Yc[None, :] * s[:, None] + ((n_det - 1) / 2.0 + origin_shift)).astype(np.float32)
    return ax, by


def detector_coordinate(ax, by):
    """t[a][i][j] = ax[a][j] + by[a][i]: one float32 addition."""
    t = by[:, :, None] + ax[:, None, :]
    assert t.dtype == np.float32
    return t


def dense_from_t(t, n_det, dtype=np.float64, drop_second=False):
    """A[(a, d), (i, j)] = max(0, 1 - |t - d|), evaluated in `dtype` from the float32 t."""
    na, H, W = t.shape
    tt = t.astype(dtype)
    d = np.arange(n_det, dtype=dtype)
    one, zero = np.dtype(dtype).type(1), np.dtype(dtype).type(0)
    w = np.maximum(zero, one - np.abs(tt[..., None] - d))            # [a, i, j, d]
    if drop_second:                                                   # planted fault: the bin floor(t) + 1 gets nothing
        w = np.where(d > np.floor(tt)[..., None], zero, w)
    return np.ascontiguousarray(w.transpose(0, 3, 1, 2).reshape(na * n_det, H * W))


def dense(shape, angles, n_det, dtype=np.float64, **faults):
    drop = faults.pop("drop_second", False)
    return dense_from_t(detector_coordinate(*tables(shape, angles, n_det, **faults)), n_det, dtype, drop)


class RadonRef:
    """The operator on arrays with the image (sinogram) on the last two axes, computed in the dtype of its operand: the interface of
    `_poisson_ref.Op`."""
    kind = "radon"

    def __init__(self, shape, angles, n_det=None, A=None):
        self.shape = (int(shape[0]), int(shape[1]))
        self.angles = angles32(angles)
        self.n_det = default_n_det(self.shape) if n_det is None else int(n_det)
        self.sino_shape = (self.angles.size, self.n_det)
        self.A = dense(self.shape, self.angles, self.n_det) if A is None else A
        self._A32 = None

    def _mat(self, dtype):
        if np.dtype(dtype) == np.float64:
            return self.A
        if self._A32 is None:
            self._A32 = dense(self.shape, self.angles, self.n_det, np.float32)
        return self._A32

    def apply(self, x):
        x = np.asarray(x)
        lead = x.shape[:-2]
        out = x.reshape(-1, self.shape[0] * self.shape[1]) @ self._mat(x.dtype).T
        assert out.dtype == x.dtype
        return out.reshape(lead + self.sino_shape)

    def apply_adjoint(self, r):
        r = np.asarray(r)
        lead = r.shape[:-2]
        out = r.reshape(-1, self.sino_shape[0] * self.sino_shape[1]) @ self._mat(r.dtype)
        assert out.dtype == r.dtype
        return out.reshape(lead + self.shape)

    fwd, adj = apply, apply_adjoint

    def norm2_bound(self):
        """max(A 1) max(A^T 1) >= sigma_max^2: A has no negative entry."""
        return float(self.A.sum(1).max() * self.A.sum(0).max())


def operator_bound(A, operand, adjoint):
    """The derived bound of every output of A x (adjoint: A^T r), [n_img, outputs]; operand: [n_img, inputs]."""
    M = A.T if adjoint else A
    nz = M > 0
    n = nz.sum(1).astype(np.float64)
    a = np.abs(np.asarray(operand, dtype=np.float64))
    return U * ((n + 2.0)[None, :] * (a @ M.T) + 2.0 * (a @ nz.T.astype(np.float64)))


# ------------------------------------------------------------------ operator cases
OpCase = namedtuple("OpCase", "name shape angles n_det")
PI = math.pi
SEVEN = [0.0, float(np.float32(PI / 2)), PI / 4, 3 * PI / 4, PI, 3.5, -0.3]      # both loop directions, both exact axes, the tie, past pi, negative


def _spread(n, shift=0.013):
    return list(np.linspace(0.0, PI, n, endpoint=False) + shift)


def _op_cases():
    out = [OpCase("12x20-seven", (12, 20), SEVEN, None),
           OpCase("5x3-4", (5, 3), _spread(4), None),
           OpCase("33x17-9", (33, 17), _spread(9), None),
           OpCase("40x136-5", (40, 136), [0.2, 1.0, 1.7, 2.4, 3.0], None),
           OpCase("136x40-5", (136, 40), [0.2, 1.0, 1.7, 2.4, 3.0], None),
           # forward: more than one band in both walking directions (110 rows and 136 columns against bands of 101 and 125 lines); adjoint: 7 x 9 tiles
           OpCase("110x136-bands", (110, 136), [0.3, 1.2, 2.0, 2.9], None),
           # forward: two minor tiles (more than 1024 pixels along a line) in either direction, two bin tiles (more than 256 bins), a clipped detector
           OpCase("3x1100-tiles", (3, 1100), [0.1, 1.3, 3.0], 300),
           OpCase("1100x3-tiles", (1100, 3), [0.1, 1.3, 3.0], 300),
           OpCase("16x16-det9", (16, 16), _spread(5), 9),
           OpCase("16x16-det1", (16, 16), _spread(5), 1),
           OpCase("1x37", (1, 37), _spread(6), None),
           OpCase("37x1", (37, 1), _spread(6), None),
           OpCase("9x11-70", (9, 11), _spread(70), None),       # nine angle chunks, the last ones short
           OpCase("9x11-1", (9, 11), [0.7], None)]
    return out


OP_CASES = _op_cases()
OP_IDS = [c.name for c in OP_CASES]
# the shapes of the bound check on the CPU (tests/test_radon_reference.py): small enough for float32 replays in several orders
BOUND_CASES = [OpCase("12x20", (12, 20), SEVEN, None), OpCase("33x17", (33, 17), _spread(9), None),
               OpCase("40x136", (40, 136), [0.0, PI / 2, PI / 4, 3.5, -0.3, 2.0, 1.0, 0.1, 3 * PI / 4, PI, 1.5], None), OpCase("5x3", (5, 3), _spread(4), None)]


def case_n_det(c):
    return default_n_det(c.shape) if c.n_det is None else c.n_det


def operand(n, size, seed):
    """Noise of unit scale with a few large entries: a large entry shows every weight it meets by itself."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, size)) + (rng.random((n, size)) < 0.02) * 40.0
    return f32(x)


OpRef = namedtuple("OpRef", "x ref64 bound")


@functools.lru_cache(maxsize=None)
def op_references(name):
    """(forward, adjoint) of an operator case: operands [N_IMG, .], float64 results and the derived bounds, flat.  The matrix is not kept."""
    c = OP_CASES[OP_IDS.index(name)]
    nd = case_n_det(c)
    A = dense(c.shape, c.angles, nd)
    x = operand(N_IMG, c.shape[0] * c.shape[1], 11)
    r = operand(N_IMG, len(c.angles) * nd, 12)
    fwd = OpRef(x, x.astype(np.float64) @ A.T, operator_bound(A, x, False))
    adj = OpRef(r, r.astype(np.float64) @ A, operator_bound(A, r, True))
    for ref in (fwd, adj):
        for a in ref:
            a.setflags(write=False)
    return fwd, adj


def worst_ratio(got, ref):
    """(max err / bound over the outputs with a bound > 0, max err over those with bound 0 -- which must be 0)."""
    err = np.abs(np.asarray(got, dtype=np.float64).reshape(ref.ref64.shape) - ref.ref64)
    err = np.where(np.isfinite(err), err, np.inf)
    pos = ref.bound > 0
    ratio = float(np.max(err[pos] / ref.bound[pos])) if pos.any() else 0.0
    return ratio, (float(np.max(err[~pos])) if (~pos).any() else 0.0)


# planted faults: what a wrong kernel computes in place of A (keyword arguments of `dense`)
FAULTS = {"sin-sign": dict(sin_sign=-1.0), "half-pixel": dict(centre_shift=0.5), "origin-one-bin": dict(origin_shift=1.0), "second-bin-dropped": dict(drop_second=True)}


def dense_swapped(shape, angles, n_det):
    """Planted fault: ax indexed with the row and by with the column, on a non-square image (index clamped to the table)."""
    H, W = shape
    ax, by = tables(shape, angles, n_det)
    i = np.minimum(np.arange(H), W - 1)
    j = np.minimum(np.arange(W), H - 1)
    t = (by[:, j][:, None, :] + ax[:, i][:, :, None]).astype(np.float32)
    return dense_from_t(t, n_det)


# ------------------------------------------------------------------ one MYULA step with the Radon operator: "restart" mode of tests/_pixel.py
StepCase = namedtuple("StepCase", "name shape term prior box K iters")
STEP_ANGLES = [0.1, 0.9, float(np.float32(PI / 2)), 2.2, 2.9]
TERMS = ("l2", "pois", "wl2", "hub")


def _step_cases():
    out = []
    for term in TERMS:
        out += [StepCase(f"{term}-grad", (12, 20), term, "grad", None, 0, 1),            # no prox, no noise: the adjoint launch writes the result alone
                StepCase(f"{term}-l1", (12, 20), term, "l1", None, 0, 2),
                StepCase(f"{term}-tv10", (12, 20), term, "tv", None, 10, 2)]             # the tile kernel in the middle
    out += [StepCase("pois-tvpos", (12, 20), "pois", "tv", (0.0, float("inf")), 10, 2),
            StepCase("l2-tv10-pipe", (24, 136), "l2", "tv", None, 10, 2)]               # the pipe kernel in the middle
    return out


STEP_CASES = _step_cases()
STEP_IDS = [c.name for c in STEP_CASES]
StepProblem = namedtuple("StepProblem", "op aux y x0 noise tau gamma sigma_f weight")


@functools.lru_cache(maxsize=None)
def step_operator(shape):
    return RadonRef(shape, STEP_ANGLES)


def term_of(term, op, y, aux, sigma_f, dtype):
    if term == "pois":
        return P.PoissonRef(op, y, aux, sigma_f, dtype=dtype)
    if term == "wl2":
        return W.WL2Ref(op, y, aux, sigma_f, dtype=dtype)
    if term == "hub":
        return HU.HuberRef(op, y, aux, sigma_f, dtype=dtype)
    return X._Data(op, y, sigma_f, dtype)


def l2_value(op, y, sigma_f, x):
    r = op.fwd(np.asarray(x, dtype=np.float64)) - np.asarray(y, dtype=np.float64)
    return 0.5 * sigma_f * (r * r).sum(axis=(-2, -1))


@functools.lru_cache(maxsize=None)
def step_problem(name):
    c = STEP_CASES[STEP_IDS.index(name)]
    rng = np.random.default_rng(1000 * c.shape[0] + c.shape[1] + TERMS.index(c.term))
    op = step_operator(c.shape)
    ss = op.sino_shape
    aux = None
    if c.term == "pois":      # emission: an image of 0 .. 8 per pixel, counts of some tens per bin, states that dip below zero
        img = X.step_image(c.shape) / 25.0
        aux = f32(np.broadcast_to(np.linspace(0.3, 1.0, ss[1])[None, :], ss))
        y = f32(rng.poisson(op.fwd(img) + aux.astype(np.float64)))
        x0 = f32(img[None] + rng.normal(0, 1.0, (N_IMG,) + c.shape) - 0.5)
        gamma, sigma_f, weight = X.POIS_GAMMA, 1.0, X.POIS_TV
    else:
        img = X.step_image(c.shape)
        y = op.fwd(img) + rng.normal(0, 5.0, ss)
        x0 = f32(img[None] + rng.normal(0, 10, (N_IMG,) + c.shape))
        gamma, sigma_f = W.GAMMA, W.SIGMA_F
        weight = X.L1_WEIGHT if c.prior == "l1" else X.TAU_REG
        if c.term == "wl2":
            w = rng.uniform(0.2, 2.0, ss)
            w[-1, :] = 0.0       # an unobserved angle and an unobserved bin
            w[:, 3] = 0.0
            aux = f32(w)
        if c.term == "hub":
            hit = rng.uniform(size=ss) < 0.1
            y = y + np.where(hit, rng.uniform(50.0, 150.0, ss) * rng.choice([-1.0, 1.0], ss), 0.0)
            aux = f32(HU.thresholds(ss))
        y = f32(y)
    tau = 0.5 / (term_of(c.term, op, y, aux, sigma_f, np.float64).grad_lipschitz() + 1.0 / gamma) if c.term != "l2" \
        else 0.5 / (sigma_f * op.norm2_bound() + 1.0 / gamma)
    noise = f32(rng.standard_normal((c.iters, N_IMG) + c.shape))
    for a in (aux, y, x0, noise):
        if a is not None:
            a.setflags(write=False)
    return StepProblem(op, aux, y, x0, noise, float(tau), gamma, sigma_f, weight)


def data_term(c, m, dtype):
    return term_of(c.term, m.op, m.y, m.aux, m.sigma_f, dtype)


def prior_term(c, m, dtype):
    return PR.prior_term(c, m, dtype)      # (reads c.box, c.prior, c.K, c.shape and m.weight)


@functools.lru_cache(maxsize=None)
def step_reference(name):
    """The stages of a step case (tests/_pixel.py's `Stage`): one per iteration, each restarting from the rounded float64 result of the one before."""
    c = STEP_CASES[STEP_IDS.index(name)]
    m = step_problem(name)
    stages = []
    start = m.x0
    for it in range(c.iters):
        res = []
        for dtype in (np.float64, np.float32):
            pf = data_term(c, m, dtype)
            x = start.astype(dtype)
            if c.prior == "grad":
                r = pf.grad(x)
            else:
                r = P.myula_step(pf, prior_term(c, m, dtype), x, m.tau, m.gamma, m.noise[it].astype(dtype), dtype=dtype)
            assert r.dtype == np.dtype(dtype), (name, r.dtype)
            res.append(r)
        stages.append(X.Stage(start, res[0], res[1], *X.bound_of(res[0], res[1]), True))
        start = f32(res[0])
    for st in stages:
        st.ref64.setflags(write=False)
        st.ref32.setflags(write=False)
    return tuple(stages)


worst = PR.worst

"""Reference of the multi-coil SENSE data term (`la.MultiCoilFourierSampling`; LMC_DATA_SENSE in include/lmc_atomi.h): the cases, the float64 reference
(`np.fft.fft2` / `ifft2(norm="ortho")` by the definition in the header), the float32 replay (the same code on float32 / complex64 input, which numpy
computes in single precision: the dtype is asserted) and the bound of tests/_pixel.py, `max(3 e32, 2 ulp32(max |ref64|))` over every chain and pixel or
bin and component, e32 measured on the replay and never on a kernel.

  e_c = M F(S_c x) - b_c,   f = sigma_f / 2 sum_c sum_k |e_c,k|^2,   grad f = sigma_f sum_c Re[conj(S_c) F^H(M e_c)],   coils in the order c = 0, 1, ...

Operands are those of tests/_fourier_ref.py (zero-mean noise of sd 30 plus point sources).  Maps: smooth off-centre Gaussian magnitudes times linear
phase ramps, complex64.  Two weights M: a 40 % binary mask, and that mask times weights in [0.5, 1.5] -- with a binary M and masked data, applying M once
or twice is the same point, so only the second kind tells a kernel that drops one factor of M.  numpy only."""
import functools
from collections import namedtuple

import numpy as np

import _fourier_ref as F
import _pixel as X

N_CHAINS = 3
f32 = X.f32
ri = F.ri
Case = namedtuple("Case", "shape n_coils")
CASES = [Case((8, 8), 1), Case((8, 16), 2), Case((16, 8), 3), Case((32, 64), 4), Case((8, 1024), 2), Case((1024, 8), 2), Case((128, 256), 4)]
IDS = [f"{c.shape[0]}x{c.shape[1]}x{c.n_coils}" for c in CASES]
WEIGHTS = ("binary", "weighted")
SIGMA_N = 5.0                  # noise of the measurements per component
SIGMA_F = 1.0 / SIGMA_N ** 2   # 0.04
FAULTS = ("noconj", "skip_last", "m_once", "drop_imag")


def case(name):
    return CASES[IDS.index(name)]


# ------------------------------------------------------------------ maps, weights
@functools.lru_cache(maxsize=None)
def maps(shape, n_coils):
    """[n_coils, H, W] complex64: coil c is a Gaussian of width 0.6 x the image centred on a circle around it, times exp(i (a_c i + b_c j + phi_c))."""
    H, W = shape
    i, j = np.meshgrid(np.arange(H) / H - 0.5, np.arange(W) / W - 0.5, indexing="ij")
    out = np.empty((n_coils, H, W), dtype=np.complex128)
    for c in range(n_coils):
        ang = 2 * np.pi * (c + 0.25) / n_coils
        ci, cj = 0.45 * np.sin(ang), 0.45 * np.cos(ang)
        mag = 0.2 + np.exp(-((i - ci) ** 2 + (j - cj) ** 2) / (2 * 0.6 ** 2))
        phase = 2 * np.pi * ((0.7 + 0.3 * c) * i - (0.4 + 0.2 * c) * j) + 0.9 * c
        out[c] = mag * np.exp(1j * phase)
    out = out.astype(np.complex64)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def weight(shape, kind):
    """M, float32 [H, W]: the 40 % sampling mask of tests/_fourier_ref.py (fully sampled 4 x 4 centre), alone or times weights in [0.5, 1.5]."""
    m = F.sampling_mask(shape, seed=11, frac=0.4)
    if kind == "weighted":
        m = m * np.random.default_rng(shape[0] * 17 + shape[1]).uniform(0.5, 1.5, shape)
    else:
        assert kind == "binary", kind
    m = f32(m)
    m.setflags(write=False)
    return m


# ------------------------------------------------------------------ the term by its definition
class SenseRef:
    """The operator and the data term in `dtype` (float32: maps and data as complex64, M as float32, numpy's single-precision transforms).  `fault`:
    one of FAULTS, what a wrong kernel computes in place of the gradient / the adjoint."""

    def __init__(self, S, M, b=None, sigma=1.0, dtype=np.float64, fault=None):
        self.dtype = np.dtype(dtype)
        self.ct = np.dtype(np.complex64 if self.dtype == np.float32 else np.complex128)
        self.S, self.M = np.asarray(S).astype(self.ct), np.asarray(M).astype(self.dtype)
        self.b = None if b is None else np.asarray(b).astype(self.ct)
        self.sigma = self.dtype.type(sigma)
        self.S64, self.M64, self.sigma64 = np.asarray(S, dtype=np.complex128), np.asarray(M, dtype=np.float64), float(sigma)
        self.b64 = None if b is None else np.asarray(b, dtype=np.complex128)
        self.fault = fault
        self.n_coils = self.S.shape[0]

    def forward(self, x):
        """[..., H, W] real -> [..., n_coils, H, W] complex: M F(S_c x)."""
        x = np.asarray(x, dtype=self.dtype)
        sx = self.S * x[..., None, :, :]
        if self.fault == "drop_imag":
            sx = sx.real.astype(self.ct)
        out = self.M * np.fft.fft2(sx, norm="ortho")
        assert out.dtype == self.ct, out.dtype
        return out

    def adjoint(self, k, weighted=True):
        """[..., n_coils, H, W] complex -> [..., H, W] real: sum_c Re[conj(S_c) F^H(M k_c)], coil by coil in the order c = 0, 1, ..."""
        k = np.asarray(k, dtype=self.ct)
        v = np.fft.ifft2(self.M * k if weighted else k, norm="ortho")
        s = self.S if self.fault == "noconj" else np.conj(self.S)
        n = self.n_coils - 1 if self.fault == "skip_last" else self.n_coils
        out = np.zeros(k.shape[:-3] + k.shape[-2:], dtype=self.dtype)
        for c in range(n):
            out = out + (s[c] * v[..., c, :, :]).real
        assert out.dtype == self.dtype, out.dtype
        return out

    def grad(self, x):
        e = self.forward(x) - self.b
        out = self.sigma * self.adjoint(e, weighted=self.fault != "m_once")
        assert out.dtype == self.dtype, out.dtype
        return out

    def value(self, x):
        """float64 whatever `dtype`: the definition."""
        x = np.asarray(x, dtype=np.float64)
        e = self.M64 * np.fft.fft2(self.S64 * x[..., None, :, :], norm="ortho") - self.b64
        return 0.5 * self.sigma64 * np.sum(np.abs(e) ** 2, axis=(-3, -2, -1))

    def norm_bound(self):
        return float(np.max(self.M64) ** 2 * np.max(np.sum(np.abs(self.S64) ** 2, axis=0)))

    def grad_lipschitz(self):
        return self.sigma64 * self.norm_bound()

    def hessian_norm(self, iters=60, seed=0):
        """sigma ||A||^2 by power iteration on x -> A^H A x, float64 (a lower bound that converges from below)."""
        x = np.random.default_rng(seed).standard_normal(self.S.shape[1:])
        lam = 0.0
        for _ in range(iters):
            y = self.adjoint(self.forward(x))
            lam = float(np.linalg.norm(y) / np.linalg.norm(x))
            x = y / np.linalg.norm(y)
        return self.sigma64 * lam


Ref = namedtuple("Ref", "x ref64 ref32 e32 bound")


def _ref(x, r64, r32):
    e32, bound = X.bound_of(r64, r32)
    r64.setflags(write=False)
    return Ref(x, r64, r32, e32, bound)


# ------------------------------------------------------------------ the problem of a case: float32 / complex64 numbers, made once
Problem = namedtuple("Problem", "S M b truth x0 noise tau gamma sigma_f")


@functools.lru_cache(maxsize=None)
def problem(shape, n_coils, wkind, iters=2):
    rng = np.random.default_rng(900 * shape[0] + shape[1] + 31 * n_coils + len(wkind))
    S, M = maps(shape, n_coils), weight(shape, wkind)
    truth = F.operand(shape, n=1, seed=5)[0].astype(np.float64)
    clean = SenseRef(S, M).forward(truth)
    b = (clean + rng.normal(0, SIGMA_N, clean.shape) + 1j * rng.normal(0, SIGMA_N, clean.shape)).astype(np.complex64)      # rounded once
    gamma = X.GAMMA
    tau = 0.5 / (SenseRef(S, M, b, SIGMA_F).grad_lipschitz() + 1.0 / gamma)
    x0 = f32(truth[None] + rng.normal(0, 10, (N_CHAINS,) + shape))
    noise = f32(rng.standard_normal((iters, N_CHAINS) + shape))
    for a in (b, x0, noise):
        a.setflags(write=False)
    return Problem(S, M, b, truth, x0, noise, float(tau), gamma, SIGMA_F)


def term(m, dtype=np.float64, fault=None):
    return SenseRef(m.S, m.M, m.b, m.sigma_f, dtype, fault)


# ------------------------------------------------------------------ references
@functools.lru_cache(maxsize=None)
def forward_reference(shape, n_coils, wkind):
    """The operator on the 3 operand images: [3, n_coils, H, W, 2]."""
    S, M = maps(shape, n_coils), weight(shape, wkind)
    x = F.operand(shape)
    return _ref(x, ri(SenseRef(S, M).forward(x)), ri(SenseRef(S, M, dtype=np.float32).forward(x)))


@functools.lru_cache(maxsize=None)
def adjoint_reference(shape, n_coils, wkind):
    """The adjoint on genuine k-space (the operator's float64 result on other operands plus noise, rounded to complex64 once)."""
    S, M = maps(shape, n_coils), weight(shape, wkind)
    rng = np.random.default_rng(shape[0] + 64 * shape[1] + n_coils)
    k = SenseRef(S, M).forward(F.operand(shape, seed=1))
    k = (k + rng.normal(0, SIGMA_N, k.shape) + 1j * rng.normal(0, SIGMA_N, k.shape)).astype(np.complex64)
    k.setflags(write=False)
    return _ref(k, SenseRef(S, M).adjoint(k), SenseRef(S, M, dtype=np.float32).adjoint(k))


@functools.lru_cache(maxsize=None)
def grad_reference(shape, n_coils, wkind):
    m = problem(shape, n_coils, wkind)
    return _ref(m.x0, term(m).grad(m.x0), term(m, np.float32).grad(m.x0))


# ------------------------------------------------------------------ one MYULA step: the "restart" mode of tests/_pixel.py
StepCase = namedtuple("StepCase", "name shape n_coils wkind prior box K")
TGV_K, TGV_ALPHA0 = 7, 2.0
WAVELET = ("db2", 2, 2)      # name, p, levels
BOX = (0.0, 255.0)
STEP_CASES = [StepCase("none", (16, 8), 3, "weighted", "none", None, 0),
              StepCase("l1", (32, 64), 4, "weighted", "l1", None, 0),
              StepCase("tv10-pipe", (16, 256), 2, "weighted", "tv", None, 10),        # the pipe kernel is the middle launch
              StepCase("aniso10", (32, 64), 4, "binary", "aniso", None, 10),
              StepCase("db2", (32, 64), 4, "weighted", "wavelet", None, 0),
              StepCase("tgv7", (32, 64), 4, "weighted", "tgv", None, TGV_K),
              StepCase("tv10-box", (32, 64), 4, "weighted", "tv", BOX, 10)]
STEP_IDS = [c.name for c in STEP_CASES]


def step_case(name):
    return STEP_CASES[STEP_IDS.index(name)]


def prior_weight(c):
    return X.L1_WEIGHT if c.prior == "l1" else X.TAU_REG


class _Prox:
    def __init__(self, fn):
        self.prox = fn


def prior_term(c, dtype):
    import _poisson_ref as P
    wgt = prior_weight(c)
    if c.prior == "none":
        return _Prox(lambda x, t: x)
    if c.prior == "tgv":
        import _tgv_ref as T
        return _Prox(lambda x, t: T.tgv_prox(x, wgt * t, TGV_ALPHA0, TGV_K))
    if c.box is not None:
        return P.TVRef(c.shape, wgt, c.K, c.box, aniso=c.prior == "aniso", dtype=dtype)
    view = namedtuple("V", "shape prior box K")(c.shape, c.prior, c.box, c.K)
    return F.prior_term(view, namedtuple("W", "weight")(wgt), dtype)


@functools.lru_cache(maxsize=None)
def step_reference(name):
    """The stages of a step case (tests/_pixel.py's `Stage`): one per iteration, each restarting from the rounded float64 result of the one before."""
    import _poisson_ref as P
    c = step_case(name)
    m = problem(c.shape, c.n_coils, c.wkind)
    stages, start = [], m.x0
    for it in range(m.noise.shape[0]):
        res = []
        for dtype in (np.float64, np.float32):
            r = P.myula_step(term(m, dtype), prior_term(c, dtype), start.astype(dtype), m.tau, m.gamma, m.noise[it].astype(dtype), dtype=dtype)
            assert r.dtype == np.dtype(dtype), (name, r.dtype)
            res.append(r)
        stages.append(X.Stage(start, res[0], res[1], *X.bound_of(res[0], res[1]), True))
        start = f32(res[0])
    for st in stages:
        st.ref64.setflags(write=False)
    return tuple(stages)


worst = F.worst

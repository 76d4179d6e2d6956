"""Reference of the Fourier-domain data term (`la.FourierSampling`, `la.PeriodicConvolve2D`, `la.rfft2` / `la.irfft2`; LMC_DATA_SPECTRAL in
include/lmc_atomi.h): the cases, the float64 references (`np.fft` in float64, and the direct wrap-around sum for the periodic blur: no FFT in that
one), the float32 replays (`np.fft` on float32 / complex64 input, which numpy computes in single precision: the dtype is asserted) and the bound of
tests/_pixel.py, `max(3 e32, 2 ulp32(max |ref64|))` over every chain and pixel or frequency bin, e32 measured on the replay and never on a kernel.

The data term's reference is its DEFINITION on the full plane, f = sigma/2 sum |G F x - b|^2 and grad f = sigma Re F^H(conj(G) (G F x - b)); the fold onto
the half plane that the library runs is restated apart (`fold`) and held against the definition by tests/test_fourier_reference.py.  Operands are zero-mean
(noise of std 30 plus a few point sources), so that the DC bin does not set the rounding scale.  numpy only."""
import functools
from collections import namedtuple

import numpy as np

from oracle import lmc_oracle as O
import _pixel as X
import _poisson_ref as P
import _tv_aniso_ref as A
import _wavelet as Wv

N_CHAINS = 3
f32 = X.f32
SHAPES = [(8, 8), (16, 64), (64, 16), (8, 1024), (1024, 8), (128, 256)]
SHAPE_IDS = [f"{h}x{w}" for h, w in SHAPES]
FOLD_SHAPES = [(8, 8), (16, 64), (64, 16)]


def ri(c):
    """A complex array as real numbers, [..., 2]: the bound and the errors are taken per component."""
    c = np.asarray(c)
    return np.stack([c.real, c.imag], axis=-1)


def minus_k(a):
    """`a` at -k = ((-i) mod H, (-j) mod W) on the last two axes."""
    return np.roll(np.flip(a, (-2, -1)), (1, 1), (-2, -1))


# ------------------------------------------------------------------ operands
@functools.lru_cache(maxsize=None)
def operand(shape, n=N_CHAINS, seed=0):
    rng = np.random.default_rng(shape[0] * 4096 + shape[1] + 7 * seed)
    x = rng.normal(0, 30.0, (n,) + tuple(shape))
    for c in range(n):
        for _ in range(max(2, shape[0] * shape[1] // 512)):
            x[c, rng.integers(0, shape[0]), rng.integers(0, shape[1])] += rng.choice([-1.0, 1.0]) * rng.uniform(150, 400)
    x -= x.mean(axis=(-2, -1), keepdims=True)
    x = f32(x)
    x.setflags(write=False)
    return x


Ref = namedtuple("Ref", "x ref64 ref32 e32 bound")


def _ref(x, r64, r32):
    e32, bound = X.bound_of(r64, r32)
    r64.setflags(write=False)
    return Ref(x, r64, r32, e32, bound)


@functools.lru_cache(maxsize=None)
def rfft2_reference(shape):
    x = operand(shape)
    r32 = np.fft.rfft2(x, norm="ortho")
    assert r32.dtype == np.complex64, r32.dtype
    return _ref(x, ri(np.fft.rfft2(x.astype(np.float64), norm="ortho")), ri(r32))


@functools.lru_cache(maxsize=None)
def irfft2_reference(shape):
    """The input is a genuine half-plane spectrum (that of the operand, rounded to complex64 once)."""
    c = np.fft.rfft2(operand(shape, seed=1).astype(np.float64), norm="ortho").astype(np.complex64)
    c.setflags(write=False)
    r32 = np.fft.irfft2(c, s=shape, norm="ortho")
    assert r32.dtype == np.float32, r32.dtype
    return _ref(c, np.fft.irfft2(c.astype(np.complex128), s=shape, norm="ortho"), r32)


@functools.lru_cache(maxsize=None)
def roundtrip_reference(shape):
    x = operand(shape)
    r32 = np.fft.irfft2(np.fft.rfft2(x, norm="ortho"), s=shape, norm="ortho")
    assert r32.dtype == np.float32, r32.dtype
    return _ref(x, x.astype(np.float64), r32)


# ------------------------------------------------------------------ the fold onto the half plane, restated from the header text
def fold(G, b):
    """(A, B) on the full plane: A_k = (|G_k|^2 + |G_-k|^2) / 2, B_k = (conj(G_k) b_k + G_-k conj(b_-k)) / 2."""
    G, b = np.asarray(G, dtype=np.complex128), np.asarray(b, dtype=np.complex128)
    return 0.5 * (np.abs(G) ** 2 + np.abs(minus_k(G)) ** 2), 0.5 * (np.conj(G) * b + minus_k(G) * np.conj(minus_k(b)))


def half(a):
    return a[..., : a.shape[-1] // 2 + 1]


def tables(G, b):
    """The [11][H][Wh] planes of the descriptor in float64."""
    Am, B = fold(G, b)
    W = G.shape[-1]
    cg, cb = np.conj(minus_k(np.asarray(G, dtype=np.complex128))), np.conj(minus_k(np.asarray(b, dtype=np.complex128)))
    cg, cb = half(cg).copy(), half(cb).copy()
    for j in (0, W // 2):
        cg[:, j] = 0
        cb[:, j] = 0
    Gh, bh = half(np.asarray(G, dtype=np.complex128)), half(np.asarray(b, dtype=np.complex128))
    return np.stack([half(Am), half(B).real, half(B).imag, Gh.real, Gh.imag, bh.real, bh.imag, cg.real, cg.imag, cb.real, cb.imag])


def grad_folded(x, G, b, sigma, fold_fn=fold):
    Am, B = fold_fn(G, b)
    s = x.shape[-2:]
    return sigma * np.fft.irfft2(half(Am) * np.fft.rfft2(x, norm="ortho") - half(B), s=s, norm="ortho")


def prox_folded(v, G, b, sigma, tau):
    Am, B = fold(G, b)
    s = v.shape[-2:]
    return np.fft.irfft2((np.fft.rfft2(v, norm="ortho") + tau * sigma * half(B)) / (1.0 + tau * sigma * half(Am)), s=s, norm="ortho")


def value_half(x, G, b, sigma):
    t = tables(G, b)
    xh = np.fft.rfft2(x, norm="ortho")
    return 0.5 * sigma * np.sum(np.abs((t[3] + 1j * t[4]) * xh - (t[5] + 1j * t[6])) ** 2 + np.abs((t[7] + 1j * t[8]) * xh - (t[9] + 1j * t[10])) ** 2,
                                axis=(-2, -1))


class SpectralRef:
    """The data term by its definition on the full plane, in `dtype` (float32: G and b as complex64, numpy's single-precision transforms)."""

    def __init__(self, G, b, sigma, dtype=np.float64):
        self.dtype = np.dtype(dtype)
        ct = np.complex64 if self.dtype == np.float32 else np.complex128
        self.G, self.b, self.sigma = np.asarray(G).astype(ct), np.asarray(b).astype(ct), self.dtype.type(sigma)
        self.G64, self.b64, self.sigma64 = np.asarray(G, dtype=np.complex128), np.asarray(b, dtype=np.complex128), float(sigma)

    def grad(self, x):
        x = np.asarray(x, dtype=self.dtype)
        xh = np.fft.fft2(x, norm="ortho")
        r = np.conj(self.G) * (self.G * xh - self.b)
        out = self.sigma * np.fft.ifft2(r, norm="ortho").real
        assert out.dtype == self.dtype, out.dtype
        return out

    def value(self, x):
        xh = np.fft.fft2(np.asarray(x, dtype=np.float64), norm="ortho")
        return 0.5 * self.sigma64 * np.sum(np.abs(self.G64 * xh - self.b64) ** 2, axis=(-2, -1))

    def prox(self, v, tau):
        return prox_folded(np.asarray(v, dtype=np.float64), self.G64, self.b64, self.sigma64, tau)

    def grad_lipschitz(self):
        return self.sigma64 * float(np.max(fold(self.G64, self.b64)[0]))


# ------------------------------------------------------------------ masks, kernels, the periodic blur without an FFT
def sampling_mask(shape, seed=3, frac=0.3):
    """A fully sampled 4 x 4 centre (the lowest frequencies, unshifted order) plus random `frac`: not Hermitian-symmetric."""
    rng = np.random.default_rng(seed + shape[0] * 31 + shape[1])
    m = (rng.uniform(size=shape) < frac).astype(np.float64)
    for i in (-2, -1, 0, 1):
        for j in (-2, -1, 0, 1):
            m[i, j] = 1.0
    assert not np.array_equal(m, minus_k(m))
    return m


def gauss2d(k, s):
    t = np.exp(-0.5 * ((np.arange(k) - k // 2) / s) ** 2)
    h = np.outer(t, t)
    return h / h.sum()


def periodic_direct(x, h, offset, adjoint=False):
    """(H x)[i, j] = sum_ab h[a, b] x[(i - a + oy) mod H, (j - b + ox) mod W] by np.roll, in the dtype of x; adjoint: the transpose."""
    x = np.asarray(x)
    out = np.zeros_like(x)
    for a in range(h.shape[0]):
        for b_ in range(h.shape[1]):
            sh = (a - offset[0], b_ - offset[1])
            if adjoint:
                sh = (-sh[0], -sh[1])
            out = out + x.dtype.type(h[a, b_]) * np.roll(x, sh, (-2, -1))
    return out


def periodic_gain(shape, h, offset):
    """G: the unnormalised DFT of the kernel wrapped about its origin."""
    k = np.zeros(shape)
    for a in range(h.shape[0]):
        for b_ in range(h.shape[1]):
            k[(a - offset[0]) % shape[0], (b_ - offset[1]) % shape[1]] += h[a, b_]
    return np.fft.fft2(k)


ConvCase = namedtuple("ConvCase", "name shape h offset")


def _conv_cases():
    rng = np.random.default_rng(21)
    out = [ConvCase("asym5x3-16x64", (16, 64), rng.uniform(0.1, 1.0, (5, 3)) * np.linspace(1, 2, 5)[:, None], (1, 2)),
           ConvCase("gauss31-64x64", (64, 64), gauss2d(31, 5.0), (15, 15)),
           ConvCase("full-16x64", (16, 64), rng.uniform(0.0, 1.0, (16, 64)) / 512.0, (3, 40))]
    out = [c._replace(h=f32(c.h / c.h.sum()).astype(np.float64)) for c in out]
    for c in out:
        c.h.setflags(write=False)
    return out


CONV_CASES = _conv_cases()
CONV_IDS = [c.name for c in CONV_CASES]


@functools.lru_cache(maxsize=None)
def conv_reference(name, adjoint):
    c = CONV_CASES[CONV_IDS.index(name)]
    x = operand(c.shape, seed=2 + int(adjoint))
    r32 = periodic_direct(x, c.h, c.offset, adjoint)
    assert r32.dtype == np.float32
    return _ref(x, periodic_direct(x.astype(np.float64), c.h, c.offset, adjoint), r32)


# ------------------------------------------------------------------ one MYULA step: the "restart" mode of tests/_pixel.py
StepCase = namedtuple("StepCase", "name shape op prior box K iters")      # op: mask / wmask / transfer / ("periodic", k)


def _step_cases():
    return [StepCase("mask-tv10-pipe", (32, 256), "mask", "tv", None, 10, 2),            # the prior launch is a pipe kernel
            StepCase("mask-tv10-split", (64, 64), "mask", "tv", None, 10, 2),             # ... the split / tile kernel
            StepCase("wmask-l1", (16, 64), "wmask", "l1", None, 0, 2),                    # non-binary weights per frequency
            StepCase("transfer-tvpos", (64, 64), "transfer", "tv", (0.0, float("inf")), 10, 2),
            StepCase("periodic15-aniso", (64, 64), ("periodic", 15), "aniso", None, 10, 2),
            StepCase("periodic-wavelet", (64, 16), ("periodic", 7), "wavelet", None, 0, 2),
            StepCase("grad-8x8", (8, 8), "mask", "grad", None, 0, 1),                     # L2.grad alone: the overwrite form
            StepCase("grad-128x256", (128, 256), "mask", "grad", None, 0, 1)]


STEP_CASES = _step_cases()
STEP_IDS = [c.name for c in STEP_CASES]
WAVELET = ("db2", 2, 2)      # name, p, levels
SIGMA_N = 4.0                # noise of the measurements per component

StepProblem = namedtuple("StepProblem", "mask transfer weights h offset G b y x0 noise tau gamma sigma_f weight")


@functools.lru_cache(maxsize=None)
def step_problem(name):
    """mask / transfer / weights / y: what the Python surface is given; G, b: the gain and data they define (G = mask transfer sqrt(w), b = y sqrt(w);
    periodic: G = DFT of the wrapped kernel, b = F(y))."""
    c = STEP_CASES[STEP_IDS.index(name)]
    shape = c.shape
    rng = np.random.default_rng(500 * shape[0] + shape[1] + len(name))
    truth = operand(shape, n=1, seed=5)[0].astype(np.float64)
    mask = transfer = weights = h = offset = None
    cn = lambda: rng.normal(0, SIGMA_N, shape) + 1j * rng.normal(0, SIGMA_N, shape)       # independent complex noise: not Hermitian
    if isinstance(c.op, tuple):
        k = c.op[1]
        h, offset = f32(gauss2d(k, k / 6.0) * (1.0 + 0.3 * np.linspace(-1, 1, k)[:, None])).astype(np.float64), (k // 2, k // 2 - 1)
        y = f32(periodic_direct(truth, h, offset) + rng.normal(0, SIGMA_N, shape))
        G, b = periodic_gain(shape, h, offset), np.fft.fft2(y.astype(np.float64), norm="ortho")
    else:
        mask = sampling_mask(shape)
        G = mask.astype(np.complex128)
        if c.op == "transfer":
            transfer = (rng.normal(1.0, 0.3, shape) + 1j * rng.normal(0, 0.3, shape)).astype(np.complex64).astype(np.complex128)
            G = G * transfer
        y = (G * np.fft.fft2(truth, norm="ortho") + cn()).astype(np.complex64).astype(np.complex128)
        b = y
        if c.op == "wmask":
            weights = f32(rng.uniform(0.25, 2.0, shape)).astype(np.float64)
            G, b = G * np.sqrt(weights), b * np.sqrt(weights)
    sigma_f, gamma = 1.0 / SIGMA_N ** 2, X.GAMMA
    weight = X.L1_WEIGHT if c.prior == "l1" else X.TAU_REG
    tau = 0.5 / (SpectralRef(G, b, sigma_f).grad_lipschitz() + 1.0 / gamma)
    x0 = f32(truth[None] + rng.normal(0, 10, (N_CHAINS,) + shape))
    noise = f32(rng.standard_normal((c.iters, N_CHAINS) + shape))
    for a in (x0, noise):
        a.setflags(write=False)
    return StepProblem(mask, transfer, weights, h, offset, G, b, y, x0, noise, float(tau), gamma, sigma_f, weight)


class _Prox:
    def __init__(self, fn):
        self.prox = fn


def prior_term(c, m, dtype):
    wgt = m.weight
    if c.box is not None:
        return P.TVRef(c.shape, wgt, c.K, c.box, aniso=c.prior == "aniso", dtype=dtype)
    if c.prior == "tv":
        return _Prox(lambda x, t: O.tv_prox_fgp(x, wgt * t, c.K))
    if c.prior == "aniso":
        return _Prox(lambda x, t: A.tv_prox_aniso(x, wgt * t, c.K))
    if c.prior == "l1":
        def soft(x, t):
            thr = x.dtype.type(wgt * t)
            return np.sign(x) * np.maximum(np.abs(x) - thr, x.dtype.type(0))
        return _Prox(soft)
    if c.prior == "wavelet":
        return _Prox(lambda x, t: Wv.prox(x, WAVELET[1], WAVELET[2], wgt * t).astype(x.dtype))
    raise ValueError(c.prior)


@functools.lru_cache(maxsize=None)
def step_reference(name):
    """The stages of a step case (tests/_pixel.py's `Stage`): one per iteration, each restarting from the rounded float64 result of the one before."""
    c = STEP_CASES[STEP_IDS.index(name)]
    m = step_problem(name)
    stages, start = [], m.x0
    for it in range(c.iters):
        res = []
        for dtype in (np.float64, np.float32):
            pf = SpectralRef(m.G, m.b, m.sigma_f, dtype)
            x = start.astype(dtype)
            r = pf.grad(x) if c.prior == "grad" else P.myula_step(pf, prior_term(c, m, dtype), x, m.tau, m.gamma, m.noise[it].astype(dtype), dtype=dtype)
            assert r.dtype == np.dtype(dtype), (name, r.dtype)
            res.append(r)
        stages.append(X.Stage(start, res[0], res[1], *X.bound_of(res[0], res[1]), True))
        start = f32(res[0])
    for st in stages:
        st.ref64.setflags(write=False)
    return tuple(stages)


def worst(got, ref64):
    """(max |got - ref64|, its index) over every chain and pixel / bin; a value that is not finite counts as infinite."""
    d = np.abs(np.asarray(got, dtype=np.float64) - ref64)
    d = np.where(np.isfinite(d), d, np.inf)
    k = np.unravel_index(int(np.argmax(d)), d.shape)
    return float(d[k]), tuple(int(v) for v in k)


# ------------------------------------------------------------------ planted faults: what a wrong transform or fold computes in place of the reference
def fault_conjugate(x):                  # the conjugate transform direction
    return np.conj(np.fft.rfft2(x, norm="ortho"))


def fault_norm(x):                       # 1 / N in place of 1 / sqrt(N)
    return np.fft.rfft2(x, norm="forward")


def fault_transposed(x):                 # transposed frequency indices (non-square cases): bin (i, j) holds frequency (j, i) where that exists
    full = np.fft.fft2(x, norm="ortho")
    H, W = x.shape[-2:]
    out = np.fft.rfft2(x, norm="ortho").copy()
    n = min(H, W // 2 + 1)
    out[..., :n, :n] = np.swapaxes(full[..., :n, :n], -2, -1)
    return out


def fault_nyquist_dropped(x):            # the Nyquist column dropped
    out = np.fft.rfft2(x, norm="ortho").copy()
    out[..., -1] = 0
    return out


def fold_at_k(G, b):                     # the fold taken at k instead of -k
    G, b = np.asarray(G, dtype=np.complex128), np.asarray(b, dtype=np.complex128)
    return np.abs(G) ** 2, 0.5 * (np.conj(G) * b + G * np.conj(b))


def mask_shifted(mask):                  # the mask applied at fftshifted positions
    return np.fft.fftshift(mask)


TRANSFORM_FAULTS = [fault_conjugate, fault_norm, fault_transposed, fault_nyquist_dropped]

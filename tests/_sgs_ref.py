"""Reference of the split Gibbs sampler (`la.SplitGibbsSampler`, lmc_sgs_* in include/lmc_atomi.h): a numpy, dtype-generic restatement of the header
text -- the x-draw through `np.fft` with the half-plane tables of tests/_fourier_ref.py, the pixel-diagonal draw, the z-step with the checker's proxes --
the cases of tests/test_gpu_sgs.py, their float64 reference, two float32 replays (the definition's form, and the kernel's order of operations with its
fused multiply-adds) and the bound of tests/_pixel.py: `max(3 e32, 2 ulp32(max |ref64|))` per plane, e32 the smaller of the two replays' errors, measured
on the replays and never on a kernel.  The planted faults are what a wrong kernel would compute in place of the float64 reference.  numpy only."""
import functools
from collections import namedtuple

import numpy as np

from oracle import lmc_oracle as O
import _fourier_ref as F
import _pixel as X
import _poisson_ref as P
import _tgv_ref as T
import _tv_aniso_ref as A
import _wavelet as Wv

f32 = X.f32
GAMMA = X.GAMMA
TAU_FRACTION = 0.8                       # tau = 0.8 sgs_step_bound(rho, gamma)
SPECTRAL_RHO, SPECTRAL_SIGMA_N = 3.0, 4.0
DIAG_RHO, DIAG_SIGMA_N = 0.9, 0.75
TGV_ALPHA0, TGV_K = 0.5, 7
WAVELET = ("db2", 2, 2)                  # name, p, levels
BOX = (0.0, 255.0)
SPECTRAL_BOX = (-40.0, 60.0)             # the spectral operands are zero-mean
FAULTS = ("noise_over_q", "rho_not_squared", "no_B", "coupling_sign", "coupling_zprime", "stale_x", "planes_swapped")

# kind: 'spectral' | 'diag'; term: 'mask' | 'periodic' (spectral), 'identity' | 'mask' | 'weights' (diag); prior: 'tv' | 'aniso' | 'l1' | 'wavelet' | 'tgv';
# box: None | (lo, hi) (TV only)
Case = namedtuple("Case", "kind shape term prior box n_inner")


def case_id(c):
    return f"{c.kind}-{c.shape[0]}x{c.shape[1]}-{c.term}-{c.prior}{'box' if c.box else ''}" + (f"-inner{c.n_inner}" if c.n_inner > 1 else "")


def _cases():
    out = []
    # 8 x 8, 16 x 8, 8 x 64: the smallest and the non-square sides, the short-line LDS layout; 64 x 128: two column strips, the second of one column;
    # 128 x 32: a partial strip of 17 columns
    for s in [(8, 8), (16, 8), (8, 64), (64, 128), (128, 32)]:
        for t in ("mask", "periodic"):
            out.append(Case("spectral", s, t, "tv", None, 1))
    for p in ("aniso", "l1", "wavelet", "tgv"):
        out.append(Case("spectral", (16, 8), "mask", p, None, 1))
    out.append(Case("spectral", (16, 8), "periodic", "tv", SPECTRAL_BOX, 1))
    out.append(Case("spectral", (8, 64), "periodic", "tv", None, 3))
    # 1 x 9, 5 x 7, 33 x 70: W % 4 != 0, the scalar form; 64 x 136: the 16-byte form, more than one workgroup
    for s in [(1, 9), (5, 7), (33, 70), (64, 136)]:
        for t in ("identity", "mask", "weights"):
            out.append(Case("diag", s, t, "tv", None, 1))
    for p in ("aniso", "l1", "tgv"):
        out.append(Case("diag", (33, 70), "weights", p, None, 1))
    out.append(Case("diag", (64, 136), "mask", "wavelet", None, 1))
    out.append(Case("diag", (33, 70), "mask", "tv", BOX, 1))
    out.append(Case("diag", (5, 7), "identity", "tv", None, 3))
    out.append(Case("diag", (33, 72), "mask", "tv", None, 1))       # W % 4 == 0 with H % 4 != 0: the 16-byte forms with a partial last quad of rows
    return out


CASES = _cases()
IDS = [case_id(c) for c in CASES]
assert len(set(IDS)) == len(IDS)


def n_chains(c):
    return 3 if c.shape[0] * c.shape[1] <= 1024 else 2


def rinv32(rho):
    """1 / rho^2 as the library forms it: float32, 1 / (rho * rho)."""
    return np.float32(1.0) / (np.float32(rho) * np.float32(rho))


def step_bound(rho, gamma):
    return 1.0 / (1.0 / rho ** 2 + 1.0 / gamma)


# ------------------------------------------------------------------ the problem of a case: float32 numbers, made once
# G, b: the spectral gain and data (complex128, what the device objects define); mask2 / h / offset / y: what the Python surface is given;
# b_img, w, m: the diagonal term (float32 or None); x0, z0: the starting planes; noise: [1 + n_inner, C, H, W]
Problem = namedtuple("Problem", "G b mask2 h offset y b_img w m x0 z0 noise rho tau gamma sigma_f weight")


def prior_weight(c):
    return {"tv": X.TAU_REG, "aniso": X.TAU_REG, "l1": X.L1_WEIGHT, "wavelet": X.TAU_REG, "tgv": 1.0}[c.prior]


@functools.lru_cache(maxsize=None)
def problem(c):
    shape, C = c.shape, n_chains(c)
    rng = np.random.default_rng(77 * shape[0] + shape[1] + 1000 * len(case_id(c)))
    G = b = mask2 = h = offset = y = b_img = w = m = None
    if c.kind == "spectral":
        truth = F.operand(shape, n=1, seed=5)[0].astype(np.float64)
        rho, sn = SPECTRAL_RHO, SPECTRAL_SIGMA_N
        if c.term == "mask":
            mask2 = F.sampling_mask(shape)
            assert (mask2 == 0).any()
            G = mask2.astype(np.complex128)
            y = (G * np.fft.fft2(truth, norm="ortho") + rng.normal(0, sn, shape) + 1j * rng.normal(0, sn, shape)).astype(np.complex64).astype(np.complex128)
            b = y
        else:
            k = 7
            h, offset = f32(F.gauss2d(k, k / 6.0)).astype(np.float64), (k // 2, k // 2)
            y = f32(F.periodic_direct(truth, h, offset) + rng.normal(0, sn, shape))
            G, b = F.periodic_gain(shape, h, offset), np.fft.fft2(y.astype(np.float64), norm="ortho")
        z0 = f32(truth[None] + rng.normal(0, 10, (C,) + shape))
    else:
        truth = X.step_image(shape, 250.0 if c.box else 190.0)
        rho, sn = DIAG_RHO, DIAG_SIGMA_N
        b_img = f32(truth + rng.normal(0, sn, shape))
        if c.term == "mask":
            m = f32(rng.uniform(size=shape) < 0.6)
            m[0, -1] = 0.0
            b_img = f32(b_img * m)
        elif c.term == "weights":
            w = f32(rng.uniform(0.25, 2.0, shape))
            w[0, 0] = 0.0
            w[-1, -1] = 0.0
        z0 = f32(truth[None] + rng.normal(0, 10, (C,) + shape))
    x0 = f32(z0 + rng.normal(0, 3, z0.shape))
    noise = f32(rng.standard_normal((1 + c.n_inner, C) + shape))
    tau = float(np.float32(TAU_FRACTION * step_bound(rho, GAMMA)))
    for a in (mask2, h, y, b_img, w, m, x0, z0, noise):
        if a is not None:
            a.setflags(write=False)
    return Problem(G, b, mask2, h, offset, y, b_img, w, m, x0, z0, noise, rho, tau, GAMMA, 1.0 / sn ** 2, prior_weight(c))


# ------------------------------------------------------------------ the two stages, in the dtype handed in
def fma(a, b, c):
    """float32 fused multiply-add: the product of two float32 is exact in float64, the sum is rounded to float64 and then to float32."""
    return (np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(c, dtype=np.float64)).astype(np.float32)


def tables(G, b, dtype):
    """(A, B) on the half plane, folded in float64 and rounded once to `dtype` (lmc_spectral_tables)."""
    Am, B = F.fold(G, b)
    ct = np.complex64 if np.dtype(dtype) == np.float32 else np.complex128
    return F.half(Am).astype(dtype), F.half(B).astype(ct)


def xdraw_spectral(z, xi, Ah, Bh, sigma_f, rho, dtype, order="definition", fault=None):
    """x = irfft2((rfft2(z) / rho^2 + sigma_f B + sqrt(q) rfft2(xi)) / q), q = sigma_f A + 1 / rho^2; xi = None: the conditional mean."""
    dt = np.dtype(dtype).type
    z = np.asarray(z, dtype=dtype)
    shape = z.shape[-2:]
    rinv = dt(rinv32(rho)) if dtype == np.float32 else dt(1.0) / (dt(rho) * dt(rho))
    if fault == "rho_not_squared":
        rinv = dt(1.0) / dt(rho)
    sf = dt(sigma_f)
    zh = np.fft.rfft2(z, norm="ortho")
    nh = np.zeros_like(zh) if xi is None else np.fft.rfft2(np.asarray(xi, dtype=dtype), norm="ortho")
    assert zh.dtype == (np.complex64 if dtype == np.float32 else np.complex128), zh.dtype
    Bs = Bh * dt(0) if fault == "no_B" else Bh
    if order == "kernel" and dtype == np.float32:
        q = fma(sf, Ah, rinv)
        g = q if fault == "noise_over_q" else np.sqrt(q)
        num = fma(zh.real, rinv, fma(sf, Bs.real, nh.real * g)) + 1j * fma(zh.imag, rinv, fma(sf, Bs.imag, nh.imag * g)).astype(np.complex64)
        sp = (num.real / q + 1j * (num.imag / q)).astype(np.complex64)
    else:
        q = sf * Ah + rinv
        g = q if fault == "noise_over_q" else np.sqrt(q)
        sp = (zh * rinv + sf * Bs + g * nh) / q
    out = np.fft.irfft2(sp.astype(zh.dtype), s=shape, norm="ortho")
    assert out.dtype == np.dtype(dtype), out.dtype
    return out


def xdraw_diag(z, xi, b, w, m, sigma_f, rho, dtype, order="definition", fault=None):
    """x_p = (z_p / rho^2 + sigma_f w_p m_p b_p + sqrt(q_p) xi_p) / q_p, q_p = sigma_f w_p m_p^2 + 1 / rho^2; b = None: no data term."""
    dt = np.dtype(dtype).type
    z = np.asarray(z, dtype=dtype)
    xi = np.zeros_like(z) if xi is None else np.asarray(xi, dtype=dtype)
    rinv = dt(rinv32(rho)) if dtype == np.float32 else dt(1.0) / (dt(rho) * dt(rho))
    if fault == "rho_not_squared":
        rinv = dt(1.0) / dt(rho)
    sf = dt(sigma_f if b is not None else 0.0)
    one = np.ones(z.shape[-2:], dtype=dtype)
    b_ = np.zeros_like(one) if b is None else np.asarray(b, dtype=dtype)
    w_ = one if w is None else np.asarray(w, dtype=dtype)
    m_ = one if m is None else np.asarray(m, dtype=dtype)
    bs = b_ * dt(0) if fault == "no_B" else b_
    cw = (sf * w_) * m_
    if order == "kernel" and dtype == np.float32:
        q = fma(cw, m_, rinv)
        g = q if fault == "noise_over_q" else np.sqrt(q)
        out = fma(z, rinv, fma(cw, bs, g * xi)) / q
    else:
        q = cw * m_ + rinv
        g = q if fault == "noise_over_q" else np.sqrt(q)
        out = (z * rinv + cw * bs + g * xi) / q
    assert out.dtype == np.dtype(dtype), out.dtype
    return out


class _Prox:
    def __init__(self, fn):
        self.prox = fn


def prior_term(c, m, dtype, tgv_form="div"):
    wgt = m.weight
    if c.box is not None:
        return P.TVRef(c.shape, wgt, 10, c.box, aniso=c.prior == "aniso", dtype=dtype)
    if c.prior == "tv":
        return _Prox(lambda x, t: O.tv_prox_fgp(x, wgt * t, 10))
    if c.prior == "aniso":
        return _Prox(lambda x, t: A.tv_prox_aniso(x, wgt * t, 10))
    if c.prior == "l1":
        def soft(x, t):
            thr = x.dtype.type(wgt * t)
            return np.sign(x) * np.maximum(np.abs(x) - thr, x.dtype.type(0))
        return _Prox(soft)
    if c.prior == "wavelet":
        return _Prox(lambda x, t: Wv.prox(x, WAVELET[1], WAVELET[2], wgt * t).astype(x.dtype))
    if c.prior == "tgv":
        return _Prox(lambda x, t: T.tgv_prox(x, wgt * t, TGV_ALPHA0, TGV_K, form=tgv_form))
    raise ValueError(c.prior)


def zstep(pg, z, x, xi, rho, tau, gamma, dtype, order="definition", fault=None, epsg=1.0):
    """z+ = z - (tau / rho^2)(z - x) - (tau / gamma)(z - prox_{epsg gamma g}(z)) + sqrt(2 tau) xi."""
    dt = np.dtype(dtype).type
    z, x, xi = (np.asarray(a, dtype=dtype) for a in (z, x, xi))
    px = pg.prox(z, epsg * gamma)
    assert px.dtype == np.dtype(dtype), px.dtype
    if dtype == np.float32:
        rinv, b, s = rinv32(rho), np.float32(tau) / np.float32(gamma), np.sqrt(np.float32(2.0) * np.float32(tau))
        coef = np.float32(tau) * rinv
    else:
        rinv, b, s = 1.0 / rho ** 2, tau / gamma, np.sqrt(2.0 * tau)
        coef = tau * rinv
    sign = dt(-1) if fault == "coupling_sign" else dt(1)
    if order == "kernel" or fault == "coupling_zprime":      # the launches: the step without a data term, then the coupling with the z it started from
        zp = (dt(1) - b) * z + b * px + s * xi
        base = zp if fault == "coupling_zprime" else z
        out = fma(-sign * coef, base - x, zp) if dtype == np.float32 else zp - sign * coef * (base - x)
    else:
        out = z - sign * coef * (z - x) - b * (z - px) + s * xi
    assert out.dtype == np.dtype(dtype), out.dtype
    return out


def iteration(c, m, x_prev, z, noise, dtype, order="definition", fault=None):
    """One iteration from (x_prev, z) with noise [1 + n_inner, C, H, W]: (x, z+).  x_prev enters through a planted fault only."""
    noise = np.asarray(noise)
    if fault == "planes_swapped":
        noise = np.concatenate([noise[1:2], noise[0:1], noise[2:]])
    if c.kind == "spectral":
        Ah, Bh = tables(m.G, m.b, dtype)
        x = xdraw_spectral(z, noise[0], Ah, Bh, m.sigma_f, m.rho, dtype, order, fault)
    else:
        x = xdraw_diag(z, noise[0], m.b_img, m.w, m.m, m.sigma_f, m.rho, dtype, order, fault)
    pg = prior_term(c, m, dtype, "kernel" if order == "kernel" else "div")      # (TGV: the displacement form the prox kernel iterates on)
    zz = np.asarray(z, dtype=dtype)
    xc = np.asarray(x_prev, dtype=dtype) if fault == "stale_x" else x
    for j in range(c.n_inner):
        zz = zstep(pg, zz, xc, noise[1 + j], m.rho, m.tau, m.gamma, dtype, order, fault)
    return x, zz


Ref = namedtuple("Ref", "x64 z64 ex bx ez bz")      # e: the better replay's error, b: the bound, per plane


@functools.lru_cache(maxsize=None)
def reference(c):
    m = problem(c)
    x64, z64 = iteration(c, m, m.x0, m.z0, m.noise, np.float64)
    reps = [iteration(c, m, m.x0, m.z0, m.noise, np.float32, order) for order in ("definition", "kernel")]
    ex, bx = min((X.bound_of(x64, r[0]) for r in reps), key=lambda eb: eb[0])
    ez, bz = min((X.bound_of(z64, r[1]) for r in reps), key=lambda eb: eb[0])
    for a in (x64, z64):
        a.setflags(write=False)
    return Ref(x64, z64, ex, bx, ez, bz)


def faulty(c, fault):
    """(x, z+) of the float64 reference with `fault` planted."""
    m = problem(c)
    return iteration(c, m, m.x0, m.z0, m.noise, np.float64, fault=fault)


def leaves_bound(c, fault):
    """Whether the planted fault is outside the bound of case `c` on either plane, and by how much: (bool, err_x / bound_x, err_z / bound_z)."""
    r = reference(c)
    x, z = faulty(c, fault)
    rx, rz = float(np.max(np.abs(x - r.x64))) / r.bx, float(np.max(np.abs(z - r.z64))) / r.bz
    return rx > 1.0 or rz > 1.0, rx, rz


# ------------------------------------------------------------------ the Gaussian-prior exactness check
# g = theta / 2 ||z||^2: pi_rho is Gaussian and diagonal in the Fourier basis.  Per frequency the precision of (x_k, z_k) is [[q_k, -r], [-r, theta + r]],
# r = 1 / rho^2, q_k = sigma_f A_k + r, so the x-marginal has variance (theta + r) / (q_k (theta + r) - r^2).
GAUSS_SHAPE, GAUSS_N, GAUSS_ITERS = (8, 8), 2000, 40
GAUSS_RHO, GAUSS_THETA, GAUSS_SIGMA_F = 1.5, 1.0 / 1.5 ** 2, 2.0
GAUSS_SE = 5.0


def gauss_problem():
    rng = np.random.default_rng(11)
    G = rng.normal(size=GAUSS_SHAPE) + 1j * rng.normal(size=GAUSS_SHAPE)
    G[rng.random(GAUSS_SHAPE) < 0.4] = 0
    mask = (G != 0).astype(np.float64)
    transfer = np.where(G != 0, G, 1.0).astype(np.complex64).astype(np.complex128)
    y = (rng.normal(size=GAUSS_SHAPE) + 1j * rng.normal(size=GAUSS_SHAPE)).astype(np.complex64).astype(np.complex128)
    return mask, transfer, mask * transfer, y


def gauss_marginal_variance(G):
    """Var of the unitary-DFT coefficient x_k under the x-marginal of pi_rho, on the full plane."""
    Am, _ = F.fold(G, np.zeros_like(G))
    r = 1.0 / GAUSS_RHO ** 2
    q = GAUSS_SIGMA_F * Am + r
    return (GAUSS_THETA + r) / (q * (GAUSS_THETA + r) - r * r)


def gauss_check(x, G, what):
    """x: [N, H, W] independent draws.  The sample variance over the draws of Re and Im of every DFT coefficient against the closed form -- v_k for the
    real coefficients (k = -k), v_k / 2 for each part of the others -- within GAUSS_SE standard errors, the relative sd of a variance estimate from N
    draws being sqrt(2 / N).  Returns the worst |ratio - 1| in standard errors."""
    N = x.shape[0]
    xh = np.fft.fft2(np.asarray(x, dtype=np.float64), norm="ortho")
    v = gauss_marginal_variance(G)
    selfc = np.zeros(G.shape, dtype=bool)
    for i in (0, G.shape[0] // 2):
        for j in (0, G.shape[1] // 2):
            selfc[i, j] = True
    want_re = np.where(selfc, v, v / 2)
    se = np.sqrt(2.0 / N)
    dev_re = np.abs(xh.real.var(axis=0, ddof=1) / want_re - 1.0) / se
    dev_im = np.abs(xh.imag.var(axis=0, ddof=1)[~selfc] / (v[~selfc] / 2) - 1.0) / se
    worst = float(max(dev_re.max(), dev_im.max()))
    print(f"{what}: worst per-frequency variance deviation {worst:.2f} standard errors (limit {GAUSS_SE}), N = {N}")
    return worst


def gauss_chain_cpu(fault=None, seed=5):
    """The two-block Gibbs sampler with the exact z | x conditional, GAUSS_N chains for GAUSS_ITERS iterations from zero: the final x [N, H, W]."""
    _, _, G, y = gauss_problem()
    Ah, Bh = tables(G, y, np.float64)
    rng = np.random.default_rng(seed)
    r = 1.0 / GAUSS_RHO ** 2
    z = np.zeros((GAUSS_N,) + GAUSS_SHAPE)
    for _ in range(GAUSS_ITERS):
        x = xdraw_spectral(z, rng.standard_normal(z.shape), Ah, Bh, GAUSS_SIGMA_F, GAUSS_RHO, np.float64, fault=fault)
        z = (x * r) / (GAUSS_THETA + r) + rng.standard_normal(z.shape) / np.sqrt(GAUSS_THETA + r)
    return x, G

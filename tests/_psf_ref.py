"""Reference of the large point-spread functions (`la.PSF`, LMC_DATA_PSF / POISSON_PSF / WL2_PSF in include/lmc_atomi.h): the case lists, the float64 and
float32 replays of the checker (oracle/lmc_oracle.py: `blur`, `blur_adjoint` take any kernel size and compute in the dtype of their input) and the bound
of tests/_pixel.py, `max(3 e32, 2 ulp32(max |ref64|))` with e32 measured on the checker's own float32 replay and never on a kernel.  Every input is rounded
to float32 once; the library gets those numbers, the checker gets them cast back to float64.  numpy only: tests/test_psf_reference.py (CPU) checks this
harness, tests/test_gpu_psf.py runs the kernels against it."""
import functools
from collections import namedtuple

import numpy as np

from oracle import lmc_oracle as O
import _pixel as X
import _poisson_ref as P
import _tv_aniso_ref as A
import _wl2_ref as W

N_CHAINS = 3
MAX_PSF = 33
SEP_RTOL = 2.0 ** -22
f32 = X.f32


# ------------------------------------------------------------------ kernels
def random_taps(kh, kw, seed):
    """Positive, asymmetric in both directions (a ramp times noise), normalised to sum 1."""
    rng = np.random.default_rng(seed)
    h = rng.uniform(0.2, 1.0, (kh, kw)) * np.linspace(1.0, 3.0, kh)[:, None] * np.linspace(2.0, 1.0, kw)[None, :]
    return h / h.sum()


def gauss1d(k, s):
    t = np.exp(-0.5 * ((np.arange(k) - k // 2) / s) ** 2)
    return t / t.sum()


OpCase = namedtuple("OpCase", "name shape h offset separable")


def _op_cases():
    out = []
    for shape, (kh, kw), off in [((37, 70), (13, 11), (4, 7)), ((5, 7), (13, 11), (6, 5)),            # the second: the image is smaller than the PSF
                                 ((20, 24), (33, 33), (16, 16)), ((70, 37), (12, 10), (3, 7)),        # even sizes, off-centre
                                 ((130, 150), (33, 21), (0, 20)),                                     # several tiles both ways, origin on an edge
                                 ((33, 65), (17, 17), (16, 0))]:
        out.append(OpCase(f"gen-{shape[0]}x{shape[1]}-{kh}x{kw}", shape, f32(random_taps(kh, kw, kh * 100 + kw)), off, False))
    rng = np.random.default_rng(77)
    sep = [((40, 72), np.outer(gauss1d(21, 3.5), gauss1d(21, 3.5)), (10, 10)),
           ((40, 200), gauss1d(31, 5.0)[None, :], (0, 15)),
           ((200, 40), gauss1d(31, 5.0)[:, None], (15, 0)),
           ((37, 70), np.outer(gauss1d(33, 5.0), gauss1d(15, 2.5)), (16, 7)),
           ((37, 70), np.outer(rng.uniform(0.2, 1.0, 12), rng.uniform(0.2, 1.0, 10)), (3, 7))]
    for shape, h, off in sep:
        h = h / h.sum()
        out.append(OpCase(f"sep-{shape[0]}x{shape[1]}-{h.shape[0]}x{h.shape[1]}", shape, f32(h), off, True))
    for c in out:
        c.h.setflags(write=False)
    return out


CASES = _op_cases()
OP_CASES = [c for c in CASES if not c.separable]
SEP_CASES = [c for c in CASES if c.separable]
IDS = [c.name for c in CASES]


def separable_factors(h):
    """(u, v, worst deviation) of the criterion of lmc_psf_separable restated: pivot of largest magnitude, u_a = h[a][pb] / h[pa][pb], v_b = h[pa][b] in
    float64; worst = max |u_a v_b - h_ab| / |h_ab| (inf where a zero tap is not reproduced as zero).  Separable: worst <= 2^-22."""
    h = np.asarray(h, dtype=np.float64)
    pa, pb = np.unravel_index(int(np.argmax(np.abs(h))), h.shape)
    if h[pa, pb] == 0:
        return None, None, np.inf
    u, v = h[:, pb] / h[pa, pb], h[pa, :].copy()
    d = np.abs(np.outer(u, v) - h)
    with np.errstate(divide="ignore", invalid="ignore"):
        worst = np.max(np.where(h != 0, d / np.abs(h), np.where(d == 0, 0.0, np.inf)))
    return u, v, float(worst)


# ------------------------------------------------------------------ operator references
@functools.lru_cache(maxsize=None)
def operand(shape, n=N_CHAINS):
    rng = np.random.default_rng(shape[0] * 1000 + shape[1])
    # a star field: point sources of 20 .. 50 on a jittered grid (each chain its own), over a block of 1 on a ramp and noise on every pixel.  A point
    # source shows every tap by itself -- the smallest too, the last row of a Gaussian at 3 sigma -- while H x, and with it the rounding scale, stays of order 1
    x = X.step_image(shape)[None] / 190.0 + rng.normal(0, 0.05, (n,) + shape)
    for c in range(n):
        for i in range(2, shape[0], 11):
            for j in range(3, shape[1], 17):
                x[c, min(i + rng.integers(0, 3), shape[0] - 1), min(j + rng.integers(0, 3), shape[1] - 1)] += rng.uniform(20, 50)
    x = f32(x)
    x.setflags(write=False)
    return x


OpRef = namedtuple("OpRef", "x ref64 ref32 e32 bound")


@functools.lru_cache(maxsize=None)
def op_reference(name, adjoint):
    c = CASES[IDS.index(name)]
    x = operand(c.shape)
    fn = O.blur_adjoint if adjoint else O.blur
    r64 = fn(x.astype(np.float64), c.h.astype(np.float64), c.offset)
    r32 = fn(x, c.h, c.offset)
    assert r64.dtype == np.float64 and r32.dtype == np.float32
    return OpRef(x, r64, r32, *X.bound_of(r64, r32))


def two_pass_f32(c, x, adjoint):
    """The separable form as the device runs it, in float32: the column factor u down the columns first, then the row factor v along the rows."""
    u, v, _ = separable_factors(c.h)
    fn = O.blur_adjoint if adjoint else O.blur
    t = fn(np.asarray(x, dtype=np.float32), f32(u)[:, None], (c.offset[0], 0))
    out = fn(t, f32(v)[None, :], (0, c.offset[1]))
    assert out.dtype == np.float32
    return out


# planted faults: what a wrong kernel computes in place of H x (float64)
def fault_correlation(x, h, off):
    return O.blur_adjoint(x, h, off)


def fault_transposed_offset(x, h, off):
    return O.blur(x, h, (off[1], off[0]))


def fault_edge_clamp(x, h, off):
    kh, kw = h.shape
    xp = np.pad(x, [(0, 0)] * (x.ndim - 2) + [(kh, kh), (kw, kw)], mode="edge")
    return O.blur(xp, h, off)[..., kh:-kh, kw:-kw]


def fault_last_row_dropped(x, h, off):
    g = h.copy()
    g[-1, :] = 0.0
    return O.blur(x, g, off)


def fault_applies(fault, c):
    if fault is fault_transposed_offset:
        return c.offset[0] != c.offset[1]
    if fault is fault_last_row_dropped:      # the last tap row reads x[i + oy - (kh - 1)]: inside the image for some i, and the kernel has another row
        return c.h.shape[0] > 1 and c.shape[0] - 1 + c.offset[0] - (c.h.shape[0] - 1) >= 0
    if fault is fault_correlation:           # a kernel that is its own mirror image about its origin has no direction
        kh, kw = c.h.shape
        return not (np.array_equal(c.h[::-1, ::-1], c.h) and c.offset == (kh - 1 - c.offset[0], kw - 1 - c.offset[1]))
    return True


FAULTS = [fault_correlation, fault_transposed_offset, fault_edge_clamp, fault_last_row_dropped]


# ------------------------------------------------------------------ one MYULA step with a PSF: "restart" mode of tests/_pixel.py
StepCase = namedtuple("StepCase", "name shape term psf prior box K iters")      # psf: a name of CASES, or (kh, kw, offset) of random taps / a Gaussian


def _step_cases():
    g21 = ("gauss", 21, 3.5, (10, 10))
    return [StepCase("l2-tv10-pipe", (24, 136), "l2", ("rand", 13, 11, (4, 7)), "tv", None, 10, 2),       # the prior launch is a pipe kernel
            StepCase("l2-tv10-split", (37, 70), "l2", ("rand", 13, 11, (4, 7)), "tv", None, 10, 2),        # ... the split / tile kernel
            StepCase("l2-l1-33", (20, 24), "l2", ("rand", 33, 33, (16, 16)), "l1", None, 0, 2),
            StepCase("wl2-tvbox", (37, 70), "wl2", ("rand", 13, 11, (4, 7)), "tv", (0.0, 255.0), 10, 2),
            StepCase("pois-tvpos-gauss21", (40, 72), "pois", g21, "tv", (0.0, float("inf")), 10, 2),
            StepCase("l2-aniso", (37, 70), "l2", ("rand", 12, 10, (3, 7)), "aniso", None, 10, 2),
            StepCase("l2-grad", (37, 70), "l2", ("rand", 13, 11, (4, 7)), "grad", None, 0, 1)]             # L2.grad alone: the overwrite form


STEP_CASES = _step_cases()
STEP_IDS = [c.name for c in STEP_CASES]


def psf_of(c):
    kind = c.psf[0]
    if kind == "rand":
        _, kh, kw, off = c.psf
        return f32(random_taps(kh, kw, kh * 100 + kw)), off
    _, k, s, off = c.psf
    h = np.outer(gauss1d(k, s), gauss1d(k, s))
    return f32(h / h.sum()), off


StepProblem = namedtuple("StepProblem", "h offset aux y x0 noise tau gamma sigma_f weight")


@functools.lru_cache(maxsize=None)
def step_problem(name):
    c = STEP_CASES[STEP_IDS.index(name)]
    rng = np.random.default_rng(1000 * c.shape[0] + c.shape[1])
    shape = c.shape
    h, off = psf_of(c)
    op = P.Op("blur", h.astype(np.float64), off)
    aux = None
    if c.term == "pois":
        aux = f32(P.ramp_background(shape))
        _, _, y, _, x0 = P.recipe(shape, n_chains=N_CHAINS, seed=shape[1], op=op, beta=aux.astype(np.float64))
        y, x0 = f32(y), f32(x0)
        gamma, sigma_f, weight = X.POIS_GAMMA, 1.0, X.POIS_TV
        tau = 0.5 / (P.PoissonRef(op, y, aux, sigma_f).grad_lipschitz() + 1.0 / gamma)
    elif c.term == "wl2":
        _, _, y, w, x0 = W.recipe(shape, n_chains=N_CHAINS, seed=shape[1], op=op)
        w[-1, :] = 0.0       # zero weights in the last row and column
        w[:, -1] = 0.0
        aux, y, x0 = f32(w), f32(y), f32(x0)
        gamma, sigma_f, weight = W.GAMMA, W.SIGMA_F, W.TV_WEIGHT
        tau = W.step_size(W.WL2Ref(op, y, aux, sigma_f))
    else:
        img = X.step_image(shape)
        y = f32(op.fwd(img) + rng.normal(0, X.SIGMA, shape))
        x0 = f32(img[None] + rng.normal(0, 10, (N_CHAINS,) + shape))
        gamma, sigma_f, tau = X.GAMMA, 1 / X.SIGMA ** 2, X.TAU
        weight = X.L1_WEIGHT if c.prior == "l1" else X.TAU_REG
    noise = f32(rng.standard_normal((c.iters, N_CHAINS) + shape))
    for a in (h, aux, y, x0, noise):
        if a is not None:
            a.setflags(write=False)
    return StepProblem(h, off, aux, y, x0, noise, tau, gamma, sigma_f, weight)


class _Prox:
    def __init__(self, fn):
        self.prox = fn


def data_term(c, m, dtype):
    op = P.Op("blur", m.h.astype(dtype), m.offset)
    if c.term == "pois":
        return P.PoissonRef(op, m.y, m.aux, m.sigma_f, dtype=dtype)
    if c.term == "wl2":
        return W.WL2Ref(op, m.y, m.aux, m.sigma_f, dtype=dtype)
    return X._Data(op, m.y, m.sigma_f, dtype)


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
    raise ValueError(c.prior)


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


def worst(got, ref64):
    """(max |got - ref64|, its index) over every chain and pixel; a value that is not finite counts as infinite."""
    d = np.abs(np.asarray(got, dtype=np.float64) - ref64)
    d = np.where(np.isfinite(d), d, np.inf)
    k = np.unravel_index(int(np.argmax(d)), d.shape)
    return float(d[k]), tuple(int(v) for v in k)

"""The lattice of step configurations: every data kind of include/lmc_atomi.h crossed with every prior, the box, array-valued `epsg` and two samplers
(MYULA, SK-ROCK with three stages).  numpy only: the cells, the table of what each cell must do (`expected`, written from the header's text of each kind
and never from the library's checks), the float64 reference of one iteration with its float32 replay, and the check both test files share.
tests/test_lattice_reference.py holds this file to itself on the CPU; tests/test_gpu_lattice.py runs the library against it.

The single-feature suites test each kernel in depth on three to seven partners of their choice; the step dispatch (`launch_step` and its routes in
csrc/lmc_problem.hip, `myula_single` in csrc/lmc_sampler.hip) hands a partly consumed argument set from route to route, and a prior that silently becomes
the identity, a box that is dropped, a clamp applied twice or a sampler that is created and cannot step shows only where two features meet.

A cell is (shape, data kind, prior, box, epsg form).  The reference is composed from the classes the single-feature suites hold (`PoissonRef`, `WL2Ref`,
`HuberRef`, `RadonRef`, `SpectralRef`, `P.Op`, `TVRef`, `SeparableRef`, the wavelet and Haar proxes, `myula_step`, the SK-ROCK recursion of
tests/_skrock_pixel.py); the device never enters it.  The bound is tests/_pixel.py's, per pixel: max(3 e32, 2 ulp32(max |ref64|)), e32 measured on the
float32 replay (for SK-ROCK: on the two float32 replays of tests/_skrock_pixel.py, the definition and the launch form)."""
import functools
import itertools
import math
from collections import namedtuple

import numpy as np

from oracle import lmc_oracle as O
import _fourier_ref as F
import _huber_ref as HU
import _pixel as X
import _poisson_ref as P
import _psf_ref as PR
import _radon_ref as R
import _skrock_pixel as S
import _wavelet as Wv
import _wl2_ref as W

f32 = X.f32
LMC_E_UNSUPPORTED = -2
N_CHAINS, ITERS = 2, 2
SK_STAGES, SK_ETA = 3, S.ETA
ENERGY_RTOL = W.ENERGY_RTOL
REL_L2 = 5e-5          # the limit of tests/test_gpu_matrix.py: reported beside the per-pixel bound, never asserted in its place

# (16, 64): a multiple of 8 and a power of two -- block, split, every precondition holds; (21, 33): unaligned rows -- tile or point; (16, 256): wider than 128
# columns, 4 pixels per lane -- pipe; (24, 264): 8 pixels per lane -- pipe, two teams where covered.  The rows kernel needs a separable blur in the step
# launch itself: kinds 2 (and the closed-form priors) reach it on every shape.
SHAPES = [(16, 64), (21, 33), (16, 256), (24, 264)]
KINDS = tuple(range(20))
KIND_NAMES = ["none", "identity", "blur", "mask", "pois-identity", "pois-blur", "pois-mask", "wl2-identity", "wl2-blur", "psf", "pois-psf", "wl2-psf", "spectral",
              "hub-identity", "hub-blur", "hub-psf", "radon", "pois-radon", "wl2-radon", "hub-radon"]
OPERATOR = ["none", "identity", "blur", "mask", "identity", "blur", "mask", "identity", "blur", "psf", "psf", "psf", "spectral", "identity", "blur", "psf",
            "radon", "radon", "radon", "radon"]
TERM = ["l2", "l2", "l2", "l2", "pois", "pois", "pois", "wl2", "wl2", "l2", "pois", "wl2", "l2", "hub", "hub", "hub", "l2", "pois", "wl2", "hub"]
# the kinds whose step is a fused kernel of the term itself (header: "LMC_PRIOR_HAAR_L1 ... LMC_E_UNSUPPORTED" in the text of kinds 4 - 8, 13, 14)
OWN_KERNEL_KINDS = (4, 5, 6, 7, 8, 13, 14)
PRIORS = ("none", "l2", "l1", "laplace", "tv10", "tv20", "aniso10", "haar", "db2", "vtv")
SEPARABLE = ("l2", "l1", "laplace")          # the priors that take one weight per pixel (lmc_problem.prox_scale)
BOX = (0.0, 255.0)
BOXES = (None, BOX)
EPSG = ("scalar", "array")
SAMPLERS = ("myula", "skrock")
DB2 = (2, 2)                                 # p, levels

Cell = namedtuple("Cell", "shape kind prior box epsg")


def cell_id(c):
    return f"{c.shape[0]}x{c.shape[1]}-{KIND_NAMES[c.kind]}-{c.prior}" + ("-box" if c.box else "") + ("-epsg[]" if c.epsg == "array" else "")


def combinations():
    """Every (data kind, prior, box, epsg form): array-valued epsg exists for the separable priors only."""
    return [(k, p, b, e) for k, p, b, e in itertools.product(KINDS, PRIORS, BOXES, EPSG) if e == "scalar" or p in SEPARABLE]


def all_cells(shape):
    return [Cell(shape, *c) for c in combinations()]


def power_of_two(n):
    return 8 <= n <= 1024 and n & (n - 1) == 0


def left_out(c):
    """The reason a shape precondition forbids the cell, or None.  These are the only cells a shape leaves out."""
    H, W = c.shape
    if OPERATOR[c.kind] == "spectral" and not (power_of_two(H) and power_of_two(W)):
        return "LMC_DATA_SPECTRAL: H and W powers of two"
    if c.prior == "haar" and (H % 8 or W % 8):
        return "LMC_PRIOR_HAAR_L1: H, W multiples of 8"
    if c.prior == "db2" and not Wv.legal(c.shape, *DB2):
        return "LMC_PRIOR_WAVELET_L1: the image does not take 2 levels of db2"
    return None


def cells(shape):
    return [c for c in all_cells(shape) if left_out(c) is None]


def expected(c, sampler):
    """"runs", or (status, phrases): creation fails with that status and lmc_last_error names one of the phrases (where two rules forbid a cell the header does
    not say which speaks first).  From include/lmc_atomi.h:
      * LMC_PRIOR_VTV: "every other entry point that takes an lmc_problem: LMC_E_UNSUPPORTED";
      * box_enable: "LMC_E_UNSUPPORTED ... LMC_PRIOR_HAAR_L1 and LMC_PRIOR_WAVELET_L1 ... lmc_skrock_create"; NONE / L2 / L1 / EPROX / TV_ISO / TV_ANISO take it
        with every data term ("box_enable with each as it is honoured for the Gaussian term", "every prior, the box ... as they are for LMC_DATA_NONE");
      * kinds 4 - 8, 13, 14: "LMC_E_UNSUPPORTED ... LMC_PRIOR_HAAR_L1"; kinds 9 - 12, 15 - 19 run the step of LMC_DATA_NONE, which takes it;
      * LMC_PRIOR_WAVELET_L1: "every data term, the Poisson and weighted Gaussian terms and the large PSF included, takes it";
      * prox_scale: "MYULA with LMC_PRIOR_L2 / L1 / EPROX only ... LMC_E_UNSUPPORTED for the other priors and samplers"; with a box "the same launch";
      * lmc_skrock_create: "every data term, prior and non-convex term of MYULA", refusing "tv_warm, tv_rtol > 0 on the prior, prox_scale"."""
    assert left_out(c) is None, c
    if c.prior == "vtv":
        return LMC_E_UNSUPPORTED, ("VTV",)
    why = []
    if c.box and c.prior in ("haar", "db2"):
        why.append("box")
    if c.prior == "haar" and c.kind in OWN_KERNEL_KINDS:
        why.append("HAAR_L1")
    if sampler == "skrock" and c.box:
        why.append("box")
    if sampler == "skrock" and c.epsg == "array":
        why.append("epsg")
    return (LMC_E_UNSUPPORTED, tuple(why)) if why else "runs"


def runs(c, sampler):
    return expected(c, sampler) == "runs"


def energies_exist(c):
    """(f, g): f of every data term is defined; g where the prior has a value (LMC_PRIOR_EPROX: "lmc_energies returns g = 0") and epsg is one number (the value
    of a per-pixel weighted prior is not in the header).  The box does not enter ("WITHOUT the indicator")."""
    return True, c.epsg == "scalar"


# ------------------------------------------------------------------ the problem of (shape, data kind, operator instance): float32 numbers, made once
# Two regimes.  Grey levels (every term but Poisson): the image of tests/_pixel.py with its block at 250 on a ramp, noise of 5 levels, sigma_f = 1 / 25,
# gamma = 25 (tests/_wl2_ref.py).  Counts (Poisson): the same image / 25, sigma_f = 1, gamma = 1, a background ramp of 0.5 .. 4 per pixel (40 .. 80 per
# detector bin: a bin sums a whole ray, and the Lipschitz bound max(y / beta^2) ||A||^2 with it).  tau = 0.5 / (L_f + 1 / gamma).
# Start states: the image plus noise, with 2 % of the pixels moved to 255 + U(10, 120) and 2 % to -U(10, 120) (past the largest threshold a prior applies): values on both sides of the box whatever the regime.
GREY = dict(gamma=W.GAMMA, sigma_f=W.SIGMA_F, weights={"none": 0.0, "l2": 0.02, "l1": 0.8, "laplace": 1.0, "tv10": 0.3, "tv20": 0.3, "aniso10": 0.3, "haar": 0.3,
                                                       "db2": 0.3, "vtv": 0.3})
COUNTS = dict(gamma=1.0, sigma_f=1.0, weights={"none": 0.0, "l2": 0.5, "l1": 8.0, "laplace": 6.0, "tv10": 5.0, "tv20": 5.0, "aniso10": 5.0, "haar": 5.0,
                                               "db2": 5.0, "vtv": 5.0})
SPECTRAL_SIGMA_F = 1.0 / F.SIGMA_N ** 2
PSF_GEOMETRY = (13, 11, (4, 7))
ANGLES = (R.STEP_ANGLES, [0.3, 1.2, float(np.float32(math.pi / 4)), 2.0, 2.7])       # operator instances A and B: the same count

Problem = namedtuple("Problem", "shape kind alt h offset mask angles n_det G b y aux x0 noise Z tau delta gamma sigma_f L")


def regime(kind):
    return COUNTS if TERM[kind] == "pois" else GREY


def weight(c):
    return regime(c.kind)["weights"][c.prior]


@functools.lru_cache(maxsize=None)
def radon_operator(shape, alt):
    return R.step_operator(shape) if alt == 0 else R.RadonRef(shape, ANGLES[alt])


def operator_of(m, dtype):
    """The operator of a problem on arrays of `dtype` (the Radon reference computes in the dtype of its operand)."""
    opk = OPERATOR[m.kind]
    if opk in ("blur", "psf"):
        return P.Op("blur", m.h.astype(dtype), m.offset)
    if opk == "mask":
        return P.Op("mask", m.mask.astype(dtype))
    if opk == "radon":
        return radon_operator(m.shape, m.alt)
    assert opk in ("identity", "none"), opk
    return P.Op("identity")


@functools.lru_cache(maxsize=None)
def problem(shape, kind, alt=0):
    """alt = 1: the same problem on a second operator instance of the same size (PSF taps, Radon angles, sampling mask) -- the stateless path's cached
    tables must follow it."""
    opk, term, reg = OPERATOR[kind], TERM[kind], regime(kind)
    assert alt == 0 or opk in ("psf", "radon", "spectral")
    H, Wd = shape
    rng = np.random.default_rng(7919 * kind + 1000 * H + Wd + 104729 * alt)
    h = offset = mask = angles = n_det = G = b = aux = None
    if opk == "blur":
        h, offset = f32(np.ones((5, 5)) / 25.0), (2, 2)
    elif opk == "psf":
        kh, kw, offset = PSF_GEOMETRY
        h = f32(PR.random_taps(kh, kw, kh * 100 + kw + 17 * alt))
    elif opk == "mask":
        mask = f32(rng.uniform(size=shape) < 0.6)
    elif opk == "radon":
        op_r = radon_operator(shape, alt)
        angles, n_det = op_r.angles, op_r.n_det
    gamma, sigma_f = reg["gamma"], reg["sigma_f"]
    img = X.step_image(shape, 250.0) / (25.0 if term == "pois" else 1.0)
    m0 = Problem(shape, kind, alt, h, offset, mask, angles, n_det, None, None, None, None, None, None, None, 0.0, 0.0, gamma, sigma_f, 0.0)
    if opk == "spectral":
        Gm = F.sampling_mask(shape, seed=3 + alt).astype(np.complex128)
        noise = rng.normal(0, F.SIGMA_N, shape) + 1j * rng.normal(0, F.SIGMA_N, shape)
        y = (Gm * np.fft.fft2(img, norm="ortho") + noise).astype(np.complex64).astype(np.complex128)
        G, b, sigma_f = Gm, y, SPECTRAL_SIGMA_F
        L = F.SpectralRef(G, b, sigma_f).grad_lipschitz()
        y = None
    elif opk == "none":
        y, L = None, 0.0
    else:
        op = operator_of(m0, np.float64)
        dshape = op.sino_shape if opk == "radon" else shape
        clean = op.fwd(img)
        if term == "pois":
            lo, hi = (40.0, 80.0) if opk == "radon" else (0.5, 4.0)
            aux = f32(np.broadcast_to(np.linspace(lo, hi, dshape[1])[None, :], dshape))
            y = f32(rng.poisson(clean + aux.astype(np.float64)))
        else:
            y = clean + rng.normal(0, 5.0, dshape) * (mask if mask is not None else 1.0)
            if term == "wl2":
                w = W.weights(dshape, seed=11 + kind) * (0.25 if opk == "radon" else 1.0)       # (a bin sums a ray: L_f = max(w) ||A||^2 sigma_f)
                w[0, :] = 0.0            # an unobserved first row (angle) and last column (bin): a weight read one off shows
                w[:, -1] = 0.0
                aux = f32(w)
            if term == "hub":
                hit = rng.uniform(size=dshape) < 0.1
                y = y + np.where(hit, rng.uniform(50.0, 150.0, dshape) * rng.choice([-1.0, 1.0], dshape), 0.0)
                aux = f32(HU.thresholds(dshape, seed=13 + kind))
            y = f32(y)
        L = sigma_f * op.norm2_bound() if term == "l2" else R.term_of(term, op, y, aux, sigma_f, np.float64).grad_lipschitz()
    x0 = img[None] + rng.normal(0, 1.0 if term == "pois" else 10.0, (N_CHAINS,) + shape) - (0.5 if term == "pois" else 0.0)
    u = rng.uniform(size=x0.shape)
    x0 = np.where(u < 0.02, 255.0 + rng.uniform(10, 120, x0.shape), np.where(u > 0.98, -rng.uniform(10, 120, x0.shape), x0))
    x0 = f32(x0)
    noise = f32(rng.standard_normal((ITERS, N_CHAINS) + shape))
    Z = f32(rng.standard_normal((ITERS, N_CHAINS) + shape))
    tau = float(np.float32(0.5 / (L + 1.0 / gamma)))
    delta = float(np.float32(S.STEP_FRACTION * S.step_factor(SK_STAGES) / (L + 1.0 / gamma)))
    for a in (h, mask, aux, y, x0, noise, Z):
        if a is not None:
            a.setflags(write=False)
    return m0._replace(G=G, b=b, y=y, aux=aux, x0=x0, noise=noise, Z=Z, tau=tau, delta=delta, sigma_f=sigma_f, L=float(L))


@functools.lru_cache(maxsize=None)
def epsg_array(shape):
    """One weight per pixel in [0.3, 2.5], float32."""
    e = f32(np.random.default_rng(31 * shape[0] + shape[1]).uniform(0.3, 2.5, shape))
    e.setflags(write=False)
    return e


# ------------------------------------------------------------------ the terms of a cell in `dtype`
class _NoData:
    def grad(self, x):
        return np.zeros_like(x)


def data_term(m, dtype, plain=False):
    """The data term of problem `m`; plain: the Gaussian term on the same operator and observation (the wrong kernel that ignores the term)."""
    opk, term = OPERATOR[m.kind], "l2" if plain else TERM[m.kind]
    if opk == "none":
        return _NoData()
    if opk == "spectral":
        return F.SpectralRef(m.G, m.b, m.sigma_f, dtype)
    return R.term_of(term, operator_of(m, dtype), m.y, m.aux, m.sigma_f, dtype)


def f_value(m, x):
    """f(x) per chain in float64."""
    opk, term = OPERATOR[m.kind], TERM[m.kind]
    x = np.asarray(x, dtype=np.float64)
    if opk == "none":
        return np.zeros(x.shape[0])
    if opk == "spectral":
        return F.SpectralRef(m.G, m.b, m.sigma_f).value(x)
    op = operator_of(m, np.float64)
    if term == "l2":
        return R.l2_value(op, m.y, m.sigma_f, x)
    return np.asarray(R.term_of(term, op, m.y, m.aux, m.sigma_f, np.float64)(x))


def g_value(c, x):
    """sigma g(x) per chain in float64 (scalar epsg, no indicator); 0 for the priors without a value."""
    x, w = np.asarray(x, dtype=np.float64), weight(c)
    if c.prior in ("none", "laplace"):
        return np.zeros(x.shape[0])
    if c.prior == "l2":
        return 0.5 * w * (x * x).sum(axis=(-2, -1))
    if c.prior == "l1":
        return w * np.abs(x).sum(axis=(-2, -1))
    if c.prior in ("tv10", "tv20"):
        return w * O.tv_value(x)
    if c.prior == "aniso10":
        return w * P.TVRef(c.shape, w, 10, aniso=True).value(x)
    if c.prior == "haar":
        return w * O.haar_l1_value(x, 3)
    assert c.prior == "db2", c.prior
    return Wv.value(x, *DB2, w)


def _soft(x, thr):
    return np.sign(x) * np.maximum(np.abs(x) - thr, x.dtype.type(0))


class Prior:
    """prox_{t (g + box)}(x) of a cell in `dtype`; t may be an array (one prox parameter per pixel).  `clamp`: "prox" -- the prox of the sum (clip of a
    separable prox, the constrained FGP of the TV priors); "state" -- the WRONG order, the unconstrained prox of the clipped state; None -- no box."""

    def __init__(self, c, dtype, drop_prior=False, clamp="prox"):
        self.c, self.dtype, self.w = c, np.dtype(dtype), weight(c)
        self.kind = "none" if drop_prior else c.prior
        self.box = c.box if clamp is not None else None
        self.clamp = clamp

    def _free(self, x, t, box):
        """The prox with the box `box` inside it (None: unconstrained)."""
        T, k, w = self.dtype.type, self.kind, self.w
        lo, hi = (T(box[0]), T(box[1])) if box else (None, None)
        clip = (lambda v: np.clip(v, lo, hi)) if box else (lambda v: v)
        if k == "none":
            return clip(x)
        if k in SEPARABLE:
            thr = np.asarray(t, dtype=self.dtype) * T(w)
            return clip(x / (T(1) + thr) if k == "l2" else _soft(x, thr))
        assert np.ndim(t) == 0, "array-valued epsg is built for the separable priors"
        if k in ("tv10", "tv20", "aniso10"):
            return P.TVRef(self.c.shape, w, 20 if k == "tv20" else 10, box, aniso=k == "aniso10", dtype=self.dtype).prox(x, t)
        assert box is None, "the wavelet priors take no box"
        if k == "haar":
            return O.haar_l1_prox(x, T(w * t), 3)
        assert k == "db2", k
        return Wv.prox(x, *DB2, w * t).astype(self.dtype)

    def prox(self, x, t):
        x = np.asarray(x, dtype=self.dtype)
        if self.box is not None and self.clamp == "state":
            out = self._free(np.clip(x, self.dtype.type(self.box[0]), self.dtype.type(self.box[1])), t, None)
        else:
            out = self._free(x, t, self.box)
        assert out.dtype == self.dtype, (cell_id(self.c), out.dtype)
        return out


class _Scaled:
    """`prior` with the prox parameter multiplied by `eps` (array-valued epsg: algs.py:569 hands epsg * gamma to the prox)."""

    def __init__(self, prior, eps):
        self.prior, self.eps = prior, eps

    def prox(self, x, t):
        return self.prior.prox(x, np.asarray(self.eps, dtype=np.float64) * t)


# the lattice neighbours of a cell: what a wrong route computes.  name -> (applies(cell), keyword arguments of `terms`)
NEIGHBOURS = {
    "prior dropped": (lambda c: c.prior != "none", dict(drop_prior=True)),
    "box dropped": (lambda c: c.box is not None, dict(clamp=None)),
    "clamp on the state": (lambda c: c.box is not None, dict(clamp="state")),
    "plain Gaussian term": (lambda c: TERM[c.kind] != "l2", dict(plain=True)),
    "epsg by its mean": (lambda c: c.epsg == "array", dict(mean_epsg=True)),
}
# Neighbours that are the cell itself, with the reason (nothing to tell apart, so nothing is skipped):
#   "clamp on the state" with no prior: the prox of the indicator alone IS the projection, clip(x) either way.


def same_by_construction(c, name):
    return name == "clamp on the state" and c.prior == "none"


def terms(c, dtype, alt=0, drop_prior=False, clamp="prox", plain=False, mean_epsg=False):
    m = problem(c.shape, c.kind, alt)
    pf = data_term(m, dtype, plain)
    pg = Prior(c, dtype, drop_prior, clamp)
    if c.epsg == "array":
        e = epsg_array(c.shape)
        pg = _Scaled(pg, float(e.astype(np.float64).mean()) if mean_epsg else e)
    return m, pf, pg


def myula(c, x, xi, dtype, alt=0, **wrong):
    """One MYULA iteration of cell `c` from `x` with the noise `xi` in `dtype`."""
    m, pf, pg = terms(c, dtype, alt, **wrong)
    out = P.myula_step(pf, pg, np.asarray(x, dtype=dtype), m.tau, m.gamma, np.asarray(xi, dtype=dtype), dtype=dtype)
    assert out.dtype == np.dtype(dtype), (cell_id(c), out.dtype)
    return out


class _Launch:
    """grad f, prox and the fused launch a x - t grad f + b prox + s n of a cell in float32: what `_skrock_pixel.iteration_launch` drives."""

    def __init__(self, c):
        self.m, self.pf, self.pg = terms(c, np.float32)
        self.dtype, self.gamma = np.dtype(np.float32), self.m.gamma

    def grad(self, x):
        return self.pf.grad(x)

    def prox(self, x):
        return self.pg.prox(x, self.gamma)

    def launch(self, a, t, b, s, x, n):
        T = np.float32
        out = T(a) * x - T(t) * self.grad(x) + T(b) * self.prox(x) + T(s) * n
        assert out.dtype == self.dtype, out.dtype
        return out


def skrock(c, x, Z, dtype, form="definition"):
    """One SK-ROCK iteration (three stages) of cell `c`: the definition in `dtype`, or the launch form in float32."""
    m, pf, pg = terms(c, dtype)
    if form == "launch":
        return S.iteration_launch(_Launch(c), x, Z, m.delta, SK_STAGES)
    advance = lambda v, t: P.myula_step(pf, pg, v, t, m.gamma, np.zeros_like(v), dtype=dtype)       # noqa: E731
    return S.iteration_definition(advance, x, Z, m.delta, SK_STAGES, dtype)


# ------------------------------------------------------------------ references ("restart" mode of tests/_pixel.py) and the check
Stage = X.Stage


def _stage(start, r64, r32s):
    e32 = max(float(np.max(np.abs(r.astype(np.float64) - r64))) for r in r32s)
    bound = max(X.FACTOR * e32, 2.0 * X.ulp32(np.max(np.abs(r64))))
    assert r64.dtype == np.float64 and all(r.dtype == np.float32 for r in r32s)
    r64.setflags(write=False)
    return Stage(start, r64, r32s[0], e32, bound, True)


@functools.lru_cache(maxsize=None)
def reference(c, sampler):
    """The stages of a running cell: one per iteration, each restarting from the rounded float64 result of the one before."""
    assert runs(c, sampler), (cell_id(c), sampler)
    m = problem(c.shape, c.kind)
    stages, start = [], m.x0
    for it in range(ITERS):
        if sampler == "myula":
            r64, r32s = myula(c, start, m.noise[it], np.float64), [myula(c, start, m.noise[it], np.float32)]
        else:
            r64 = skrock(c, start, m.Z[it], np.float64)
            r32s = [skrock(c, start, m.Z[it], np.float32), skrock(c, start, m.Z[it], np.float32, "launch")]
        stages.append(_stage(start, r64, r32s))
        start = f32(r64)
    return tuple(stages)


def coefficients(m):
    """(a, t, b, pt) of the noise-free MYULA update as lmc_fused_eval takes them."""
    return 1.0 - m.tau / m.gamma, m.tau, m.tau / m.gamma, m.gamma


@functools.lru_cache(maxsize=None)
def stateless_reference(c, alt):
    """The noise-free update of the start state on operator instance `alt`: one stage."""
    m = problem(c.shape, c.kind, alt)
    zero = np.zeros_like(m.x0)
    return _stage(m.x0, myula(c, m.x0, zero, np.float64, alt), [myula(c, m.x0, zero, np.float32, alt)])


Verdict = namedtuple("Verdict", "ok err bound ratio where rel message")


def check(what, got, stage):
    """Every pixel of every chain inside the stage's bound, nothing that is not finite; the rel-L2 figure of tests/test_gpu_matrix.py is reported beside it."""
    got = np.asarray(got)
    assert got.shape == stage.ref64.shape, (got.shape, stage.ref64.shape)
    finite = bool(np.isfinite(got).all())
    err, where = PR.worst(got, stage.ref64)
    rel = X.rel(got, stage.ref64) if finite else float("inf")
    ratio = err / stage.bound
    msg = (f"{what}: err {err:.3e} at {where}, e32 {stage.e32:.3e}, bound {stage.bound:.3e}, err / bound {ratio:.2f}, rel-L2 {rel:.2e} (limit {REL_L2:.0e})"
           + ("" if finite else ", NaN or inf in the state"))
    return Verdict(finite and err <= stage.bound, err, stage.bound, ratio, where, rel, msg)

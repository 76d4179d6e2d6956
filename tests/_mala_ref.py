"""A float64 reference of MYMALA that takes the proposal mean m(v) and the potential U(v) as callables, and the test problems of
tests/test_mala_reference.py (CPU) and tests/test_gpu_mymala_matrix.py (GPU), built from the checker's classes (oracle/lmc_oracle.py) the way
tests/test_gpu_matrix.py::build builds them:

    U(v) = of(v) + epsg og(v),        m(v) = O.myula(of, og, v, tau, gamma, epsg=epsg, niter=1, noise=[0])[-1]

so the non-log-concave terms of L2_ncvx_tv and epsg != 1 go through the code of the checker's MYULA.  numpy only, no GPU, no torch."""
import collections
import functools
import typing

import numpy as np

from oracle import lmc_oracle as O
from tests._tv_aniso_ref import tv_aniso_value, tv_prox_aniso

SIG = 0.75
GAM = SIG ** 2
N_CHAINS, N_ITERS, SEED, CHAIN_OFFSET = 6, 3, 1234, 40


def bound_of(U0):
    """The fp32 error allowed on log alpha (tests/test_gpu_mymala.py): 2e-6 of the largest potential plus 2e-3."""
    return 2e-6 * float(np.max(np.abs(U0))) + 2e-3


def mymala(mean, U, x0, tau, noise, uniforms, g=None, decisions=None):
    """MYMALA on the chains ``x0[C, H, W]`` with the accept rule of ``O.mymala_batched``:

        log alpha = U(x) - U(x') - (||x - m(x')||^2 - ||x' - m(x)||^2) / (4 tau),    accepted iff log u <= log alpha,

    a rejected chain keeping x, m(x) and U(x).  ``mean(v) -> [C, H, W]``, ``U(v) -> [C]``, ``noise[nit, C, H, W]``, ``uniforms[nit, C]``.
    ``g(v) -> [C]`` (optional): the part of U whose change is returned as ``dg`` (zeros without it).  ``decisions[nit, C]`` (optional): 0 / 1
    force the outcome of that chain at that iteration, a negative entry leaves it to the rule -- the replay of a device's borderline decisions.
    Returns ``(x, accepted[C], log_alpha[nit, C], dU[nit, C], dg[nit, C])``, dU = U(x') - U(x), dg = g(x') - g(x)."""
    x = np.array(x0, dtype=np.float64)
    nit, C = np.shape(uniforms)
    mx, Ux = np.array(mean(x), dtype=np.float64), np.array(U(x), dtype=np.float64)
    gx = np.array(g(x), dtype=np.float64) if g is not None else np.zeros(C)
    acc = np.zeros(C, dtype=np.int64)
    las, dUs, dgs = np.zeros((nit, C)), np.zeros((nit, C)), np.zeros((nit, C))
    for k in range(nit):
        xp = mx + np.sqrt(2 * tau) * noise[k]
        mxp, Uxp = np.asarray(mean(xp), dtype=np.float64), np.asarray(U(xp), dtype=np.float64)
        gxp = np.asarray(g(xp), dtype=np.float64) if g is not None else np.zeros(C)
        d1 = np.sum((xp - mx) ** 2, axis=(-2, -1))
        d2 = np.sum((x - mxp) ** 2, axis=(-2, -1))
        la = (Ux - Uxp) - (d2 - d1) / (4 * tau)
        ok = np.log(uniforms[k]) <= la
        if decisions is not None:
            forced = np.asarray(decisions[k])
            ok = np.where(forced >= 0, forced > 0, ok)
        las[k], dUs[k], dgs[k] = la, Uxp - Ux, gxp - gx
        x[ok], mx[ok], Ux[ok], gx[ok] = xp[ok], mxp[ok], Uxp[ok], gxp[ok]
        acc += ok
    return x, acc, las, dUs, dgs


# ---- the test problems --------------------------------------------------------------------------------------------------------------------

class Case(typing.NamedTuple):
    shape: tuple
    data: str
    prior: str
    ncvx: str = "none"
    epsg: float = 1.0
    tau_scale: float = 1.0

    @property
    def id(self):
        return (f"{self.shape[0]}x{self.shape[1]}-{self.data}-{self.prior}" + (f"-{self.ncvx}" if self.ncvx != "none" else "") +
                (f"-epsg{self.epsg:g}" if self.epsg != 1.0 else "") + (f"-tau{self.tau_scale:g}" if self.tau_scale != 1.0 else ""))


# 17 x 67: an odd pixel count, H % 4 != 0, the edge of the separable energy kernel's 32 x 64 tile; 24 x 136: the full-width pipeline, one team, with
# the energies as its by-products; 20 x 150: the same with rows that are not 16-byte aligned; 16 x 520: column strips
ODD, PIPE, UNALIGNED, STRIPS = (17, 67), (24, 136), (20, 150), (16, 520)
SHAPES = [ODD, PIPE, UNALIGNED, STRIPS]
# blur6: the reference's 6 x 6 kernel with its centre at (3, 3); blur5off: 5 x 5 with the origin in its first row, which no separable kernel centres.
# The data of blur5, blur7 and blur6 are the image under the 5 x 5 blur whatever the model's kernel, as in tests/test_gpu_matrix.py::build: for 6 and 7
# taps the model does not match its data, U(x0) is large and the bound on log alpha with it (0.2 to 3).  blur7m, blur6m and blur5off are the same
# models on data blurred with their own kernel and origin: bounds like blur5's (0.03 to 0.08) on the 7-tap kernels and on the direct energy kernel.
BLURS = {"blur5": (5, (2, 2)), "blur7": (7, (3, 3)), "blur6": (6, (3, 3)), "blur7m": (7, (3, 3)), "blur6m": (6, (3, 3)), "blur5off": (5, (0, 1))}
MATCHED = ("blur7m", "blur6m", "blur5off")
CENTRED = ("blur5", "blur7", "blur6", "blur7m", "blur6m")
# TV: (dual iterations asked for, lagged_output); the iterate comes after niter - lagged dual updates
TV_PRIORS = {"tv10": (10, False), "tv5": (5, False), "tv6": (6, False), "tv11lag": (11, True), "tv10lag": (10, True)}
NCVX = ("mc", "me", "me_rtol", "mc_aniso")
NCVX_KW = dict(sigma=1 / SIG ** 2, lamda=0.3, gamma=15.0, niter=20)


def _cases():
    out = []
    for shape in SHAPES:
        for data in ("blur5", "blur7", "identity", "mask"):
            for prior in ("tv10", "tv5", "aniso", "l1", "l2", "none"):
                # identity + l2 on the strips: two chains of six are clear-cut at tau = sigma^2, all six at half of it
                out.append(Case(shape, data, prior, tau_scale=0.5 if (shape, data, prior) == (STRIPS, "identity", "l2") else 1.0))
        out += [Case(shape, "blur6", "tv10"), Case(shape, "blur6", "l1")]
        # (matched data with the l1 prior: two clear-cut chains of six at 24 x 136; without a prior U is f alone and the bound at its smallest)
        out += [Case(shape, data, prior) for data in ("blur7m", "blur6m") for prior in ("tv10", "none")]
    out += [Case(shape, "blur5off", prior) for shape in (ODD, PIPE) for prior in ("tv10", "l2")]
    out += [Case(PIPE, data, prior) for data in ("blur5", "blur7") for prior in ("tv6", "tv11lag", "tv10lag")]      # the pipeline's other instantiations
    out += [Case(PIPE, data, "haar") for data in ("blur5", "identity", "mask")]
    for shape in (PIPE, ODD):
        out += [Case(shape, data, "tv10", ncvx) for data in ("blur5", "mask") for ncvx in NCVX]
    out += [Case(PIPE, "blur5", "l1", "mc"), Case(PIPE, "blur5", "l1", "me"), Case(ODD, "identity", "none", "mc")]
    out += [Case(PIPE, "mask", "tv10", epsg=2.5), Case(STRIPS, "mask", "tv10", epsg=2.5), Case(STRIPS, "blur5", "tv10", epsg=2.5),
            Case(ODD, "identity", "l1", epsg=2.5)]
    assert len(set(out)) == len(out)
    return out


CASES = _cases()


class _NoPrior:
    def __call__(self, x):
        return 0.0

    def prox(self, x, t):
        return x


class _AnisoTV:
    def __init__(self, dims, sigma, niter):
        self.dims, self.sigma, self.niter = dims, sigma, niter

    def __call__(self, x):
        return self.sigma * float(tv_aniso_value(np.asarray(x).reshape(self.dims)))

    def prox(self, x, t):
        return tv_prox_aniso(np.asarray(x).reshape(self.dims), self.sigma * t, self.niter).ravel()


class Model:
    """One test problem: the arrays the device sampler is built from (``y``, ``h``, ``offset``, ``mask``), the checker's ``of`` / ``og``, the inputs
    of the run (``x0``, ``noise``, ``uniforms``) and the float64 callables ``mean``, ``f``, ``g``, ``U`` on ``[C, H, W]`` states."""

    def __init__(self, case):
        self.case = case
        shape = self.shape = case.shape
        n = shape[0] * shape[1]
        rng = np.random.default_rng(shape[1])
        img = np.zeros(shape)
        img[3:shape[0] - 4, shape[1] // 8:shape[1] // 2] = 150.0
        img += np.linspace(0, 30, shape[1])[None, :]
        self.h = self.offset = self.mask = None
        if case.data in BLURS:
            k, self.offset = BLURS[case.data]
            self.h = np.ones((k, k)) / k ** 2
            hy, oy = (self.h, self.offset) if case.data in MATCHED else (np.ones((5, 5)) / 25, (2, 2))
            self.y = O.blur(img, hy, oy) + rng.normal(0, SIG, shape)
            oOp = O.Convolve2D(shape, self.h, self.offset)
        elif case.data == "identity":
            self.y = img + rng.normal(0, SIG, shape)
            oOp = None
        else:
            self.mask = (rng.uniform(size=shape) < 0.5).astype(np.float64)
            self.y = self.mask * (img + rng.normal(0, SIG, shape))
            oOp = O.Diagonal(self.mask)
        if case.ncvx == "none":
            self.of = O.L2(Op=oOp, b=self.y.ravel(), sigma=1 / SIG ** 2)
        else:
            kw = dict(dims=shape, b=self.y.ravel(), Op=oOp if oOp is not None else O.Identity(n), **NCVX_KW)
            if case.ncvx in ("mc", "mc_aniso"):
                self.of = O.L2NcvxTV(Op2=O.Gradient(shape), isotropic=case.ncvx == "mc", **kw)
            else:
                self.of = O.L2NcvxTV(isotropic=True, tv_kwargs={"rtol": 1e-4} if case.ncvx == "me_rtol" else None, **kw)
        if case.prior in TV_PRIORS:
            niter, lagged = TV_PRIORS[case.prior]
            self.og = O.TV(shape, sigma=0.3, niter=niter - lagged)
        elif case.prior == "aniso":
            self.og = _AnisoTV(shape, 0.3, 10)
        elif case.prior == "l2":
            self.og = O.L2(sigma=0.05)
        elif case.prior == "l1":
            self.og = O.L1(sigma=0.8)
        elif case.prior == "haar":
            self.og = O.WaveletL1(shape, sigma=0.3)
        else:
            self.og = _NoPrior()
        self.epsg, self.gamma, self.tau = case.epsg, GAM, case.tau_scale * SIG ** 2
        self.x0 = img[None] + rng.normal(0, 3, (N_CHAINS,) + shape)
        self.noise = rng.standard_normal((N_ITERS, N_CHAINS) + shape)
        self.uniforms = np.stack([O.philox_uniforms(SEED, k, CHAIN_OFFSET + np.arange(N_CHAINS)) for k in range(N_ITERS)])

    def mean(self, v):
        return np.stack([O.myula(self.of, self.og, vc.ravel(), self.tau, self.gamma, epsg=self.epsg, niter=1, noise=[0.0])[-1].reshape(self.shape)
                         for vc in np.asarray(v, dtype=np.float64)])

    def f(self, v):
        return np.array([float(self.of(vc.ravel())) for vc in np.asarray(v, dtype=np.float64)])

    def g(self, v):
        return np.array([float(self.og(vc.ravel())) for vc in np.asarray(v, dtype=np.float64)])

    def U(self, v):
        return self.f(v) + self.epsg * self.g(v)

    def run(self, noise=None, decisions=None):
        """(x, accepted, log_alpha, dU, dg) of the problem's own inputs; ``noise`` replaces the injected field (the Philox test)."""
        return mymala(self.mean, self.U, self.x0, self.tau, self.noise if noise is None else noise, self.uniforms, g=self.g, decisions=decisions)


Reference = collections.namedtuple("Reference", "model x accepted log_alpha dU dg bound margin safe")


@functools.lru_cache(maxsize=None)
def reference(case):
    """The problem of ``case`` and its float64 run, computed once per process and shared; nothing may write to its arrays.  ``bound``: the error
    allowed on log alpha; ``margin[nit, C]`` = |log u - log alpha|; ``safe[C]``: every decision of the chain is clear-cut (margin > 10 bound)."""
    m = Model(case)
    x, acc, las, dU, dg = m.run()
    bound = bound_of(m.U(m.x0))
    margin = np.abs(np.log(m.uniforms) - las)
    safe = (margin > 10 * bound).all(axis=0)
    for a in (x, acc, las, dU, dg, margin, safe, m.x0, m.noise, m.uniforms, m.y):
        a.setflags(write=False)
    return Reference(m, x, acc, las, dU, dg, bound, margin, safe)

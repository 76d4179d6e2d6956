"""Per-pixel parity of SK-ROCK (lmc_skrock_create / SKROCKSampler; csrc/lmc_sampler.hip: skrock_step, csrc/lmc_skrock.hip) against the float64 checker:
the case lists, the references and the bound.  numpy only; tests/test_skrock_pixel_reference.py (CPU) checks this harness on every case and plants the
faults the bound has to see, tests/test_gpu_skrock_pixel.py runs the sampler against it.  The conventions are those of tests/_pixel.py, whose `problem`,
`Stepper`, `region`, `region_pixels`, `check`, `ulp32` and `FACTOR` = 3 are used as they are: every input is rounded to float32 once, the library gets
those numbers and the checker gets them cast back to float64.

What SK-ROCK does with the step kernels that no case of tests/_pixel.py does: a stage j >= 2 is the fused launch a x - t grad f(x) + b prox(x) + s n with
a = nu_j - mu_j delta / gamma (near 2), s = kappa_j (near -1) and n = K_{j-2}, a state of magnitude 200 read through noise_mode = INJECTED on a handle the
user may have made in Philox mode; stage 1 runs on Y = X + nu_1 q Z made by the perturbation kernels of lmc_skrock.hip, whose field must be the one the
step launch draws again; three arrays rotate, so which one holds K_s depends on s mod 3.

Definition (`iteration_definition`; the header of include/lmc_atomi.h as tests/test_gpu_skrock.py::skrock_iteration states it), q = sqrt(2 delta):

    K_0 = X,  K_1 = X + mu_1 delta drift(X + nu_1 q Z) + kappa_1 q Z,  K_j = mu_j delta drift(K_{j-1}) + nu_j K_{j-1} + kappa_j K_{j-2},  X' = K_s

with v + t drift(v) = `Stepper.advance(v, t)`, the checker's step with tau = t and no noise.  The coefficients come from numpy.polynomial.chebyshev
(`coefficients`), never from the library; ETA = 0.05.  Step: delta = 0.8 l_s / L rounded to float32 once (the handle keeps it as a float),
l_s = (s - 1/2)^2 (2 - 4 eta / 3) - 3/2, L = L_f + 1 / gamma, L_f = sigma_f for the plain Gaussian term (the tap sets sum to about 1), what the reference
class reports as `grad_lipschitz` for the Poisson and the weighted term; gamma is the case's.

`ref64` is the definition in float64.  Two float32 replays, `e32` the larger of their distances to ref64 (as tests/_ulpda_pixel.py):
  (a) the definition with every array and coefficient in float32;
  (b) the launch form of DESIGN 3.4 (`iteration_launch`), the coefficients formed in double and rounded to float32 once as `skrock_step` does:
      Y = fma(f32(nu_1 q), Z, X); K_1 = advance(Y, mu_1 delta) + f32((kappa_1 - nu_1) q) Z;
      K_j = f32(nu_j - mu_j delta / gamma) K_{j-1} - f32(mu_j delta) grad f + f32(mu_j delta / gamma) prox + f32(kappa_j) K_{j-2}.
      `Terms` states grad f and prox of a case apart (the checker's step only returns their combination); the CPU file holds
      `Terms.launch(1 - t / gamma, t, t / gamma, 0, v, 0)` bit-equal to `Stepper.advance(v, t)` in both dtypes on every case.
`bound = max(3 e32, 2 ulp32(max |ref64|))` at every chain and pixel, measured on the reference and never on a kernel; the factor and the floor are
tests/_pixel.py's, for the same reasons.  A third replay in another association (`iteration_third`) exists for the CPU file only: it has to pass.

Modes.  "restart" (injected noise, two iterations): after the first, both sides restart from f32(ref64).  "carried" (Philox noise, or none): the
iterations run from x0 without a restart, each replay carrying its own drift; the device runs `step(n)` in one call and is compared after the last
iteration, and a second handle runs `step(1)` and is compared after the first.  The checker's Philox field is
`O.philox_normals(SEED, it, CHAIN_OFFSET + arange(C), H, W)` (`_pixel.problem` in its "fused" mode makes exactly that); the device's deviates differ
from it by up to PHILOX_DXI = 2e-5 (hardware log2 / sqrt / sin / cos; rung R3, tests/test_gpu_parity.py::test_philox_*), and the noise gain |B_s| of a
stable iteration is at most 1, so a Philox case adds `q * 2e-5` to the bound; `SStage.rounding` and `SStage.philox` keep the two parts apart.  Over
the 68 Philox stages of parts D and E the addition is 0.03 to 0.19 of 3 e32: under a tenth on 56 of them and 0.10 to 0.19 on twelve, ten of which
are the FIRST iteration (one iteration's rounding only) of (9, 4), (5, 65), (16, 72), (8, 264) and (6, 264) -- the small shapes that are there for the
edges of the perturbation kernels, where e32 is a maximum over few pixels.  ((1, 256) runs without a data term for this reason: 0.29 with the identity
term, 0.09 without.)  The bound is not widened for them; the CPU file prints the share of every stage.

Parts (`CASES`).
  A  every case of `_pixel.CASES` with mode "restart" and no box at s = 5, with the case's variant and exact kernel name: a step kernel that adds its
     cases to tests/_pixel.py is covered here too.  165 cases today; past A_MAX = 150 `_thin_a` keeps four tap sets of the groups that differ in their
     blur taps alone (153 stay; every family, shape, data term, prior and tap set of a family stays).  Two box cases (`BOX_CASES`) must raise
     before a handle exists.
  B  one case per family at s in {2, 3, 4, 10, 15}: the three residues of the buffer rotation, and the largest count scripts/bench_skrock.py uses.
  C  noise="none", s = 3: stage 1 runs on X itself with s = 0.
  D  Philox, carried, s = 5 and 2, on shapes that pick each perturbation form and its edges: (8, 264) whole 4 x 4 blocks; (6, 264) two rows past the
     image; (5, 65) the one-quad form, tail rows, odd width; (1, 256), H = 1; (9, 4) one thread column; (16, 72) the block kernel; (16, 264) l2 and
     (40, 132) l1, where MYULA in Philox mode picks the two-iteration rows_pair launch and a stage launch must not.
  E  rotation and reductions (`E_CASES`): Philox, s in {2, 3, 4}, moments with burn_in = 1 and thin = 2, six iterations as six `step(1)` calls.
  F  the strided part of the perturbation grid (`F_CASES`), more than 8192 x 256 units, by the closed form of a linear drift: grad f = l x,
     prox = x / (1 + gamma sp), so X' = R_s x0 + q B_s Z per pixel costs nothing and the float32 replays are the stage recursion on flat arrays.

Out of scope: SK-ROCK with a non-convex term (MC-TV, ME-TV) -- tests/_ncvx_pixel.py holds the terms per pixel in the MYULA step kernels, which are the stage
launches, and in ULPDA; the stage recurrence with the term stays with the rel-L2 tests (tests/test_gpu_skrock.py); `tv_rtol`, `tv_warm` and
array-valued `epsg`, which SK-ROCK refuses (tests/test_gpu_skrock.py::test_c_abi_refusals)."""
import functools
import math
from collections import namedtuple

import numpy as np
from numpy.polynomial import chebyshev as cheb

from oracle import lmc_oracle as O
import _pixel as X
from _pixel import FACTOR, Stepper, check, f32, problem, region, region_pixels, ulp32      # noqa: F401  (re-exported to the two test files)

ETA = 0.05
STEP_FRACTION = 0.8
PHILOX_DXI = 2e-5
N_CHAINS = X.N_CHAINS
SEED, CHAIN_OFFSET = X.SEED, X.CHAIN_OFFSET
PERTURB_STRIDE = 8192 * 256          # kPerturbMaxBlocks x 256 threads: the units of one pass of the capped grid (lmc_skrock.hip)


# ------------------------------------------------------------------ coefficients and step
def _T(j, x):
    return cheb.chebval(x, [0.0] * j + [1.0])


def _dT(j, x):
    return cheb.chebval(x, cheb.chebder([0.0] * j + [1.0]))


@functools.lru_cache(maxsize=None)
def coefficients(s, eta=ETA):
    """(w0, w1, mu, nu, kappa): entry j - 1 of an array is stage j."""
    w0 = 1.0 + eta / s ** 2
    w1 = _T(s, w0) / _dT(s, w0)
    mu = np.array([w1 / w0] + [2 * w1 * _T(j - 1, w0) / _T(j, w0) for j in range(2, s + 1)])
    nu = np.array([s * w1 / 2] + [2 * w0 * _T(j - 1, w0) / _T(j, w0) for j in range(2, s + 1)])
    kappa = np.array([s * w1 / w0] + [-_T(j - 2, w0) / _T(j, w0) for j in range(2, s + 1)])
    for a in (mu, nu, kappa):
        a.setflags(write=False)
    return w0, w1, mu, nu, kappa


def step_factor(s, eta=ETA):
    return (s - 0.5) ** 2 * (2 - 4 * eta / 3) - 1.5


def closed_forms(s, z, eta=ETA):
    """(R_s, B_s) of a linear drift with delta times its eigenvalue = z: X' = R_s X + q B_s Z."""
    w0, w1, _, _, _ = coefficients(s, eta)
    return _T(s, w0 + w1 * z) / _T(s, w0), _dT(s, w0 + w1 * z) / _dT(s, w0) * (1 + w1 * z / 2)


# ------------------------------------------------------------------ cases
# part; base: the `_pixel.Case` whose problem, checker step and regions are used (mode "fused": its noise is the Philox field); s; noise ('injected' |
# 'philox' | 'none'); mode ('restart' | 'carried'); iters
SCase = namedtuple("SCase", "part base s noise mode iters")


def case_id(sc):
    return f"{sc.part}-{X.case_id(sc.base)}-s{sc.s}-{sc.noise}"


def label(sc):
    """The case `_pixel.check` prints and takes the regions of."""
    return sc.base._replace(tag=f"{sc.base.tag}-{sc.part}-s{sc.s}-{sc.noise}")


def _find(family, shape, tag):
    got = [c for c in X.CASES if (c.family, c.shape, c.tag) == (family, shape, tag)]
    assert len(got) == 1, (family, shape, tag, len(got))
    return got[0]


# list B: one case per family
B_BASES = [("pipe", (6, 264), "tv8-A"), ("pipe2", (6, 264), "tv10-B"), ("tile", (66, 67), "tv10-A"), ("split", (6, 257), "tv10-A"),
           ("point", (33, 65), "l1-A"), ("rows", (9, 516), "l1-A"), ("block", (16, 72), "haar-mask"), ("pois", (6, 264), "pipe-tv10-A"),
           ("wl2", (17, 67), "tile-tv10-A")]
B_STAGES = (2, 3, 4, 10, 15)
A_MAX = 150


def _thin_a(cases, keep=4):
    """Past A_MAX cases: of the cases of one family and shape that differ in their blur taps alone, `keep` tap sets stay -- the first and three of the
    others, rotating from one shape of the family to the next, so that every tap set a family has stays in it.  No family, seam class (shape) or data
    term leaves."""
    if len(cases) <= A_MAX:
        return cases
    groups = {}
    for c in cases:
        if c.data in X.BLURS:
            groups.setdefault((c.family, c.shape, c.term, c.prior, c.K, c.lagged, c.variant, c.tag.replace(f"-{c.data}", "-*")), []).append(c)
    dropped, ordinal = set(), {}
    for key, grp in groups.items():
        if len(grp) <= keep:
            continue
        g = ordinal.get(key[0], 0)
        ordinal[key[0]] = g + 1
        others = grp[1:]
        kept = {others[((keep - 1) * g + k) % len(others)] for k in range(keep - 1)}
        dropped |= set(others) - kept
    return [c for c in cases if c not in dropped]


def _philox(base, iters=2):
    return base._replace(mode="fused", iters=iters)


def _build_cases():
    out = []
    a = _thin_a([c for c in X.CASES if c.mode == "restart" and c.box is None])
    out += [SCase("A", c, 5, "injected", "restart", 2) for c in a]
    for key in B_BASES:
        out += [SCase("B", _find(*key), s, "injected", "restart", 2) for s in B_STAGES]
    for key in [("pipe", (6, 264), "tv8-A"), ("rows", (17, 67), "l1-A"), ("block", (8, 8), "haar-identity")]:
        out.append(SCase("C", _find(*key), 3, "none", "carried", 2))
    pipe = _find("pipe", (6, 264), "tv8-A")
    rows_pair = lambda shape, tag: _find("rows_pair", shape, tag)._replace(family="rows", kernel="myula_step_rows_kernel")
    d = [pipe._replace(shape=(8, 264)), pipe, _find("split", (5, 65), "tv10-A"), _find("pipe", (1, 256), "tv10-none"), _find("rows", (9, 4), "l1-A"),
         _find("block", (16, 72), "haar-identity"), rows_pair((16, 264), "l2-A-2it"), rows_pair((40, 132), "l1-A-2it")]
    # the pipe shapes the perturbation's draw had not seen: 4 pixels per lane, rows that are not 16-byte aligned, two column strips
    d += [_find("pipe", (6, 132), "tv8-A"), _find("pipe", (6, 261), "tv10-A-unaligned"), _find("pipe", (6, 1026), "tv10-A-strips")]
    for c in d:
        out += [SCase("D", _philox(c), s, "philox", "carried", 2) for s in (5, 2)]
    return out


CASES = _build_cases()
IDS = [case_id(sc) for sc in CASES]
assert len(set(IDS)) == len(IDS), "case ids must be unique"
BOX_CASES = [_find("pipe", (6, 264), "tv10box-A"), _find("tile", (66, 67), "tv10box-A")]
E_ITERS, E_BURN_IN, E_THIN = 6, 1, 2
E_CASES = [SCase("E", _philox(c, E_ITERS), s, "philox", "carried", E_ITERS)
           for c in (_find("pipe", (6, 264), "tv8-A"), _find("rows", (9, 4), "l1-A")) for s in (2, 3, 4)]
E_IDS = [case_id(sc) for sc in E_CASES]


def lipschitz(sc):
    c, m = sc.base, problem(sc.base)
    if c.term in ("pois", "wl2"):
        return float(Stepper(c, np.float64).pf.grad_lipschitz())
    return float(m.sigma_f)


def delta_of(sc):
    m = problem(sc.base)
    return float(np.float32(STEP_FRACTION * step_factor(sc.s) / (lipschitz(sc) + 1.0 / m.gamma)))


# ------------------------------------------------------------------ the terms of a case apart, in the dtype of a stepper
class Terms:
    """grad f and prox_{gamma g} of the case of `stepper`, as the checker's step forms them inside, and the fused launch over them:
    `launch(a, t, b, s, x, n)` = a x - t grad f(x) + b prox(x) + s n, the coefficients rounded to the stepper's dtype (from double, once)."""

    def __init__(self, stepper):
        self.st, self.dtype = stepper, stepper.dtype
        self.gamma = stepper.m.gamma

    def grad(self, x):
        st, T = self.st, self.dtype.type
        if not st.standard:
            return st.pf.grad(x)
        sf = T(st.m.sigma_f)
        if st.mask is not None:
            return sf * (st.mask * (st.mask * x - st.y))
        if st.h is not None:
            return sf * O.blur_adjoint(O.blur(x, st.h, st.m.offset) - st.y, st.h, st.m.offset)
        return sf * (x - st.y)

    def prox(self, x):
        st, T = self.st, self.dtype.type
        if not st.standard:
            return st.pg.prox(x, self.gamma)
        p = st.prior
        t = T(p["t"])
        if p["kind"] == "l2":
            return x / (T(1) + t * T(p["sigma"]))
        if p["kind"] == "l1":
            return np.sign(x) * np.maximum(np.abs(x) - t * T(p["sigma"]), 0)
        if p["kind"] == "tv":
            return O.tv_prox_fgp(x, float(t) * p["sigma"], p["niter"])
        if p["kind"] == "haar":
            return O.haar_l1_prox(x, float(t) * p["sigma"], 3)
        assert p["kind"] == "none", p["kind"]
        return x

    def launch(self, a, t, b, s, x, n):
        T = self.dtype.type
        out = T(a) * x - T(t) * self.grad(x) + T(b) * self.prox(x) + T(s) * n
        assert out.dtype == self.dtype, out.dtype
        return out

    def drift(self, x):
        return -self.grad(x) - (x - self.prox(x)) / self.dtype.type(self.gamma)


def fma32(a, b, c):
    """fma in float32: the product of two float32 numbers is exact in float64, the sum is rounded there and once more to float32 (the double
    rounding moves the result only where the float64 sum sits within 2^-29 of a float32 tie)."""
    return (np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(c, dtype=np.float64)).astype(np.float32)


# ------------------------------------------------------------------ one iteration, three ways
def iteration_definition(advance, x, Z, delta, s, dtype, stages=None):
    """The definition in `dtype` (arrays and coefficients).  advance(v, t) = v + t drift(v); Z = None: no noise.  `stages`: a list that receives
    K_1 .. K_s."""
    T = np.dtype(dtype).type
    _, _, mu, nu, kappa = coefficients(s)
    mu, nu, kappa = mu.astype(dtype), nu.astype(dtype), kappa.astype(dtype)
    delta = T(delta)
    q = np.sqrt(T(2) * delta)
    x = np.asarray(x, dtype=dtype)
    if Z is None:
        k1 = advance(x, float(mu[0] * delta))
    else:
        Z = np.asarray(Z, dtype=dtype)
        y = x + nu[0] * q * Z
        k1 = x + (advance(y, float(mu[0] * delta)) - y) + kappa[0] * q * Z
    k2 = x
    if stages is not None:
        stages.append(k1)
    for j in range(2, s + 1):
        k1, k2 = (advance(k1, float(mu[j - 1] * delta)) - k1) + nu[j - 1] * k1 + kappa[j - 1] * k2, k1
        if stages is not None:
            stages.append(k1)
    assert k1.dtype == np.dtype(dtype), k1.dtype
    return k1


def launch_coefficients(s, delta, gamma, noisy=True):
    """What `skrock_step` hands the launches, formed in double: (coef of Y, [(a, t, b, s_noise) per stage])."""
    _, _, mu, nu, kappa = coefficients(s)
    dg, q = delta / gamma, math.sqrt(2.0 * delta)
    out = [(1.0 - mu[0] * dg, mu[0] * delta, mu[0] * dg, (kappa[0] - nu[0]) * q if noisy else 0.0)]
    out += [(nu[j] - mu[j] * dg, mu[j] * delta, mu[j] * dg, kappa[j]) for j in range(1, s)]
    return nu[0] * q, out


def iteration_launch(terms, x, Z, delta, s, fault=None, stages=None):
    """The launch form in float32 (module docstring).  `fault(name, j, arrays)` may replace an array on the way (the planted faults of the CPU file):
    it is called with ("Y", 1, {Y, X, Z}), ("in", j, {K1, K2}) before stage j >= 2 forms its sum, ("out", j, {K}) after every stage and
    ("final", s, {K, Kprev})."""
    assert terms.dtype == np.float32
    T = np.float32
    gamma = terms.gamma
    hook = fault or (lambda name, j, a: a[next(iter(a))])
    coef, cs = launch_coefficients(s, delta, gamma, Z is not None)
    x = np.asarray(x, dtype=T)
    a, t, b, sn = cs[0]
    if Z is None:
        k1 = terms.launch(a, t, b, 0.0, x, T(0))
    else:
        Z = np.asarray(Z, dtype=T)
        y = hook("Y", 1, {"Y": fma32(T(coef), Z, x), "X": x, "Z": Z})
        sn = hook("s1", 1, {"s": np.full(x.shape, T(sn)), "coef": coef, "Y": y})
        k1 = T(a) * y - T(t) * terms.grad(y) + T(b) * terms.prox(y) + sn * Z
    k1 = hook("out", 1, {"K": k1})
    k2 = x
    if stages is not None:
        stages.append(k1)
    for j in range(2, s + 1):
        a, t, b, sn = cs[j - 1]
        n = hook("in", j, {"K2": k2, "K1": k1})
        new = hook("out", j, {"K": terms.launch(a, t, b, sn, k1, n)})
        k1, k2 = new, k1
        if stages is not None:
            stages.append(k1)
    k1 = hook("final", s, {"K": k1, "Kprev": k2})
    assert k1.dtype == T
    return k1


def iteration_third(terms, x, Z, delta, s):
    """A third float32 replay in another association: Y without fma, K_1 = Y + mu_1 delta drift(Y) + f32((kappa_1 - nu_1) q) Z, stage j as
    (nu_j K_{j-1} + kappa_j K_{j-2}) + mu_j delta drift(K_{j-1}).  A legitimate kernel could compute this; the CPU file holds it inside the bound."""
    assert terms.dtype == np.float32
    T = np.float32
    _, _, mu, nu, kappa = coefficients(s)
    q = math.sqrt(2.0 * delta)
    x = np.asarray(x, dtype=T)
    if Z is None:
        k1 = x + T(mu[0] * delta) * terms.drift(x)
    else:
        Z = np.asarray(Z, dtype=T)
        y = x + T(nu[0] * q) * Z
        k1 = (y + T(mu[0] * delta) * terms.drift(y)) + T((kappa[0] - nu[0]) * q) * Z
    k2 = x
    for j in range(1, s):
        k1, k2 = (T(nu[j]) * k1 + T(kappa[j]) * k2) + T(mu[j] * delta) * terms.drift(k1), k1
    assert k1.dtype == T
    return k1


# ------------------------------------------------------------------ references
# start: the float32 state both sides start this iteration from (None: they carry their own); ref32 / alt32: replays (a) and (b); rounding: the part of
# the bound that comes from the reference's float32 rounding, philox: the part that comes from the deviates; bound = rounding + philox
SStage = namedtuple("SStage", "start ref64 ref32 alt32 e32 bound rounding philox compare")


def make_stage(start, r64, ra, rb, philox_extra, compare):
    e32 = max(float(np.max(np.abs(r.astype(np.float64) - r64))) for r in (ra, rb))
    rounding = max(FACTOR * e32, 2.0 * ulp32(np.max(np.abs(r64))))
    assert r64.dtype == np.float64 and ra.dtype == np.float32 and rb.dtype == np.float32
    for a in (r64, ra, rb):
        a.setflags(write=False)
    return SStage(start, r64, ra, rb, e32, rounding + philox_extra, rounding, philox_extra, compare)


def noise_of(sc, it, dtype):
    return None if sc.noise == "none" else problem(sc.base).noise[it].astype(dtype)


def compute_reference(sc, order=("definition", "launch")):
    """The stages of case `sc`: a tuple of `SStage`, one per iteration.  `order`: which float32 replay runs first (nothing may depend on it)."""
    c, m = sc.base, problem(sc.base)
    s64, s32 = Stepper(c, np.float64), Stepper(c, np.float32)
    terms = Terms(s32)
    delta = delta_of(sc)
    extra = math.sqrt(2.0 * delta) * PHILOX_DXI if sc.noise == "philox" else 0.0

    def three(x64, xa, xb, it):
        r64 = iteration_definition(s64.advance, x64, noise_of(sc, it, np.float64), delta, sc.s, np.float64)
        Z = noise_of(sc, it, np.float32)
        out = {}
        for which in order:
            if which == "definition":
                out[which] = iteration_definition(s32.advance, xa, Z, delta, sc.s, np.float32)
            else:
                out[which] = iteration_launch(terms, xb, Z, delta, sc.s)
        return r64, out["definition"], out["launch"]

    stages = []
    if sc.mode == "restart":
        start = m.x0
        for it in range(sc.iters):
            r64, ra, rb = three(start, start, start, it)
            stages.append(make_stage(start, r64, ra, rb, extra, True))
            start = f32(r64)
    else:
        x64, xa, xb = m.x0.astype(np.float64), m.x0, m.x0
        for it in range(sc.iters):
            x64, xa, xb = three(x64, xa, xb, it)
            stages.append(make_stage(m.x0 if it == 0 else None, x64, xa, xb, extra, True))
    return tuple(stages)


@functools.lru_cache(maxsize=None)
def reference(sc):
    return compute_reference(sc)


# ------------------------------------------------------------------ part F: the strided perturbation grid by the closed form
F_ELL, F_SP, F_GAMMA = (float(np.float32(v)) for v in (1.3, 0.7, 0.4))      # tests/test_gpu_skrock.py::test_linear_drift_..., as float32 numbers
F_S = 2
F_KERNEL = "myula_step_point_kernel"       # identity data term + l2 prior on a thin image, variant="point"
# form: the perturbation kernel the shape picks; units = the (chain, quad) or element count its grid strides over
FCase = namedtuple("FCase", "form shape chains noise")
F_CASES = [FCase("injected-float4", (4, 32), 65543, "injected"),       # C H W / 4 = 2097376
           FCase("injected-scalar", (5, 7), 65543, "injected"),        # C H W = 2294005, odd
           FCase("philox-4x4", (2, 4), 2098151, "philox"),             # ceil(H / 4) (W / 4) C = C; two rows of every block past the image
           FCase("philox-quad", (2, 5), 419500, "philox")]             # ceil(H / 4) W C = 2097500
F_IDS = [f"F-{fc.form}-{fc.shape[0]}x{fc.shape[1]}x{fc.chains}" for fc in F_CASES]


def f_units(fc):
    H, W = fc.shape
    n = fc.chains * H * W
    return {"injected-float4": n // 4, "injected-scalar": n, "philox-4x4": -(-H // 4) * (W // 4) * fc.chains, "philox-quad": -(-H // 4) * W * fc.chains}[fc.form]


def f_unit_of(fc, chain, i, j):
    """The unit of the perturbation kernel's loop that writes pixel (i, j) of `chain`."""
    H, W = fc.shape
    flat = (chain * H + i) * W + j
    nq = -(-H // 4)
    return {"injected-float4": flat // 4, "injected-scalar": flat, "philox-4x4": chain * nq * (W // 4) + (i // 4) * (W // 4) + j // 4,
            "philox-quad": chain * nq * W + (i // 4) * W + j}[fc.form]


def f_form_expected(fc):
    """The form `launch_skrock_perturb*` picks for the shape (arrays from the allocator are 16-byte aligned)."""
    H, W = fc.shape
    if fc.noise == "philox":
        return "philox-4x4" if W % 4 == 0 else "philox-quad"
    return "injected-float4" if (fc.chains * H * W) % 4 == 0 else "injected-scalar"


def f_delta():
    return float(np.float32(0.9 * step_factor(F_S) / (F_ELL + 1.0 / F_GAMMA)))


FProblem = namedtuple("FProblem", "x0 Z")


def f_problem(fc):
    """x0 = 250 + N(0, 20) (the magnitudes of the image cases, so that the allowance for the deviates stays under a tenth of 3 e32) and the field,
    float32 [C, H, W].  Not cached: a case holds up to 70 MB per array."""
    H, W = fc.shape
    rng = np.random.default_rng(500 + 10 * H + W)
    x0 = np.float32(250.0) + np.float32(20.0) * rng.standard_normal((fc.chains, H, W), dtype=np.float32)
    assert x0.dtype == np.float32
    if fc.noise == "philox":
        Z = np.empty((fc.chains, H, W), dtype=np.float32)
        for a in range(0, fc.chains, 1 << 18):
            b = min(a + (1 << 18), fc.chains)
            Z[a:b] = O.philox_normals(SEED, 0, CHAIN_OFFSET + np.arange(a, b), H, W)
    else:
        Z = rng.standard_normal((fc.chains, H, W), dtype=np.float32)
    return FProblem(x0, Z)


class _LinearAdvance:
    """v + t drift(v) of the linear drift in `dtype`, in the form of the checker's step: (1 - t / gamma) v - t l v + (t / gamma) v / (1 + gamma sp)."""

    def __init__(self, dtype):
        self.dtype = np.dtype(dtype)
        self.gamma = F_GAMMA

    def grad(self, x):
        return self.dtype.type(F_ELL) * x

    def prox(self, x):
        T = self.dtype.type
        return x / (T(1) + T(F_GAMMA) * T(F_SP))

    def launch(self, a, t, b, s, x, n):
        T = self.dtype.type
        return T(a) * x - T(t) * self.grad(x) + T(b) * self.prox(x) + T(s) * n

    def advance(self, x, t):
        return self.launch(1 - t / F_GAMMA, t, t / F_GAMMA, 0.0, x, self.dtype.type(0))

    def drift(self, x):
        return -self.grad(x) - (x - self.prox(x)) / self.dtype.type(F_GAMMA)


def f_reference(fc, m):
    """One `SStage` of case `fc` on the problem `m`: ref64 = R_s x0 + q B_s Z, the two float32 replays on the whole arrays."""
    delta = f_delta()
    l_eff = F_ELL + F_SP / (1 + F_GAMMA * F_SP)
    R, B = closed_forms(F_S, -delta * l_eff)
    assert abs(R) <= 1.0 and abs(B) <= 1.0, (R, B)
    r64 = R * m.x0.astype(np.float64) + math.sqrt(2 * delta) * B * m.Z.astype(np.float64)
    lin = _LinearAdvance(np.float32)
    ra = iteration_definition(lin.advance, m.x0, m.Z, delta, F_S, np.float32)
    rb = iteration_launch(lin, m.x0, m.Z, delta, F_S)
    extra = math.sqrt(2.0 * delta) * PHILOX_DXI if fc.noise == "philox" else 0.0
    return make_stage(m.x0, r64, ra, rb, extra, True)


def f_check(fc, got, st):
    """Every chain and pixel against the bound; reports the worst pixel, its unit in the perturbation kernel's loop and the stride that unit is in."""
    d = np.abs(np.asarray(got, dtype=np.float64) - st.ref64)
    d = np.where(np.isfinite(d), d, np.inf)
    k = tuple(int(v) for v in np.unravel_index(int(np.argmax(d)), d.shape))
    err = float(d[k])
    unit = f_unit_of(fc, *k)
    stride = "second" if unit >= PERTURB_STRIDE else "first"
    second = d.reshape(-1)[_second_stride_mask(fc)]
    msg = (f"pixel F-{fc.form} {fc.shape} x {fc.chains}: err {err:.3e} at chain {k[0]} pixel ({k[1]}, {k[2]}), unit {unit} of {f_units(fc)} [{stride} stride], "
           f"e32 {st.e32:.3e}, ratio {err / st.e32:.2f}, bound {st.bound:.3e} = rounding {st.rounding:.3e} + philox {st.philox:.3e}; worst of the "
           f"{second.size} pixels of the second stride {float(second.max()):.3e}")
    print(msg)
    return X.Verdict(err <= st.bound, err, st.bound, st.e32, err / st.e32, k, f"{stride} stride", msg)


def _second_stride_mask(fc):
    """Flat indices of the pixels whose unit is in the second pass of the grid (units >= PERTURB_STRIDE)."""
    H, W = fc.shape
    n = fc.chains * H * W
    if fc.form == "injected-float4":
        return np.arange(4 * PERTURB_STRIDE, n)
    if fc.form == "injected-scalar":
        return np.arange(PERTURB_STRIDE, n)
    per_chain = -(-H // 4) * (W // 4 if fc.form == "philox-4x4" else W)
    # units are ordered by chain first: whole chains from the first one whose first unit is past the stride, and the tail of the chain before it
    idx = np.arange(n)
    chain, rem = idx // (H * W), idx % (H * W)
    i, j = rem // W, rem % W
    unit = chain * per_chain + (i // 4) * (W // 4 if fc.form == "philox-4x4" else W) + (j // 4 if fc.form == "philox-4x4" else j)
    return idx[unit >= PERTURB_STRIDE]


def worst(verdicts):
    return max(verdicts, key=lambda v: v.ratio)

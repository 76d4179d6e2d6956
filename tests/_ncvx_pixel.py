"""Per-pixel parity of the non-convex data terms of L2_ncvx_tv (MC-TV isotropic and anisotropic, ME-TV) against float64: the case lists, the references
and the bound.  numpy only; tests/test_ncvx_pixel_reference.py (CPU) checks this harness on every case and plants the faults the bound has to see,
tests/test_gpu_ncvx_pixel.py runs the kernels against it.  The conventions are those of tests/_pixel.py, whose `problem`, `Stepper`, `bound_of`, `region`,
`check`, `ulp32` and FACTOR = 3 are used as they are: every input is rounded to float32 once, the library gets those numbers and the reference gets them
cast back to float64; `bound = max(3 e32, 2 ulp32(max |ref64|))` at every chain and pixel, measured on the reference and never on a kernel.

The term.  `O.L2NcvxTV.grad_moreau` returns the dtype of its input, but the class is built around float64 operators; `moreau` below restates it so that
"every routine computes in the dtype of its input": MC-TV isotropic A^T(min(1 / gamma, 1 / |A x|) A x) with the reference's 1e-9 branch at |A x| = 0,
MC-TV anisotropic A^T(v - soft(v, gamma)) / gamma (= v_i / max(|v_i|, gamma) component by component), ME-TV (x - O.tv_prox_fgp(x, gamma, niter)) / gamma.
The CPU file holds it equal to `O.L2NcvxTV.grad_moreau` and the gradient built on it equal to `O.L2NcvxTV.grad` to 1e-12 in float64 on every case.  The
step is the checker's (`O.myula`): a x - tau (grad f(x) - lamda moreau(x)) + b prox(x) + sqrt(2 tau) xi, grad f and prox taken from
`_skrock_pixel.Terms` (the checker's own, stated apart).

Two float32 replays, `e32` the larger of their distances to ref64 (as tests/_ulpda_pixel.py and tests/_skrock_pixel.py):
  (a) the definition with every array and coefficient in float32;
  (b) the launch form (`moreau_launch`, `Step.launch`): the weights as the reciprocal of max(sqrt(fma(dx, dx, dy dy)), gamma) (of max(|v_i|, gamma)), the
      divergence in the kernels' order (vx - vx_up) + (vy - vy_left), the term subtracted from the gradient by one fma with -lamda (ME-TV: one fma with
      -lamda / gamma rounded once on x - prox), and the combine as a chain of fma.

Two weightings per case group, because the floor of a state of 200 hides a small term:
  "cfg"   lamda = 0.3, gamma = 15 (tests/golden/algs.npz, tests/test_gpu_ncvx.py; `_mala_ref.NCVX_KW` has the same two numbers for ME-TV);
  "prom"  tau lamda = 1 (MC-TV), tau lamda / gamma = 1 (ME-TV): the state inherits the term, or the inner prox's error, at full size.  One such step need
          not be stable; the restart after the first iteration keeps the second a single step.

Conditions on the inputs (`conditions`; asserted on the CPU for every case -- conditions, not measurements): the share of pixels of x0 with
|grad x| < gamma lies in [0.2, 0.8]; a block of min(3, H) x 3 pixels of x0 is one constant in both chains (`flat_block`), so that 2 x 2 pixels (1 x 2
where H = 1, a single row) have |grad x| = 0 exactly: the reference's 1e-9 branch; for "prom" cases the median over pixels of |tau lamda moreau(x0)|, the
term's contribution to the state, is at least 1e3 bounds.

Parts.  `CASES`: the MYULA step kernels with the term (tile, split, point, block, rows, pipe, pipe2), each with the exact `kernel_name` the dispatch of
lmc_problem.hip gives (None: the variant must refuse with LMC_E_UNSUPPORTED).  `P_CASES`: `L2_ncvx_tv.prox` with a pointwise data term -- the pre-step
(ulpda_ncvx_rhs_kernel, ulpda_me_rhs_kernel) followed by the closed-form solve out = (pre + tau sigma m b) / (1 + tau sigma m m).  `S_CASES`: the same with blur A in front of the converged solve of tests/_ulpda_pixel.py (its
truncation condition and floors), and ULPDA sampler iterations in restart mode with the identity and with blur A, state and dual.  `E_CASES`: the value
`L2_ncvx_tv.__call__` at the "prom" weight over the 32 x 64 tile of the energy kernels.

Out of this rung: ME-TV with rtol > 0 (its pass count is a discontinuous function of the state; pinned by the pass-count tests), anisotropic ME-TV (a 1-D
TV of the flattened image, which the checker's class does not restate either), and SK-ROCK and MYMALA with a non-convex term (rel-L2 in
tests/test_gpu_skrock.py and tests/test_gpu_mymala_matrix.py)."""
import functools
from collections import namedtuple

import numpy as np

from oracle import lmc_oracle as O
import _pixel as X
import _skrock_pixel as S
import _ulpda_pixel as U
from _pixel import FACTOR, check, f32, region, ulp32      # noqa: F401  (re-exported to the two test files)
from _skrock_pixel import fma32

N_CHAINS = X.N_CHAINS
CFG_LAMBDA, CFG_GAMMA = 0.3, 15.0
FLAT_LEVEL = 100.0
NORM_RTOL = 5e-5       # what the rel-L2 tests of trajectories assert (tests/test_gpu_ncvx.py, tests/test_gpu_matrix.py)

# base: the `_pixel.Case` whose problem recipe, checker step and regions are used; nc ('mc' | 'mca' | 'me'); niter: dual iterations of the inner prox
# (ME-TV); weight ('cfg' | 'prom')
NCase = namedtuple("NCase", "base nc niter weight")


def case_id(n):
    return X.case_id(n.base)


def lam_of(n, tau=X.TAU):
    """lamda of the case, rounded to float32 once (the library keeps it as a float)."""
    if n.weight == "cfg":
        return float(np.float32(CFG_LAMBDA))
    return float(np.float32((CFG_GAMMA if n.nc == "me" else 1.0) / tau))


def _mult(step, n):
    return tuple(range(step, n, step))


def _build_cases():
    out = []

    def add(family, shape, tag, nc, niter=0, data="A", prior="tv", K=10, lagged=False, variant=None, kernel=None, mode="restart", iters=2, rows=(), cols=()):
        for w in ("cfg", "prom"):
            t = f"{nc}{niter if nc == 'me' else ''}-{tag}-{w}"
            base = X.Case(family, shape, "l2", data, prior, K if prior in ("tv", "aniso") else 0, lagged, None, variant or family, kernel, mode, iters,
                          tuple(rows), tuple(cols), t)
            out.append(NCase(base, nc, niter, w))

    # ---- tile: output tiles of at most 64 x 64 with a halo; ME-TV: the inner prox in chunks of 8 (10: one launch; 17, 18: a last chunk of 1, 2; 50)
    def tile(shape, tag, nc, **kw):
        add("tile", shape, tag, nc, kernel="myula_step_tile_kernel", rows=_mult(64, shape[0]), cols=_mult(64, shape[1]), **kw)
    for nc in ("mc", "mca"):
        for s in [(3, 5), (17, 67), (66, 67), (65, 130)]:
            for b in "AB":
                tile(s, f"tv10-{b}", nc, data=b)
        for d in ("identity", "mask"):
            tile((66, 67), f"tv10-{d}", nc, data=d)
        tile((66, 67), "l1-A", nc, prior="l1")
    for k in (10, 17, 18, 50):
        for s in [(17, 67), (66, 67)]:
            tile(s, "tv10-A", "me", niter=k)

    # ---- split: one wave per 64 columns
    def split(shape, tag, nc, **kw):
        add("split", shape, tag, nc, kernel="myula_step_split_kernel", cols=_mult(64, shape[1]), **kw)
    for s in [(5, 64), (5, 65), (5, 129), (6, 257), (1, 300)]:
        split(s, "tv10-A", "mc")
    split((5, 65), "tv5-A", "mc", K=5)
    for s in [(5, 65), (6, 257)]:
        split(s, "tv10-A", "mca")
    # ME-TV: a forced variant runs the inner prox too (me_tv_prox); the split kernel has instantiations up to 12 dual iterations, so 50 must refuse
    add("split", (5, 129), "tv10-A", "me", niter=50, kernel=None, cols=(64, 128))
    for s in [(5, 65), (5, 129)]:
        split(s, "tv10-A", "me", niter=10)

    # ---- point: tiles of 32 rows x 64 columns
    for nc in ("mc", "mca"):
        for s in [(33, 65), (34, 130)]:
            for p, b in (("l1", "A"), ("l2", "B")):
                add("point", s, f"{p}-{b}", nc, data=b, prior=p, kernel="myula_step_point_kernel", rows=_mult(32, s[0]), cols=_mult(64, s[1]))

    # ---- block: the fused Haar + MC-TV kernel (a rolling window over the 8 x 8 register blocks); l1 / l2: the block kernel without the term, then
    # mc_tv_add_kernel on its output (launch_step_nobox) -- `kernel_name` is the block kernel's in both
    for s in [(8, 8), (16, 72)]:
        for nc in ("mc", "mca"):
            for d in ("identity", "mask"):
                add("block", s, f"haar-{d}", nc, data=d, prior="haar", kernel="myula_step_block_kernel", rows=_mult(8, s[0]), cols=_mult(8, s[1]))
        for p in ("l1", "l2"):
            add("block", s, f"{p}-identity-add", "mc", data="identity", prior=p, kernel="myula_step_block_kernel", rows=_mult(8, s[0]), cols=_mult(8, s[1]))
    add("block", (16, 72), "l1-mask-add", "mca", data="mask", prior="l1", kernel="myula_step_block_kernel", rows=(8,), cols=_mult(8, 72))

    # ---- rows: ME-TV reaches the row kernel as a ready-made gradient array (StepArgs::extra).  The row kernel has no TV prox, so variant="rows" refuses
    # the inner prox; the library's own choice runs the inner prox where it fits and the step on the row kernel.  MC-TV is not covered (rows_supported).
    for s in [(9, 4), (17, 67), (9, 516)]:
        for p in ("l1", "l2", "none"):
            add("rows", s, f"{p}-A", "me", niter=10, prior=p, variant="auto", kernel="myula_step_rows_kernel", rows=_mult(16, s[0]),
                cols=_mult(496, s[1]) if s[1] > 512 else ())
    add("rows", (17, 67), "l1-A-forced", "me", niter=10, prior="l1", kernel=None, rows=(16,))
    add("rows", (17, 67), "l1-A", "mc", prior="l1", kernel=None, rows=(16,))

    # ---- pipe (blur only with a term, pipe_geometry_ok): vx of the previous row in registers, vy across lanes, column strips of 512
    def pipe(shape, tag, nc, kernel="myula_step_pipe_kernel", variant="pipe", family="pipe", **kw):
        cols = _mult(512, shape[1]) if shape[1] > 512 else _mult(64, shape[1]) if nc != "me" else ()
        add(family, shape, tag, nc, variant=variant, kernel=kernel, cols=cols, **kw)
    for nc in ("mc", "mca"):
        for s in [(6, 132), (6, 264), (1, 256)]:
            pipe(s, "tv10-A", nc)
        for s in [(6, 133), (6, 261)]:
            pipe(s, "tv10-A-unaligned", nc)
    for s in [(6, 513), (6, 1026)]:
        pipe(s, "tv10-A-strips", "mc")
    pipe((6, 513), "tv10-A-strips", "mca")
    for K in (2, 6, 8):
        pipe((6, 264), f"tv{K}-A", "mc", K=K)
    pipe((6, 264), "tv9lagged-A", "mc", K=9, lagged=True)
    pipe((6, 264), "tv20-A-chained", "mc", K=20)
    pipe((6, 264), "tv2-A-warm", "mc", K=2, mode="warm", iters=3, variant="auto", kernel="myula_step_pipe_kernel(warm)")
    for b in "BD":
        pipe((6, 264), f"tv10-{b}", "mc", data=b)
    pipe((6, 264), "aniso10-A", "mc", prior="aniso", kernel="myula_step_pipe_aniso_kernel")
    for s in [(6, 264), (6, 132)]:
        pipe(s, "tv10-A", "me", niter=50)
    # ---- pipe2: the two-team layout exchanges no seam columns of the term (pipe_teams_covered): it must refuse
    pipe((6, 264), "tv10-A", "mc", variant="pipe2", family="pipe2", kernel=None)
    pipe((6, 264), "tv10-A", "me", niter=50, variant="pipe2", family="pipe2", kernel=None)
    return out


CASES = _build_cases()
IDS = [case_id(n) for n in CASES]
assert len(set(IDS)) == len(IDS), "case ids must be unique"
FAMILIES = ("tile", "split", "point", "block", "rows", "pipe", "pipe2")


# ------------------------------------------------------------------ the term, in the dtype handed in
def moreau(x, nc, gamma, niter=0):
    """grad of the Moreau envelope, `O.L2NcvxTV.grad_moreau` on [..., H, W] in the dtype of x."""
    x = np.asarray(x)
    T = x.dtype.type
    g = T(gamma)
    if nc == "me":
        out = (x - O.tv_prox_fgp(x, gamma, niter)) / g
    else:
        dr, dc = O.grad2d(x)
        if nc == "mc":
            e = np.sqrt(dr * dr + dc * dc)
            e = np.where(e != 0, e, T(1e-9))
            w = np.minimum(T(1) / g, T(1) / e)
            out = -O.div2d(w * dr, w * dc)
        else:
            soft = lambda v: np.sign(v) * np.maximum(np.abs(v) - g, T(0))
            out = -O.div2d(dr - soft(dr), dc - soft(dc)) / g
    assert out.dtype == x.dtype, (nc, out.dtype)
    return out


def _weights_launch(dr, dc, nc, g):
    if nc == "mc":
        w = np.float32(1) / np.maximum(np.sqrt(fma32(dr, dr, dc * dc)), g)
        return w, w
    return np.float32(1) / np.maximum(np.abs(dr), g), np.float32(1) / np.maximum(np.abs(dc), g)


def _shift(v, axis):
    """v of the upper (axis -2) or left (axis -1) neighbour, zero outside the image."""
    out = np.zeros_like(v)
    if axis == -2:
        out[..., 1:, :] = v[..., :-1, :]
    else:
        out[..., :, 1:] = v[..., :, :-1]
    return out


def moreau_launch(x, nc, gamma, niter=0, fault=None):
    """The term as `mc_tv_grad` of lmc_device.h states it, in float32: A^T v summed as -((vx - vx_up) + (vy - vy_left)), the neighbour outside the image
    taken as zero.  ME-TV: x - prox, the division left to the coefficient (`Step.launch`).  `fault`: a planted fault, (kind, ...) --
    tests/test_ncvx_pixel_reference.py."""
    x = np.asarray(x, dtype=np.float32)
    g = np.float32(gamma)
    kind = fault[0] if fault is not None else None
    if nc == "me":
        p = O.tv_prox_fgp(x, gamma, niter)
        if kind == "short-row":         # the inner prox one dual iteration short along one row of one tile
            _, row, c0, c1 = fault
            p = p.copy()
            p[..., row, c0:c1] = O.tv_prox_fgp(x, gamma, niter - 1)[..., row, c0:c1]
        return x - p
    dr, dc = O.grad2d(x)
    wx, wy = _weights_launch(dr, dc, nc, g)
    if kind == "iso-row":               # the isotropic weight on one row of an anisotropic case
        wi, _ = _weights_launch(dr, dc, "mc", g)
        wx, wy = wx.copy(), wy.copy()
        wx[..., fault[1], :] = wi[..., fault[1], :]
        wy[..., fault[1], :] = wi[..., fault[1], :]
    vx, vy = wx * dr, wy * dc
    vy_left = _shift(vy, -1)
    if kind == "row-below":             # the (i, j-1) neighbour's dx formed as if a row existed below the last row (x there read as zero): its weight
        assert nc == "mc"               # as the left neighbour of the last row changes; its own pixel still uses the right one
        ghost = -x[..., -1, :]
        wl = np.float32(1) / np.maximum(np.sqrt(fma32(ghost, ghost, dc[..., -1, :] * dc[..., -1, :])), g)
        vy_left = vy_left.copy()
        vy_left[..., -1, 1:] = (wl * dc[..., -1, :])[..., :-1]
    if kind == "seam-vy":               # vy of the column left of a seam taken as zero at that one column
        vy_left = vy_left.copy()
        vy_left[..., :, fault[1]] = 0
    out = -((vx - _shift(vx, -2)) + (vy - vy_left))
    if kind == "last-row":              # the term's last row scaled by 1 - 5e-3
        out = out.copy()
        out[..., -1, :] *= np.float32(1 - 5e-3)
    assert out.dtype == np.float32
    return out


# ------------------------------------------------------------------ the problem of a case
def flat_block(shape):
    """(r0, r1, c0, c1): the block of x0 that is one constant in both chains."""
    H, W = shape
    r0 = max(0, min(H - 3, H // 2 - 1))
    c0 = max(0, min(W - 3, W // 3))
    return r0, min(H, r0 + 3), c0, min(W, c0 + 3)


@functools.lru_cache(maxsize=None)
def problem(n):
    """`_pixel.problem` of the base case with the flat block written into x0."""
    m = X.problem(n.base)
    x0 = m.x0.copy()
    r0, r1, c0, c1 = flat_block(n.base.shape)
    x0[:, r0:r1, c0:c1] = np.float32(FLAT_LEVEL)
    x0.setflags(write=False)
    return m._replace(x0=x0)


class Step:
    """One replay of the step with the term in `dtype`: `step` the definition, `launch` the launch form (float32 only).  The warm mode carries the TV
    dual in the object."""

    def __init__(self, n, dtype, fault=None):
        self.n, self.dtype, self.fault = n, np.dtype(dtype), fault
        self.st = X.Stepper(n.base._replace(mode="restart"), dtype)
        self.terms = S.Terms(self.st)
        self.m = self.st.m
        self.lam = lam_of(n, self.m.tau)
        self.dual = None

    def prox(self, x):
        c = self.n.base
        if c.mode != "warm":
            return self.terms.prox(x)
        px, self.dual = O.tv_prox_fgp(x, self.m.gamma * X.weight(c), c.K, dual0=self.dual, return_dual=True)
        return px

    def term(self, x):
        return moreau(np.asarray(x, dtype=self.dtype), self.n.nc, CFG_GAMMA, self.n.niter)

    def grad(self, x):
        """grad f(x) - lamda moreau(x): `O.L2NcvxTV.grad`."""
        x = np.asarray(x, dtype=self.dtype)
        return self.terms.grad(x) - self.dtype.type(self.lam) * self.term(x)

    def step(self, x, xi):
        T, m = self.dtype.type, self.m
        x, xi = np.asarray(x, dtype=self.dtype), np.asarray(xi, dtype=self.dtype)
        out = T(1 - m.tau / m.gamma) * x - T(m.tau) * self.grad(x) + T(m.tau / m.gamma) * self.prox(x) + T(np.sqrt(2 * m.tau)) * xi
        assert out.dtype == self.dtype, out.dtype
        return out

    def launch(self, x, xi):
        assert self.dtype == np.float32
        T, m, n = np.float32, self.m, self.n
        x, xi = np.asarray(x, dtype=T), np.asarray(xi, dtype=T)
        t = moreau_launch(x, n.nc, CFG_GAMMA, n.niter, self.fault)
        coef = T(-self.lam / CFG_GAMMA) if n.nc == "me" else T(-self.lam)
        g = fma32(coef, t, self.terms.grad(x))
        out = fma32(T(np.sqrt(2 * m.tau)), xi, fma32(T(m.tau / m.gamma), self.prox(x), fma32(-T(m.tau), g, T(1 - m.tau / m.gamma) * x)))
        assert out.dtype == T
        return out


# the fields of `_pixel.Stage`, then alt32 (the launch-form replay) and contrib (|tau lamda moreau(start)| in float64: what the term moves the state by)
NStage = namedtuple("NStage", X.Stage._fields + ("alt32", "contrib"))


def _stage(n, start, r64, r32, alt, compare, contrib):
    e32 = max(X.bound_of(r64, r)[0] for r in (r32, alt))
    bound = max(FACTOR * e32, 2.0 * ulp32(np.max(np.abs(r64))))
    for a in (r64, r32, alt):
        a.setflags(write=False)
    assert r64.dtype == np.float64 and r32.dtype == np.float32 and alt.dtype == np.float32
    return NStage(start, r64, r32, e32, bound, compare, alt, contrib)


def _reference(n, order=(0, 1, 2)):
    m, c = problem(n), n.base
    steps = [Step(n, np.float64), Step(n, np.float32), Step(n, np.float32)]
    fns = [steps[0].step, steps[1].step, steps[2].launch]
    stages = []
    cur = [m.x0.astype(np.float64), m.x0, m.x0]
    for it in range(c.iters):
        contrib = m.tau * steps[0].lam * np.abs(steps[0].term(cur[0]))
        res = [None, None, None]
        for k in order:
            res[k] = fns[k](cur[k], m.noise[it])
        if c.mode == "restart":
            stages.append(_stage(n, f32(cur[0]), res[0], res[1], res[2], True, contrib))
            nxt = f32(res[0])
            cur = [nxt.astype(np.float64), nxt, nxt]
        else:       # warm: carried, compared after every iteration
            stages.append(_stage(n, m.x0 if it == 0 else None, res[0], res[1], res[2], True, contrib))
            cur = res
    return tuple(stages)


@functools.lru_cache(maxsize=None)
def reference(n):
    """The stages of case `n`, computed once."""
    return _reference(n)


def conditions(n, x0, gamma=CFG_GAMMA):
    """(share of pixels with |grad x0| < gamma, number of pixels with |grad x0| = 0 inside the flat block in every chain)."""
    x = np.asarray(x0, dtype=np.float64)
    dr, dc = O.grad2d(x)
    e = np.sqrt(dr * dr + dc * dc)
    r0, r1, c0, c1 = flat_block(x.shape[-2:])
    flat = int(np.sum(np.all(e[:, r0:r1, c0:c1] == 0, axis=0)))
    return float(np.mean(e < gamma)), flat


# ====================================================================== L2_ncvx_tv.prox with a pointwise data term
P_TAU, P_SIGMA = 0.25, 1.75       # tau sigma = 0.4375, exact in float32
PCase = namedtuple("PCase", "family shape data nc niter weight K seam_rows seam_cols tag")      # K, seams: read by `_pixel.region` (no seams here)


def _build_p():
    out = []
    for s in [(3, 5), (17, 67), (33, 130)]:
        for d in ("identity", "mask"):
            for nc, k in (("mc", 0), ("mca", 0), ("me", 10), ("me", 50)):
                for w in ("cfg", "prom"):
                    out.append(PCase("prox", s, d, nc, k, w, 0, (), (), f"{nc}{k or ''}-{d}-{w}"))
    return out


P_CASES = _build_p()
P_IDS = [X.case_id(c) for c in P_CASES]
assert len(set(P_IDS)) == len(P_IDS)
PProblem = namedtuple("PProblem", "x0 b mask")


@functools.lru_cache(maxsize=None)
def _p_problem(shape, data):
    rng = np.random.default_rng(5000 + 1000 * shape[0] + shape[1])
    img = X.step_image(shape)
    mask = f32(rng.uniform(size=shape) < 0.6) if data == "mask" else None
    b = f32((img + rng.normal(0, X.SIGMA, shape)) * (mask if mask is not None else 1.0))
    x0 = f32(img[None] + rng.normal(0, 10, (N_CHAINS,) + shape))
    r0, r1, c0, c1 = flat_block(shape)
    x0[:, r0:r1, c0:c1] = np.float32(FLAT_LEVEL)
    for a in (x0, b, mask):
        if a is not None:
            a.setflags(write=False)
    return PProblem(x0, b, mask)


def p_problem(c):
    return _p_problem(c.shape, c.data)


def p_lam(c):
    return lam_of(c, P_TAU)


def p_prestep(c, x):
    """x + tau lamda moreau(x) in the dtype of x (algs.py:213-223)."""
    T = x.dtype.type
    return x + T(P_TAU) * T(p_lam(c)) * moreau(x, c.nc, CFG_GAMMA, c.niter)


def p_solve(c, pre):
    """(pre + tau sigma m b) / (1 + tau sigma m m) in the dtype of pre."""
    m, T = p_problem(c), pre.dtype.type
    ts = T(P_TAU) * T(P_SIGMA)
    mk = T(1) if m.mask is None else m.mask.astype(pre.dtype)
    return (pre + ts * mk * m.b.astype(pre.dtype)) / (T(1) + ts * mk * mk)


def p_launch(c, x):
    """The same in the kernels' form, float32: rhs = fma(coef, term, x) with coef = tau lamda (ME-TV: tau lamda / gamma on x - prox) rounded once, then
    fma(ts m, b, rhs) / fma(ts m, m, 1)."""
    T, m = np.float32, p_problem(c)
    x = np.asarray(x, dtype=T)
    t = moreau_launch(x, c.nc, CFG_GAMMA, c.niter)
    coef = T(P_TAU * p_lam(c) / CFG_GAMMA) if c.nc == "me" else T(T(P_TAU) * T(p_lam(c)))
    rhs = fma32(coef, t, x)
    tm = T(P_TAU * P_SIGMA) * (T(1) if m.mask is None else m.mask)
    out = fma32(tm, m.b, rhs) / fma32(tm, T(1) if m.mask is None else m.mask, T(1))
    assert out.dtype == T
    return out


@functools.lru_cache(maxsize=None)
def p_reference(c):
    m = p_problem(c)
    x64 = m.x0.astype(np.float64)
    pre64 = p_prestep(c, x64)
    r64, r32, alt = p_solve(c, pre64), p_solve(c, p_prestep(c, m.x0)), p_launch(c, m.x0)
    contrib = np.abs(pre64 - x64)
    return _stage(c, m.x0, r64, r32, alt, True, contrib)


# ====================================================================== L2_ncvx_tv.prox with blur A, and one ULPDA sampler iteration
# The converged-solve machinery of tests/_ulpda_pixel.py: tau sigma = 127 / 128 x 1.75 exact in float32, 50 fixed CG iterations (tolerance 0), ref64 the
# float64 solve run to 1e-13, ref32 `O.cg_solve` in float32 for 50 iterations; its `trunc` condition: float64 CG two iterations short (48) within e32 / 10
# of the solution.  ME-TV runs at niter = 50 only here: the class uses one `niter` for the inner prox and for the solve, and 10 CG iterations do not
# converge.
S_TAU, S_MU, S_THETA = U.B_TAU, U.A_MU, 1.0
SCase = namedtuple("SCase", "family shape entry data nc niter weight K seam_rows seam_cols tag")      # entry: 'prox' | 'sampler'; data: 'A' | 'identity'


def _build_s():
    out = []
    for s in [(17, 67), (40, 64)]:
        for nc, k in (("mc", 0), ("mca", 0), ("me", 50)):
            for w in ("cfg", "prom"):
                out.append(SCase("proxblur", s, "prox", "A", nc, k, w, 0, _mult(16, s[0]), (), f"{nc}{k or ''}-A-{w}"))
    for d in ("identity", "A"):
        for nc, k in (("mc", 0), ("me", 50 if d == "A" else 10)):
            for w in ("cfg", "prom"):
                out.append(SCase("ulpda", (17, 67), "sampler", d, nc, k, w, 0, (16,) if d == "A" else (), (), f"{nc}{k or ''}-{d}-{w}"))
    return out


S_CASES = _build_s()
S_IDS = [X.case_id(c) for c in S_CASES]
assert len(set(S_IDS)) == len(S_IDS)
SProblem = namedtuple("SProblem", "h offset b x0 y0 noise")


@functools.lru_cache(maxsize=None)
def _s_problem(shape, data):
    rng = np.random.default_rng(6000 + 1000 * shape[0] + shape[1])
    img = X.step_image(shape)
    h, off = (f32(X.BLURS["A"][0]), X.BLURS["A"][1]) if data == "A" else (None, None)
    b = f32((O.blur(img, h.astype(np.float64), off) if h is not None else img) + rng.normal(0, X.SIGMA, shape))
    x0 = f32(img[None] + rng.normal(0, 10, (N_CHAINS,) + shape))
    r0, r1, c0, c1 = flat_block(shape)
    x0[:, r0:r1, c0:c1] = np.float32(FLAT_LEVEL)
    y0 = f32(rng.normal(0, 0.5 * U.RADIUS, (N_CHAINS, 2) + shape))
    noise = f32(rng.standard_normal((2, N_CHAINS) + shape))
    for a in (h, b, x0, y0, noise):
        if a is not None:
            a.setflags(write=False)
    return SProblem(h, off, b, x0, y0, noise)


def s_problem(c):
    return _s_problem(c.shape, c.data)


def s_lam(c):
    return lam_of(c, S_TAU)


class SProx:
    """prox_{tau f} of `L2_ncvx_tv` for case `c`, batched over the chains: the pre-step, then the solve.  kind: 'exact' (float64: the closed form, or the
    solve run to 1e-13), 'def' (the definition in float32: closed form / 50 CG iterations), 'launch' (the kernels' form), 'short' (float64, CG two
    iterations short: the truncation condition)."""

    def __init__(self, c, kind):
        self.c, self.kind, self.m = c, kind, s_problem(c)
        self.dtype = np.dtype(np.float64 if kind in ("exact", "short") else np.float32)
        self.log = []

    def __call__(self, v):
        c, m, T = self.c, self.m, self.dtype.type
        assert v.dtype == self.dtype
        ts = U.b_ts(self.dtype)
        assert float(ts) == S_TAU * U.SIGMA_F
        b = m.b.astype(self.dtype)
        src = b if m.h is None else O.blur_adjoint(b, m.h.astype(self.dtype), m.offset)
        if self.kind == "launch":
            coef = T(S_TAU * s_lam(c) / CFG_GAMMA) if c.nc == "me" else T(T(S_TAU) * T(s_lam(c)))
            rhs = fma32(ts, src, fma32(coef, moreau_launch(v, c.nc, CFG_GAMMA, c.niter), v))
        else:
            rhs = (v + T(S_TAU) * T(s_lam(c)) * moreau(v, c.nc, CFG_GAMMA, c.niter)) + ts * src
        assert rhs.dtype == self.dtype
        self.log.append(rhs)
        if m.h is None:
            return rhs / (T(1) + ts)
        if self.kind == "exact":
            return U.exact_solve(rhs, m.h, m.offset, float(ts))
        return U.cg32(rhs, m.h, m.offset, ts, U.CG_ITERS - (2 if self.kind == "short" else 0))


def s_iteration(prox, x, y, xi, dtype):
    """One iteration of `O.ulpda` with gfirst=False, L21 and no z on [C][H][W] at once, in `dtype`: (x', y')."""
    T = np.dtype(dtype).type
    tau, mu = T(S_TAU), T(S_MU)
    x, y, xi = x.astype(dtype), y.astype(dtype), xi.astype(dtype)
    aty = -O.div2d(y[:, 0], y[:, 1])
    xn = prox(x - tau * aty) + np.sqrt(2 * tau) * xi
    xhat = xn + T(S_THETA) * (xn - x)
    yn = U.l21_proj(y + mu * np.stack(O.grad2d(xhat), axis=1), T(U.RADIUS))
    assert xn.dtype == np.dtype(dtype) and yn.dtype == np.dtype(dtype)
    return xn, yn


def s_iteration_launch(prox, x, y, xi):
    """The same as the kernels of lmc_ulpda.hip state it (tests/_ulpda_pixel.py: a_step_fma), float32."""
    T = np.float32
    tau, mu, radius = T(S_TAU), T(S_MU), T(U.RADIUS)
    yr, yc = y[:, 0], y[:, 1]
    aty = np.zeros_like(x)
    aty[:, :-1, :] -= yr[:, :-1, :]
    aty[:, 1:, :] += yr[:, :-1, :]
    aty[:, :, :-1] -= yc[:, :, :-1]
    aty[:, :, 1:] += yc[:, :, :-1]
    xn = fma32(np.sqrt(T(2) * tau), xi, prox(fma32(-tau, aty, x)))
    xhat = fma32(T(S_THETA), xn - x, xn)
    dr, dc = O.grad2d(xhat)
    a, b = fma32(mu, dr, yr), fma32(mu, dc, yc)
    sc = T(1) / np.maximum(T(1), np.sqrt(fma32(a, a, b * b)) / radius)
    yn = np.stack([a * sc, b * sc], axis=1)
    assert xn.dtype == T and yn.dtype == T
    return xn, yn


# x: `_ulpda_pixel.Ref` of the state; y: (Ref, Ref) of the dual or None; start_x, start_y; trunc: the truncation condition's left side (None: closed form);
# contrib: |tau lamda moreau| at the point the pre-step is taken
SStage = namedtuple("SStage", "start_x start_y x y trunc contrib")


def _ref(r64, r32, alt, floor):
    e32, bound = U.bound_with_floor(r64, r32, floor, alt32=alt)
    for a in (r64, r32, alt):
        a.setflags(write=False)
    return U.Ref(r64, r32, e32, bound, alt)


@functools.lru_cache(maxsize=None)
def s_reference(c):
    m = s_problem(c)
    stages = []
    if c.entry == "prox":
        ex, df, la_, sh = (SProx(c, k) for k in ("exact", "def", "launch", "short"))
        x64 = m.x0.astype(np.float64)
        star = ex(x64)
        x = _ref(star, df(m.x0), la_(m.x0), U.primal_floor(star))
        trunc = float(np.max(np.abs(sh(x64) - star)))
        contrib = S_TAU * s_lam(c) * np.abs(moreau(x64, c.nc, CFG_GAMMA, c.niter))
        return (SStage(m.x0, None, x, None, trunc, contrib),)
    sx, sy = m.x0, m.y0
    for it in range(2):
        ex, df, la_, sh = (SProx(c, k) for k in ("exact", "def", "launch", "short"))
        x64, y64 = s_iteration(ex, sx, sy, m.noise[it], np.float64)
        x32, y32 = s_iteration(df, sx, sy, m.noise[it], np.float32)
        xl, yl = s_iteration_launch(la_, sx, sy, m.noise[it])
        trunc = None
        if m.h is not None:
            xs, _ = s_iteration(sh, sx, sy, m.noise[it], np.float64)
            trunc = float(np.max(np.abs(xs - x64)))
        v64 = sx.astype(np.float64) + S_TAU * O.div2d(sy[:, 0].astype(np.float64), sy[:, 1].astype(np.float64))
        contrib = S_TAU * s_lam(c) * np.abs(moreau(v64, c.nc, CFG_GAMMA, c.niter))
        ry = tuple(_ref(np.ascontiguousarray(y64[:, k]), np.ascontiguousarray(y32[:, k]), np.ascontiguousarray(yl[:, k]), U.dual_floor(True)) for k in range(2))
        stages.append(SStage(sx, sy, _ref(x64, x32, xl, U.primal_floor(x64)), ry, trunc, contrib))
        sx, sy = f32(x64), f32(y64)
    return tuple(stages)


def s_check(c, it, got_x, got_y, st):
    """`_pixel.check` on the state and, where the stage has one, on both dual components: the list of verdicts."""
    out = [check(c, f"{it} x", got_x, st.x)]
    if st.y is not None:
        for k in range(2):
            out.append(check(c, f"{it} y{k}", np.asarray(got_y)[:, k], st.y[k]))
    return out


# ====================================================================== the value at the prominent weight
ECase = namedtuple("ECase", "shape nc tag")
E_CASES = [ECase((h, w), nc, f"{nc}-{h}x{w}") for nc in ("mc", "mca") for h in (1, 31, 33) for w in (3, 63, 65, 129)]
E_IDS = [c.tag for c in E_CASES]
E_FLOOR = 1e-6


def e_lam():
    return float(np.float32(1.0 / X.TAU))


@functools.lru_cache(maxsize=None)
def e_problem(shape):
    rng = np.random.default_rng(3000 + 1000 * shape[0] + shape[1])
    h, off = f32(X.BLURS["A"][0]), X.BLURS["A"][1]
    img = X.step_image(shape)
    y = f32(O.blur(img, h.astype(np.float64), off) + rng.normal(0, X.SIGMA, shape))
    x0 = f32(img[None] + rng.normal(0, 10, (N_CHAINS,) + shape))
    for a in (h, y, x0):
        a.setflags(write=False)
    return h, off, y, x0


def _huber(e, g):
    return np.where(e <= g, e * e / (2 * g), e - g / 2)


def e_value(c, dtype):
    """sigma / 2 |H x - b|^2 - lamda sum env_gamma(|.|)(grad x) per chain (algs.py:173-190): the residual and the envelope per pixel in `dtype`, the two
    sums in float64."""
    h, off, y, x0 = e_problem(c.shape)
    T = np.dtype(dtype).type
    x = x0.astype(dtype)
    r = O.blur(x, h.astype(dtype), off) - y.astype(dtype)
    dr, dc = O.grad2d(x)
    g = T(CFG_GAMMA)
    env = _huber(np.sqrt(dr * dr + dc * dc), g) if c.nc == "mc" else _huber(np.abs(dr), g) + _huber(np.abs(dc), g)
    assert r.dtype == np.dtype(dtype) and env.dtype == np.dtype(dtype)
    r, env = r.astype(np.float64), env.astype(np.float64)
    return 0.5 * (1 / X.SIGMA ** 2) * np.sum(r * r, axis=(-2, -1)) - e_lam() * np.sum(env, axis=(-2, -1))


@functools.lru_cache(maxsize=None)
def e_reference(c):
    """(float64 value per chain, tolerance per chain = max(3 |float32 replay - float64|, 1e-6 |float64|), the replay's own error)."""
    v64, v32 = e_value(c, np.float64), e_value(c, np.float32)
    e32 = np.abs(v32 - v64)
    return v64, np.maximum(FACTOR * e32, E_FLOOR * np.abs(v64)), e32


def rel(a, b):
    return X.rel(a, b)

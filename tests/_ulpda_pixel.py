"""Per-pixel parity of ULPDA and of its implicit solve against the float64 checker (oracle/lmc_oracle.py): the case lists, the references and the
bounds.  numpy only; tests/test_ulpda_pixel_reference.py (CPU) checks this harness on every case, tests/test_gpu_ulpda_pixel.py runs the kernels of
lmc_ulpda.hip, lmc_solve.hip, lmc_cheb_pair.hip and the solver's modes of myula_step_rows_kernel against it.  The conventions are those of
tests/_pixel.py, whose `bound_of`, `ulp32`, `region`, `check`, `step_image` and `BLURS` are used as they are:

* every input -- x0, y0, b, h, z, the noise, tau, mu, sigma -- is rounded to float32 ONCE; the library gets those numbers, the checker gets them cast
  back to float64;
* every case has a float64 reference `ref64` and a float32 replay `ref32` of the checker (`O.ulpda`, `O.L2.prox`, `O.cg_solve`, `O.Gradient`, `O.L21`,
  `O.L1` compute in the dtype of their input; the replays assert it);
* `e32 = max |ref32 - ref64|`, `bound = max(FACTOR e32, floor)` with FACTOR = 3 (`_pixel.FACTOR`: a margin over the reference, never fitted to a kernel);
  a result passes when `max |got - ref64| <= bound` over EVERY chain and pixel.  The primal state and both components of the dual are judged this way.

Floors.  Primal: `2 ulp32(max |ref64|)`, as in tests/_pixel.py.  Clipped (anisotropic) dual: `2 ulp32(radius)` -- the fma y + mu d and nothing after
it (min and max are exact), with the same allowance of four half-ulps as the primal floor.  Isotropic dual: `ulpda_dual_kernel` forms
`a = fma(mu, d, y)`, `n2 = fma(a, a, b b)`, `n = sqrt(n2)`, `q = n / radius`, `sc = 1 / max(1, q)`, `a sc`: SIX rounded operations on the way to a
number of magnitude <= radius (the fma, the squared norm -- its two roundings are halved by the square root and count as one -- the sqrt, the division by
the radius, the reciprocal, the product), each by at most half an ulp; with the same factor of two over the half-ulps as the primal floor that is
`DUAL_ISO_OPS ulp32(radius) = 6 ulp32(radius)`.

Part A (`A_CASES`): the kernels around the solve as finite computations.  Data terms whose implicit step is closed form (identity, mask, none), so one
iteration is ulpda_dual*, ulpda_rhs*, ulpda_pointwise_prox and ulpda_finish* with nothing iterative in between.  "restart": injected noise, two
iterations; `set_state` sets xhat = x, so the second starts from ref64 rounded to float32 for both x and y.  "philox": two iterations in one call on the
device's own field (ulpda_finish_philox_kernel where W % 4 == 0, launch_noise + ulpda_finish elsewhere), no restart; the reference runs on
`O.philox_normals`, which the device's normals match to 2e-5 (hardware log2 / sqrt / sin / cos; tests/test_gpu_mymala_matrix.py derives the term), so the
primal bound gains `2e-5 sqrt(2 tau)` per iteration and the dual bound `mu 2 (1 + theta)` times that (a difference of two xhat, each 1 + theta states).
The identity term is `O.L2`; the mask and the absent term have no closed form in the checker (`O.L2` with a Diagonal runs CG), `_Pointwise` states them.
Part A has a second float32 replay, `a_step_fma`: the checker's step with every a * b + c contracted to one fma and the sums in the kernels' order (a
different, valid association); e32 is the larger of the two replays' errors (`a_reference` says what showed the need).

Part B (`B_CASES`): (I + ts H^T H) u = v + ts H^T b per pixel on every path of `cg_solve_fused`, through `L2.prox` and through one sampler iteration
without noise (gfirst=False, zero dual: the state is u).  `ref64` is u*, the float64 solve run until |r| <= 1e-12 |rhs|.  The device stops by a
tolerance, so truncation is taken out before rounding is judged: the Chebyshev cases run at tolerance CHEB_TOL (below), the replay (`cheb_replay`) is
the recurrence of lmc_solve.hip, u_{k+1} = a u_k - t sigma_f H^T H u_k + b rhs + s u_{k-1} with lmax = 1 + ts (sum |h|)^2 1.0001 and coefficients
computed in float64 and rounded to float32, it forms the adaptive count K by the formula of cheb_count_kernel from its own |r_0| and |rhs|, `e32` is
the larger of the float32 replay's errors at K and K + 2, and the float64 replay at K - 2 must be within e32 / 10 of u* (`trunc`; asserted on the CPU), so that a device
count one even step lower is no error.  The CG cases run 50 fixed iterations (tolerance 0 / implicit_tol=-1): `ref32` is `O.cg_solve` in float32 for 50
iterations, and float64 CG at 48 must be within e32 / 10 of u*.  "warm": three sampler iterations with injected noise, warm=True, no restart; state and
dual compared after each; the float32 replay carries its own warm start and its own count (the maximum over the chains, as the device's atomicMax), once
with every solve at K and once at K + 2, and the truncation condition holds for each of the three solves.  Second quantity: the residual
rhs - A (x_got - sqrt(2 tau) xi) per pixel in float64 against max(3 r32, 2 ulp32(max |rhs|)), r32 the float32 replay's own residual: it localises a
seam fault to the rows that caused it.

CHEB_TOL = 1e-9, not the 1e-8 first meant for these cases.  The Chebyshev error polynomial equi-oscillates, so the iterate two steps short of the count
for a tolerance t is off by about 2 c^(K-2) max |u*| ~ t / c^2 (c = 0.18 .. 0.24 here): at 1e-8 the float64 replay at K - 2 sat 1.2e-5 to 2.9e-5 from u*
against e32 / 10 of 7.6e-6 to 1.9e-5, and 28 of the 59 cases missed the truncation condition, whatever the image.  The condition and its margin stand; the
cases changed: at 1e-9 (a-priori count 18 for the box at ts = 1.74, cold count 16, cap 50) the same distance is 1e-6 to 6e-6 (see also SIGMA_F below).

Paths (`expected_path`), from the dispatch of `cg_solve_fused` / `chebyshev_solve` / `launch_step`:
  1 "cheb"       tolerance > 0, `centred_blur_taps` accepts the taps, a-priori count <= 50: single launches of myula_step_rows_kernel, general taps;
  2 "cheb-uni"   the same with a uniform box: lmc_step_rows_uni.hip from the second launch on (the first carries the DOT statistics: general form);
  3 "cheb-pairs" LMC_CHEB_PAIR=2, sampler only (`lmc_l2_prox` passes no second array), uniform 5-tap box, W % 4 == 0, W <= 512: lmc_cheb_pair.hip;
                 `kernel_name` contains "pairs";
  4 "cg-rows"    tolerance 0, centred separable taps: CG with the operator on myula_step_rows_kernel<DOT>, p.Ap fused;
  5 "cg-general" tolerance 0, taps `centred_blur_taps` refuses (rank 2, or an offset outside the centred window): the split or tile kernel + cg_dot.
Seams: bands of 16 rows (two chains: 4096 / C bands wanted, at least 16 rows each) and column strips of 496 past 512 columns for the row kernel; bands
of LMC_PAIR_BAND=32 rows with a recomputed halo of 8 for the pairs; 64 columns (and 64 rows) for the split and tile kernels.

The L2_ncvx_tv pre-steps of ULPDA (ulpda_ncvx_rhs_kernel, ulpda_me_rhs_kernel) are in tests/_ncvx_pixel.py, which restates the term in the dtype of its input and
uses this file's solves, truncation condition and floors.  Out of scope: truncated solves at the default tolerance 1e-6 (the answer depends on the solver by design; rel-L2 tests); the
chunking past 65535 chains (tests/test_gpu_many_images.py)."""
import functools
import math
from collections import namedtuple

import numpy as np

from oracle import lmc_oracle as O
import _pixel as X
from _pixel import BLURS, FACTOR, bound_of, check, f32, region, step_image, ulp32      # noqa: F401  (re-exported to the two test files)

N_CHAINS = 2
assert N_CHAINS == X.N_CHAINS
SEED, CHAIN_OFFSET = 17, 5
SIGMA = 0.75                                 # the noise of the observations
# sigma_f = 1.75 (1 / 0.756^2) and the Part B step 127 / 128 have short mantissas, so that ts = tau sigma_f = 1.736328125 is exact in float32: the
# float64 solve and the device then solve the SAME system.  The step is also one at which the float32 rounding of the recurrence's coefficients is
# benign: they become stationary after a few iterations, and the limit of the recurrence with the ROUNDED (a, t, b, s) is u* (1 + d), where
# d = b (1 + ts m) / ((1 - a - s) + t m) - 1 and m = (sum |h|)^2 on the smooth part of the image, m = 0 on its noise.  At 127 / 128 |d| <= 1.7e-9 for the
# taps that sum to one and <= 1.4e-8 for blur B (sum 0.795); at 124 / 128 it is -4.6e-8 and -6.5e-8, at 126 / 128 -4.2e-8 and -5.6e-8 for B, at 1
# 4.3e-8: 1.3e-5 on a state of 230, which is e32 / 10 by itself at any tolerance, so the truncation condition could not tell truncation from it
# (measured: the float64 replay with the device's coefficients levels off 1.2e-5 to 1.3e-5 from u* from iteration 14 on at 0.95 x 1.7777778 and at
# 124 / 128 x 1.75, 1.1e-5 for B at 126 / 128).  That offset is under one ulp of the state and inside every e32; no kernel is involved in it.
SIGMA_F = 1.75
RADIUS = float(np.float32(0.3))              # sigma of L21 / L1: the dual ball
DUAL_ISO_OPS = 6
PHILOX_DXI = 2e-5                            # device normals vs O.philox_normals (tests/test_gpu_mymala_matrix.py)
# Part A steps: tau small enough that a dropped dual term (tau radius / (1 + ts) = 0.044) stays under the 0.05 of the row criterion
A_TAU, A_MU = float(np.float32(0.2)), float(np.float32(0.4))
B_TAU, B_MU, B_THETA = 127.0 / 128.0, 1.0, 1.0
assert float(np.float32(B_TAU) * np.float32(SIGMA_F)) == B_TAU * SIGMA_F
CHEB_TOL, CG_ITERS, CAP = 1e-9, 50, 50

# what `_pixel.check` reads of a stage; alt32: the second float32 replay where a case has one (e32 is then the larger of the two errors)
Ref = namedtuple("Ref", "ref64 ref32 e32 bound alt32", defaults=(None,))


def bound_with_floor(ref64, ref32, floor, extra=0.0, alt32=None):
    e32 = max(bound_of(ref64, r)[0] for r in (ref32, alt32) if r is not None)
    return e32, max(FACTOR * e32, floor) + extra


def primal_floor(ref64):
    return 2.0 * ulp32(np.max(np.abs(ref64)))


def dual_floor(iso):
    return (DUAL_ISO_OPS if iso else 2) * ulp32(RADIUS)


def _ro(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)


# ====================================================================== Part A
# family ("ulpda"), shape, gfirst, prior ('l21' | 'l1'), theta, z (bool), data ('identity' | 'mask' | 'none'), mode ('restart' | 'philox'), tag;
# K, seam_rows, seam_cols: read by `_pixel.region` (these kernels have no seams)
ACase = namedtuple("ACase", "family shape gfirst prior theta z data mode iters K seam_rows seam_cols tag")

A_SHAPES4 = [(9, 12), (17, 64), (1, 8), (8, 4)]          # W % 4 == 0: the 4-pixel kernels
A_SHAPES1 = [(17, 67), (5, 7), (1, 5), (3, 1)]           # the scalar kernels
A_FULL = [(17, 64), (17, 67)]                            # every combination of the axes; the other shapes take six each, every value of every axis
A_PHILOX = [(16, 64), (17, 64), (3, 12), (16, 67), (17, 67), (3, 7)]      # heights 16, 17 (a last quad of one row) and 3
A_PHILOX += [(5, 65), (6, 66), (7, 69)]       # the draw is four columns per thread: H % 4 = 1, 2, 3 with W % 4 = 1, 2, 1 (W % 4 = 3: above)


def case_id(c):
    return f"{c.family}-{c.shape[0]}x{c.shape[1]}-{c.tag}"


def _build_a():
    combos = [(g, p, t, z, d) for g in (True, False) for p in ("l21", "l1") for t in (1.0, 0.5) for z in (True, False) for d in ("identity", "mask", "none")]
    out = []

    def add(shape, g, p, t, z, d, mode):
        tag = f"{mode}-{'gfirst' if g else 'glast'}-{p}-th{t:g}-{'z' if z else 'noz'}-{d}"
        out.append(ACase("ulpda", shape, g, p, t, z, d, mode, 2, 0, (), (), tag))
    for n, shape in enumerate(A_SHAPES4 + A_SHAPES1):
        # 48 combinations; a stride of 7 is coprime to every axis length, so six of them in a row still take every value of every axis
        picked = combos if shape in A_FULL else [combos[(7 * (6 * n + k)) % 48] for k in range(6)]
        for cb in picked:
            add(shape, *cb, "restart")
    for shape in A_PHILOX:
        for g in (True, False):
            for p in ("l21", "l1"):
                add(shape, g, p, 1.0 if p == "l21" else 0.5, g, "identity" if p == "l21" else "mask", "philox")
    return out


A_CASES = _build_a()
A_IDS = [case_id(c) for c in A_CASES]
assert len(set(A_IDS)) == len(A_IDS)

AProblem = namedtuple("AProblem", "x0 y0 b mask z noise low")


@functools.lru_cache(maxsize=None)
def a_problem(c):
    """x0: a block of 190 on zero with noise of 10 grey levels on one half of the pixels (drawn per pixel) and 0.01 on the other, so that the dual update
    meets gradients far outside the ball and well inside it; the injected noise is scaled the same way, so that xhat after the step has both too."""
    H, W = c.shape
    rng = np.random.default_rng(7000 + 100 * H + W)
    img = step_image(c.shape) - np.linspace(0, 30, W)[None, :]
    low = rng.uniform(size=c.shape) < 0.5
    scale = np.where(low, 0.01, 10.0)
    x0 = f32(img[None] + rng.normal(0, 1, (N_CHAINS,) + c.shape) * scale)
    y0 = f32(rng.normal(0, 0.5 * RADIUS, (N_CHAINS, 2) + c.shape))
    mask = f32(rng.uniform(size=c.shape) < 0.6) if c.data == "mask" else None
    b = None if c.data == "none" else f32((img + rng.normal(0, 0.01, c.shape)) * (mask if mask is not None else 1.0))
    z = f32(rng.normal(0, 0.1, c.shape)) if c.z else None
    if c.mode == "philox":
        noise = np.stack([O.philox_normals(SEED, i, np.arange(CHAIN_OFFSET, CHAIN_OFFSET + N_CHAINS), H, W) for i in range(c.iters)])
        assert noise.dtype == np.float32
    else:
        noise = f32(rng.standard_normal((c.iters, N_CHAINS) + c.shape) * np.where(low, 1e-3, 1.0))
    _ro(x0, y0, b, mask, z, noise)
    return AProblem(x0, y0, b, mask, z, noise, low)


class _Pointwise:
    """The closed-form implicit steps the checker's L2 does not state: mask u = (v + ts m b) / (1 + ts m^2), none u = v; in the dtype of v."""

    def __init__(self, b, mask, sigma):
        self.b, self.mask, self.sigma = b, mask, sigma

    def prox(self, v, tau):
        if self.b is None:
            return v.copy()
        ts = tau * self.sigma
        return (v + ts * self.mask * self.b) / (1.0 + ts * self.mask * self.mask)


def _a_terms(c, m, dtype):
    cast = lambda a: None if a is None else a.astype(dtype).ravel()
    if c.data == "identity":
        pf = O.L2(b=cast(m.b), sigma=SIGMA_F)
    else:
        pf = _Pointwise(cast(m.b), cast(m.mask), SIGMA_F)
    pg = O.L21(ndim=2, sigma=RADIUS) if c.prior == "l21" else O.L1(sigma=RADIUS)
    return pf, pg, cast(m.z)


def a_run(c, dtype, x, y, noise):
    """`O.ulpda` for `len(noise)` iterations from (x, y) with xhat = x, chain by chain, in `dtype`: (states, duals) per iteration, [n][C][H][W] and
    [n][C][2][H][W]."""
    m, (H, W) = a_problem(c), c.shape
    pf, pg, z = _a_terms(c, m, dtype)
    G = O.Gradient(c.shape, dtype=dtype)
    xs, ys = [], []
    for ch in range(N_CHAINS):
        a, d = O.ulpda(pf, pg, G, x[ch].astype(dtype).ravel(), A_TAU, A_MU, y0=y[ch].astype(dtype).ravel(), z=z, theta=c.theta, niter=len(noise),
                       gfirst=c.gfirst, returny=True, noise=noise[:, ch].astype(dtype).reshape(len(noise), -1))
        assert a.dtype == dtype and d.dtype == dtype, (case_id(c), a.dtype, d.dtype)
        xs.append(a.reshape(-1, H, W))
        ys.append(d.reshape(-1, 2, H, W))
    return np.stack(xs, axis=1), np.stack(ys, axis=1)


def fma32(a, b, c):
    """fma in float32: the product of two float32 numbers is exact in float64, the sum is rounded there and once more to float32."""
    return (np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(c, dtype=np.float64)).astype(np.float32)


def a_step_fma(c, x, xhat, y, xi):
    """One iteration in the form the kernels of lmc_ulpda.hip state it, in float32 on [C][H][W]: (x, xhat, y).  The same operations as `O.ulpda` with every
    a * b + c contracted to one fma and the sums in the kernels' order: a = fma(mu, d, y), n2 = fma(a, a, b b), sc = 1 / max(1, sqrt(n2) / radius);
    aty = ((0 - yr[p]) + yr[p - W] - yc[p]) + yc[p - 1] (+ z), v = fma(-tau, aty, x); u = fma(ts, b, v) / (1 + ts), or
    fma(ts m, b, v) / fma(ts m, m, 1); x' = fma(sqrt(2 tau), xi, u), xhat = fma(theta, x' - x, x').  See `a_reference` for why it exists."""
    T = np.float32
    m = a_problem(c)
    tau, mu, theta, radius = T(A_TAU), T(A_MU), T(c.theta), T(RADIUS)
    ts = T(tau * T(SIGMA_F))
    x, xhat, y, xi = (np.asarray(v, dtype=T) for v in (x, xhat, y, xi))

    def dual(y, xhat):
        dr, dc = O.grad2d(xhat)
        a, b = fma32(mu, dr, y[:, 0]), fma32(mu, dc, y[:, 1])
        if c.prior == "l21":
            sc = T(1) / np.maximum(T(1), np.sqrt(fma32(a, a, b * b)) / radius)
            a, b = a * sc, b * sc
        else:
            a, b = np.clip(a, -radius, radius), np.clip(b, -radius, radius)
        return np.stack([a, b], axis=1)
    if c.gfirst:
        y = dual(y, xhat)
    yr, yc = y[:, 0], y[:, 1]
    aty = np.zeros_like(x)
    aty[:, :-1, :] -= yr[:, :-1, :]
    aty[:, 1:, :] += yr[:, :-1, :]
    aty[:, :, :-1] -= yc[:, :, :-1]
    aty[:, :, 1:] += yc[:, :, :-1]
    if m.z is not None:
        aty += m.z
    v = fma32(-tau, aty, x)
    if c.data == "identity":
        u = fma32(ts, m.b, v) / (T(1) + ts)
    elif c.data == "mask":
        tm = ts * m.mask
        u = fma32(tm, m.b, v) / fma32(tm, m.mask, T(1))
    else:
        u = v
    xn = fma32(np.sqrt(T(2) * tau), xi, u)
    xhat = fma32(theta, xn - x, xn)
    if not c.gfirst:
        y = dual(y, xhat)
    assert xn.dtype == T and xhat.dtype == T and y.dtype == T and u.dtype == T
    return xn, xhat, y


# start_x, start_y: what both sides start this iteration from (None: they carry their own); x: Ref; y: (Ref, Ref) of the two dual components;
# compare: whether the device is compared after this iteration
AStage = namedtuple("AStage", "start_x start_y x y compare")


def _a_stage(c, sx, sy, x64, x32, y64, y32, it, compare, xf, yf):
    px = dy = 0.0
    if c.mode == "philox":
        px = (it + 1) * PHILOX_DXI * math.sqrt(2 * A_TAU)
        dy = A_MU * 2 * (1 + c.theta) * px
    rx = Ref(x64, x32, *bound_with_floor(x64, x32, primal_floor(x64), px, xf), xf)
    ry = tuple(Ref(y64[:, k], y32[:, k], *bound_with_floor(y64[:, k], y32[:, k], dual_floor(c.prior == "l21"), dy, yf[:, k]), yf[:, k]) for k in range(2))
    for r in (rx,) + ry:
        assert r.ref64.dtype == np.float64 and r.ref32.dtype == np.float32 and r.alt32.dtype == np.float32
        _ro(r.ref64, r.ref32, r.alt32)
    return AStage(sx, sy, rx, ry, compare)


@functools.lru_cache(maxsize=None)
def a_reference(c):
    """The stages of case `c`.  Two float32 replays, e32 the larger of their errors: `O.ulpda` in float32, and `a_step_fma`, the same step with the
    kernels' fma contractions.  The second was added after the first run on an MI355X: with the dual formed last (gfirst=False) it is
    y + mu grad(xhat) inside the ball, so it inherits the rounding of xhat = x' + theta (x' - x) -- one ulp of a state of 200 is 1.5e-5, times
    mu (1 + theta) -- and whether a pixel of x' rounds up or down differs between x - tau aty + ... formed with separate roundings (numpy) and with
    fma (the kernels; both valid).  Over the 3 to 35 pixels of the smallest shapes the separate-rounding replay alone happened to sit 3.3e-7 to 7e-6
    from ref64 where the kernels -- bit-equal to the fma form there -- sat 1.7e-6 to 2.6e-5: (8, 4), (5, 7) and (3, 1) missed 3 e32 by factors of
    1.2 to 1.7, every larger shape passed."""
    m = a_problem(c)
    stages = []
    if c.mode == "restart":
        sx, sy = m.x0, m.y0
        for it in range(c.iters):
            x64, y64 = a_run(c, np.float64, sx, sy, m.noise[it:it + 1])
            x32, y32 = a_run(c, np.float32, sx, sy, m.noise[it:it + 1])
            xf, _, yf = a_step_fma(c, sx, sx, sy, m.noise[it])
            stages.append(_a_stage(c, sx, sy, x64[0], x32[0], y64[0], y32[0], it, True, xf, yf))
            sx, sy = f32(x64[0]), f32(y64[0])
    else:
        x64, y64 = a_run(c, np.float64, m.x0, m.y0, m.noise)
        x32, y32 = a_run(c, np.float32, m.x0, m.y0, m.noise)
        xf, xh, yf = m.x0, m.x0, m.y0
        for it in range(c.iters):
            xf, xh, yf = a_step_fma(c, xf, xh, yf, m.noise[it])
            stages.append(_a_stage(c, m.x0 if it == 0 else None, m.y0 if it == 0 else None, x64[it], x32[it], y64[it], y32[it], it, it == c.iters - 1,
                                   xf, yf))
    return tuple(stages)


def check_stage(c, it, got_x, got_y, st):
    """`_pixel.check` on the state and on both dual components of one stage: the list of verdicts."""
    out = [check(c, f"{it} x", got_x, st.x)]
    for k in range(2):
        out.append(check(c, f"{it} y{k}", np.asarray(got_y)[:, k], st.y[k]))
    return out


# ====================================================================== Part B
B_BLURS = dict(BLURS)
B_BLURS["A0"] = (BLURS["A"][0], (0, 0))      # the 5 x 5 box with its origin in the corner: outside the centred window of 5 or 7 taps

# family: the path; entry ('prox' | 'sampler'); blur: a B_BLURS key; data: the BLURS key `_pixel.reach_of` reads the taps of; K: the reach of a seam
# fault beyond the taps (8: the recomputed halo of the pairs); mode ('cold' | 'warm')
BCase = namedtuple("BCase", "family shape entry blur data solver pairs mode iters K seam_rows seam_cols tag")


def _mult(step, n):
    return tuple(range(step, n, step))


def _rows_seams(shape):
    return _mult(16, shape[0]), (_mult(496, shape[1]) if shape[1] > 512 else ())


def _build_b():
    out = []

    def add(family, shape, entry, blur, solver, seams, pairs=False, mode="cold", K=0):
        tag = f"{entry}-{blur}" + ("-warm" if mode == "warm" else "")
        out.append(BCase(family, shape, entry, blur, blur[0], solver, pairs, mode, 3 if mode == "warm" else 1, K, tuple(seams[0]), tuple(seams[1]), tag))
    for entry in ("prox", "sampler"):
        for b in "BDE":
            for s in [(40, 64), (40, 264), (37, 67), (20, 520), (20, 515)]:
                add("cheb", s, entry, b, "cheb", _rows_seams(s))
        for s in [(40, 64), (20, 520)]:
            add("cheb-uni", s, entry, "A", "cheb", _rows_seams(s))
        for b in "AD":
            for s in [(40, 64), (37, 67), (20, 520)]:
                add("cg-rows", s, entry, b, "cg", _rows_seams(s))
        add("cg-general", (33, 70), entry, "G", "cg", (_mult(64, 33), _mult(64, 70)))
        for s in [(24, 40), (20, 200)]:
            add("cg-general", s, entry, "A0", "cg", (_mult(64, s[0]), _mult(64, s[1])))
    for s in [(72, 128), (72, 264), (37, 36), (100, 512)]:
        add("cheb-pairs", s, "sampler", "A", "cheb", (_mult(32, s[0]), ()), pairs=True, K=8)
    add("cheb", (40, 64), "sampler", "B", "cheb", _rows_seams((40, 64)), mode="warm")
    add("cheb-uni", (40, 64), "sampler", "A", "cheb", _rows_seams((40, 64)), mode="warm")
    add("cheb-pairs", (72, 128), "sampler", "A", "cheb", (_mult(32, 72), ()), pairs=True, mode="warm", K=8)
    return out


B_CASES = _build_b()
B_IDS = [case_id(c) for c in B_CASES]
assert len(set(B_IDS)) == len(B_IDS)


def centred_taps(h, offset):
    """`centred_blur_taps` of lmc_step_rows.hip: 5 or 7 if the taps are rank 1 and fit a window of that many taps centred on the pixel, else 0."""
    h = np.asarray(h, dtype=np.float64)
    kh, kw = h.shape
    if kh > 7 or kw > 7 or np.linalg.matrix_rank(h, tol=1e-6 * np.abs(h).max()) != 1:
        return 0
    for KT in (5, 7):
        hw = (KT - 1) // 2
        if all(0 <= hw - o and n + hw - o <= KT for n, o in ((kh, offset[0]), (kw, offset[1]))):
            return KT
    return 0


def is_uniform_box(h):
    h = np.asarray(h, dtype=np.float64)
    return h.shape == (5, 5) and np.allclose(h, h[0, 0], rtol=1e-6, atol=0)


def expected_path(c):
    """The path the dispatch takes for case `c` (module docstring)."""
    h, off = B_BLURS[c.blur]
    h32 = f32(h)
    kt = centred_taps(h32, off)
    if c.solver == "cheb":      # tolerance CHEB_TOL
        assert kt and cheb_plan(b_ts(np.float32), h32) is not None
        H, W = c.shape
        if c.pairs and c.entry == "sampler" and is_uniform_box(h32) and kt == 5 and W % 4 == 0 and 4 <= W <= 512:
            return "cheb-pairs"
        return "cheb-uni" if is_uniform_box(h32) else "cheb"
    return "cg-rows" if kt else "cg-general"


BProblem = namedtuple("BProblem", "h offset b x0 noise")


@functools.lru_cache(maxsize=None)
def _b_problem(shape, blur, iters):
    rng = np.random.default_rng(9000 + 1000 * shape[0] + shape[1])
    h, off = B_BLURS[blur]
    h = f32(h)
    img = step_image(shape)
    b = f32(O.blur(img, h.astype(np.float64), off) + rng.normal(0, SIGMA, shape))
    x0 = f32(img[None] + rng.normal(0, 10, (N_CHAINS,) + shape))
    noise = f32(rng.standard_normal((iters, N_CHAINS) + shape))
    _ro(h, b, x0, noise)
    return BProblem(h, off, b, x0, noise)


def b_problem(c):
    return _b_problem(c.shape, c.blur, c.iters)


def b_ts(dtype):
    T = np.dtype(dtype).type
    return T(T(B_TAU) * T(SIGMA_F))       # the device: float ts = tau * sigma_f


def hth(u, h, off):
    return O.blur_adjoint(O.blur(u, h, off), h, off)


def apply_A(u, h, off, ts):
    """(I + ts H^T H) u in the dtype of u."""
    return u + u.dtype.type(ts) * hth(u, h.astype(u.dtype), off)


def exact_solve(rhs, h, off, ts):
    """u* of (I + ts H^T H) u = rhs in float64, chain by chain: `O.cg_solve` until |r| <= 1e-13 |rhs| (300 iterations at most), the true residual
    asserted below 1e-12 |rhs|."""
    rhs = np.asarray(rhs, dtype=np.float64)
    h = np.asarray(h, dtype=np.float64)
    out = np.empty_like(rhs)
    for ch in range(rhs.shape[0]):
        nb = float(np.linalg.norm(rhs[ch]))
        out[ch] = O.cg_solve(lambda v: apply_A(v, h, off, ts), rhs[ch], np.zeros_like(rhs[ch]), 300, tol=(1e-13 * nb) ** 2)
        assert np.linalg.norm(rhs[ch] - apply_A(out[ch], h, off, ts)) <= 1e-12 * nb
    return out


ChebPlan = namedtuple("ChebPlan", "kmax adaptive inv_log_inv_c tol ts theta delta")


def cheb_plan(ts, h32, tol=CHEB_TOL, cap=CAP):
    """The host side of `chebyshev_solve`: None where it leaves the problem to CG."""
    ts = float(ts)
    tol = float(np.float32(tol))
    hsum = float(np.abs(np.asarray(h32, dtype=np.float64)).sum())
    lmax = 1.0 + ts * hsum * hsum * 1.0001
    theta, delta = 0.5 * (lmax + 1.0), 0.5 * (lmax - 1.0)
    sk = math.sqrt(lmax)
    cc = (sk - 1.0) / (sk + 1.0)
    k_need = int(math.ceil(math.log(2.0 / tol) / math.log(1.0 / cc))) + 1
    if k_need > cap:
        return None
    adaptive = k_need > 2 and ((k_need + 1) & ~1) <= cap
    return ChebPlan(((k_need + 1) & ~1) if adaptive else k_need, adaptive, 1.0 / math.log(1.0 / cc), tol, ts, theta, delta)


def cheb_coefs(plan, n):
    """(a, t sigma_f, b, s) of the first n iterations, computed in float64 and rounded to float32."""
    out = []
    rho, sigma1 = plan.delta / plan.theta, plan.theta / plan.delta
    for k in range(n):
        if k == 0:
            alpha, beta = 1.0 / plan.theta, 0.0
        else:
            rho_new = 1.0 / (2.0 * sigma1 - rho)
            alpha, beta = 2.0 * rho_new / plan.delta, rho_new * rho
            rho = rho_new
        out.append(tuple(float(np.float32(v)) for v in (1.0 - alpha + beta, alpha * plan.ts, alpha, -beta)))
    return out


def cheb_replay(dtype, u0, rhs, h, off, plan, extra=2):
    """The recurrence in `dtype` from u0 for kmax + extra iterations: (iterates [u_0, u_1, ...], K); K the adaptive count of cheb_count_kernel from this
    replay's own first step, the maximum over the chains."""
    dtype = np.dtype(dtype)
    T = dtype.type
    u0, rhs, h = u0.astype(dtype), rhs.astype(dtype), h.astype(dtype)
    its, prev, u = [u0], u0, u0
    K = plan.kmax
    for k, (a, tg, b, s) in enumerate(cheb_coefs(plan, plan.kmax + extra)):
        new = T(a) * u - T(tg) * hth(u, h, off) + T(b) * rhs + T(s) * prev
        assert new.dtype == dtype
        prev, u = u, new
        its.append(new)
        if k == 0 and plan.adaptive:
            need = 2
            for ch in range(u0.shape[0]):
                r2 = float(np.sum((new[ch].astype(np.float64) - u0[ch]) ** 2)) / (b * b)
                b2 = float(np.sum(rhs[ch].astype(np.float64) ** 2))
                kk = 1
                if not (b2 > 0.0) or r2 != r2:
                    kk = plan.kmax
                elif r2 > plan.tol * plan.tol * b2:
                    kk = int(math.ceil(math.log(2.0 * math.sqrt(r2 / b2) / plan.tol) * plan.inv_log_inv_c))
                kk = (kk + 1) & ~1
                need = max(need, min(kk, plan.kmax))
            K = need
    return its, K


def cg32(rhs, h, off, ts, niter):
    """`O.cg_solve` from zero for `niter` iterations in the dtype of rhs, chain by chain (the device's CG scalars are per chain)."""
    hh = h.astype(rhs.dtype)
    out = np.stack([O.cg_solve(lambda v: apply_A(v, hh, off, ts), rhs[ch], np.zeros_like(rhs[ch]), niter) for ch in range(rhs.shape[0])])
    assert out.dtype == rhs.dtype
    return out


class Solver:
    """prox_{tau f} of Part B in `dtype`, batched over the chains: rhs = v + ts H^T b, then the exact solve ('exact'), the Chebyshev replay at its own
    count + `extra` ('cheb'), or `niter` CG iterations ('cg').  Keeps the warm start and, per solve, what the CPU file asserts."""

    def __init__(self, c, dtype, kind, extra=0, niter=CG_ITERS, warm=False):
        m = b_problem(c)
        self.c, self.m, self.dtype, self.kind, self.extra, self.niter, self.warm = c, m, np.dtype(dtype), kind, extra, niter, warm
        self.h = m.h.astype(dtype)
        self.ts = b_ts(dtype)
        self.htb = O.blur_adjoint(m.b.astype(dtype), self.h, m.offset)
        self.plan = cheb_plan(b_ts(np.float32), m.h) if kind == "cheb" else None
        self.u0 = None
        self.log = []       # per solve: dict(rhs, K, trunc)

    def prox(self, v, tau=None):
        m = self.m
        rhs = v + self.ts * self.htb
        assert rhs.dtype == self.dtype
        rec = {"rhs": rhs}
        if self.kind == "exact":
            u = exact_solve(rhs, self.h, m.offset, self.ts)
        elif self.kind == "cg":
            u = cg32(rhs, self.h, m.offset, self.ts, self.niter)
        else:
            u0 = self.u0 if (self.warm and self.u0 is not None) else np.zeros_like(rhs)
            its, K = cheb_replay(self.dtype, u0, rhs, self.h, m.offset, self.plan)
            u = its[K + self.extra]
            rec["K"] = K
            if self.dtype == np.float32 and self.extra == 0:
                # the truncation of a count one even step lower, in float64 on the numbers this solve was handed
                r64 = rhs.astype(np.float64)
                its64, K64 = cheb_replay(np.float64, u0, r64, self.h, m.offset, self.plan)
                star = exact_solve(r64, self.h, m.offset, float(self.ts))
                rec["K64"] = K64
                rec["trunc"] = float(np.max(np.abs(its64[max(K - 2, 0)] - star)))
        if self.warm:
            self.u0 = u
        self.log.append(rec)
        return u


def l21_proj(y, radius):
    """`O.L21.proxdual` on [C][2][H][W]."""
    nrm = np.sqrt(np.sum(y * y, axis=1, keepdims=True))
    return y / np.maximum(1.0, nrm / radius)


def ulpda_batched(prox, x0, noise, dtype, tau=B_TAU, mu=B_MU, theta=B_THETA):
    """`O.ulpda` with gfirst=False, L21, zero initial dual and no z, on [C][H][W] at once (the device's Chebyshev count is one number for the batch):
    the same operations in the same order; tests/test_ulpda_pixel_reference.py holds it bit-equal to `O.ulpda` chain by chain."""
    dtype = np.dtype(dtype)
    T = dtype.type
    tau, mu = T(tau), T(mu)
    x = x0.astype(dtype)
    y = np.zeros((x.shape[0], 2) + x.shape[1:], dtype=dtype)
    xs, ys = [], []
    for k in range(len(noise)):
        xold = x.copy()
        ATy = -O.div2d(y[:, 0], y[:, 1])
        x = prox(x - tau * ATy, tau) + np.sqrt(2 * tau) * noise[k].astype(dtype)
        xhat = x + theta * (x - xold)
        y = l21_proj(y + mu * np.stack(O.grad2d(xhat), axis=1), RADIUS)
        assert x.dtype == dtype and y.dtype == dtype
        xs.append(x)
        ys.append(y)
    return xs, ys


# x: Ref of the state; y: (Ref, Ref) or None; res: Ref of the residual (ref64 = 0); rhs: the float64 right-hand side; xi: sqrt(2 tau) * noise or None;
# K: the replay's count; K64: the float64 replay's; trunc: the truncation condition's left side (<= x.e32 / 10)
BStage = namedtuple("BStage", "x y res rhs xi K K64 trunc")


def residual(c, got, st):
    """rhs - A (got - sqrt(2 tau) xi) per pixel, in float64."""
    m = b_problem(c)
    u = np.asarray(got, dtype=np.float64) - (0.0 if st.xi is None else st.xi)
    return st.rhs - apply_A(u, m.h.astype(np.float64), m.offset, float(b_ts(np.float32)))


def _res_ref(c, rhs, xi, candidates):
    m = b_problem(c)
    h64, ts = m.h.astype(np.float64), float(b_ts(np.float32))
    r32 = 0.0
    for u in candidates:
        uu = u.astype(np.float64) - (0.0 if xi is None else xi)
        r32 = max(r32, float(np.max(np.abs(rhs - apply_A(uu, h64, m.offset, ts)))))
    zero = np.zeros_like(rhs)
    _ro(zero)
    return Ref(zero, None, r32, max(FACTOR * r32, 2.0 * ulp32(np.max(np.abs(rhs)))))


def _x_ref(star, candidates):
    e32 = max(float(np.max(np.abs(u.astype(np.float64) - star))) for u in candidates)
    for u in candidates:
        assert u.dtype == np.float32
    assert star.dtype == np.float64
    _ro(star, *candidates)
    return Ref(star, candidates[0], e32, max(FACTOR * e32, primal_floor(star)))


@functools.lru_cache(maxsize=None)
def _b_reference(c):
    """(`entry` left out of the key: both entry points solve the same system)"""
    m = b_problem(c)
    if c.mode == "cold":
        exact = Solver(c, np.float64, "exact")
        star = exact.prox(m.x0.astype(np.float64))
        rhs = exact.log[0]["rhs"]
        if c.solver == "cheb":
            s0, s2 = Solver(c, np.float32, "cheb"), Solver(c, np.float32, "cheb", extra=2)
            cands = [s0.prox(m.x0), s2.prox(m.x0)]
            K, K64, trunc = s0.log[0]["K"], s0.log[0]["K64"], s0.log[0]["trunc"]
            # the truncation on the float64 right-hand side itself
            its64, _ = cheb_replay(np.float64, np.zeros_like(rhs), rhs, m.h, m.offset, s0.plan)
            trunc = max(trunc, float(np.max(np.abs(its64[K - 2] - star))))
        else:
            cands = [Solver(c, np.float32, "cg").prox(m.x0)]
            K = K64 = CG_ITERS
            trunc = float(np.max(np.abs(Solver(c, np.float64, "cg", niter=CG_ITERS - 2).prox(m.x0.astype(np.float64)) - star)))
        return (BStage(_x_ref(star, cands), None, _res_ref(c, rhs, None, cands), rhs, None, K, K64, trunc),)
    exact = Solver(c, np.float64, "exact")
    x64, y64 = ulpda_batched(exact.prox, m.x0, m.noise, np.float64)
    runs = []
    for extra in (0, 2):
        s = Solver(c, np.float32, "cheb", extra=extra, warm=True)
        runs.append((s,) + ulpda_batched(s.prox, m.x0, m.noise, np.float32))
    stages = []
    for it in range(c.iters):
        xi = math.sqrt(2 * B_TAU) * m.noise[it].astype(np.float64)
        cx = [r[1][it] for r in runs]
        rx = _x_ref(x64[it], cx)
        ry = []
        for k in range(2):
            cy = [np.ascontiguousarray(r[2][it][:, k]) for r in runs]
            y_ = np.ascontiguousarray(y64[it][:, k])
            e32 = max(float(np.max(np.abs(v.astype(np.float64) - y_))) for v in cy)
            _ro(y_, *cy)
            ry.append(Ref(y_, cy[0], e32, max(FACTOR * e32, dual_floor(True))))
        rhs = exact.log[it]["rhs"]
        lg = runs[0][0].log[it]
        stages.append(BStage(rx, tuple(ry), _res_ref(c, rhs, xi, cx), rhs, xi, lg["K"], lg["K64"], lg["trunc"]))
    return tuple(stages)


def b_reference(c):
    return _b_reference(c._replace(entry="", tag="", family=""))


def check_b(c, it, got_x, got_y, st):
    """The verdicts of one Part B stage: the state, the residual, and the dual where the stage has one."""
    out = [check(c, f"{it} x (K {st.K})", got_x, st.x), check(c, f"{it} residual", residual(c, got_x, st), st.res)]
    if st.y is not None:
        for k in range(2):
            out.append(check(c, f"{it} y{k}", np.asarray(got_y)[:, k], st.y[k]))
    return out


def worst(verdicts):
    return max(verdicts, key=lambda v: v.ratio)

"""GPU: the Daubechies wavelet-l1 prior (LMC_PRIOR_WAVELET_L1) against the float64 checker of tests/_wavelet.py -- the transform and its transpose, the
prox and the value, the samplers that consume it, SAPG, and the refusals of the C ABI.

Bound for every array compared, per pixel over every image (tests/_pixel.bound_of, the project's rule):

    max |got - ref64| <= max(3 e32, 2 ulp32(max |ref64|))

e32: the larger of the deviations from float64 of the checker's two float32 replays (matrix form, tap-loop form) on that case -- measured on the
reference, never on a kernel.  Every case prints err / bound.  Values: rtol 1e-5 against float64 (the tolerance of tests/test_gpu_haar.py) and equal
bit for bit on a repeat."""
import ctypes as C
import functools

import numpy as np
import pytest

import _mala_ref as MR
import _pixel as X
import _poisson_ref as P
import _wavelet as Wv
import _wl2_ref as WL
from oracle import lmc_oracle as O

pytestmark = pytest.mark.gpu

LMC_E_INVALID, LMC_E_UNSUPPORTED = -1, -2
NAMES = {1: "db1", 2: "db2", 3: "db3", 4: "db4"}
SHAPES = [((8, 8), 1), ((16, 24), 1), ((16, 24), 2), ((32, 40), 3), ((48, 136), 3), ((64, 520), 3), ((256, 256), 5)]
CASES = [(p, L, s) for s, L in SHAPES for p in (1, 2, 3, 4) if Wv.legal(s, p, L)]       # skipped only where the preconditions forbid
IDS = [f"db{p}-L{L}-{s[0]}x{s[1]}" for p, L, s in CASES]
THRESHOLDS = (0.0, 5.0, 1e9)
SIGMA = 0.4


@pytest.fixture(scope="module")
def la():
    import torch
    assert torch.cuda.is_available()
    import lmc_atomi_amd as la
    return la


def test_the_case_list_leaves_out_only_what_the_preconditions_forbid():
    left_out = [(p, L, s) for s, L in SHAPES for p in (1, 2, 3, 4) if (p, L, s) not in CASES]
    assert left_out == [(3, 2, (16, 24)), (4, 2, (16, 24)), (3, 3, (32, 40))] or all(not Wv.legal(s, p, L) for p, L, s in left_out)
    assert (4, 1, (8, 8)) in CASES and (4, 3, (32, 40)) in CASES and (4, 5, (256, 256)) in CASES


@functools.lru_cache(maxsize=None)
def images(shape):
    """Three images of different content, rounded to float32 once: a block on a ramp with noise, white noise, a smooth wave."""
    rng = np.random.default_rng(100 * shape[0] + shape[1])
    i, j = np.meshgrid(np.arange(shape[0]), np.arange(shape[1]), indexing="ij")
    x = np.stack([X.step_image(shape) + rng.normal(0, 10, shape), rng.normal(0, 30, shape), 100 * np.sin(0.31 * i) * np.cos(0.17 * j) + 0.5 * j])
    x = X.f32(x)
    x.setflags(write=False)
    return x


def within(what, got, ref64, ref32):
    e32, bound = X.bound_of(ref64, ref32)
    err = float(np.max(np.abs(np.asarray(got, dtype=np.float64) - ref64)))
    print(f"{what}: err {err:.3e} bound {bound:.3e} err/bound {err / bound:.3f} (e32 {e32:.3e})")
    assert np.isfinite(err) and err <= bound, (what, err, bound, e32)
    return err / bound


def tensor(a):
    import torch
    return torch.as_tensor(np.array(a, dtype=np.float32), device="cuda")      # a copy: the cached inputs are read-only


# ------------------------------------------------------------------ 1. W and W^T apart, adjointness
@pytest.mark.parametrize("p,L,shape", CASES, ids=IDS)
def test_transform_and_transpose_per_pixel_and_adjointness(la, p, L, shape):
    x = images(shape)
    rng = np.random.default_rng(7)
    c = X.f32(rng.normal(0, 20, x.shape))
    op = la.Wavelet2D(shape, NAMES[p], L)
    wx = op.matvec(tensor(x)).cpu().numpy().reshape(x.shape)
    r64, r32 = Wv.replays(lambda a: Wv.dwt2(a, p, L), lambda a: Wv.dwt2(a, p, L), lambda a: Wv.dwt2_taps(a, p, L), x)
    within(f"W x db{p} L{L} {shape}", wx, r64, r32)
    e_fwd = X.bound_of(r64, r32)[0]
    wtc = op.H.matvec(tensor(c)).cpu().numpy().reshape(x.shape)
    r64, r32 = Wv.replays(lambda a: Wv.idwt2(a, p, L), lambda a: Wv.idwt2(a, p, L), lambda a: Wv.idwt2_taps(a, p, L), c)
    within(f"W^T c db{p} L{L} {shape}", wtc, r64, r32)
    e_inv = X.bound_of(r64, r32)[0]
    # <W x, c> = <x, W^T c> from the device outputs in float64: each side carries the rounding of one transform, at most 3 e32 per coefficient
    n = float(np.sqrt(x[0].size))
    for i in range(x.shape[0]):
        a = float(np.sum(wx[i].astype(np.float64) * c[i]))
        b = float(np.sum(x[i].astype(np.float64) * wtc[i]))
        tol = 3.0 * n * (e_fwd * np.linalg.norm(c[i].astype(np.float64)) + e_inv * np.linalg.norm(x[i].astype(np.float64)))
        print(f"adjointness db{p} L{L} {shape} image {i}: |<Wx,c> - <x,W^Tc>| = {abs(a - b):.3e}, tolerance {tol:.3e}, scale {abs(a):.3e}")
        assert abs(a - b) <= tol
    with pytest.raises(ValueError):
        op.matvec(tensor(np.zeros((shape[0] + 1, shape[1]))))


# ------------------------------------------------------------------ 2. prox and value
@pytest.mark.parametrize("p,L,shape", CASES, ids=IDS)
def test_prox_and_value(la, p, L, shape):
    x = images(shape)
    w = la.WaveletL1(shape, sigma=SIGMA, levels=L, wavelet=NAMES[p])
    from lmc_atomi_amd import _capi
    assert w.prior_descriptor()["prior_kind"] == _capi.PRIOR_WAVELET_L1
    xt = tensor(x)
    for t in THRESHOLDS:
        got = w.prox(xt.reshape(3, -1), t).cpu().numpy().reshape(x.shape)
        thr = np.float32(SIGMA * float(t))          # the threshold the library forms in float32
        r64, r32 = Wv.replays(lambda a: Wv.prox(a, p, L, float(thr)), lambda a: Wv.prox(a, p, L, thr), lambda a: Wv.prox_taps(a, p, L, thr), x)
        within(f"prox db{p} L{L} {shape} t={t:g}", got, r64, r32)
        if t == 1e9:        # every detail vanishes: the projection onto the approximation space
            cg = Wv.dwt2(got.astype(np.float64), p, L)
            scale = float(np.max(np.abs(x)))
            assert np.abs(cg[..., Wv.detail_mask(shape, L)]).max() <= 1e-5 * scale
    vals = w(xt.reshape(3, -1)).cpu().numpy()
    again = w(xt.reshape(3, -1)).cpu().numpy()
    ref = Wv.value(x.astype(np.float64), p, L, SIGMA)
    rel = np.max(np.abs(vals - ref) / np.abs(ref))
    print(f"value db{p} L{L} {shape}: rel {rel:.2e}")
    assert vals.shape == (3,) and rel <= 1e-5, (vals, ref)
    assert np.array_equal(vals, again), "two evaluations of g differ: the sum is not formed in a fixed order"
    stat = la.prior_statistic(w, xt).cpu().numpy()
    assert np.allclose(stat * SIGMA, ref, rtol=1e-5) and np.array_equal(stat, la.prior_statistic(w, xt).cpu().numpy())


# ------------------------------------------------------------------ 3. p = 1, L = 3 through the new kernels against the block-Haar kernel
@pytest.mark.parametrize("shape", [(16, 24), (48, 136), (64, 520)])
def test_db1_three_levels_against_the_block_haar_kernel(la, shape):
    x = images(shape)
    xt = tensor(x)
    new, old = la.WaveletL1(shape, sigma=SIGMA, levels=3, wavelet="db1"), la.WaveletL1(shape, sigma=SIGMA)
    assert new.prior_descriptor()["prior_kind"] == 7 and old.prior_descriptor()["prior_kind"] == 5
    for t in (0.0, 5.0):
        thr = np.float32(SIGMA * t)
        a = new.prox(xt.reshape(3, -1), t).cpu().numpy().reshape(x.shape)
        b = old.prox(xt.reshape(3, -1), t).cpu().numpy().reshape(x.shape)
        r64, r32 = Wv.replays(lambda v: O.haar_l1_prox(v, float(thr)), lambda v: Wv.prox(v, 1, 3, thr), lambda v: Wv.prox_taps(v, 1, 3, thr), x)
        within(f"db1 L3 {shape} t={t:g} (wavelet kernels)", a, r64, r32)
        _, bound = X.bound_of(r64, r32)
        d = float(np.max(np.abs(a.astype(np.float64) - b)))
        print(f"db1 L3 {shape} t={t:g}: |wavelet kernels - block-Haar kernel| = {d:.3e}, bound {bound:.3e}")
        assert d <= bound
    va, vb = np.asarray(new(xt.reshape(3, -1)).cpu()), np.asarray(old(xt.reshape(3, -1)).cpu())
    assert np.allclose(va, vb, rtol=1e-5)


# ------------------------------------------------------------------ 4. more images than a grid dimension holds
def test_65537_images(la):
    import torch
    n, shape = 65537, (8, 8)
    x = torch.as_tensor(np.random.default_rng(2).normal(0, 30, (n,) + shape).astype(np.float32), device="cuda")
    w = la.WaveletL1(shape, sigma=1.0, levels=1, wavelet="db2")
    out = w.prox(x.reshape(n, -1), 5.0).reshape(x.shape)
    vals = w(x.reshape(n, -1))
    for i in (0, 65535, 65536):
        one = w.prox(x[i].reshape(1, -1).clone(), 5.0).reshape(shape)
        assert torch.equal(out[i], one), i
        assert float(vals[i]) == float(w(x[i].reshape(1, -1).clone())), i
    assert torch.isfinite(out).all()


# ------------------------------------------------------------------ 5. MYULA steps with injected noise
N_CHAINS, N_ITERS = 2, 3
STEPS = [("blur", (48, 136), 2, 2), ("mask", (48, 136), 2, 2), ("identity", (48, 136), 2, 2), ("pois-identity", (48, 136), 2, 2), ("wl2-blur", (48, 136), 2, 2),
         ("psf11", (48, 136), 2, 2), ("blur", (64, 520), 4, 3)]


def _gauss(k, s):
    t = np.exp(-0.5 * ((np.arange(k) - k // 2) / s) ** 2)
    return np.outer(t, t) / np.sum(np.outer(t, t))


class StepProblem:
    """The inputs of one case, float32 numbers made once; `terms(dtype, form)` -> the checker's data term and prior in that dtype."""

    def __init__(self, data, shape, p, L):
        self.data, self.shape, self.p, self.L = data, shape, p, L
        rng = np.random.default_rng(11 * shape[1] + len(data))
        self.h = self.off = self.mask = self.aux = None
        if data in ("blur", "wl2-blur"):
            self.h, self.off = X.f32(np.ones((5, 5)) / 25.0), (2, 2)
        if data == "psf11":
            self.h, self.off = X.f32(_gauss(11, 2.0)), (5, 5)
        if data == "mask":
            self.mask = X.f32(rng.uniform(size=shape) < 0.6)
        op = self.op(np.float64)
        if data == "pois-identity":
            self.aux = X.f32(P.ramp_background(shape))
            _, _, y, _, x0 = P.recipe(shape, n_chains=N_CHAINS, seed=shape[1], op=op, beta=self.aux.astype(np.float64))
            self.y, self.x0 = X.f32(y), X.f32(x0)
            self.gamma, self.sigma_f, self.weight = 0.02, 1.0, 5.0
            self.tau = 0.5 / (P.PoissonRef(op, self.y, self.aux, 1.0).grad_lipschitz() + 1.0 / self.gamma)
        elif data == "wl2-blur":
            _, _, y, w, x0 = WL.recipe(shape, n_chains=N_CHAINS, seed=shape[1], op=op)
            self.aux, self.y, self.x0 = X.f32(w), X.f32(y), X.f32(x0)
            self.gamma, self.sigma_f, self.weight = WL.GAMMA, WL.SIGMA_F, 0.3
            self.tau = WL.step_size(WL.WL2Ref(op, self.y, self.aux, self.sigma_f))
        else:
            img = X.step_image(shape)
            self.y = X.f32(op.fwd(img) + rng.normal(0, X.SIGMA, shape) * (self.mask if self.mask is not None else 1.0))
            self.x0 = X.f32(img[None] + rng.normal(0, 10, (N_CHAINS,) + shape))
            self.gamma, self.sigma_f, self.tau, self.weight = X.GAMMA, 1 / X.SIGMA ** 2, X.TAU, 2.0
        self.noise = X.f32(rng.standard_normal((N_ITERS, N_CHAINS) + shape))

    def op(self, dtype):
        if self.h is not None:
            return P.Op("blur", self.h.astype(dtype), self.off)
        return P.Op("mask", self.mask.astype(dtype)) if self.mask is not None else P.Op("identity")

    def terms(self, dtype, taps=False):
        op = self.op(dtype)
        if self.data == "pois-identity":
            pf = P.PoissonRef(op, self.y, self.aux, self.sigma_f, dtype=dtype)
        elif self.data == "wl2-blur":
            pf = WL.WL2Ref(op, self.y, self.aux, self.sigma_f, dtype=dtype)
        else:
            pf = X._Data(op, self.y, self.sigma_f, dtype)
        fn = Wv.prox_taps if taps else Wv.prox
        # the threshold as the library forms it: float32(epsg gamma) * float32(weight), in float32
        thr = np.float32(np.float32(self.gamma) * np.float32(self.weight))
        pg = X._Prox(lambda x, t: fn(x, self.p, self.L, thr if x.dtype == np.float32 else float(thr)))
        return pf, pg

    def device_terms(self, la, prior=None):
        s = self.shape
        if self.data == "psf11":
            pf = la.L2(Op=la.PSF(s, self.h, offset=self.off), b=self.y, sigma=self.sigma_f)
        elif self.data == "blur":
            pf = la.L2(Op=la.Convolve2D(s, self.h, offset=self.off), b=self.y, sigma=self.sigma_f)
        elif self.data == "mask":
            pf = la.L2(Op=la.Diagonal(self.mask, dims=s), b=self.y, sigma=self.sigma_f, dims=s)
        elif self.data == "identity":
            pf = la.L2(b=self.y, sigma=self.sigma_f, dims=s)
        elif self.data == "pois-identity":
            pf = la.Poisson(la.Identity(s[0] * s[1]), self.y, self.aux, sigma=self.sigma_f, dims=s)
        else:
            pf = la.L2(Op=la.Convolve2D(s, self.h, offset=self.off), b=self.y, sigma=self.sigma_f, weights=self.aux)
        pg = prior or la.WaveletL1(s, sigma=self.weight, levels=self.L, wavelet=NAMES[self.p])
        return pf, pg


@functools.lru_cache(maxsize=None)
def step_problem(case):
    return StepProblem(*case)


@functools.lru_cache(maxsize=None)
def step_reference(case):
    """Restart mode (tests/_pixel.py): every iteration starts from the float32 rounding of the float64 reference of the one before."""
    m = step_problem(case)
    (f64, g64), (fa, ga), (fb, gb) = m.terms(np.float64), m.terms(np.float32), m.terms(np.float32, taps=True)
    out, start = [], m.x0
    for it in range(N_ITERS):
        r64 = P.myula_step(f64, g64, start.astype(np.float64), m.tau, m.gamma, m.noise[it].astype(np.float64))
        ra = P.myula_step(fa, ga, start, m.tau, m.gamma, m.noise[it], dtype=np.float32)
        rb = P.myula_step(fb, gb, start, m.tau, m.gamma, m.noise[it], dtype=np.float32)
        worse = ra if np.max(np.abs(ra - r64)) >= np.max(np.abs(rb - r64)) else rb
        out.append((start, r64, worse))
        start = X.f32(r64)
    return out


@pytest.mark.parametrize("case", STEPS, ids=[f"{d}-db{p}-L{L}-{s[0]}x{s[1]}" for d, s, p, L in STEPS])
def test_myula_steps_per_pixel(la, case):
    m = step_problem(case)
    pf, pg = m.device_terms(la)
    smp = la.MYULASampler(pf, pg, m.shape, n_chains=N_CHAINS, tau=m.tau, gamma=m.gamma, noise="injected")
    try:
        for it, (start, r64, r32) in enumerate(step_reference(case)):
            smp.set_state(start)
            smp.step(1, noise=m.noise[it:it + 1])
            within(f"MYULA {case} it {it} ({smp.kernel_name})", smp.get_state().cpu().numpy(), r64, r32)
        name = smp.kernel_name
        _, g = smp.energies()
        gref = Wv.value(smp.get_state().cpu().numpy().astype(np.float64), m.p, m.L, m.weight)
        assert np.allclose(g.cpu().numpy(), gref, rtol=1e-5)
    finally:
        smp.close()
    # the kernel the same problem gets with prior NONE and a ready-made prox: an l1 prior with array-valued epsg takes that route
    pf2, pg2 = m.device_terms(la, prior=la.L1(sigma=m.weight))
    other = la.MYULASampler(pf2, pg2, m.shape, n_chains=N_CHAINS, tau=m.tau, gamma=m.gamma, noise="injected", epsg=np.ones(N_CHAINS))
    try:
        other.set_state(m.x0)
        other.step(1, noise=m.noise[:1])
        print(f"kernel_name {case}: {name}; prior NONE + ready-made prox: {other.kernel_name}")
        assert name == other.kernel_name
    finally:
        other.close()


# ------------------------------------------------------------------ 6. SK-ROCK, MYMALA
def test_skrock_matches_the_restated_recursion(la):
    s, eta, nit = 3, 0.05, 2
    case = STEPS[0]
    m = step_problem(case)
    pf, pg = m.device_terms(la)
    f64, g64 = m.terms(np.float64)
    Z = np.random.default_rng(4).standard_normal((nit,) + m.x0.shape)
    smp = la.SKROCKSampler(pf, pg, m.shape, n_stages=s, eta=eta, n_chains=N_CHAINS, tau=m.tau, gamma=m.gamma, noise="injected")
    try:
        smp.set_state(m.x0)
        x = m.x0.astype(np.float64)
        for it in range(nit):
            x = P.skrock_iteration(f64, g64, x, Z[it], m.tau, m.gamma, s, eta)
            smp.step(1, noise=Z[it:it + 1])
            e = X.rel(smp.get_state().cpu().numpy(), x)
            print(f"SK-ROCK iteration {it + 1}: rel {e:.3e} ({smp.kernel_name})")
            assert e <= 1e-5 * (it + 1), (it, e)
    finally:
        smp.close()


def test_mymala_log_ratios_and_decisions(la):
    """Four chains, three iterations, identity data term on a small image of O(1) values, so that the potentials (~ 540) leave the log ratios their
    digits; the case (seed 45, tau 0.25) was picked on the float64 restatement alone: every |log alpha| >= 1.3, every decision clear by >= 1.1."""
    shape, p, L, C_, nit, seed, off = (16, 24), 2, 2, 4, 3, 7, 3
    rng = np.random.default_rng(45)
    img = np.zeros(shape)
    img[4:10, 6:15] = 4.0
    y = X.f32(img + rng.normal(0, 1.0, shape))
    x0 = X.f32(img[None] + rng.normal(0, 1.0, (C_,) + shape))
    noise = X.f32(rng.standard_normal((nit, C_) + shape))
    tau, sigma_f, gamma, wgt = 0.25, 1.0, 0.5, 0.5
    pf64 = X._Data(P.Op("identity"), y.astype(np.float64), sigma_f, np.float64)
    thr = float(np.float32(np.float32(gamma) * np.float32(wgt)))
    pg64 = X._Prox(lambda v, t: Wv.prox(v, p, L, thr))
    mean = lambda v: P.myula_step(pf64, pg64, np.asarray(v, dtype=np.float64), tau, gamma, 0.0)
    U = lambda v: 0.5 * sigma_f * ((np.asarray(v) - y) ** 2).sum(axis=(-2, -1)) + Wv.value(v, p, L, wgt)
    un = np.stack([O.philox_uniforms(seed, k, off + np.arange(C_)) for k in range(nit)])
    _, acc_ref, la_ref, _, _ = MR.mymala(mean, U, x0, tau, noise, un)
    assert np.abs(la_ref).min() >= 1.0 and np.abs(np.log(un) - la_ref).min() >= 1.0      # of the case, not of the code
    smp = la.MYMALASampler(la.L2(b=y, sigma=sigma_f, dims=shape), la.WaveletL1(shape, sigma=wgt, levels=L, wavelet="db2"), shape, n_chains=C_, tau=tau,
                           gamma=gamma, noise="injected", seed=seed, chain_offset=off)
    try:
        smp.set_state(x0)
        las, accs = [], []
        for k in range(nit):
            smp.step(1, noise=noise[k:k + 1])
            acc, la_d = smp.acceptance()
            las.append(la_d.cpu().numpy())
            accs.append(acc.cpu().numpy().astype(np.int64))
        las = np.array(las)
        dec_d = np.diff(np.array([np.zeros_like(accs[0])] + accs), axis=0)
        dec_r = (np.log(un) <= la_ref).astype(np.int64)
        rel = np.max(np.abs(las - la_ref) / np.abs(la_ref))
        print(f"MYMALA ({smp.kernel_name}): max relative error of log alpha {rel:.2e}; accepted {accs[-1].tolist()} (reference {acc_ref.tolist()})")
        assert rel <= 1e-4, (las, la_ref)
        assert np.array_equal(dec_d, dec_r) and np.array_equal(accs[-1], acc_ref)
    finally:
        smp.close()


# ------------------------------------------------------------------ 7. SAPG
def test_sapg_trace_is_the_host_replay_of_the_device_statistics(la):
    case = STEPS[0]
    m = step_problem(case)
    pf, pg = m.device_terms(la)
    d, k = la.sapg_dimension(pg)
    assert (d, k) == (48 * 136 - 12 * 34, 1.0)
    n_updates, bounds = 20, (1e-3, 1e2)
    smp = la.MYULASampler(pf, pg, m.shape, n_chains=N_CHAINS, tau=m.tau, gamma=m.gamma, seed=5)
    try:
        smp.set_state(m.x0)
        res = smp.estimate_prior_weight(n_updates, bounds, theta0=m.weight, step_scale=10.0, step_exponent=0.8)
        # the statistic of the final state against the checker
        stat = la.prior_statistic(pg, smp.get_state()).cpu().numpy()
        ref = Wv.value(smp.get_state().cpu().numpy().astype(np.float64), m.p, m.L, 1.0)
        assert np.allclose(stat, ref, rtol=1e-5), (stat, ref)
        assert abs(smp.prior_weight - res.theta) <= 1e-6 * res.theta
    finally:
        smp.close()
    theta, trace = m.weight, [m.weight]
    for n in range(n_updates):
        theta = la.sapg_update(theta, res.stat_trace[n], n, d, k, theta_bounds=bounds, step_scale=10.0, step_exponent=0.8)
        trace.append(theta)
    err = np.max(np.abs(res.theta_trace - np.array(trace)) / np.array(trace))
    print(f"SAPG: theta trace against the host replay of lmc_sapg_update: max relative difference {err:.2e}; trace {res.theta_trace}")
    assert res.theta_trace.shape == (n_updates + 1,) and res.stat_trace.shape == (n_updates,)
    # the replay restarts every update from the device's own theta_n in float64: exp and log of the two sides within a few ulp
    step = [la.sapg_update(res.theta_trace[n], res.stat_trace[n], n, d, k, theta_bounds=bounds, step_scale=10.0, step_exponent=0.8) for n in range(n_updates)]
    assert np.max(np.abs(res.theta_trace[1:] - np.array(step)) / np.array(step)) <= 1e-13
    assert err <= 1e-11
    assert np.all((res.theta_trace >= bounds[0]) & (res.theta_trace <= bounds[1])) and np.all(np.isfinite(res.stat_trace)) and np.all(res.stat_trace > 0)


# ------------------------------------------------------------------ 8. refusals of the C ABI
def last_error():
    from lmc_atomi_amd import _dev
    return _dev.lib().lmc_last_error().decode()


def myula_config(la, shape, data, prior, **fields):
    from lmc_atomi_amd import _capi
    from lmc_atomi_amd.proximal import _Problem
    prob = _Problem(shape, data, prior)
    for k, v in fields.items():
        setattr(prob.c, k, v)
    cfg = _capi.lmc_myula_config()
    cfg.struct_size = C.sizeof(_capi.lmc_myula_config)
    cfg.problem = prob.c
    cfg.n_chains = 2
    cfg.tau, cfg.gamma, cfg.epsg = 1e-3, X.GAMMA, 1.0
    cfg.noise_mode = _capi.NOISE_PHILOX
    cfg.thin = 1
    return prob, cfg


def test_c_abi_refusals(la):
    import torch
    from lmc_atomi_amd import _capi, _dev
    lib = _dev.lib()
    shape = (16, 24)
    y = np.zeros(shape, dtype=np.float32)
    data = la.L2(b=y, sigma=1.0, dims=shape).descriptor()
    prior = la.WaveletL1(shape, sigma=0.5, levels=2, wavelet="db2").prior_descriptor()
    x = torch.zeros((2,) + shape, dtype=torch.float32, device="cuda")
    out = torch.empty_like(x)
    scale = torch.ones(2, dtype=torch.float32, device="cuda")
    stream = _dev.stream_ptr(x.device)
    creates = (lambda cfg, h: lib.lmc_myula_create(C.byref(cfg), C.byref(h)), lambda cfg, h: lib.lmc_mymala_create(C.byref(cfg), C.byref(h)),
               lambda cfg, h: lib.lmc_skrock_create(C.byref(cfg), 3, 0.05, C.byref(h)))

    def refused(fields, want):
        prob, cfg = myula_config(la, shape, data, prior, **fields)
        for create in creates:
            hnd = C.c_void_p()
            rc = create(cfg, hnd)
            msg = last_error()
            if rc == 0:
                lib.lmc_sampler_destroy(hnd)
            assert rc == want and msg and not hnd.value, (fields, rc, msg)
        rc = lib.lmc_fused_eval(C.byref(prob.c), _dev.ptr(x), _dev.ptr(out), 2, 1.0, 0.1, 0.5, 0.1, stream)
        assert rc == want and last_error(), (fields, rc, last_error())

    prob, _ = myula_config(la, shape, data, prior)
    assert (prob.c.prior_kind, prob.c.tv_niter, prob.c.eprox_kind, prob.c.prior_sigma) == (7, 2, 2, 0.5)      # levels and p ride in tv_niter and eprox_kind
    refused(dict(box_enable=1, box_lo=0.0, box_hi=1.0), LMC_E_UNSUPPORTED)
    refused(dict(prox_scale=_dev.ptr(scale), prox_scale_chain_stride=1, prox_scale_pixel_stride=0), LMC_E_UNSUPPORTED)
    # bad p, bad levels, 24 % 16 != 0, db4 at three levels (16 >> 2 = 4 < 8), sides that are no multiples of 4
    for bad in (dict(eprox_kind=0), dict(eprox_kind=5), dict(tv_niter=0), dict(tv_niter=9), dict(tv_niter=4), dict(eprox_kind=4, tv_niter=3), dict(H=10), dict(W=22)):
        refused(bad, LMC_E_INVALID)
    # ULPDA
    prob, _ = myula_config(la, shape, data, prior)
    u = _capi.lmc_ulpda_config()
    u.struct_size = C.sizeof(_capi.lmc_ulpda_config)
    u.problem = prob.c
    u.n_chains, u.tau, u.mu, u.theta, u.cg_niter, u.thin = 2, 0.1, 0.1, 1.0, 5, 1
    hnd = C.c_void_p()
    rc = lib.lmc_ulpda_create(C.byref(u), C.byref(hnd))
    assert rc == LMC_E_UNSUPPORTED and last_error() and not hnd.value, (rc, last_error())
    # the stateless entry points
    for args in ((0, 2), (5, 2), (2, 0), (2, 9), (2, 4), (4, 3)):
        assert lib.lmc_wavelet_apply(_dev.ptr(x), _dev.ptr(out), 2, 16, 24, args[0], args[1], 0, stream) == LMC_E_INVALID, args
        assert lib.lmc_wavelet_l1_prox(_dev.ptr(x), _dev.ptr(out), 2, 16, 24, args[0], args[1], C.c_float(1.0), stream) == LMC_E_INVALID, args
    assert lib.lmc_wavelet_apply(_dev.ptr(x), _dev.ptr(x), 2, 16, 24, 2, 2, 0, stream) == LMC_E_INVALID           # in place
    assert lib.lmc_wavelet_l1_prox(_dev.ptr(x), _dev.ptr(out), 2, 16, 24, 2, 2, C.c_float(-1.0), stream) == LMC_E_INVALID
    assert lib.lmc_wavelet_l1_prox(_dev.ptr(x), _dev.ptr(out), 0, 16, 24, 2, 2, C.c_float(1.0), stream) == LMC_E_INVALID
    stat = torch.zeros(2, dtype=torch.float64, device="cuda")
    prob_b, _ = myula_config(la, shape, data, prior, tv_niter=4)
    assert lib.lmc_prior_statistic(C.byref(prob_b.c), _dev.ptr(x), 2, _dev.ptr(stat), stream) == LMC_E_INVALID
    # what is not refused: the problem as it stands, iterations_per_launch (ignored), a forced variant
    for fields in (dict(), dict(iterations_per_launch=2), dict(step_variant=1)):
        prob_ok, cfg_ok = myula_config(la, shape, data, prior, **fields)
        hnd = C.c_void_p()
        assert lib.lmc_myula_create(C.byref(cfg_ok), C.byref(hnd)) == 0, last_error()
        assert lib.lmc_sampler_step(hnd, 2, None, stream) == 0, last_error()
        assert lib.lmc_sampler_set_prior_sigma(hnd, C.c_float(0.7)) == 0, last_error()
        lib.lmc_sampler_destroy(hnd)
    torch.cuda.synchronize()

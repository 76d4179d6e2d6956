"""GPU parity of SK-ROCK (lmc_skrock_create / SKROCKSampler / StabilisedLangevin) against a float64 restatement of its definition
(include/lmc_atomi.h):

    K_0 = X,   K_1 = X + mu_1 delta drift(X + nu_1 q Z) + kappa_1 q Z,   K_j = mu_j delta drift(K_{j-1}) + nu_j K_{j-1} + kappa_j K_{j-2},   q = sqrt(2 delta)

-- the textbook form of stage 1, not the two-launch form the library runs.  `v + t drift(v)` is the checker's MYULA step with step t and no
noise: `O.myula_step(v, ..., tau=t, xi=0)` where that function has the model, the same formula over the checker's prox objects for the two it does
not have (anisotropic TV, the MC-TV term; as tests/test_gpu_tv_aniso.py does).  The coefficients come from numpy.polynomial.chebyshev, not from the
library.

Tolerances are the suite's (tests/_many.py, tests/test_gpu_parity.py): one step rel-L2 < 1e-5, a trajectory < 5e-5.  An fp32 restatement of the
scheme in numpy differs from float64 by <= 3.4e-7 (closed forms) and <= 2.7e-6 (three iterations at s = 10, states bounded by ~200)."""
import ctypes as C

import numpy as np
import pytest
from numpy.polynomial import chebyshev as cheb

from oracle import lmc_oracle as O

pytestmark = pytest.mark.gpu

STEP_TOL, TRAJ_TOL = 1e-5, 5e-5
LMC_E_INVALID, LMC_E_UNSUPPORTED, LMC_E_STATE = -1, -2, -5
SIGMA, TAU_REG, ETA = 0.75, 0.3, 0.05
GAMMA = SIGMA ** 2


def rel(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


@pytest.fixture(scope="module")
def la():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import lmc_atomi_amd as la
    return la


# ------------------------------------------------------------------ the reference
def T(j, x):
    return cheb.chebval(x, [0.0] * j + [1.0])


def dT(j, x):
    return cheb.chebval(x, cheb.chebder([0.0] * j + [1.0]))


def coefficients(s, eta=ETA):
    w0 = 1.0 + eta / s ** 2
    w1 = T(s, w0) / dT(s, w0)
    mu = np.array([w1 / w0] + [2 * w1 * T(j - 1, w0) / T(j, w0) for j in range(2, s + 1)])
    nu = np.array([s * w1 / 2] + [2 * w0 * T(j - 1, w0) / T(j, w0) for j in range(2, s + 1)])
    kappa = np.array([s * w1 / w0] + [-T(j - 2, w0) / T(j, w0) for j in range(2, s + 1)])
    return w0, w1, mu, nu, kappa


def step_factor(s, eta=ETA):
    return (s - 0.5) ** 2 * (2 - 4 * eta / 3) - 1.5


def skrock_iteration(advance, x, Z, delta, s, eta=ETA):
    """One iteration of the definition in float64.  advance(v, t) = v + t drift(v); Z = None: no noise."""
    _, _, mu, nu, kappa = coefficients(s, eta)
    q = np.sqrt(2 * delta)
    if Z is None:
        k1 = advance(x, mu[0] * delta)
    else:
        y = x + nu[0] * q * Z
        k1 = x + (advance(y, mu[0] * delta) - y) + kappa[0] * q * Z
    k2 = x
    for j in range(2, s + 1):
        k1, k2 = (advance(k1, mu[j - 1] * delta) - k1) + nu[j - 1] * k1 + kappa[j - 1] * k2, k1
    return k1


class AnisoTV:
    """Checker-side anisotropic TV prior: the checker's FGP loop with the dual clipped per component (as in tests/test_gpu_tv_aniso.py)."""

    def __init__(self, dims, sigma, niter):
        self.dims, self.sigma, self.niter = dims, sigma, niter

    def prox(self, x, t):
        x = np.asarray(x).reshape(self.dims)
        gam = self.sigma * t
        c = 0.125 / gam
        betas = np.asarray(O.fgp_betas(self.niter, "unlocbox"), dtype=np.float64)
        rr, ss, p, q = (np.zeros_like(x) for _ in range(4))
        for k in range(self.niter):
            dr, dc = O.grad2d(x - gam * O.div2d(rr, ss))
            pn, qn = np.clip(rr - c * dr, -1.0, 1.0), np.clip(ss - c * dc, -1.0, 1.0)
            rr, ss = pn + betas[k] * (pn - p), qn + betas[k] * (qn - q)
            p, q = pn, qn
        return (x - gam * O.div2d(rr, ss)).ravel()


class Model:
    """A posterior on the device (pf, pg) and in the checker (advance)."""

    def __init__(self, la, kind, shape, rng):
        self.shape = shape
        img = np.zeros(shape)
        img[shape[0] // 4:shape[0] // 2, shape[1] // 4:3 * shape[1] // 4] = 150.0
        img += np.linspace(0, 30, shape[1])[None, :]
        self.img = img
        sf = 1 / SIGMA ** 2
        h, off = np.ones((5, 5)) / 25, (2, 2)
        if kind == "haar":
            mask = (rng.uniform(size=shape) < 0.6).astype(np.float64)
            y = mask * (img + rng.normal(0, SIGMA, shape))
            self.pf = la.L2(Op=la.Diagonal(mask, dims=shape), b=y, sigma=sf, dims=shape)
            self.pg = la.WaveletL1(shape, sigma=2.0)
            prior = {"kind": "haar", "sigma": 2.0, "t": GAMMA}
            self.advance = lambda v, t: O.myula_step(v, y, None, None, sf, t, GAMMA, prior, 0.0, mask=mask)
            return
        y = O.blur(img, h, off) + rng.normal(0, SIGMA, shape)
        Op = la.Convolve2D(shape, h, offset=off)
        if kind in ("tv10", "tv5", "l2"):
            self.pf = la.L2(Op=Op, b=y, sigma=sf)
            if kind == "l2":
                self.pg, prior = la.L2(sigma=0.05), {"kind": "l2", "sigma": 0.05, "t": GAMMA}
            else:
                K = 10 if kind == "tv10" else 5
                self.pg, prior = la.TV(shape, sigma=TAU_REG, niter=K), {"kind": "tv", "sigma": TAU_REG, "niter": K, "t": GAMMA}
            self.advance = lambda v, t: O.myula_step(v, y, h, off, sf, t, GAMMA, prior, 0.0)
            return
        # the two models O.myula_step does not have: the same formula over the checker's objects, chain by chain
        if kind == "aniso":
            self.pf, of = la.L2(Op=Op, b=y, sigma=sf), O.L2(Op=O.Convolve2D(shape, h, off), b=y.ravel(), sigma=sf)
            self.pg, og = la.TV(shape, sigma=TAU_REG, niter=10, isotropic=False), AnisoTV(shape, TAU_REG, 10)
        elif kind == "mctv":
            kw = dict(dims=shape, b=y.ravel(), sigma=sf, lamda=0.3, gamma=15.0, isotropic=True, niter=20)
            self.pf, of = la.L2_ncvx_tv(Op=Op, Op2=la.Gradient(shape), **kw), O.L2NcvxTV(Op=O.Convolve2D(shape, h, off), Op2=O.Gradient(shape), **kw)
            self.pg, og = la.TV(shape, sigma=TAU_REG, niter=10), O.TV(shape, sigma=TAU_REG, niter=10)
        else:
            raise ValueError(kind)

        def advance(v, t):
            out = np.empty_like(v)
            for c in range(v.shape[0]):
                vc = v[c].ravel()
                out[c] = ((1 - t / GAMMA) * vc - t * of.grad(vc) + t / GAMMA * og.prox(vc, GAMMA)).reshape(shape)
            return out
        self.advance = advance

    def delta(self, s, frac=0.8):
        return frac * step_factor(s) / (1 / SIGMA ** 2 + 1 / GAMMA)


# ------------------------------------------------------------------ 1. closed forms of a linear drift
@pytest.mark.parametrize("s", (2, 3, 10))
@pytest.mark.parametrize("noise", ("injected", "none"))
def test_linear_drift_reproduces_the_closed_forms(la, s, noise):
    shape, C_ = (16, 32), 3
    ell, sp, gamma = 1.3, 0.7, 0.4
    l_eff = ell + sp / (1 + gamma * sp)                     # drift = -l x - (x - x / (1 + gamma sp)) / gamma
    delta = 0.9 * step_factor(s) / (ell + 1 / gamma)
    rng = np.random.default_rng(s)
    x0 = rng.normal(0, 20, (C_,) + shape)
    Z = rng.standard_normal((1, C_) + shape)
    pf = la.L2(Op=None, b=np.zeros(shape), sigma=ell, dims=shape)
    smp = la.SKROCKSampler(pf, la.L2(sigma=sp), shape, n_stages=s, eta=ETA, n_chains=C_, tau=delta, gamma=gamma, noise=noise)
    smp.set_state(x0)
    if noise == "injected":
        smp.step(1, noise=Z)
    else:
        smp.step(1)
    got = smp.get_state().cpu().numpy()
    w0, w1, _, _, _ = coefficients(s)
    z = -delta * l_eff
    R = T(s, w0 + w1 * z) / T(s, w0)
    B = dT(s, w0 + w1 * z) / dT(s, w0) * (1 + w1 * z / 2)          # U_{s-1} = T_s' / s
    ref = R * x0 + (np.sqrt(2 * delta) * B * Z[0] if noise == "injected" else 0.0)
    e = rel(got, ref)
    print(f"s={s} noise={noise}: R={R:.6f} B={B:.6f} rel {e:.3e} ({smp.kernel_name})")
    assert abs(R) <= 1.0
    assert e < STEP_TOL, e
    assert smp.iteration == 1 and smp.n_stages == s and smp.eta == ETA
    smp.close()


# ------------------------------------------------------------------ 2. trajectories, injected noise
TRAJ_CASES = [("tv10", (24, 160), 2), ("tv10", (24, 160), 5), ("tv10", (24, 160), 10), ("tv10", (20, 264), 5), ("tv5", (32, 32), 5),
              ("l2", (32, 32), 5), ("haar", (32, 32), 5), ("aniso", (24, 160), 5), ("mctv", (24, 160), 5)]


@pytest.mark.parametrize("kind,shape,s", TRAJ_CASES)
def test_trajectory_matches_the_definition_with_injected_noise(la, kind, shape, s):
    rng = np.random.default_rng(17)
    m = Model(la, kind, shape, rng)
    C_, nit = 3, 3
    delta = m.delta(s)
    x0 = m.img[None] + rng.normal(0, 3, (C_,) + shape)
    noise = rng.standard_normal((nit, C_) + shape)
    smp = la.SKROCKSampler(m.pf, m.pg, shape, n_stages=s, n_chains=C_, tau=delta, gamma=GAMMA, noise="injected")
    smp.set_state(x0)
    smp.step(nit, noise=noise)
    got = smp.get_state().cpu().numpy()
    ref = x0
    for k in range(nit):
        ref = skrock_iteration(m.advance, ref, noise[k], delta, s)
    e = rel(got, ref)
    print(f"{kind} {shape} s={s} delta={delta:.3f}: rel {e:.3e}, max |x| {np.abs(ref).max():.1f} ({smp.kernel_name})")
    assert e < TRAJ_TOL, e
    assert smp.iteration == nit
    plain = la.MYULASampler(m.pf, m.pg, shape, n_chains=C_, tau=0.2 * GAMMA, gamma=GAMMA, noise="injected")
    plain.set_state(x0)
    plain.step(1, noise=noise[:1])
    assert smp.kernel_name == plain.kernel_name, (smp.kernel_name, plain.kernel_name)
    plain.close()
    smp.close()


# ------------------------------------------------------------------ 3. Philox noise, sharding
@pytest.mark.parametrize("shape", [(24, 40), (12, 18)])
def test_philox_trajectory_and_field(la, shape):
    rng = np.random.default_rng(5)
    m = Model(la, "tv5", shape, rng)
    C_, nit, s, seed, off_c = 3, 4, 5, 77, 40
    delta = m.delta(s)
    x0 = m.img[None] + rng.normal(0, 3, (C_,) + shape)
    smp = la.SKROCKSampler(m.pf, m.pg, shape, n_stages=s, n_chains=C_, tau=delta, gamma=GAMMA, seed=seed, chain_offset=off_c)
    smp.set_state(x0)
    smp.step(nit)
    got = smp.get_state().cpu().numpy()
    ref = x0
    for k in range(nit):
        xi = O.philox_normals(seed, k, off_c + np.arange(C_), *shape).astype(np.float64)
        ref = skrock_iteration(m.advance, ref, xi, delta, s)
    e = rel(got, ref)
    print(f"philox {shape}: rel {e:.3e} ({smp.kernel_name})")
    assert e < TRAJ_TOL, e
    assert smp.iteration == nit
    smp.close()


def test_sharding_is_bit_identical(la):
    shape = (24, 40)
    rng = np.random.default_rng(6)
    m = Model(la, "tv5", shape, rng)
    s, nit = 5, 4
    delta = m.delta(s)
    x0 = m.img[None] + rng.normal(0, 3, (6,) + shape)
    kw = dict(n_stages=s, tau=delta, gamma=GAMMA, seed=11)
    whole = la.SKROCKSampler(m.pf, m.pg, shape, n_chains=6, **kw)
    a = la.SKROCKSampler(m.pf, m.pg, shape, n_chains=3, chain_offset=0, **kw)
    b = la.SKROCKSampler(m.pf, m.pg, shape, n_chains=3, chain_offset=3, **kw)
    whole.set_state(x0)
    a.set_state(x0[:3])
    b.set_state(x0[3:])
    for smp in (whole, a, b):
        smp.step(nit)
    w = whole.get_state().cpu().numpy()
    np.testing.assert_array_equal(w[:3], a.get_state().cpu().numpy())
    np.testing.assert_array_equal(w[3:], b.get_state().cpu().numpy())
    assert np.isfinite(w).all() and not np.array_equal(w[:3], w[3:])
    for smp in (whole, a, b):
        smp.close()


# ------------------------------------------------------------------ 4. moments ride along; 6. the driver
MOM = dict(shape=(24, 40), C=4, s=5, nit=6, burn_in=1, thin=2, seed=21, bins=8)


@pytest.fixture(scope="module")
def moments_run(la):
    """Six step(1) calls with the state read after each: the float64 sums over the kept iterations, the sampler's own accumulators and its final
    state -- shared by the tests below."""
    p = MOM
    rng = np.random.default_rng(8)
    m = Model(la, "tv5", p["shape"], rng)
    delta = m.delta(p["s"])
    x0 = m.img[None] + rng.normal(0, 3, (p["C"],) + p["shape"])
    lo, hi = float(m.img.min() - 40), float(m.img.max() + 40)
    kw = dict(n_stages=p["s"], n_chains=p["C"], tau=delta, gamma=GAMMA, seed=p["seed"], moments=True, burn_in=p["burn_in"], thin=p["thin"],
              moment_scales=(2,), hist_bins=p["bins"], hist_range=(lo, hi))
    one = la.SKROCKSampler(m.pf, m.pg, p["shape"], **kw)
    one.set_state(x0)
    s1, s2, kept = np.zeros(p["shape"]), np.zeros(p["shape"]), 0
    for k in range(p["nit"]):
        one.step(1)
        if k >= p["burn_in"] and (k - p["burn_in"]) % p["thin"] == 0:
            x = one.get_state().cpu().numpy().astype(np.float64)
            s1 += x.sum(axis=0)
            s2 += (x * x).sum(axis=0)
            kept += 1
    out = dict(m=m, delta=delta, x0=x0, kw=kw, s1=s1, s2=s2, kept=kept, state=one.get_state().cpu().numpy(),
               moments=tuple(v.cpu().numpy() if hasattr(v, "cpu") else v for v in one.moments()),
               block=tuple(v.cpu().numpy() if hasattr(v, "cpu") else v for v in one.block_moments(2)),
               hist=one.histogram()[0].cpu().numpy(), iteration=one.iteration, range=(lo, hi))
    one.close()
    return out


def test_moments_reduce_the_kept_iterations(la, moments_run):
    r, p = moments_run, MOM
    d1, d2, cnt = r["moments"]
    assert r["kept"] == 3 and cnt == p["C"] * 3
    assert rel(d1, r["s1"]) < TRAJ_TOL and rel(d2, r["s2"]) < TRAJ_TOL
    S1, S2, bc = r["block"]
    assert bc == cnt
    H, W = p["shape"]
    assert rel(S1, r["s1"].reshape(H // 2, 2, W // 2, 2).sum(axis=(1, 3))) < TRAJ_TOL
    assert r["hist"].shape == (p["bins"] + 2, H, W) and (r["hist"].sum(axis=0) == cnt).all()
    assert r["iteration"] == p["nit"]


def test_one_call_equals_single_steps(la, moments_run):
    r, p = moments_run, MOM
    smp = la.SKROCKSampler(r["m"].pf, r["m"].pg, p["shape"], **r["kw"])
    smp.set_state(r["x0"])
    smp.step(p["nit"])
    np.testing.assert_array_equal(smp.get_state().cpu().numpy(), r["state"])
    d1, d2, cnt = smp.moments()
    assert cnt == r["moments"][2] and smp.iteration == r["iteration"]
    np.testing.assert_array_equal(smp.histogram()[0].cpu().numpy(), r["hist"])
    assert rel(d1.cpu().numpy(), r["moments"][0]) < 1e-12 and rel(d2.cpu().numpy(), r["moments"][1]) < 1e-12
    smp.close()


def test_stabilised_langevin_driver(la, moments_run):
    r, p = moments_run, MOM
    res = la.StabilisedLangevin(r["m"].pf, r["m"].pg, r["x0"], r["delta"], gamma=GAMMA, niter=p["nit"], n_stages=p["s"], seed=p["seed"],
                                n_chains=p["C"], dims=p["shape"], burn_in=p["burn_in"], thin=p["thin"], moment_scales=(2,), hist_bins=p["bins"],
                                hist_range=r["range"])
    cnt = p["C"] * 3
    assert res.count == cnt and res.n_stages == p["s"] and res.gradient_evaluations == p["nit"] * p["s"]
    mean = r["s1"] / cnt
    var = r["s2"] / cnt - mean * mean
    assert rel(res.mean.cpu().numpy(), mean) < TRAJ_TOL
    assert np.abs(res.var.cpu().numpy() - var).max() < TRAJ_TOL * (r["s2"] / cnt).max()
    np.testing.assert_array_equal(res.state.cpu().numpy(), r["state"])
    np.testing.assert_array_equal(res.hist.cpu().numpy(), r["hist"])
    assert set(res.scale_mean) == {2} and set(res.quantiles) == {0.05, 0.5, 0.95}
    seen = []
    res2 = la.StabilisedLangevin(r["m"].pf, r["m"].pg, r["x0"], r["delta"], gamma=GAMMA, niter=2, n_stages=p["s"], seed=p["seed"],
                                 callback=lambda x: seen.append(x.shape), n_chains=p["C"], dims=p["shape"])
    assert len(seen) == 2 and res2.gradient_evaluations == 2 * p["s"]


# ------------------------------------------------------------------ 5. the C ABI: refusals, counters, timing
def c_config(la, shape, prob, n_chains=2):
    from lmc_atomi_amd import _capi
    cfg = _capi.lmc_myula_config()
    cfg.struct_size = C.sizeof(_capi.lmc_myula_config)
    cfg.problem = prob.c
    cfg.n_chains = n_chains
    cfg.tau, cfg.gamma, cfg.epsg = 0.2 * GAMMA, GAMMA, 1.0
    cfg.noise_mode = _capi.NOISE_PHILOX
    cfg.thin = 1
    return cfg


@pytest.mark.parametrize("what,status", [("tv_warm", LMC_E_UNSUPPORTED), ("tv_rtol", LMC_E_UNSUPPORTED), ("prox_scale", LMC_E_UNSUPPORTED),
                                         ("one_stage", LMC_E_INVALID), ("ok", 0)])
def test_c_abi_refusals(la, what, status):
    import torch
    from lmc_atomi_amd import _dev
    from lmc_atomi_amd.proximal import _Problem
    shape = (24, 264)
    m = Model(la, "tv10" if what != "prox_scale" else "l2", shape, np.random.default_rng(3))
    prior = m.pg.prior_descriptor()
    opts = {}
    keep = None
    if what == "tv_warm":
        prior = la.TV(shape, sigma=TAU_REG, niter=3, warm=True).prior_descriptor()
    elif what == "tv_rtol":
        prior = la.TV(shape, sigma=TAU_REG, niter=10, rtol=1e-4).prior_descriptor()
    elif what == "prox_scale":
        keep = torch.full((shape[0] * shape[1],), 0.5, dtype=torch.float32, device="cuda")
        opts["prox_scale"] = (keep, 0, 1)
    prob = _Problem(shape, m.pf.descriptor(), prior, options=opts)
    cfg = c_config(la, shape, prob)
    lib = _dev.lib()
    hnd = C.c_void_p()
    rc = lib.lmc_skrock_create(C.byref(cfg), 1 if what == "one_stage" else 5, ETA, C.byref(hnd))
    msg = lib.lmc_last_error().decode()
    print(what, "->", rc, msg if rc else "")
    assert rc == status, (rc, msg)
    if rc:
        assert msg and not hnd.value
        return
    st = _dev.stream_ptr()
    assert lib.lmc_sampler_get_acceptance(hnd, None, None, st) == LMC_E_STATE
    assert lib.lmc_sampler_enable_timing(hnd, 1) == 0
    assert lib.lmc_sampler_step(hnd, 3, None, st) == 0
    ms, n = C.c_float(), C.c_int32()
    assert lib.lmc_sampler_last_step_timing(hnd, C.byref(ms), C.byref(n)) == 0
    torch.cuda.synchronize()
    assert n.value == 3 * 5 and ms.value > 0
    assert lib.lmc_sampler_iteration(hnd) == 3
    assert lib.lmc_sampler_kernel_name(hnd).decode() == "myula_step_pipe_kernel"
    lib.lmc_sampler_destroy(hnd)


def test_me_tv_early_exit_stays_allowed(la):
    """ncvx_rtol > 0 (the inner prox of the ME-TV term leaves early, chain by chain) runs per evaluation and is not refused."""
    shape = (24, 160)
    rng = np.random.default_rng(4)
    m = Model(la, "tv10", shape, rng)
    y = O.blur(m.img, np.ones((5, 5)) / 25, (2, 2))
    pf = la.L2_ncvx_tv(dims=shape, Op=la.Convolve2D(shape, np.ones((5, 5)) / 25, offset=(2, 2)), b=y.ravel(), sigma=1 / SIGMA ** 2, lamda=0.3,
                       gamma=15.0, isotropic=True, niter=20, rtol=1e-4)
    smp = la.SKROCKSampler(pf, m.pg, shape, n_stages=3, n_chains=2, tau=m.delta(3, 0.5), gamma=GAMMA)
    smp.set_state(m.img)
    smp.step(2)
    assert smp.iteration == 2 and np.isfinite(smp.get_state().cpu().numpy()).all()
    smp.close()

"""GPU tests of the SAPG estimation of the prior weight (include/lmc_atomi.h: lmc_prior_statistic, lmc_sampler_set_prior_sigma, lmc_sampler_sapg;
Python: prior_statistic, MYULASampler.set_prior_weight / estimate_prior_weight, EstimatePriorWeight).

The float64 reference is built here from the checker as it stands: `O.myula_step` for the sampler iteration, `O.tv_value`, `O.haar_l1_value` and an
anisotropic sum from `O.grad2d` for the statistic, and the update

    delta_n = c0 (n + 1)^(-p) / d,   theta_{n+1} = exp(clamp(log theta_n + delta_n (d / k - theta_n gbar), log lo, log hi))

in numpy.  The handle's weight is a float: the reference runs its sampler iterations at float32(theta_n), as the library does.

The per-image sum of the statistic is ORDER-FIXED (no atomics: a thread's partial sum, wave shuffles, per-wave slots, then the bands of an image in
order), so two runs must give equal bits per image.

Bounds: the statistic rtol 1e-5 (the figure per-image prior values are held to in tests/test_gpu_haar.py); the loop max(1e-5, 4 x the gap between
the reference loop in float32 and in float64), computed and printed here; fused loop against its public pieces 1e-12 (the order of one float64
mean); the known answer 4 s sqrt(1 + 1/8) with s the standard deviation (n - 1 in the denominator) of 8 float64 replicas."""
import ctypes as C

import numpy as np
import pytest

from oracle import lmc_oracle as O

pytestmark = pytest.mark.gpu

LMC_E_INVALID, LMC_E_UNSUPPORTED = -1, -2
SIGMA = 0.75
GAMMA = SIGMA ** 2
TAU = 0.2
BOUNDS = (1e-3, 1e2)
H5, OFF = np.ones((5, 5)) / 25, (2, 2)


@pytest.fixture(scope="module")
def la():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import lmc_atomi_amd as la
    return la


# ------------------------------------------------------------------ the reference
def statistic(kind, x):
    """g(x_i) with weight 1 per image of x[..., H, W]: per-pixel terms in the dtype of x, summed in float64."""
    if kind == "tv":
        dr, dc = O.grad2d(x)
        return np.sum(np.sqrt(dr * dr + dc * dc), axis=(-2, -1), dtype=np.float64)
    if kind == "aniso":
        dr, dc = O.grad2d(x)
        return np.sum(np.abs(dr), axis=(-2, -1), dtype=np.float64) + np.sum(np.abs(dc), axis=(-2, -1), dtype=np.float64)
    if kind == "l1":
        return np.sum(np.abs(x), axis=(-2, -1), dtype=np.float64)
    if kind == "l2":
        return 0.5 * np.sum(x * x, axis=(-2, -1), dtype=np.float64)
    if kind == "haar":
        cf = O.haar_fwd(x, 3)
        Hc, Wc = cf.shape[-2] >> 3, cf.shape[-1] >> 3
        return np.sum(np.abs(cf), axis=(-2, -1), dtype=np.float64) - np.sum(np.abs(cf[..., :Hc, :Wc]), axis=(-2, -1), dtype=np.float64)
    raise ValueError(kind)


def dimension(kind, shape):
    n = shape[0] * shape[1]
    return {"tv": (n - 1.0, 1.0), "aniso": (n - 1.0, 1.0), "l1": (float(n), 1.0), "l2": (float(n), 2.0),
            "haar": (float(n - (shape[0] // 8) * (shape[1] // 8)), 1.0)}[kind]


def next_theta(n, theta, gbar, d, k, c0=10.0, p=0.8, lo=BOUNDS[0], hi=BOUNDS[1]):
    delta = c0 * (n + 1.0) ** (-p) / d
    eta = np.log(theta) + delta * (d / k - theta * gbar)
    if eta <= np.log(lo) or eta >= np.log(hi):       # a clamped step is the bound itself (exp(log(1e-3)) is not 1e-3)
        return lo if eta <= np.log(lo) else hi
    return float(np.exp(eta))


def make_prior(la, kind, shape, weight, **kw):
    if kind in ("tv", "aniso"):
        return la.TV(shape, sigma=weight, niter=10, isotropic=kind == "tv", **kw)
    if kind == "l1":
        return la.L1(sigma=weight, dims=shape)
    if kind == "l2":
        return la.L2(sigma=weight, dims=shape)
    return la.WaveletL1(shape, sigma=weight)


class Model:
    """A posterior on the device (proxf, prior(weight)) and in the checker (step)."""

    def __init__(self, data, kind, shape, seed=11):
        rng = np.random.default_rng(seed)
        self.data, self.kind, self.shape = data, kind, shape
        img = np.zeros(shape)
        img[shape[0] // 4:shape[0] // 2, shape[1] // 4:3 * shape[1] // 4] = 150.0
        img += np.linspace(0, 30, shape[1])[None, :]
        self.sf = 1 / SIGMA ** 2
        self.mask = None
        if data == "blur":
            self.y = O.blur(img, H5, OFF) + rng.normal(0, SIGMA, shape)
        elif data == "mask":
            self.mask = (rng.uniform(size=shape) < 0.6).astype(np.float64)
            self.y = self.mask * (img + rng.normal(0, SIGMA, shape))
        else:
            self.y = img + rng.normal(0, SIGMA, shape)
        # the chains start at the observation plus strong noise: the statistic is large, and the first update lands on the lower bound
        self.x0 = (self.y[None] + rng.normal(0, 10.0, (8,) + shape)).astype(np.float32)
        self.d, self.k = dimension(kind, shape)

    def proxf(self, la):
        if self.data == "blur":
            return la.L2(Op=la.Convolve2D(self.shape, H5, offset=OFF), b=self.y, sigma=self.sf)
        if self.data == "mask":
            return la.L2(Op=la.Diagonal(self.mask, dims=self.shape), b=self.y, sigma=self.sf, dims=self.shape)
        return la.L2(b=self.y, sigma=self.sf, dims=self.shape)

    def step(self, x, theta, xi):
        dt = x.dtype
        prior = {"kind": "tv" if self.kind == "tv" else self.kind, "sigma": float(np.float32(theta)), "niter": 10, "t": GAMMA}
        y = self.y.astype(dt)
        mask = None if self.mask is None else self.mask.astype(dt)
        h = H5.astype(dt) if self.data == "blur" else None
        return O.myula_step(x, y, h, OFF if h is not None else None, self.sf, TAU, GAMMA, prior, xi.astype(dt), mask=mask)

    def loop(self, noise, dtype, warmup, n_updates, ipu, theta0=0.3):
        x = self.x0.astype(dtype)
        it = 0
        for _ in range(warmup):
            x = self.step(x, theta0, noise[it]).astype(dtype)
            it += 1
        theta, trace, gbars = theta0, [theta0], []
        for n in range(n_updates):
            for _ in range(ipu):
                x = self.step(x, theta, noise[it]).astype(dtype)
                it += 1
            gbar = float(np.mean(statistic(self.kind, x)))
            theta = next_theta(n, theta, gbar, self.d, self.k)
            trace.append(theta)
            gbars.append(gbar)
        return np.array(trace), np.array(gbars), x


# ------------------------------------------------------------------ 1. the statistic
STAT_SHAPES = [(8, 8), (24, 136), (16, 520), (17, 67), (1, 64), (64, 1)]


def stat_input(shape, n, seed=2):
    rng = np.random.default_rng(seed)
    img = np.zeros(shape)
    img[shape[0] // 4:max(shape[0] // 2, 1), shape[1] // 4:max(3 * shape[1] // 4, 1)] = 200.0
    img += np.linspace(0, 55, shape[1])[None, :]
    return (img[None] + rng.normal(0, 8.0, (n,) + shape)).astype(np.float32)


# the Haar prior needs sides that are multiples of 8: it has no 17 x 67 and no thin case
STAT_CASES = [(k, s) for k in ("tv", "aniso", "l1", "l2", "haar") for s in STAT_SHAPES if k != "haar" or not (s[0] % 8 or s[1] % 8)]


@pytest.mark.parametrize("kind,shape", STAT_CASES, ids=[f"{k}-{s[0]}x{s[1]}" for k, s in STAT_CASES])
def test_statistic_matches_the_reference(la, kind, shape):
    import torch
    x = stat_input(shape, 3)
    ref = statistic(kind, x.astype(np.float64))
    xt = torch.from_numpy(x).cuda()
    pg = make_prior(la, kind, shape, 0.3)            # the weight does not enter: the statistic has weight 1
    a = la.prior_statistic(pg, xt, dims=shape).cpu().numpy()
    b = la.prior_statistic(pg, xt, dims=shape).cpu().numpy()
    err = np.abs(a - ref) / np.abs(ref)
    print(f"{kind} {shape}: statistic {a}, max relative error {err.max():.2e}")
    assert a.dtype == np.float64 and a.shape == (3,)
    assert err.max() <= 1e-5
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), "the per-image sum is order-fixed: two runs give equal bits"


@pytest.mark.parametrize("kind", ["l1", "tv"])
def test_statistic_of_65537_images(la, kind):
    import torch
    x = stat_input((8, 8), 65537, seed=4)
    ref = statistic(kind, x.astype(np.float64))
    xt = torch.from_numpy(x).cuda()
    pg = make_prior(la, kind, (8, 8), 1.0)
    a = la.prior_statistic(pg, xt, dims=(8, 8)).cpu().numpy()
    b = la.prior_statistic(pg, xt, dims=(8, 8)).cpu().numpy()
    err = np.abs(a - ref) / np.abs(ref)
    print(f"{kind} 65537 x 8x8: max relative error {err.max():.2e} (image {int(err.argmax())})")
    assert err.max() <= 1e-5
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))


def test_statistic_refusals(la):
    import torch
    from lmc_atomi_amd import _capi, _dev
    x = torch.zeros(2, 8, 8, device="cuda")
    with pytest.raises(NotImplementedError):
        la.prior_statistic(la.Laplace(0.1), x, dims=(8, 8))
    out = torch.zeros(2, dtype=torch.float64, device="cuda")
    p = _capi.lmc_problem()
    p.struct_size = C.sizeof(_capi.lmc_problem)
    p.H, p.W = 8, 8
    for kind in (_capi.PRIOR_NONE, _capi.PRIOR_EPROX):
        p.prior_kind = kind
        assert _dev.lib().lmc_prior_statistic(C.byref(p), _dev.ptr(x), 2, _dev.ptr(out), None) == LMC_E_UNSUPPORTED
    p.prior_kind = _capi.PRIOR_L1
    assert _dev.lib().lmc_prior_statistic(C.byref(p), None, 2, _dev.ptr(out), None) == LMC_E_INVALID
    assert _dev.lib().lmc_prior_statistic(C.byref(p), _dev.ptr(x), 0, _dev.ptr(out), None) == LMC_E_INVALID


# ------------------------------------------------------------------ 2. the setter
SETTER_CASES = {
    "blur+l1 rows": ("blur", "l1", (24, 136), {}, {}),
    "blur+l1 rows, 2 iterations per launch": ("blur", "l1", (24, 136), {"policy": {"iterations_per_launch": 2}}, {}),
    "mask+haar block": ("mask", "haar", (16, 16), {}, {}),
    "tv tile 16x16": ("blur", "tv", (16, 16), {}, {}),
    "tv pipe 24x136": ("blur", "tv", (24, 136), {}, {}),
    "aniso tv 24x136": ("blur", "aniso", (24, 136), {}, {}),
    "tv rtol 24x136": ("blur", "tv", (24, 136), {}, {"rtol": 1e-4}),
    "skrock tv 24x136": ("blur", "tv", (24, 136), {"n_stages": 3}, {}),
}


@pytest.mark.parametrize("case", list(SETTER_CASES))
def test_setter_equals_a_sampler_created_with_the_weight(la, case):
    data, kind, shape, skw, pkw = SETTER_CASES[case]
    m = Model(data, kind, shape)
    a, b = 0.3, 0.07
    cls = la.SKROCKSampler if "n_stages" in skw else la.MYULASampler
    kw = dict(n_chains=8, tau=TAU, gamma=GAMMA, seed=17, **skw)
    with cls(m.proxf(la), make_prior(la, kind, shape, a, **pkw), shape, **kw) as s1, \
            cls(m.proxf(la), make_prior(la, kind, shape, b, **pkw), shape, **kw) as s2:
        s1.set_prior_weight(b)
        for s in (s1, s2):
            s.set_state(m.x0)
            s.step(3)
        x1, x2 = s1.get_state().cpu().numpy(), s2.get_state().cpu().numpy()
        print(f"{case}: kernel {s1.kernel_name} / {s2.kernel_name}")
        assert s1.kernel_name == s2.kernel_name
    assert np.isfinite(x2).all() and not np.array_equal(x2, m.x0)
    assert np.array_equal(x1.view(np.uint32), x2.view(np.uint32)), "the same arguments give the same launches: bit-identical states"


# ------------------------------------------------------------------ 3. the loop against the float64 reference
LOOP_MODELS = {"blur+tv 24x136": ("blur", "tv", (24, 136)), "blur+l1 24x136": ("blur", "l1", (24, 136)), "blur+tv 16x16": ("blur", "tv", (16, 16)),
               "mask+haar 16x16": ("mask", "haar", (16, 16)), "identity+l2 16x16": ("identity", "l2", (16, 16))}
WARMUP, N_UPDATES = 5, 25
_loop_cache = {}


def loop_reference(name, ipu):
    """(model, noise, float64 trace, gbar trace, float32-against-float64 gap), computed once per case."""
    key = (name, ipu)
    if key not in _loop_cache:
        data, kind, shape = LOOP_MODELS[name]
        m = Model(data, kind, shape)
        noise = np.random.default_rng(5).standard_normal((WARMUP + N_UPDATES * ipu, 8) + shape).astype(np.float32)
        t64, g64, _ = m.loop(noise, np.float64, WARMUP, N_UPDATES, ipu)
        t32, g32, _ = m.loop(noise, np.float32, WARMUP, N_UPDATES, ipu)
        gap = max(np.max(np.abs(t32 - t64) / t64), np.max(np.abs(g32 - g64) / g64))
        _loop_cache[key] = (m, noise, t64, g64, float(gap))
    return _loop_cache[key]


@pytest.mark.parametrize("ipu", [1, 2])
@pytest.mark.parametrize("name", list(LOOP_MODELS))
def test_loop_matches_the_float64_reference(la, name, ipu):
    m, noise, t64, g64, gap = loop_reference(name, ipu)
    bound = max(1e-5, 4 * gap)
    with la.MYULASampler(m.proxf(la), make_prior(la, m.kind, m.shape, 0.3), m.shape, n_chains=8, tau=TAU, gamma=GAMMA, noise="injected") as smp:
        smp.set_state(m.x0)
        res = smp.estimate_prior_weight(N_UPDATES, BOUNDS, theta0=0.3, warmup=WARMUP, iters_per_update=ipu, step_scale=10.0, step_exponent=0.8,
                                        noise=noise)
        assert smp.iteration == WARMUP + N_UPDATES * ipu
    et = np.max(np.abs(res.theta_trace - t64) / t64)
    eg = np.max(np.abs(res.stat_trace - g64) / g64)
    print(f"{name} ipu={ipu}: float32-float64 gap of the reference {gap:.2e}, bound {bound:.2e}; theta trace error {et:.2e}, gbar trace error {eg:.2e}; "
          f"theta_1 = {res.theta_trace[1]:.4g}, last theta = {res.theta_trace[-1]:.5f} (reference {t64[-1]:.5f}), theta_bar = {res.theta:.5f}")
    assert res.theta_trace.shape == (N_UPDATES + 1,) and res.stat_trace.shape == (N_UPDATES,)
    assert res.theta_trace[0] == 0.3
    assert (res.dim_eff, res.degree) == (m.d, m.k)
    assert t64[1] == BOUNDS[0] and res.theta_trace[1] == BOUNDS[0], "the first update is projected onto the lower bound"
    assert et <= bound and eg <= bound
    avg = np.mean(res.theta_trace[N_UPDATES // 2 + 1:])
    assert abs(res.theta - avg) <= 1e-14 * avg


# ------------------------------------------------------------------ 4. the fused loop equals its public pieces
@pytest.mark.parametrize("which", ["myula", "skrock"])
def test_fused_loop_equals_its_public_pieces(la, which):
    m = Model("blur", "tv", (24, 136))
    kw = dict(n_chains=8, tau=TAU, gamma=GAMMA, seed=23)
    if which == "skrock":
        cls, kw = la.SKROCKSampler, dict(kw, n_stages=3)
    else:
        cls = la.MYULASampler
    warmup, n_updates, ipu = 3, 12, 2
    pg = make_prior(la, "tv", m.shape, 0.3)
    with cls(m.proxf(la), pg, m.shape, **kw) as fused, cls(m.proxf(la), pg, m.shape, **kw) as hand:
        fused.set_state(m.x0)
        res = fused.estimate_prior_weight(n_updates, BOUNDS, theta0=0.3, warmup=warmup, iters_per_update=ipu)
        hand.set_state(m.x0)
        hand.set_prior_weight(0.3)
        hand.step(warmup)
        theta, trace = 0.3, [0.3]
        for n in range(n_updates):
            hand.step(ipu)
            gbar = float(np.mean(la.prior_statistic(pg, hand.get_state()).cpu().numpy()))
            theta = la.sapg_update(theta, gbar, n, m.d, m.k, theta_bounds=BOUNDS, step_scale=10.0, step_exponent=0.8)
            hand.set_prior_weight(theta)
            trace.append(theta)
        assert fused.iteration == hand.iteration == warmup + n_updates * ipu
    err = np.max(np.abs(res.theta_trace - np.array(trace)) / np.array(trace))
    print(f"{which}: fused against step / prior_statistic / sapg_update / set_prior_weight: max relative difference {err:.2e}; trace {res.theta_trace}")
    assert err <= 1e-12


# ------------------------------------------------------------------ 5. a known answer
def test_known_answer_identity_l2(la):
    """Identity data term + l2 prior: MYULA is x' = a x + b y + sqrt(2 tau) xi per pixel with a = 1 - tau/gamma - tau/sigma^2 + (tau/gamma) / (1 + gamma theta)
    and b = tau / sigma^2, so its stationary E[1/2 ||x||^2] = 1/2 sum_i ((b y_i / (1 - a))^2 + 2 tau / (1 - a^2)) is in closed form, and SAPG converges
    to the root theta+ of d / 2 - theta E_theta[1/2 ||x||^2] = 0."""
    from scipy.optimize import brentq
    shape, Cn = (16, 16), 32
    sigma = 0.5
    gamma, tau = sigma ** 2, 0.2 * sigma ** 2
    rng = np.random.default_rng(3)
    xs = rng.normal(0, np.sqrt(1 / 0.25), shape)
    y = xs + rng.normal(0, sigma, shape)
    d = float(shape[0] * shape[1])

    def stationary(theta):
        a = 1 - tau / gamma - tau / sigma ** 2 + (tau / gamma) / (1 + gamma * theta)
        b = tau / sigma ** 2
        return 0.5 * np.sum((b * y / (1 - a)) ** 2 + 2 * tau / (1 - a * a))

    root = brentq(lambda t: d / 2 - t * stationary(t), 1e-3, 1e2, xtol=1e-14, rtol=1e-14)
    warmup, n_updates, avg_from, lo, hi = 50, 300, 100, 1e-3, 1e2

    def replica(seed):
        r = np.random.default_rng(seed)
        x = np.broadcast_to(y, (Cn,) + shape).copy()
        prior = {"kind": "l2", "sigma": 1.0, "t": gamma}
        for _ in range(warmup):
            x = O.myula_step(x, y, None, None, 1 / sigma ** 2, tau, gamma, prior, r.standard_normal(x.shape))
        theta, tr = 1.0, []
        for n in range(n_updates):
            prior["sigma"] = float(np.float32(theta))
            x = O.myula_step(x, y, None, None, 1 / sigma ** 2, tau, gamma, prior, r.standard_normal(x.shape))
            theta = next_theta(n, theta, float(np.mean(statistic("l2", x))), d, 2.0, lo=lo, hi=hi)
            tr.append(theta)
        return np.mean(tr[avg_from:])

    reps = np.array([replica(s) for s in range(8)])
    s = reps.std(ddof=1)
    bound = 4 * s * np.sqrt(1 + 1 / 8)
    pf = la.L2(b=y, sigma=1 / sigma ** 2, dims=shape)
    res = la.EstimatePriorWeight(pf, la.L2(sigma=1.0, dims=shape), y, tau, gamma, n_updates, (lo, hi), theta0=1.0, warmup=warmup, step_scale=10.0,
                                 average_from=avg_from, n_chains=Cn, seed=5, dims=shape)
    print(f"theta+ = {root:.5f}; 8 float64 replicas {reps.mean():.5f} +- {s:.5f}; GPU theta_bar = {res.theta:.5f}; bound {bound:.5f}")
    assert abs(reps.mean() - root) <= bound
    assert abs(res.theta - root) <= bound
    assert tuple(res.state.shape) == (Cn,) + shape and (res.dim_eff, res.degree) == (d, 2.0)


# ------------------------------------------------------------------ 6. refusals and state
def sapg_call(smp, cfg):
    from lmc_atomi_amd import _dev
    trace = (C.c_double * (cfg.n_updates + 1))()
    return _dev.lib().lmc_sampler_sapg(smp._h, C.byref(cfg), None, trace, None, None, _dev.stream_ptr(smp.device))


def test_refusals(la):
    from lmc_atomi_amd import _dev
    from lmc_atomi_amd.algs import _sapg_config
    lib = _dev.lib()
    m = Model("blur", "tv", (24, 136))
    shape = m.shape
    n = shape[0] * shape[1]
    cfg = _sapg_config(4, BOUNDS, 0.3)
    kw = dict(n_chains=2, tau=TAU, gamma=GAMMA)
    handles = {
        "mymala": lambda: la.MYMALASampler(m.proxf(la), la.TV(shape, 0.3), shape, **kw),
        "ulpda": lambda: la.ULPDASampler(m.proxf(la), la.L21(sigma=0.3), la.Gradient(shape), shape, n_chains=2, tau=0.1, mu=0.1),
        "tv_warm": lambda: la.MYULASampler(m.proxf(la), la.TV(shape, 0.3, niter=3, warm=True), shape, **kw),
        "prox_scale": lambda: la.MYULASampler(m.proxf(la), la.L2(sigma=0.05), shape, epsg=np.full(n, 0.5), **kw),
        "eprox": lambda: la.MYULASampler(m.proxf(la), la.Laplace(0.1), shape, **kw),
    }
    for name, make in handles.items():
        with make() as smp:
            assert lib.lmc_sampler_set_prior_sigma(smp._h, 0.1) == LMC_E_UNSUPPORTED, name
            assert lib.lmc_last_error()
            assert sapg_call(smp, cfg) == LMC_E_UNSUPPORTED, name
            with pytest.raises(NotImplementedError):
                smp.set_prior_weight(0.1)
            with pytest.raises(NotImplementedError):
                smp.estimate_prior_weight(4, BOUNDS, theta0=0.3)
            assert smp.iteration == 0
    with la.MYULASampler(m.proxf(la), la.TV(shape, 0.3), shape, **kw) as smp:
        for bad in (0.0, -0.1, float("nan"), float("inf")):
            assert lib.lmc_sampler_set_prior_sigma(smp._h, bad) == LMC_E_INVALID, bad
            with pytest.raises(ValueError):
                smp.set_prior_weight(bad)
        bad_cfg = _sapg_config(4, BOUNDS, 0.3)
        bad_cfg.step_exponent = 0.5
        assert sapg_call(smp, bad_cfg) == LMC_E_INVALID
        bad_cfg = _sapg_config(4, BOUNDS, 0.3)
        bad_cfg.struct_size = 8
        assert sapg_call(smp, bad_cfg) == LMC_E_INVALID
        assert lib.lmc_sampler_sapg(smp._h, C.byref(cfg), None, None, None, None, None) == LMC_E_INVALID       # no trace array
        assert lib.lmc_sampler_set_prior_sigma(None, 0.1) == LMC_E_INVALID
        assert smp.iteration == 0


def test_accumulators_are_suspended_and_the_counter_advances(la):
    m = Model("blur", "tv", (24, 136))
    Cn, warmup, n_updates, ipu = 8, 4, 6, 2
    with la.MYULASampler(m.proxf(la), la.TV(m.shape, 0.3), m.shape, n_chains=Cn, tau=TAU, gamma=GAMMA, moments=True, burn_in=0,
                         moment_scales=(4,), hist_bins=8, hist_range=(0.0, 255.0)) as smp:
        smp.set_state(m.x0)
        res = smp.estimate_prior_weight(n_updates, BOUNDS, warmup=warmup, iters_per_update=ipu)
        s1, s2, cnt = smp.moments()
        assert cnt == 0 and float(s1.abs().sum()) == 0.0 and float(s2.sum()) == 0.0
        assert smp.block_moments(4)[2] == 0 and float(smp.block_moments(4)[1].sum()) == 0.0
        counts, hc = smp.histogram()[:2]
        assert hc == 0 and int(counts.sum()) == 0
        assert smp.iteration == warmup + n_updates * ipu
        smp.step(3)
        assert smp.moments()[2] == 3 * Cn
        assert smp.iteration == warmup + n_updates * ipu + 3
        # on return the handle's weight is theta_bar: three more steps equal those of a sampler created with it, from the same state and iteration
        x_after = smp.get_state().cpu().numpy()
    with la.MYULASampler(m.proxf(la), la.TV(m.shape, float(np.float32(res.theta))), m.shape, n_chains=Cn, tau=TAU, gamma=GAMMA) as ref, \
            la.MYULASampler(m.proxf(la), la.TV(m.shape, 0.3), m.shape, n_chains=Cn, tau=TAU, gamma=GAMMA) as again:
        again.set_state(m.x0)
        again.estimate_prior_weight(n_updates, BOUNDS, warmup=warmup, iters_per_update=ipu)
        ref.set_state(again.get_state())
        ref.iteration = again.iteration
        ref.step(3)
        assert np.array_equal(ref.get_state().cpu().numpy().view(np.uint32), x_after.view(np.uint32))

"""GPU: the second-order TGV prior (LMC_PRIOR_TGV) against the float64 restatement of tests/_tgv_ref.py -- the prox through `TGV.prox` and through
lmc_tgv_prox (u and the auxiliary field w), the box forms, 70000 images, one MYULA step with six data terms, one SK-ROCK iteration, a Philox
trajectory, sharded moments, the accumulator keywords and every refusal.

Bound for every array compared, per pixel over every image (tests/_pixel.bound_of, the project's rule):

    max |got - ref64| <= max(3 e32, 2 ulp32(max |ref64|))

e32: the BETTER (smaller) of the deviations from float64 of the restatement's two float32 replays -- the definition's form, which divides, and the
kernel's, which multiplies by lam / sqrt(n2) and by 1 / (1 + s) -- measured on the reference, never on a kernel.  No pixel is excluded.  Every case
family prints its worst err / bound.  L = lmc_tgv_launch_iters(): niter in {1, L, L + 1, 2 L + 3} reaches the single-launch limit, the first chained
launch, a third launch and partial tiles."""
import ctypes as C

import numpy as np
import pytest

import _lattice as LT
import _pixel as X
import _poisson_ref as P
import _psf_ref as PR
import _radon_ref as R
import _skrock_pixel as S
import _tgv_ref as T
from oracle import lmc_oracle as O

pytestmark = pytest.mark.gpu

LMC_E_INVALID, LMC_E_UNSUPPORTED = -1, -2
SHAPE_IDS = [f"{s[0]}x{s[1]}" for s in T.SHAPES]
ALPHA0 = 0.5                                  # of the sampler tests: the second-order ball is active from the fifth iteration
GREY_W, COUNTS_W = 0.25, 4.0                  # prior weights: gamma * weight is 6.25 and 4, exact in float32
C_ = LT.N_CHAINS


@pytest.fixture(scope="module")
def la():
    import torch
    assert torch.cuda.is_available()
    import lmc_atomi_amd as la
    return la


def launch_iters():
    from lmc_atomi_amd import _capi
    return _capi.tgv_launch_iters()


def iters_of(name):
    L = launch_iters()
    return {"1": 1, "L": L, "L+1": L + 1, "2L+3": 2 * L + 3}[name]


def last_error():
    from lmc_atomi_amd import _dev
    return (_dev.lib().lmc_last_error() or b"").decode()


def report(tag, got, ref64, bound, e32):
    err, where = PR.worst(got, ref64)
    print(f"tgv {tag}: err {err:.3e} at {where} bound {bound:.3e} e32 {e32:.3e} err/bound {err / bound:.3f}")
    return err / bound


def raw_prox(x, lam, alpha0, K, bounds=None, want_w=True, step=0.0):
    """lmc_tgv_prox on an [n, H, W] array: (u, w)."""
    import torch
    from lmc_atomi_amd import _dev
    n, H, W = x.shape
    xt = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()
    out = torch.full_like(xt, -3.0)
    w = torch.full((n, 2, H, W), -3.0, dtype=torch.float32, device="cuda") if want_w else None
    lo, hi = bounds if bounds is not None else (0.0, 0.0)
    rc = _dev.lib().lmc_tgv_prox(_dev.ptr(xt), _dev.ptr(out), _dev.ptr(w), n, H, W, C.c_float(lam), C.c_float(alpha0), K, C.c_float(step),
                                 1 if bounds is not None else 0, C.c_float(lo), C.c_float(hi), _dev.stream_ptr(xt.device))
    assert rc == 0, last_error()
    torch.cuda.synchronize()
    return out.cpu().numpy(), (w.cpu().numpy() if want_w else None)


def check_prox(la, shape, lam, alpha0, K, bounds=None, tag=""):
    """`TGV.prox` with return_w on the case's images against float64: the worst err / bound of u and of w."""
    x = T.images(shape)
    (u64, eu, bu), (w64, ew, bw) = T.prox_reference(shape, lam, alpha0, K, bounds)
    pg = la.TGV(shape, sigma=1.0, alpha0=alpha0, niter=K, bounds=bounds)
    u, w = pg.prox(x, lam, return_w=True)
    assert u.shape == x.shape and u.dtype == np.float32 and w.shape == (x.shape[0], 2) + shape
    name = f"{shape[0]}x{shape[1]} a0={alpha0} lam={lam} K={K}{tag}"
    ru, rw = report(name + " u", u, u64, bu, eu), report(name + " w", w, w64, bw, ew)
    assert ru <= 1.0 and rw <= 1.0, (name, ru, rw)
    return u, w, max(ru, rw)


def test_the_case_list_holds_the_seams():
    L = launch_iters()
    assert 1 <= L < 32
    tile = 64 - 2 * L
    assert any(s[0] > tile and s[1] > tile for s in T.SHAPES), "more than one tile in both directions"
    assert any(s[0] % tile and s[1] % tile for s in T.SHAPES if s[0] > tile), "a partial last tile"
    assert -(-iters_of("L+1") // L) == 2 and -(-iters_of("2L+3") // L) == 3, "the first chained launch, and a third"


@pytest.mark.parametrize("shape", T.SHAPES, ids=SHAPE_IDS)
def test_prox_per_pixel(la, shape):
    worst = {}
    for it in ("1", "L", "L+1", "2L+3"):
        K = iters_of(it)
        cross = [(a, t) for a in T.ALPHAS for t in T.PROX_PARAMS] if it in ("L+1", "2L+3") else [(0.5, 2.5), (0.1, 40.0)]
        for alpha0, lam in cross:
            u, w, r = check_prox(la, shape, lam, alpha0, K)
            worst[it] = max(worst.get(it, 0.0), r)
    print(f"tgv prox {shape[0]}x{shape[1]}: worst err / bound " + ", ".join(f"niter {k}: {v:.3f}" for k, v in worst.items()))
    # the forms of the operand: one image [H, W], flat, and without w
    x = T.images(shape)
    pg = la.TGV(shape, sigma=0.5, alpha0=0.5, niter=iters_of("L+1"))
    batch = pg.prox(x, 5.0)
    one = pg.prox(x[1], 5.0)
    assert one.shape == shape and np.array_equal(one, batch[1]), "an image's prox does not depend on its batch"
    flat = pg.prox(x.ravel(), 5.0)
    assert flat.shape == (x.size,) and np.array_equal(flat.reshape(x.shape), batch)
    u1, w1 = pg.prox(x[0].ravel(), 5.0, return_w=True)
    assert u1.shape == (shape[0] * shape[1],) and w1.shape == (2,) + shape and np.array_equal(u1.reshape(shape), batch[0])


def test_two_hundred_iterations_on_a_small_shape(la):
    _, _, r = check_prox(la, (16, 24), 2.5, 0.5, 200)
    print(f"tgv prox 16x24 niter 200: worst err / bound {r:.3f}")


@pytest.mark.parametrize("shape", [(5, 7), (33, 70), (97, 261)], ids=["5x7", "33x70", "97x261"])
@pytest.mark.parametrize("bounds", [(80.0, 200.0), (0.0, np.inf)], ids=["80-200", "positive"])
def test_bounds(la, shape, bounds):
    worst = 0.0
    for it in ("L", "L+1", "2L+3"):
        for alpha0, lam in [(0.5, 2.5), (0.1, 40.0), (2.0, 40.0)]:
            K = iters_of(it)
            u, w, r = check_prox(la, shape, lam, alpha0, K, bounds, tag=f" box {bounds}")
            worst = max(worst, r)
            assert u.min() >= bounds[0] and u.max() <= bounds[1], "inside the box exactly"
            ru, rw = raw_prox(T.images(shape), lam, alpha0, K, bounds)
            assert np.array_equal(ru, u) and np.array_equal(rw, w), "TGV.prox and lmc_tgv_prox agree bit for bit"
    print(f"tgv box {bounds} {shape[0]}x{shape[1]}: worst err / bound {worst:.3f}")
    if bounds[1] < np.inf:
        K = iters_of("2L+3")
        free, (boxed, _, bound) = T.prox_reference(shape, 2.5, 0.5, K)[0][0], T.prox_reference(shape, 2.5, 0.5, K, bounds)[0]
        assert np.max(np.abs(boxed - np.clip(free, *bounds))) > 100 * bound, "the case tells the constrained prox from a clip afterwards"


@pytest.mark.parametrize("shape", [(5, 7), (64, 136), (97, 261)], ids=["5x7", "64x136", "97x261"])
def test_the_two_entry_points_agree_and_a_repeat_is_bit_equal(la, shape):
    x = T.images(shape)
    for it in ("1", "L", "L+1", "2L+3"):
        K = iters_of(it)
        pg = la.TGV(shape, sigma=1.0, alpha0=0.5, niter=K)
        u, w = pg.prox(x, 2.5, return_w=True)
        ru, rw = raw_prox(x, 2.5, 0.5, K)
        assert np.array_equal(u, ru) and np.array_equal(w, rw), "TGV.prox and lmc_tgv_prox agree bit for bit"
        u2, w2 = pg.prox(x, 2.5, return_w=True)
        assert np.array_equal(u, u2) and np.array_equal(w, w2), "equal runs give equal bits"
        assert np.array_equal(raw_prox(x, 2.5, 0.5, K, want_w=False)[0], u), "w_out = NULL changes nothing"
        assert np.array_equal(raw_prox(x, 2.5, 0.5, K, step=float(T.STEP))[0], u), "step 0 is the default step"
    pg = la.TGV(shape, sigma=1.0, niter=3)
    assert np.array_equal(pg.prox(x, 0.0), x) and np.array_equal(la.TGV(shape, sigma=0.0, niter=3).prox(x, 3.0), x), "a zero weight is the identity"
    u, w = la.TGV(shape, sigma=0.0, niter=3, bounds=(80.0, 200.0)).prox(x, 1.0, return_w=True)
    assert np.array_equal(u, np.clip(x, 80.0, 200.0)) and not w.any(), "with a box: the projection"


def test_seventy_thousand_images(la):
    """Images sit on gridDim.x: more than 65535 of them, with a chained prox."""
    n, shape, lam, alpha0, K = 70000, (4, 4), 2.5, 0.5, iters_of("L+1")
    rng = np.random.default_rng(5)
    x = X.f32(X.step_image(shape)[None] + rng.normal(0, 10, (n,) + shape))
    u64, w64 = T.tgv_prox(x.astype(np.float64), lam, alpha0, K, return_w=True)
    eu, bu = T.bound_from(u64, T.tgv_prox(x, lam, alpha0, K), T.tgv_prox(x, lam, alpha0, K, form="kernel"))
    ew, bw = T.bound_from(w64, T.tgv_prox(x, lam, alpha0, K, return_w=True)[1], T.tgv_prox(x, lam, alpha0, K, form="kernel", return_w=True)[1])
    u, w = la.TGV(shape, alpha0=alpha0, niter=K).prox(x, lam, return_w=True)
    assert report("70000 images u", u, u64, bu, eu) <= 1.0 and report("70000 images w", w, w64, bw, ew) <= 1.0
    last = la.TGV(shape, alpha0=alpha0, niter=K).prox(x[-1], lam)
    assert np.array_equal(last, u[-1])


# ------------------------------------------------------------------ the samplers: problems of tests/_lattice.py, two of them on operators of this file
DATA = ["none", "blur5", "poisson-positive", "psf15", "fourier16", "radon8"]
RADON8 = [0.1, 0.5, 0.9, float(np.float32(np.pi / 2)), 1.9, 2.2, 2.6, 2.9]


class _Custom:
    """A lattice problem on an operator of this file's choice: its float64 / float32 data term and its device descriptor."""

    def __init__(self, m, term, desc):
        self.m, self.term, self.desc = m, term, desc


def setup_of(data):
    """(problem of tests/_lattice.py, data term factory dtype -> term, device data descriptor, box)."""
    from lmc_atomi_amd.operators import spectral_tables
    if data in ("none", "blur5", "poisson-positive", "fourier16"):
        shape, kind = {"none": ((33, 70), 0), "blur5": ((33, 70), 2), "poisson-positive": ((33, 70), 5), "fourier16": ((16, 16), 12)}[data]
        m = LT.problem(shape, kind)
        d = {"data_kind": kind, "sigma_f": m.sigma_f}
        if data == "fourier16":
            d["y"] = spectral_tables(m.G, m.b)
        elif data != "none":
            d["y"] = m.y if m.aux is None else np.stack([m.y, m.aux])
            d["h"], d["offset"] = m.h, m.offset
        return _Custom(m, lambda dtype: LT.data_term(m, dtype), d), ((0.0, np.inf) if data == "poisson-positive" else None)
    shape = (33, 70) if data == "psf15" else (16, 24)
    rng = np.random.default_rng(17)
    img = X.step_image(shape, 250.0)
    base = LT.problem(shape, 9 if data == "psf15" else 16)
    if data == "psf15":
        h, off = X.f32(PR.random_taps(15, 15, 1515)), (7, 7)
        op = lambda dtype: P.Op("blur", h.astype(dtype), off)
        d = {"data_kind": 9, "sigma_f": base.sigma_f, "h": h, "offset": off}
    else:
        rad = R.RadonRef(shape, RADON8)
        op = lambda dtype: rad
        d = {"data_kind": 16, "sigma_f": base.sigma_f, "angles": rad.angles, "n_det": rad.n_det}
    y = X.f32(op(np.float64).fwd(img) + rng.normal(0, 5.0, op(np.float64).fwd(img).shape))
    d["y"] = y
    Lf = base.sigma_f * op(np.float64).norm2_bound()
    m = base._replace(y=y, tau=float(np.float32(0.5 / (Lf + 1.0 / base.gamma))), delta=float(np.float32(S.STEP_FRACTION * S.step_factor(3) / (Lf + 1.0 / base.gamma))))
    return _Custom(m, lambda dtype: R.term_of("l2", op(dtype), y, None, base.sigma_f, dtype), d), None


class _Prior:
    def __init__(self, weight, K, bounds, form):
        self.weight, self.K, self.bounds, self.form = weight, K, bounds, form

    def prox(self, x, t):
        return T.tgv_prox(x, self.weight * t, ALPHA0, self.K, bounds=self.bounds, form=self.form)


def weight_of(m):
    return COUNTS_W if LT.TERM[m.kind] == "pois" else GREY_W


def ref_step(cu, K, bounds, x, xi, dtype, form="div", tau=None):
    m = cu.m
    out = P.myula_step(cu.term(dtype), _Prior(weight_of(m), K, bounds, form), np.asarray(x, dtype=dtype), m.tau if tau is None else tau, m.gamma,
                       np.asarray(xi, dtype=dtype), dtype=dtype)
    assert out.dtype == np.dtype(dtype)
    return out


class Handle:
    """A sampler through the C ABI (lmc_myula_create / lmc_skrock_create on an lmc_problem with LMC_PRIOR_TGV)."""

    def __init__(self, cu, K, bounds, sampler="myula", noise="injected", seed=0, fields=None):
        from lmc_atomi_amd import _capi, _dev
        from lmc_atomi_amd.proximal import _Problem
        self.lib, self.dev, m = _dev.lib(), _dev, cu.m
        prior = {"prior_kind": _capi.PRIOR_TGV, "prior_sigma": weight_of(m), "tgv_niter": K, "tgv_alpha0": ALPHA0, "tgv_step": 0.0}
        if bounds is not None:
            prior["box"] = bounds
        self.prob = _Problem(m.shape, cu.desc, prior)
        for k, v in (fields or {}).items():
            setattr(self.prob.c, k, v)
        cfg = _capi.lmc_myula_config()
        cfg.struct_size = C.sizeof(_capi.lmc_myula_config)
        cfg.problem = self.prob.c
        cfg.n_chains, cfg.tau, cfg.gamma, cfg.epsg, cfg.seed, cfg.thin = C_, (m.tau if sampler != "skrock" else m.delta), m.gamma, 1.0, seed, 1
        cfg.noise_mode = _capi.NOISE_INJECTED if noise == "injected" else _capi.NOISE_PHILOX
        self.h = C.c_void_p()
        create = {"myula": lambda: self.lib.lmc_myula_create(C.byref(cfg), C.byref(self.h)),
                  "mymala": lambda: self.lib.lmc_mymala_create(C.byref(cfg), C.byref(self.h)),
                  "skrock": lambda: self.lib.lmc_skrock_create(C.byref(cfg), 3, S.ETA, C.byref(self.h))}[sampler]
        self.rc = create()
        self.msg = last_error() if self.rc else ""
        self.shape = (C_,) + m.shape

    def call(self, fn, *args):
        return getattr(self.lib, fn)(self.h, *args, self.dev.stream_ptr())

    def run(self, x, noise):
        import torch
        xt, nt = self.dev.to_dev(x), self.dev.to_dev(noise)
        assert self.call("lmc_sampler_set_state", self.dev.ptr(xt)) == 0, last_error()
        rc = self.call("lmc_sampler_step", 1, self.dev.ptr(nt))
        torch.cuda.synchronize()
        assert rc == 0, last_error()
        out = torch.empty(self.shape, dtype=torch.float32, device="cuda")
        assert self.call("lmc_sampler_get_state", self.dev.ptr(out)) == 0, last_error()
        torch.cuda.synchronize()
        return out.cpu().numpy()

    @property
    def kernel_name(self):
        return self.lib.lmc_sampler_kernel_name(self.h).decode()

    def close(self):
        if self.h.value:
            self.lib.lmc_sampler_destroy(self.h)
            self.h = C.c_void_p()


@pytest.mark.parametrize("data", DATA)
def test_one_myula_step_per_pixel(la, data):
    cu, bounds = setup_of(data)
    m, K = cu.m, iters_of("L+1")
    x0, xi = m.x0, m.noise[0]
    r64 = ref_step(cu, K, bounds, x0, xi, np.float64)
    e32, bound = T.bound_from(r64, ref_step(cu, K, bounds, x0, xi, np.float32), ref_step(cu, K, bounds, x0, xi, np.float32, "kernel"))
    h = Handle(cu, K, bounds)
    try:
        assert h.rc == 0, h.msg
        got = h.run(x0, xi[None])
        name = h.kernel_name
        import torch
        ft, gt = torch.empty(C_, dtype=torch.float64, device="cuda"), torch.full((C_,), 7.0, dtype=torch.float64, device="cuda")
        assert h.call("lmc_sampler_energies", h.dev.ptr(ft), h.dev.ptr(gt)) == 0, last_error()
        torch.cuda.synchronize()
        assert not gt.cpu().numpy().any(), "the value of the prior is not built: g = 0"
        f = ft.cpu().numpy()
    finally:
        h.close()
    if data not in ("psf15", "radon8"):      # (f of the lattice's own operators; the two operators of this file have no value helper there)
        assert np.allclose(f, LT.f_value(m, got), rtol=LT.ENERGY_RTOL, atol=0), "f at the new state"
    r = report(f"step {data} {m.shape} K={K} bounds={bounds} [{name}]", got, r64, bound, e32)
    assert r <= 1.0
    free = ref_step(cu, K, None, x0, xi, np.float64) if bounds else None
    if bounds:
        assert np.max(np.abs(free - r64)) > 10 * bound, "the case tells the box from no box"
    none = P.myula_step(cu.term(np.float64), type("I", (), {"prox": staticmethod(lambda x, t: x)})(), x0.astype(np.float64), m.tau, m.gamma,
                        xi.astype(np.float64), dtype=np.float64)
    assert np.max(np.abs(none - r64)) > 10 * bound, "the case tells the prior from none"


def test_one_skrock_iteration_of_three_stages(la):
    cu, _ = setup_of("blur5")
    m, K = cu.m, iters_of("L+1")
    x0, Z = m.x0, m.Z[0]

    def definition(dtype, form="div"):
        advance = lambda v, t: ref_step(cu, K, None, v, np.zeros_like(v), dtype, form, tau=t)       # noqa: E731
        return S.iteration_definition(advance, np.asarray(x0, dtype=dtype), np.asarray(Z, dtype=dtype), m.delta, 3, dtype)

    class Launch:
        dtype, gamma = np.dtype(np.float32), m.gamma
        pf, pg = cu.term(np.float32), _Prior(weight_of(m), K, None, "kernel")

        def grad(self, x):
            return self.pf.grad(x)

        def prox(self, x):
            return self.pg.prox(x, self.gamma)

        def launch(self, a, t, b, s, x, n):
            f = np.float32
            return f(a) * x - f(t) * self.grad(x) + f(b) * self.prox(x) + f(s) * n

    r64 = definition(np.float64)
    e32, bound = T.bound_from(r64, definition(np.float32), definition(np.float32, "kernel"), S.iteration_launch(Launch(), x0, Z, m.delta, 3))
    h = Handle(cu, K, None, sampler="skrock")
    try:
        assert h.rc == 0, h.msg
        got = h.run(x0, Z[None])
        name = h.kernel_name
    finally:
        h.close()
    assert report(f"SK-ROCK 3 stages blur5 {m.shape} K={K} [{name}]", got, r64, bound, e32) <= 1.0
    boxed = Handle(cu, K, (0.0, 255.0), sampler="skrock")
    assert boxed.rc == LMC_E_UNSUPPORTED and "box" in boxed.msg and not boxed.h.value, "SK-ROCK with the box stays refused"


def python_terms(la, shape, seed=0):
    rng = np.random.default_rng(100 * shape[0] + shape[1] + seed)
    h = X.f32(np.ones((5, 5)) / 25.0)
    img = X.step_image(shape, 190.0)
    y = X.f32(O.blur(img, h.astype(np.float64), (2, 2)) + rng.normal(0, X.SIGMA, shape))
    x0 = X.f32(img[None] + rng.normal(0, 10, (4,) + shape))
    pf = la.L2(Op=la.Convolve2D(shape, h, offset=(2, 2)), b=y, sigma=1 / X.SIGMA ** 2)
    return h, y, x0, pf


def test_five_step_philox_trajectory(la):
    shape, K, seed, off, sig = (33, 70), iters_of("L+1"), X.SEED_P, 4, 4.0          # prox parameter gamma * 4 = 2.25
    h, y, x0, pf = python_terms(la, shape)
    x0 = x0[:C_]
    pg = la.TGV(shape, sigma=sig, alpha0=ALPHA0, niter=K)
    with la.MYULASampler(pf, pg, shape, n_chains=C_, tau=X.TAU, gamma=X.GAMMA, seed=seed, chain_offset=off) as smp:
        smp.set_state(x0)
        smp.step(5)
        got = smp.get_state().cpu().numpy()
        f, g = smp.energies()
        assert not g.cpu().numpy().any()
    data = X._Data(P.Op("blur", h.astype(np.float64), (2, 2)), y, 1 / X.SIGMA ** 2, np.float64)
    x = x0.astype(np.float64)
    for it in range(5):
        xi = O.philox_normals(seed, it, off + np.arange(C_), *shape).astype(np.float64)
        x = P.myula_step(data, _Prior(sig, K, None, "div"), x, X.TAU, X.GAMMA, xi, dtype=np.float64)
    rel = X.rel(got, x)
    print(f"tgv five Philox steps {shape}: rel-L2 {rel:.2e} (limit {LT.REL_L2:.0e})")
    assert rel <= LT.REL_L2


def test_moments_over_a_sharded_and_an_unsharded_run_are_equal(la):
    shape, K = (16, 24), iters_of("L+1")
    h, y, x0, pf = python_terms(la, shape, seed=1)
    pg = la.TGV(shape, sigma=4.0, alpha0=ALPHA0, niter=K, bounds=(0.0, 255.0))
    kw = dict(tau=X.TAU, gamma=X.GAMMA, seed=11, moments=True, burn_in=1, thin=1)
    with la.MYULASampler(pf, pg, shape, n_chains=4, **kw) as whole:
        whole.set_state(x0)
        whole.step(4)
        ref = whole.get_state().cpu().numpy()
        s1, s2, cnt = whole.moments()
        s1, s2 = s1.cpu().numpy(), s2.cpu().numpy()
    parts = []
    for lo in (0, 2):
        with la.MYULASampler(pf, pg, shape, n_chains=2, chain_offset=lo, **kw) as part:
            part.set_state(np.ascontiguousarray(x0[lo:lo + 2]))
            part.step(4)
            assert np.array_equal(part.get_state().cpu().numpy(), ref[lo:lo + 2]), "a shard reproduces its chains bit for bit"
            a, b, c = part.moments()
            parts.append((a.cpu().numpy(), b.cpu().numpy(), c))
    assert cnt == parts[0][2] + parts[1][2] == 12
    assert np.allclose(parts[0][0] + parts[1][0], s1, rtol=1e-13, atol=0) and np.allclose(parts[0][1] + parts[1][1], s2, rtol=1e-13, atol=0)
    assert not np.array_equal(ref[0], ref[1])


def test_the_drivers_take_the_prior_with_every_accumulator_keyword(la):
    shape = (16, 24)
    h, y, x0, pf = python_terms(la, shape, seed=2)
    pg = la.TGV(shape, sigma=4.0, niter=iters_of("L+1"))
    probes = np.zeros((2,) + shape, dtype=np.float32)
    probes[0, :8], probes[1, 8:] = 1.0, 1.0
    res = la.MoreauYosidaUnadjustedLangevin(pf, pg, x0, tau=X.TAU, gamma=X.GAMMA, niter=6, seed=3, n_chains=4, burn_in=2, moment_scales=(2, 4), hist_bins=8,
                                            hist_range=(0.0, 255.0), chain_groups=2, cov_probes=probes, cov_center=y)
    assert res.mean.shape == shape and np.isfinite(res.mean.cpu().numpy()).all() and res.count == 16
    assert not res.energy_g.cpu().numpy().any() and res.energy_f.cpu().numpy().all()
    assert set(res.scale_mean) == {2, 4} and res.hist.shape[1:] == shape and res.mcse_mean.shape == shape and res.cov_sketch is not None
    sk = la.StabilisedLangevin(pf, pg, x0, tau=X.TAU, gamma=X.GAMMA, niter=2, n_stages=3, n_chains=4)
    assert sk.state.shape == (4,) + shape and np.isfinite(sk.state.cpu().numpy()).all()
    one = la.MoreauYosidaUnadjustedLangevin(pf, pg, x0[0], tau=X.TAU, gamma=X.GAMMA, niter=2)       # the reference form: every iterate of one chain
    assert one.shape == (2, shape[0] * shape[1]) and np.isfinite(one).all()


# ------------------------------------------------------------------ refusals
def test_python_refusals(la):
    shape = (16, 24)
    h, y, x0, pf = python_terms(la, shape)
    pg = la.TGV(shape, sigma=4.0)
    with pytest.raises(NotImplementedError, match="minimisation"):
        pg(x0)
    with pytest.raises(NotImplementedError, match="TGV"):
        la.MoreauYosidaMetropolisAdjustedLangevin(pf, pg, x0[0], tau=X.TAU, gamma=X.GAMMA, niter=2, n_chains=2)
    with pytest.raises(NotImplementedError, match="TGV"):
        la.UnadjustedLangevinPrimalDual(pf, pg, la.Gradient(shape), x0[0], tau=0.1, mu=0.1, niter=2, n_chains=2)
    with pytest.raises(NotImplementedError, match="TGV"):
        la.EstimatePriorWeight(pf, pg, x0[0], tau=X.TAU, gamma=X.GAMMA, n_updates=2, theta_bounds=(0.01, 10.0))
    with pytest.raises(NotImplementedError, match="TGV"):
        la.MYULASampler(pf, pg, shape, tau=X.TAU, gamma=X.GAMMA, epsg=np.ones(shape))
    with pytest.raises(NotImplementedError, match="bounds"):
        la.StabilisedLangevin(pf, la.TGV(shape, bounds=(0, 255)), x0[0], tau=X.TAU, gamma=X.GAMMA, niter=2, n_chains=2)
    with la.MYULASampler(pf, pg, shape, n_chains=2, tau=X.TAU, gamma=X.GAMMA) as smp:
        with pytest.raises(NotImplementedError, match="TGV"):
            smp.set_prior_weight(2.0)
        with pytest.raises(NotImplementedError, match="TGV"):
            smp.estimate_prior_weight(2, (0.01, 10.0))
    with pytest.raises(ValueError, match="operand of shape"):
        pg.prox(np.zeros((3, 5)), 1.0)


def test_c_abi_refusals(la):
    import torch
    from lmc_atomi_amd import _capi, _dev
    lib = _dev.lib()
    cu, _ = setup_of("blur5")
    K = iters_of("L+1")
    stream = _dev.stream_ptr(torch.device("cuda", torch.cuda.current_device()))

    def create(want, phrase, sampler="myula", bounds=None, **fields):
        h = Handle(cu, K, bounds, sampler=sampler, fields=fields)
        ok = h.rc == want and (want == 0 or (phrase.lower() in h.msg.lower() and not h.h.value))
        h.close()
        assert ok, (sampler, fields, h.rc, h.msg)

    create(0, "")
    create(0, "", bounds=(0.0, 255.0))
    create(0, "", tv_step=0.25)
    create(LMC_E_UNSUPPORTED, "LMC_PRIOR_TGV", sampler="mymala")
    create(LMC_E_UNSUPPORTED, "tv_rtol", tv_rtol=1e-4)
    create(LMC_E_UNSUPPORTED, "tv_warm", tv_warm=1)
    create(LMC_E_UNSUPPORTED, "tv_lagged_output", tv_lagged_output=1)
    scale = torch.ones(C_, dtype=torch.float32, device="cuda")
    create(LMC_E_UNSUPPORTED, "prox_scale", prox_scale=_dev.ptr(scale), prox_scale_chain_stride=1)
    create(LMC_E_UNSUPPORTED, "box", sampler="skrock", bounds=(0.0, 255.0))
    for bad in (dict(tv_niter=0), dict(tv_niter=257), dict(eprox_p0=0.0), dict(eprox_p0=-1.0), dict(eprox_p0=float("nan")), dict(eprox_p0=float("inf")),
                dict(tv_step=0.3), dict(tv_step=-0.1), dict(tv_step=float("nan"))):
        create(LMC_E_INVALID, "", **bad)
        assert last_error()
    # the handle-level and stateless entry points
    h = Handle(cu, K, None)
    try:
        assert h.rc == 0
        assert lib.lmc_sampler_set_prior_sigma(h.h, C.c_float(2.0)) == LMC_E_UNSUPPORTED and "LMC_PRIOR_TGV" in last_error()
        cfg = _capi.lmc_sapg_config()
        cfg.struct_size = C.sizeof(_capi.lmc_sapg_config)
        cfg.theta_min, cfg.theta0, cfg.theta_max, cfg.step_scale, cfg.step_exponent, cfg.n_updates, cfg.iters_per_update = 0.01, 1.0, 10.0, 10.0, 0.8, 2, 1
        trace = (C.c_double * 3)()
        assert lib.lmc_sampler_sapg(h.h, C.byref(cfg), None, trace, None, None, stream) == LMC_E_UNSUPPORTED and "LMC_PRIOR_TGV" in last_error()
        prob = h.prob
        x = torch.zeros((C_,) + cu.m.shape, dtype=torch.float32, device="cuda")
        f = torch.zeros(C_, dtype=torch.float64, device="cuda")
        assert lib.lmc_prior_statistic(C.byref(prob.c), _dev.ptr(x), C_, _dev.ptr(f), stream) == LMC_E_UNSUPPORTED and "LMC_PRIOR_TGV" in last_error()
        assert lib.lmc_sapg_dimension(C.byref(prob.c), None, None) == LMC_E_UNSUPPORTED and "LMC_PRIOR_TGV" in last_error()
        g = torch.full((C_,), 7.0, dtype=torch.float64, device="cuda")
        assert lib.lmc_energies(C.byref(prob.c), _dev.ptr(x), C_, _dev.ptr(f), _dev.ptr(g), stream) == 0, last_error()
        torch.cuda.synchronize()
        assert not g.cpu().numpy().any(), "lmc_energies reports g = 0"
        u = _capi.lmc_ulpda_config()
        u.struct_size = C.sizeof(_capi.lmc_ulpda_config)
        u.problem = prob.c
        u.n_chains, u.tau, u.mu, u.theta, u.cg_niter, u.thin = C_, 0.1, 0.1, 1.0, 5, 1
        hu = C.c_void_p()
        assert lib.lmc_ulpda_create(C.byref(u), C.byref(hu)) == LMC_E_UNSUPPORTED and "LMC_PRIOR_TGV" in last_error() and not hu.value
        mc = _capi.lmc_mch_config()
        mc.struct_size = C.sizeof(_capi.lmc_mch_config)
        mc.problem = prob.c
        mc.n_channels, mc.n_chains, mc.tau, mc.gamma, mc.epsg, mc.thin = 2, C_, 0.1, 0.5, 1.0, 1
        hm = C.c_void_p()
        assert lib.lmc_mch_create(C.byref(mc), C.byref(hm)) == LMC_E_UNSUPPORTED and "LMC_PRIOR_TGV" in last_error() and not hm.value
    finally:
        h.close()
    # lmc_fused_eval honours the prior: the prox alone (a = t = 0, b = 1) is lmc_tgv_prox bit for bit
    shape = cu.m.shape
    xs = T.images(shape)
    from lmc_atomi_amd.proximal import _Problem
    pr = _Problem(shape, prior={"prior_kind": _capi.PRIOR_TGV, "prior_sigma": 1.0, "tgv_niter": K, "tgv_alpha0": ALPHA0, "tgv_step": 0.0})
    assert np.array_equal(pr.eval(xs, 0.0, 0.0, 1.0, 2.5), raw_prox(xs, 2.5, ALPHA0, K)[0])
    # the stateless prox
    x3 = torch.zeros((2,) + shape, dtype=torch.float32, device="cuda")
    o3 = torch.empty_like(x3)
    prox = lambda **kw: lib.lmc_tgv_prox(_dev.ptr(kw.get("x", x3)), _dev.ptr(kw.get("out", o3)), None, kw.get("n", 2), shape[0], shape[1],       # noqa: E731
                                         C.c_float(kw.get("t", 1.0)), C.c_float(kw.get("a0", 2.0)), kw.get("K", 10), C.c_float(kw.get("step", 0.0)),
                                         kw.get("box", 0), C.c_float(kw.get("lo", 0.0)), C.c_float(kw.get("hi", 1.0)), stream)
    assert prox() == 0, last_error()
    for bad in (dict(t=-1.0), dict(t=float("nan")), dict(a0=0.0), dict(a0=float("inf")), dict(K=0), dict(K=257), dict(out=x3), dict(n=0), dict(step=0.3),
                dict(step=-1.0), dict(box=1, lo=1.0, hi=1.0), dict(box=1, lo=float("nan")), dict(box=2)):
        assert prox(**bad) == LMC_E_INVALID and last_error(), bad
    torch.cuda.synchronize()

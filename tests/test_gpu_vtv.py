"""GPU: the vectorial TV prior (LMC_PRIOR_VTV) and the multi-channel MYULA sampler against the float64 restatement of tests/_vtv_ref.py -- the prox through
VectorialTV.prox and through lmc_vtv_prox in both batch layouts, the value, one and five sampler steps, the Philox fields of the channels, sharding, the
energies, the driver and the refusals.

Bound for every array compared, per pixel over every image (tests/_pixel.bound_of, the project's rule):

    max |got - ref64| <= max(3 e32, 2 ulp32(max |ref64|))

e32: the larger of the deviations from float64 of the restatement's two float32 replays -- the definition's form, which divides by the root, and the
kernel's, which multiplies by the reciprocal root -- measured on the reference, never on a kernel.  Every case prints err / bound.  Values: rtol 1e-5
against float64 and equal bit for bit on a repeat."""
import ctypes as C

import numpy as np
import pytest

import _pixel as X
import _vtv_ref as V
from oracle import lmc_oracle as O

pytestmark = pytest.mark.gpu

LMC_E_INVALID, LMC_E_UNSUPPORTED = -1, -2
CASES = [(s, n) for s in V.SHAPES for n in V.CHANNELS]
IDS = [f"{s[0]}x{s[1]}-{n}ch" for s, n in CASES]
SIGMA_F, TAU, GAMMA = 1 / X.SIGMA ** 2, X.TAU, X.GAMMA
WEIGHT, NITER = 3.0, 10          # sigma of the prior in the sampler tests: prox parameter gamma * 3 = 1.69
C_ = 2


@pytest.fixture(scope="module")
def la():
    import torch
    assert torch.cuda.is_available()
    import lmc_atomi_amd as la
    return la


def last_error():
    from lmc_atomi_amd import _dev
    return _dev.lib().lmc_last_error().decode()


def report(tag, got, ref64, bound, e32):
    err = float(np.max(np.abs(np.asarray(got, dtype=np.float64) - ref64)))
    print(f"vtv {tag}: err {err:.3e} bound {bound:.3e} e32 {e32:.3e} err/bound {err / bound:.3f}")
    return err


def raw_prox(x_dev_layout, nch, n, shape, t, K, bounds=None, stride=None):
    """lmc_vtv_prox on a [nch, n, H, W] array; `stride`: a channel stride of its own (the array is then padded to it)."""
    import torch
    from lmc_atomi_amd import _dev
    cs = n * shape[0] * shape[1] if stride is None else stride
    buf = torch.full((nch, cs), 7.0, dtype=torch.float32, device="cuda")
    buf[:, :n * shape[0] * shape[1]] = torch.from_numpy(x_dev_layout.reshape(nch, -1)).cuda()
    out = torch.full_like(buf, -3.0)
    lo, hi = bounds if bounds is not None else (0.0, 0.0)
    rc = _dev.lib().lmc_vtv_prox(_dev.ptr(buf), _dev.ptr(out), n, nch, cs, shape[0], shape[1], C.c_float(t), K, C.c_float(0.125), None,
                                 1 if bounds is not None else 0, C.c_float(lo), C.c_float(hi), _dev.stream_ptr(buf.device))
    assert rc == 0, last_error()
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert np.all(o[:, n * shape[0] * shape[1]:] == -3.0), "nothing is written between the channels"
    return o[:, :n * shape[0] * shape[1]].reshape((nch, n) + shape)


def test_the_case_list_holds_the_seams():
    """More than one tile in both directions, and more than one chained launch: otherwise the list would hide the seams."""
    from lmc_atomi_amd import _capi
    tiles = lambda s, n, K: tuple(-(-d // t) for d, t in zip(s, _capi.vtv_plan(s, n, K)[:2]))
    assert any(min(tiles(s, n, K)) > 1 for s, n in CASES for K in V.ITERS)
    assert any(_capi.vtv_plan(s, n, K)[3] > 1 for s, n in CASES for K in V.ITERS)
    assert all(_capi.vtv_plan(s, n, K)[3] == 1 for s, n in CASES for K in V.ITERS if K <= 10)
    for n in V.CHANNELS:      # every channel count has both, at the largest shape
        assert min(tiles((97, 261), n, 10)) > 1 and _capi.vtv_plan((97, 261), n, 64)[3] > 1


@pytest.mark.parametrize("shape,nch", CASES, ids=IDS)
def test_prox_per_pixel(la, shape, nch):
    x = V.images(shape, nch)
    xd = V.to_device_layout(x)
    worst = 0.0
    for t in V.PROX_PARAMS:
        for K in V.ITERS:
            ref64, e32, bound = V.prox_reference(shape, nch, t, K)
            ref = V.to_device_layout(ref64)
            tag = f"{shape[0]}x{shape[1]}-{nch}ch t={t} K={K}"
            batch = la.VectorialTV(shape, nch, sigma=1.0, niter=K).prox(xd, t)
            assert batch.shape == xd.shape and batch.dtype == np.float32
            errs = [report(tag + " VectorialTV.prox", batch, ref, bound, e32)]
            errs.append(report(tag + " lmc_vtv_prox batch", raw_prox(xd, nch, V.N_IMAGES, shape, t, K), ref, bound, e32))
            errs.append(report(tag + " lmc_vtv_prox padded stride", raw_prox(xd, nch, V.N_IMAGES, shape, t, K, stride=V.N_IMAGES * shape[0] * shape[1] + 5),
                               ref, bound, e32))
            single = raw_prox(np.ascontiguousarray(xd[:, :1]), nch, 1, shape, t, K)
            errs.append(report(tag + " lmc_vtv_prox single", single, ref[:, :1], bound, e32))
            assert np.array_equal(single, batch[:, :1]), "an image's prox does not depend on its batch"
            one = la.VectorialTV(shape, nch, sigma=0.5, niter=K).prox(x[0], 2 * t)          # [nch, H, W], sigma * tau = t
            assert one.shape == (nch,) + shape and np.array_equal(one, batch[:, 0])
            flat = la.VectorialTV(shape, nch, niter=K).prox(xd.ravel(), t)
            assert flat.shape == (xd.size,) and np.array_equal(flat.reshape(xd.shape), batch)
            assert max(errs) <= bound, (tag, max(errs), bound)
            worst = max(worst, max(errs) / bound)
    print(f"vtv prox {shape[0]}x{shape[1]}-{nch}ch: worst err / bound {worst:.3f}")


@pytest.mark.parametrize("shape,nch", [((5, 7), 2), ((33, 70), 3), ((97, 261), 4)])
def test_zero_parameter_is_the_identity_and_a_repeat_is_bit_equal(la, shape, nch):
    xd = V.to_device_layout(V.images(shape, nch))
    for bounds in (None, (60.0, 170.0)):
        pg = la.VectorialTV(shape, nch, niter=10, bounds=bounds)
        assert np.array_equal(pg.prox(xd, 0.0), xd)
        assert np.array_equal(la.VectorialTV(shape, nch, sigma=0.0, niter=10, bounds=bounds).prox(xd, 3.0), xd)
    for K in (10, 23):
        pg = la.VectorialTV(shape, nch, niter=K)
        a, b = pg.prox(xd, 2.5), pg.prox(xd, 2.5)
        assert np.array_equal(a, b)
        assert np.array_equal(pg(xd), pg(xd))


@pytest.mark.parametrize("shape", V.SHAPES, ids=[f"{s[0]}x{s[1]}" for s in V.SHAPES])
def test_one_channel_agrees_with_the_isotropic_tv_prox(la, shape):
    """Both are within the bound of the same float64 reference (tests/test_vtv_reference.py: the restatements are equal bit for bit)."""
    xd = V.to_device_layout(V.images(shape, 1))
    for t, K in [(0.75, 1), (2.5, 10), (40.0, 23), (2.5, 64)]:
        ref64, e32, bound = V.prox_reference(shape, 1, t, K)
        got = la.VectorialTV(shape, 1, niter=K).prox(xd, t)
        tv = la.TV(shape, sigma=1.0, niter=K).prox(xd[0], t)
        d = float(np.max(np.abs(got[0].astype(np.float64) - tv)))
        print(f"vtv 1ch vs TV {shape} t={t} K={K}: {d:.3e} (2 x bound {2 * bound:.3e})")
        assert d <= 2 * bound
        assert report(f"TV.prox {shape} t={t} K={K}", tv, ref64[:, 0], bound, e32) <= bound


@pytest.mark.parametrize("shape,nch", [((5, 7), 3), ((33, 70), 2), ((64, 136), 4), ((97, 261), 3)])
@pytest.mark.parametrize("bounds", [(60.0, 170.0), (0.0, np.inf)], ids=["60-170", "positive"])
def test_bounds(la, shape, nch, bounds):
    xd = V.to_device_layout(V.images(shape, nch))
    for t, K in [(2.5, 10), (40.0, 23)]:
        ref64, e32, bound = V.prox_reference(shape, nch, t, K, bounds)
        got = la.VectorialTV(shape, nch, niter=K, bounds=bounds).prox(xd, t)
        assert report(f"box {bounds} {shape}-{nch}ch t={t} K={K}", got, V.to_device_layout(ref64), bound, e32) <= bound
        assert got.min() >= bounds[0] and got.max() <= bounds[1], "inside the box exactly"
        assert np.array_equal(got, raw_prox(xd, nch, V.N_IMAGES, shape, t, K, bounds=bounds))
    if bounds[1] < np.inf:
        free, _, _ = V.prox_reference(shape, nch, 2.5, 10)
        boxed, _, _ = V.prox_reference(shape, nch, 2.5, 10, bounds)
        assert np.max(np.abs(boxed - np.clip(free, *bounds))) > 0.1, "the case tells the constrained prox from a clip afterwards"


@pytest.mark.parametrize("shape,nch", CASES, ids=IDS)
def test_value(la, shape, nch):
    import torch
    from lmc_atomi_amd import _dev
    x = V.images(shape, nch)
    xd = V.to_device_layout(x)
    ref = V.vtv_value(x.astype(np.float64))
    pg = la.VectorialTV(shape, nch, sigma=0.3)
    got = pg(xd)
    print(f"vtv value {shape}-{nch}ch: rel {np.max(np.abs(got / (0.3 * ref) - 1)):.2e}")
    assert np.allclose(got, 0.3 * ref, rtol=1e-5, atol=0)
    assert np.array_equal(got, pg(xd))
    assert np.isclose(pg(x[0]), 0.3 * ref[0], rtol=1e-5, atol=0)
    xt = torch.from_numpy(xd).cuda()
    out = torch.zeros(V.N_IMAGES, dtype=torch.float64, device="cuda")
    rc = _dev.lib().lmc_vtv_value(_dev.ptr(xt), _dev.ptr(out), V.N_IMAGES, nch, xt[0].numel(), shape[0], shape[1], _dev.stream_ptr(xt.device))
    assert rc == 0, last_error()
    assert np.allclose(out.cpu().numpy(), ref, rtol=1e-5, atol=0), "unweighted"


# ------------------------------------------------------------------ the sampler
def _gauss7():
    t = np.exp(-0.5 * ((np.arange(7) - 3) / 1.5) ** 2)
    return np.outer(t, t) / np.sum(np.outer(t, t))


DATA = ["none", "identity", "box5", "gauss7", "mask", "bayer"]
STEP_SHAPES = [(16, 24), (33, 70), (40, 136), (24, 261)]
STEP_CASES = [(d, s, n) for d in DATA for s in STEP_SHAPES for n in (2, 3) if d != "bayer" or n == 3]


def bayer_masks(shape):
    i, j = np.indices(shape)
    r = (i % 2 == 0) & (j % 2 == 0)
    b = (i % 2 == 1) & (j % 2 == 1)
    return X.f32(np.stack([r, ~(r | b), b]))


def problem(data, shape, nch, seed=0):
    """float32 numbers made once: (h, offset, masks, y [nch, H, W] or None, x0 [nch, C, H, W], xi [5, nch, C, H, W])."""
    rng = np.random.default_rng(100 * shape[0] + shape[1] + 7 * nch + seed)
    h, off, masks = None, None, None
    if data == "box5":
        h, off = X.f32(np.ones((5, 5)) / 25.0), (2, 2)
    elif data == "gauss7":
        h, off = X.f32(_gauss7()), (3, 3)
    elif data == "mask":
        masks = X.f32(rng.uniform(size=shape) < 0.6)
    elif data == "bayer":
        masks = bayer_masks(shape)
    img = np.stack([X.step_image(shape, 190.0 - 40.0 * ch) for ch in range(nch)])
    y = None
    if data != "none":
        u = O.blur(img, h.astype(np.float64), off) if h is not None else (img * masks if masks is not None else img)
        noise = rng.normal(0, X.SIGMA, img.shape)
        y = X.f32(u + (noise * masks if masks is not None else noise))
    x0 = X.f32(img[:, None] + rng.normal(0, 10, (nch, C_) + shape))
    xi = X.f32(rng.standard_normal((5, nch, C_) + shape))
    return h, off, masks, y, x0, xi


def terms(la, data, shape, nch, h, off, masks, y):
    if data == "none":
        return None
    out = []
    for ch in range(nch):
        if h is not None:
            out.append(la.L2(Op=la.Convolve2D(shape, h, offset=off), b=y[ch], sigma=SIGMA_F))
        elif masks is not None:
            out.append(la.L2(Op=la.Diagonal(masks if masks.ndim == 2 else masks[ch], dims=shape), b=y[ch], sigma=SIGMA_F, dims=shape))
        else:
            out.append(la.L2(b=y[ch], sigma=SIGMA_F, dims=shape))
    return out


def ref_step(p, x, xi, dtype, bounds=None, form="div", niter=NITER):
    h, off, masks, y, _, _ = p
    c = lambda a: None if a is None else a.astype(dtype)
    return V.myula_step(np.asarray(x, dtype=dtype), c(y), c(h), off, c(masks), SIGMA_F, TAU, GAMMA, GAMMA * WEIGHT, niter, np.asarray(xi, dtype=dtype), bounds, form)


def step_bound(p, x, xi, bounds=None, niter=NITER):
    r64 = ref_step(p, x, xi, np.float64, bounds, niter=niter)
    e32, bound = V.bound_from(r64, ref_step(p, x, xi, np.float32, bounds, niter=niter), ref_step(p, x, xi, np.float32, bounds, "rsqrt", niter=niter))
    return r64, e32, bound


def sampler(la, data, shape, nch, p, niter=NITER, bounds=None, **kw):
    pg = la.VectorialTV(shape, nch, sigma=WEIGHT, niter=niter, bounds=bounds)
    return la.MultichannelMYULASampler(terms(la, data, shape, nch, *p[:4]), pg, shape, n_chains=kw.pop("n_chains", C_), tau=TAU, gamma=GAMMA, **kw)


@pytest.mark.parametrize("data,shape,nch", STEP_CASES, ids=[f"{d}-{s[0]}x{s[1]}-{n}ch" for d, s, n in STEP_CASES])
def test_one_step_with_injected_noise(la, data, shape, nch):
    p = problem(data, shape, nch)
    x0, xi = p[4], p[5]
    r64, e32, bound = step_bound(p, x0, xi[0])
    with sampler(la, data, shape, nch, p, noise="injected") as smp:
        assert smp.shape == (nch, C_) + shape
        smp.set_state(x0)
        smp.step(1, noise=xi[:1])
        got = smp.get_state().cpu().numpy()
        assert smp.iteration == 1
        name = smp.kernel_name
    assert name.startswith("vtv_prox_kernel + "), name
    err = report(f"step {data} {shape}-{nch}ch [{name}]", got, r64, bound, e32)
    assert err <= bound


def test_one_step_with_bounds_and_with_chained_prox_launches(la):
    for data, shape, nch, niter, bounds in [("box5", (33, 70), 3, 10, (0.0, 255.0)), ("box5", (40, 136), 2, 23, None), ("mask", (24, 261), 3, 23, (0.0, 255.0))]:
        p = problem(data, shape, nch, seed=1)
        x0, xi = p[4], p[5]
        r64, e32, bound = step_bound(p, x0, xi[0], bounds, niter)
        with sampler(la, data, shape, nch, p, niter=niter, bounds=bounds, noise="injected") as smp:
            smp.set_state(x0)
            smp.step(1, noise=xi[:1])
            got = smp.get_state().cpu().numpy()
            assert ("(box)" in smp.kernel_name) == (bounds is not None)
        assert report(f"step {data} {shape}-{nch}ch K={niter} bounds={bounds}", got, r64, bound, e32) <= bound


@pytest.mark.parametrize("data,shape,nch", [("box5", (16, 24), 3), ("bayer", (33, 70), 3), ("identity", (24, 261), 2)])
def test_five_steps_and_moments(la, data, shape, nch):
    p = problem(data, shape, nch, seed=2)
    x0, xi = p[4], p[5]
    x = x0.astype(np.float64)
    kept = []
    for it in range(5):
        x = ref_step(p, x, xi[it], np.float64)
        if it >= 1 and (it - 1) % 2 == 0:
            kept.append(x)
    with sampler(la, data, shape, nch, p, noise="injected", moments=True, burn_in=1, thin=2) as smp:
        smp.set_state(x0)
        smp.step(5, noise=xi)
        got = smp.get_state().cpu().numpy()
        s1, s2, cnt = smp.moments()
        rel = X.rel(got, x)
        print(f"five steps {data} {shape}-{nch}ch: rel-L2 {rel:.2e}")
        assert rel <= 1e-5
        assert cnt == len(kept) * C_ == 4
        k = np.stack(kept)                       # [kept, nch, C, H, W]
        assert s1.shape == (nch,) + shape
        # per channel, relative in the l2 norm like the state (the project's rule for moments, tests/_pixel.rel): a pixel whose kept iterates cancel has
        # no relative error of its own -- the float32 states it sums are spaced 1.5e-5 apart at 255
        for ch in range(nch):
            r1, r2 = X.rel(s1[ch].cpu().numpy(), k[:, ch].sum(axis=(0, 1))), X.rel(s2[ch].cpu().numpy(), (k[:, ch] ** 2).sum(axis=(0, 1)))
            print(f"moments {data} {shape} channel {ch}: rel {r1:.2e} {r2:.2e}")
            assert r1 <= 1e-5 and r2 <= 1e-5
        smp.reset_moments()
        s1, s2, cnt = smp.moments()
        assert cnt == 0 and not s1.any() and not s2.any()


def test_philox_fields_and_a_philox_step(la):
    data, shape, nch, seed, off = "box5", (33, 70), 3, X.SEED_P, 4
    p = problem(data, shape, nch, seed=3)
    x0 = p[4]
    with sampler(la, data, shape, nch, p, seed=seed, chain_offset=off) as smp:
        fields = {}
        for it in (0, 7):
            f = smp.noise_field(it).cpu().numpy()
            fields[it] = f
            for ch in range(nch):
                ref = O.philox_normals((seed + (ch << 32)) % (1 << 64), it, off + np.arange(C_), *shape)
                err = float(np.max(np.abs(f[ch].astype(np.float64) - ref)))
                print(f"philox channel {ch} iteration {it}: err {err:.2e}")
                assert err <= X.NOISE_TOL
            for a in range(nch):
                for b in range(a + 1, nch):
                    assert not np.array_equal(f[a], f[b])
        grey = la.MYULASampler(la.L2(b=p[3][0], sigma=SIGMA_F, dims=shape), la.TV(shape, 0.3), shape, n_chains=C_, tau=TAU, gamma=GAMMA, seed=seed, chain_offset=off)
        with grey:
            for it in (0, 7):
                assert np.array_equal(grey.noise_field(it).cpu().numpy(), fields[it][0]), "channel 0 is the grey sampler's field"
        smp.set_state(x0)
        smp.iteration = 7
        smp.step(1)
        got = smp.get_state().cpu().numpy()
    xi = np.stack([O.philox_normals((seed + (ch << 32)) % (1 << 64), 7, off + np.arange(C_), *shape) for ch in range(nch)])
    r64, e32, bound = step_bound(p, x0, xi)
    bound += float(np.sqrt(np.float32(2.0 * TAU))) * X.NOISE_TOL          # the rule of tests/_pixel.philox_bound_of
    assert report("philox step", got, r64, bound, e32) <= bound


def test_sharding_reproduces_the_chains(la):
    data, shape, nch = "gauss7", (16, 24), 3
    p = problem(data, shape, nch, seed=4)
    rng = np.random.default_rng(9)
    x0 = X.f32(p[4][:, :1] + rng.normal(0, 5, (nch, 5) + shape))
    with sampler(la, data, shape, nch, p, n_chains=5, seed=11) as whole:
        whole.set_state(x0)
        whole.step(3)
        ref = whole.get_state().cpu().numpy()
    with sampler(la, data, shape, nch, p, n_chains=2, seed=11, chain_offset=3) as part:
        part.set_state(np.ascontiguousarray(x0[:, 3:5]))
        part.step(3)
        got = part.get_state().cpu().numpy()
    assert np.array_equal(got, ref[:, 3:5])
    assert not np.array_equal(ref[:, 0], ref[:, 1])


@pytest.mark.parametrize("data,shape,nch", [("none", (16, 24), 2), ("box5", (33, 70), 3), ("bayer", (40, 136), 3), ("identity", (24, 261), 2), ("mask", (97, 261), 2)])
def test_energies(la, data, shape, nch):
    p = problem(data, shape, nch, seed=5)
    h, off, masks, y, x0, _ = p
    with sampler(la, data, shape, nch, p) as smp:
        smp.set_state(x0)
        f, g = (a.cpu().numpy() for a in smp.energies())
    f_ref = V.data_value(x0, y, h, off, masks, SIGMA_F)
    g_ref = WEIGHT * V.vtv_value(np.moveaxis(x0.astype(np.float64), 0, 1))
    print(f"energies {data} {shape}-{nch}ch: f {f} g {g}")
    assert np.allclose(f, f_ref, rtol=1e-5, atol=0) and np.allclose(g, g_ref, rtol=1e-5, atol=0)


def test_the_driver_routes_to_the_sampler(la):
    data, shape, nch, n = "box5", (16, 24), 3, 6
    p = problem(data, shape, nch, seed=6)
    pf = terms(la, data, shape, nch, *p[:4])
    pg = la.VectorialTV(shape, nch, sigma=WEIGHT, niter=NITER)
    res = la.MoreauYosidaUnadjustedLangevin(pf, pg, p[4], tau=TAU, gamma=GAMMA, niter=n, seed=5, n_chains=C_, burn_in=2, thin=2)
    assert res.mean.shape == res.var.shape == (nch,) + shape and res.state.shape == (nch, C_) + shape
    assert res.energy_f.shape == res.energy_g.shape == (C_,) and res.count == 2 * C_
    with la.MultichannelMYULASampler(pf, pg, shape, n_chains=C_, tau=TAU, gamma=GAMMA, seed=5, moments=True, burn_in=2, thin=2) as smp:
        smp.set_state(p[4])
        smp.step(n)
        s1, s2, cnt = smp.moments()
        assert np.array_equal(res.state.cpu().numpy(), smp.get_state().cpu().numpy())
        mean, var = la.mean_var_from_moments(s1, s2, cnt)
    assert np.array_equal(res.mean.cpu().numpy(), mean.cpu().numpy()) and np.array_equal(res.var.cpu().numpy(), var.cpu().numpy())
    one = la.MoreauYosidaUnadjustedLangevin(pf, pg, p[4][:, 0], tau=TAU, gamma=GAMMA, niter=2, n_chains=C_)      # x0 [nch, H, W]: every chain starts there
    assert one.state.shape == (nch, C_) + shape


def mch_config(la, shape, nch, data_desc=None, **fields):
    """(problem, config) of a valid multi-channel sampler with `fields` written over the problem or, where the config has a field of that name, over it."""
    import torch
    from lmc_atomi_amd import _capi
    from lmc_atomi_amd.proximal import _Problem
    y = torch.zeros((nch,) + shape, dtype=torch.float32, device="cuda")
    prob = _Problem(shape, data_desc or {"data_kind": _capi.DATA_IDENTITY, "sigma_f": 1.0}, la.VectorialTV(shape, nch, sigma=0.5).prior_descriptor(),
                    options={"multichannel": True})
    prob._keep.append(y)
    prob.c.y_dev = y.data_ptr()
    cfg = _capi.lmc_mch_config()
    cfg.struct_size = C.sizeof(_capi.lmc_mch_config)
    cfg.n_channels, cfg.n_chains, cfg.tau, cfg.gamma, cfg.epsg, cfg.thin = nch, 2, 0.1, 0.5, 1.0, 1
    for k, v in fields.items():
        setattr(cfg if k in dict(_capi.lmc_mch_config._fields_) and k != "problem" else prob.c, k, v)
    cfg.problem = prob.c
    return prob, cfg


def test_c_abi_refusals(la):
    import torch
    from lmc_atomi_amd import _capi, _dev
    lib = _dev.lib()
    shape, nch = (16, 24), 3
    stream = _dev.stream_ptr(torch.device("cuda", torch.cuda.current_device()))
    scale = torch.ones(2, dtype=torch.float32, device="cuda")

    def create(want, **fields):
        prob, cfg = mch_config(la, shape, nch, **fields)
        hnd = C.c_void_p()
        rc = lib.lmc_mch_create(C.byref(cfg), C.byref(hnd))
        msg = last_error()
        if rc == 0:
            lib.lmc_mch_destroy(hnd)
        assert rc == want and (rc == 0 or (msg and not hnd.value)), (fields, rc, msg)

    create(0)
    create(0, mask_channel_stride=shape[0] * shape[1])
    for kind in (4, 7, 9, 12, 13, 16, 19):
        create(LMC_E_UNSUPPORTED, data_kind=kind)
    create(LMC_E_UNSUPPORTED, ncvx_kind=_capi.NCVX_MC_TV, ncvx_gamma=1.0)
    create(LMC_E_UNSUPPORTED, tv_rtol=1e-4)
    create(LMC_E_UNSUPPORTED, tv_warm=1)
    create(LMC_E_UNSUPPORTED, prox_scale=_dev.ptr(scale), prox_scale_chain_stride=1)
    create(LMC_E_UNSUPPORTED, tv_lagged_output=1)
    for bad in (dict(n_channels=0), dict(n_channels=5), dict(tv_niter=0), dict(tv_niter=65), dict(box_enable=1, box_lo=1.0, box_hi=1.0),
                dict(box_enable=1, box_lo=float("nan"), box_hi=1.0), dict(box_enable=2, box_lo=0.0, box_hi=1.0), dict(mask_channel_stride=5),
                dict(prior_kind=_capi.PRIOR_TV_ISO), dict(n_chains=0), dict(tau=0.0), dict(struct_size=8), dict(data_kind=99)):
        create(LMC_E_INVALID, **bad)
    # LMC_PRIOR_VTV handed to the entry points for single-plane images
    prob, _ = mch_config(la, shape, nch)
    x = torch.zeros((2,) + shape, dtype=torch.float32, device="cuda")
    out = torch.empty_like(x)
    f = torch.zeros(2, dtype=torch.float64, device="cuda")
    m = _capi.lmc_myula_config()
    m.struct_size = C.sizeof(_capi.lmc_myula_config)
    m.problem = prob.c
    m.n_chains, m.tau, m.gamma, m.epsg, m.thin = 2, 0.1, 0.5, 1.0, 1
    for fn in (lambda h: lib.lmc_myula_create(C.byref(m), C.byref(h)), lambda h: lib.lmc_mymala_create(C.byref(m), C.byref(h)),
               lambda h: lib.lmc_skrock_create(C.byref(m), 3, 0.05, C.byref(h))):
        hnd = C.c_void_p()
        assert fn(hnd) == LMC_E_UNSUPPORTED and "LMC_PRIOR_VTV" in last_error() and not hnd.value
    assert lib.lmc_fused_eval(C.byref(prob.c), _dev.ptr(x), _dev.ptr(out), 2, 0.0, 0.0, 1.0, 1.0, stream) == LMC_E_UNSUPPORTED and "LMC_PRIOR_VTV" in last_error()
    assert lib.lmc_energies(C.byref(prob.c), _dev.ptr(x), 2, _dev.ptr(f), _dev.ptr(f), stream) == LMC_E_UNSUPPORTED and "LMC_PRIOR_VTV" in last_error()
    # (the statistic and its dimension read the prior kinds with a value alone: their range check, LMC_E_INVALID, is held by tests/test_wavelet_api.py)
    assert lib.lmc_prior_statistic(C.byref(prob.c), _dev.ptr(x), 2, _dev.ptr(f), stream) == LMC_E_INVALID and last_error()
    assert lib.lmc_sapg_dimension(C.byref(prob.c), None, None) == LMC_E_INVALID and last_error()
    # the stateless calls
    x3 = torch.zeros((nch, 2) + shape, dtype=torch.float32, device="cuda")
    o3 = torch.empty_like(x3)
    cs = 2 * shape[0] * shape[1]
    prox = lambda **kw: lib.lmc_vtv_prox(_dev.ptr(kw.get("x", x3)), _dev.ptr(kw.get("out", o3)), kw.get("n", 2), kw.get("nch", nch), kw.get("cs", cs), shape[0], shape[1],
                                         C.c_float(kw.get("t", 1.0)), kw.get("K", 10), C.c_float(0.125), None, kw.get("box", 0), C.c_float(kw.get("lo", 0.0)),
                                         C.c_float(kw.get("hi", 1.0)), stream)
    assert prox() == 0, last_error()
    for bad in (dict(t=-1.0), dict(t=float("nan")), dict(nch=0), dict(nch=5), dict(K=0), dict(K=65), dict(out=x3), dict(n=0), dict(cs=cs - 1),
                dict(box=1, lo=1.0, hi=1.0), dict(box=1, lo=float("nan")), dict(box=2)):
        assert prox(**bad) == LMC_E_INVALID and last_error(), bad
    g = torch.zeros(2, dtype=torch.float64, device="cuda")
    assert lib.lmc_vtv_value(_dev.ptr(x3), _dev.ptr(g), 2, nch, cs, shape[0], shape[1], stream) == 0
    assert lib.lmc_vtv_value(_dev.ptr(x3), _dev.ptr(g), 2, 5, cs, shape[0], shape[1], stream) == LMC_E_INVALID
    assert lib.lmc_vtv_value(_dev.ptr(x3), _dev.ptr(g), 2, nch, cs - 1, shape[0], shape[1], stream) == LMC_E_INVALID
    torch.cuda.synchronize()


def test_python_refusals(la):
    shape, nch = (16, 24), 3
    pg = la.VectorialTV(shape, nch)
    p = problem("identity", shape, nch)
    pf = terms(la, "identity", shape, nch, *p[:4])
    x0 = p[4][:, 0]
    run = lambda **kw: la.MoreauYosidaUnadjustedLangevin(pf, pg, x0, tau=TAU, gamma=GAMMA, n_chains=2, **kw)
    for kw in ({"moment_scales": (2,)}, {"hist_bins": 8}, {"hist_range": (0, 1)}, {"chain_groups": 2}, {"cov_probes": np.zeros((1,) + shape)},
               {"cov_center": np.zeros(shape)}, {"quantiles": (0.5,)}, {"callback": lambda x: None}):
        with pytest.raises(NotImplementedError, match=next(iter(kw))):
            run(**kw)
    one = la.VectorialTV(shape, 1)
    f1 = la.L2(b=p[3][0], sigma=SIGMA_F, dims=shape)
    x1 = x0[0]
    with pytest.raises(NotImplementedError):
        la.MYULASampler(f1, one, shape, tau=TAU, gamma=GAMMA)
    with pytest.raises(NotImplementedError):
        la.MoreauYosidaMetropolisAdjustedLangevin(f1, one, x1, tau=TAU, gamma=GAMMA, niter=2, n_chains=2)
    with pytest.raises(NotImplementedError):
        la.StabilisedLangevin(f1, one, x1, tau=TAU, gamma=GAMMA, niter=2, n_chains=2)
    with pytest.raises(NotImplementedError):
        la.UnadjustedLangevinPrimalDual(f1, one, la.Gradient(shape), x1, tau=0.1, mu=0.1, niter=2, n_chains=2)
    with pytest.raises(NotImplementedError):
        la.EstimatePriorWeight(f1, one, x1, tau=TAU, gamma=GAMMA, n_updates=2, theta_bounds=(0.01, 10.0))
    with pytest.raises(NotImplementedError):
        la.MultichannelMYULASampler([la.Poisson(la.Identity(shape[0] * shape[1]), np.ones(shape), np.ones(shape), dims=shape)] * nch, pg, shape, tau=TAU, gamma=GAMMA)

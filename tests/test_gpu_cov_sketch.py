"""Covariance sketch on the device (lmc_cov_sketch / lmc_sampler_set_cov_sketch / lmc_sampler_get_cov_sketch): Y = sum t d, s = sum t, Q = sum t t^T of
the kept samples, d = x - m (fp32), t = P d.

Exact: integer-valued inputs whose partial sums of |terms| stay below 2^24 are summed without rounding by fp32 and float64 alike, in any order, so the
device must give the float64 reference bit for bit -- at shapes, chain counts and probe counts off every tile of the kernels.
Rounding: on float data the yardstick is the fp32 restatement of the arithmetic contract (tests/_cov_sketch_ref.py); the device may be 3 times as far
from the float64 reference as the restatement is, the margin tests/_pixel.py gives the step kernels.
Samplers: the handle's accumulators equal, bit for bit, the stateless pass over the kept states -- one owner per element and ordered launches."""
import functools

import numpy as np
import pytest

from tests import _cov_sketch_ref as R
from tests import test_gpu_block_moments as BM

pytestmark = pytest.mark.gpu

TAU, GAMMA = BM.TAU, BM.GAMMA
E_INVALID, E_STATE = -1, -5
FACTOR = 3.0
EXACT = 2.0 ** 24


@pytest.fixture(scope="module")
def la():
    import torch
    assert torch.cuda.is_available()
    import lmc_atomi_amd as la
    return la


def host(ts):
    return tuple(t.cpu().numpy() for t in ts)


# ------------------------------------------------------------------ exact
@functools.lru_cache(maxsize=None)
def integer_case(shape, C_, k):
    """three iterates x [3][C, H, W], probes [k, H, W] in {-1, 0, 1}, centre [H, W]: integers, m non-zero, x - m in {-3 .. 3}.  With k >= 3 the first
    three probes are the edge content: one pixel at the first pixel, one at the last, and one that is non-zero only in the last partial slab."""
    rng = np.random.default_rng(1000 * shape[1] + 10 * C_ + k)
    N = shape[0] * shape[1]
    m = rng.integers(90, 111, size=shape).astype(np.float32)
    xs = [(m[None] + rng.integers(-3, 4, size=(C_,) + shape)).astype(np.float32) for _ in range(3)]
    P = rng.integers(-1, 2, size=(k, N)).astype(np.float32)
    if k >= 3:
        P[:3] = 0
        P[0, 0] = 1
        P[1, N - 1] = -1
        last = ((N - 1) // R.PIXEL_RUN) * R.PIXEL_RUN
        P[2, last:] = rng.choice([-1.0, 1.0], size=N - last)
    return xs, P.reshape((k,) + shape), m


@pytest.mark.parametrize("k", [1, 3, 16, 32])
@pytest.mark.parametrize("C_", [1, 5, 33, 70])
@pytest.mark.parametrize("shape", [(20, 23), (24, 40), (72, 136)])
def test_integer_data_give_the_reference_bit_for_bit(la, shape, C_, k):
    import torch
    xs, P, m = integer_case(shape, C_, k)
    assert (m != 0).all() and set(np.unique(P)) <= {-1.0, 0.0, 1.0}
    want = None
    for x in xs:
        d = R.centred(x, m).astype(np.float64)
        assert np.abs(d).max() <= 3 and (d == np.round(d)).all()
        Pa = np.abs(P.reshape(k, -1).astype(np.float64))
        t = d @ P.reshape(k, -1).astype(np.float64).T
        assert (np.abs(d) @ Pa.T).max() < EXACT, "a projection's sum of |terms| reaches 2^24"
        assert (np.abs(t).T @ np.abs(d)).max() < EXACT, "a Y entry's sum of |terms| reaches 2^24"
        assert np.abs(t).max() < EXACT
        ref = R.sketch_ref(x, P, m)
        want = ref if want is None else tuple(a + b for a, b in zip(want, ref))
    out = None
    for x in xs:
        out = la.cov_sketch(torch.from_numpy(x).cuda(), P, m, out=out)
    Y, s, Q = host(out)
    assert Y.dtype == np.float64 and Y.shape == (k,) + shape and s.shape == (k,) and Q.shape == (k, k)
    np.testing.assert_array_equal(Y.reshape(k, -1), want[0])
    np.testing.assert_array_equal(s, want[1])
    np.testing.assert_array_equal(Q, want[2])


def test_a_misaligned_view_and_no_centre_give_the_same_exact_sums(la):
    """(24, 40) takes the float4 loads; a view 4 bytes past a 16-byte boundary takes the scalar loads.  Both must be exact.  center=None: x itself is the
    operand, integers near 100, so the bound is checked for those."""
    import torch
    shape, C_, k = (24, 40), 5, 3
    xs, P, m = integer_case(shape, C_, k)
    x = xs[0]
    buf = torch.zeros(x.size + 4, dtype=torch.float32, device="cuda")
    view = buf[1:1 + x.size].view((C_,) + shape)
    view.copy_(torch.from_numpy(x))
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    ref = R.sketch_ref(x, P, m)
    for got in (la.cov_sketch(view, P, m), la.cov_sketch(torch.from_numpy(x).cuda(), P, m)):
        for g, r in zip(host(got), ref):
            np.testing.assert_array_equal(g.reshape(r.shape), r)
    d = x.reshape(C_, -1).astype(np.float64)
    t = d @ P.reshape(k, -1).astype(np.float64).T
    assert (np.abs(d) @ np.abs(P.reshape(k, -1)).T.astype(np.float64)).max() < EXACT and (np.abs(t).T @ np.abs(d)).max() < EXACT
    ref0 = R.sketch_ref(x, P, None)
    for g, r in zip(host(la.cov_sketch(view, P)), ref0):
        np.testing.assert_array_equal(g.reshape(r.shape), r)


# ------------------------------------------------------------------ rounding
ROUND_SHAPE, ROUND_C, ROUND_K = (72, 136), 70, 32


@functools.lru_cache(maxsize=None)
def float_case(centre):
    """x = 100 + 5 N(0, 1), Gaussian probes; the centre is the fp32 mean over the chains, or None"""
    rng = np.random.default_rng(2024)
    x = (100.0 + 5.0 * rng.standard_normal((ROUND_C,) + ROUND_SHAPE)).astype(np.float32)
    P = rng.standard_normal((ROUND_K,) + ROUND_SHAPE).astype(np.float32)
    m = x.mean(axis=0, dtype=np.float64).astype(np.float32) if centre else None
    ref = R.sketch_ref(x, P, m)
    e32 = R.max_abs_errors(R.sketch_fp32(x, P, m), ref)
    return x, P, m, ref, e32


@pytest.mark.parametrize("centre", [True, False], ids=["centre=mean", "centre=None"])
def test_float_data_round_like_the_fp32_restatement(la, centre):
    import torch
    x, P, m, ref, e32 = float_case(centre)
    xd = torch.from_numpy(x).cuda()
    got = host(la.cov_sketch(xd, P, m))
    err = R.max_abs_errors(got, ref)
    for name, e, y, r in zip("YsQ", err, e32, ref):
        print(f"cov sketch rounding centre={'mean' if centre else 'None'} {name}: err {e:.3e}  fp32 restatement {y:.3e}  ratio {e / y:.3f}  max |ref| {np.abs(r).max():.3e}")
    again = host(la.cov_sketch(xd, P, m))                      # reproducible: equal bits
    for a, b in zip(got, again):
        np.testing.assert_array_equal(a, b)
    # what the missing centre costs cov_xt: the same host arithmetic on the device's sums and on the float64 sums
    s1 = x.astype(np.float64).sum(axis=0)
    have = la.cov_from_sketch(*got, ROUND_C, s1, m).cov_xt
    want = la.cov_from_sketch(ref[0].reshape(got[0].shape), ref[1], ref[2], ROUND_C, s1, m).cov_xt
    print(f"cov sketch rounding centre={'mean' if centre else 'None'} cov_xt: max err {np.abs(have - want).max():.3e} of max |cov_xt| {np.abs(want).max():.3e}"
          f" (relative {np.abs(have - want).max() / np.abs(want).max():.3e})")
    for name, e, y in zip("YsQ", err, e32):
        assert y > 0 and e <= FACTOR * y, (name, e, y)


# ------------------------------------------------------------------ samplers
BURN, THIN, NIT = 2, 3, 9          # kept: the iterations 2, 5, 8 counted from 0
TILE_SHAPE, PIPE_SHAPE = (3, 5), (6, 132)       # the smallest tile-kernel shape and the smallest shape wider than 128 of tests/_pixel.py


def sampler_case(la, kind, C_):
    """-> (make(**extra) -> sampler, x0, shape, step sizes of the calls, kernel the sampler must report or None, takes a policy)"""
    rng = np.random.default_rng(7)
    calls, kernel, policy = [1] * NIT, None, False
    if kind in ("myula_tile", "myula_pipe"):
        shape = TILE_SHAPE if kind == "myula_tile" else PIPE_SHAPE
        y, pf, pg = BM.blur_problem(la, shape, rng, "tv", level=100.0)
        make = lambda **kw: la.MYULASampler(pf, pg, shape, n_chains=C_, tau=TAU, gamma=GAMMA, seed=5, variant=kind[6:], **kw)
        kernel, policy = kind[6:], True
    elif kind == "myula_pair":
        # two iterations per launch: every call is a pair launch and a single one, and its last iterate is the kept one (2, 5, 8)
        shape = (40, 64)
        y, pf, pg = BM.blur_problem(la, shape, rng, "l2", level=100.0)
        make = lambda policy=None, **kw: la.MYULASampler(pf, pg, shape, n_chains=C_, tau=TAU, gamma=GAMMA, seed=5,
                                                         policy=dict(policy or {}, iterations_per_launch=2), **kw)
        calls, kernel, policy = [3, 3, 3], "rows", True
    elif kind == "mymala":
        shape = (24, 96)
        img = np.zeros(shape)
        img[6:12, 24:72] = 150.0
        img += np.linspace(0, 30, shape[1])[None, :]
        pf = la.L2(Op=la.Convolve2D(shape, np.ones((5, 5)) / 25.0, offset=(2, 2)), b=img + rng.normal(0, BM.SIGMA, shape), sigma=1 / BM.SIGMA ** 2)
        pg = la.TV(shape, sigma=0.3, niter=5)
        make = lambda **kw: la.MYMALASampler(pf, pg, shape, n_chains=C_, tau=0.0003 * GAMMA, gamma=GAMMA, seed=9, **kw)
        return make, np.broadcast_to(img.astype(np.float32), (C_,) + shape).copy(), shape, calls, None, False
    elif kind == "skrock":
        shape = (16, 136)
        y, pf, pg = BM.blur_problem(la, shape, rng, "tv", level=100.0)
        make = lambda **kw: la.SKROCKSampler(pf, pg, shape, n_stages=3, n_chains=C_, tau=TAU, gamma=GAMMA, seed=5, **kw)
    else:
        shape = (16, 40)
        y, pf, _ = BM.blur_problem(la, shape, rng, level=100.0)
        make = lambda **kw: la.ULPDASampler(pf, la.L21(sigma=0.3), la.Gradient(shape), shape, n_chains=C_, tau=0.95 * GAMMA, mu=1.0, theta=1.0,
                                            gfirst=False, seed=3, **kw)
    x0 = (100.0 + rng.normal(0, 1.0, (C_,) + shape)).astype(np.float32)
    return make, x0, shape, calls, kernel, policy


def run(smp, x0, calls, on_kept=None):
    """steps `smp` by `calls`; on_kept(state) after every call whose last iteration is a kept one.  -> (moments, sketch or None, final state, kernel name)"""
    try:
        smp.set_state(x0)
        done = 0
        for n in calls:
            smp.step(n)
            done += n
            it = done - 1
            if on_kept is not None and it >= BURN and (it - BURN) % THIN == 0:
                on_kept(smp.get_state())
        s1, s2, cnt = smp.moments()
        sk = None
        if smp.cov_k is not None:
            Y, s, Q, n = smp.cov_sketch()
            sk = host((Y, s, Q)) + (n,)
        return host((s1, s2)) + (cnt,), sk, smp.get_state().cpu().numpy(), smp.kernel_name
    finally:
        smp.close()


@pytest.mark.parametrize("kind", ["myula_tile", "myula_pipe", "myula_pair", "skrock", "mymala", "ulpda"])
def test_sampler_sketch_equals_the_stateless_pass_over_its_kept_states(la, kind):
    C_, k = 5, 3
    make, x0, shape, calls, kernel, policy = sampler_case(la, kind, C_)
    rng = np.random.default_rng(11)
    P = rng.standard_normal((k,) + shape).astype(np.float32)
    m = (100.0 + rng.normal(0, 0.5, shape)).astype(np.float32)
    kw = dict(moments=True, burn_in=BURN, thin=THIN)
    acc = [None]

    def on_kept(state):
        acc[0] = la.cov_sketch(state, P, m, out=acc[0])

    mom, sk, final, name = run(make(cov_probes=P, cov_center=m, **kw), x0, calls, on_kept)
    if kernel:
        assert kernel in name, name
    assert sk[3] == mom[2] == 3 * C_
    want = host(acc[0])
    assert np.abs(want[0]).max() > 0
    for g, w in zip(sk[:3], want):
        np.testing.assert_array_equal(g, w)
    # the same run without the sketch: the pixel moments (hence mean and var) keep their bits
    plain, none, final0, _ = run(make(**kw), x0, calls)
    assert none is None
    np.testing.assert_array_equal(final0, final)
    for a, b in zip(plain[:2], mom[:2]):
        np.testing.assert_array_equal(a, b)
    mean_var = lambda mo: la.mean_var_from_moments(mo[0], mo[1], mo[2])
    for a, b in zip(mean_var(plain), mean_var(mom)):
        np.testing.assert_array_equal(a, b)
    # the whole run in as few calls as the launches allow, reductions beside the step kernels and in line: equal bits
    whole = calls if kind == "myula_pair" else [NIT]
    for pol in ([{"moments_overlap": 1}, {"moments_overlap": -1}] if policy else [None]):
        extra = {"policy": pol} if pol else {}
        mom2, sk2, final2, _ = run(make(cov_probes=P, cov_center=m, **kw, **extra), x0, whole)
        np.testing.assert_array_equal(final2, final)
        assert sk2[3] == sk[3]
        for a, b in zip(sk2[:3] + mom2[:2], sk[:3] + mom[:2]):
            np.testing.assert_array_equal(a, b)


def test_pair_launches_that_keep_the_iterate_in_between_give_equal_bits_on_both_streams(la):
    """thin = 1 under two iterations per launch: the first iterate of every pair is kept too -- beside the next launch it is reduced out of an array of its
    own.  No step(1) replay reproduces these states, so the two routes are compared with each other; s = sum t ties the sketch to the pixel moments of
    the same handle: with one probe of ones and no centre, s is the sum of s1 over the pixels up to the roundings of both."""
    C_ = 5
    make, x0, shape, _, kernel, _ = sampler_case(la, "myula_pair", C_)
    P = np.ones((1,) + shape, dtype=np.float32)
    out = []
    for ov in (1, -1):
        mom, sk, final, name = run(make(policy={"moments_overlap": ov}, cov_probes=P, moments=True, burn_in=1, thin=1), x0, [10])
        assert "rows_pair" in name, name
        assert sk[3] == mom[2] == 9 * C_
        total = mom[0].sum()
        assert abs(sk[1][0] - total) <= 2048 * 2.0 ** -24 * abs(total), (sk[1][0], total)      # fp32 runs of 2048 positive terms: n u relative at worst
        out.append(sk[:3] + mom[:2] + (final,))
    for a, b in zip(*out):
        np.testing.assert_array_equal(a, b)


def test_reset_refusals_switching_off_and_a_sapg_call(la):
    import torch
    shape = (16, 32)
    rng = np.random.default_rng(41)
    y, pf, pg = BM.blur_problem(la, shape, rng, level=100.0)
    lib = la._dev.lib()
    p = la._dev.ptr

    def refused(rc, code):
        assert rc == code, (rc, code)
        assert lib.lmc_last_error(), "lmc_last_error() is empty"

    k = 2
    P = rng.standard_normal((k,) + shape).astype(np.float32)
    m = np.full(shape, 100.0, dtype=np.float32)
    Pd, md = torch.from_numpy(P).cuda(), torch.from_numpy(m).cuda()
    big = torch.zeros((33,) + shape, dtype=torch.float32, device="cuda")
    kw = dict(n_chains=3, tau=TAU, gamma=GAMMA, seed=1)
    smp = la.MYULASampler(pf, pg, shape, moments=True, **kw)
    off = la.MYULASampler(pf, pg, shape, **kw)
    try:
        smp.set_state(np.full(shape, 100.0, dtype=np.float32))
        refused(lib.lmc_sampler_get_cov_sketch(smp._h, None, None, None, None, None), E_INVALID)      # get without set
        with pytest.raises(ValueError):
            smp.cov_sketch()
        refused(lib.lmc_sampler_set_cov_sketch(smp._h, 33, p(big), None), E_INVALID)
        refused(lib.lmc_sampler_set_cov_sketch(smp._h, -1, p(Pd), None), E_INVALID)
        refused(lib.lmc_sampler_set_cov_sketch(smp._h, k, None, p(md)), E_INVALID)                    # NULL probes
        refused(lib.lmc_sampler_set_cov_sketch(off._h, k, p(Pd), p(md)), E_STATE)                     # moments = 0
        x3 = torch.zeros((3,) + shape, dtype=torch.float32, device="cuda")
        outs = [torch.zeros(n, dtype=torch.float64, device="cuda") for n in (33 * shape[0] * shape[1], 33, 33 * 33)]
        ws = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
        assert lib.lmc_cov_sketch_workspace_bytes(3, *shape, 33) == 0 and 0 < lib.lmc_cov_sketch_workspace_bytes(3, *shape, 32) <= ws.numel()
        refused(lib.lmc_cov_sketch(p(x3), 3, *shape, 33, p(big), None, p(outs[0]), p(outs[1]), p(outs[2]), p(ws), None), E_INVALID)
        refused(lib.lmc_cov_sketch(p(x3), 3, *shape, 2, None, None, p(outs[0]), p(outs[1]), p(outs[2]), p(ws), None), E_INVALID)
        assert lib.lmc_sampler_set_cov_sketch(smp._h, k, p(Pd), p(md)) == 0
        smp.cov_k, smp.cov_probes, smp.cov_center = k, Pd, md
        Pd.zero_()                                                                                     # the handle keeps copies of its own
        md.zero_()
        assert lib.lmc_sampler_get_cov_sketch(smp._h, None, None, None, None, None) == 0              # every output is nullable
        smp.step(2)
        kept = [smp.get_state()]
        Y, s, Q, n = smp.cov_sketch()
        assert n == 6 == smp.moments()[2] and bool(Y.abs().max() > 0)
        refused(lib.lmc_sampler_set_cov_sketch(smp._h, k, p(Pd), None), E_STATE)                      # after a kept sample
        refused(lib.lmc_sampler_set_cov_sketch(smp._h, 0, None, None), E_STATE)
        smp.reset_moments()
        Y, s, Q, n = smp.cov_sketch()
        assert n == 0 and not Y.any() and not s.any() and not Q.any()
        smp.step(1)
        want = la.cov_sketch(smp.get_state(), P, m)
        before = host(smp.cov_sketch()[:3])
        for g, w in zip(before, host(want)):
            np.testing.assert_array_equal(g, w)
        # lmc_sampler_sapg: the accumulators take nothing while the weight moves
        w0, it0 = smp.prior_weight, smp.iteration
        smp.estimate_prior_weight(4, (1e-3, 1e2), theta0=0.3, warmup=2, iters_per_update=2)
        assert smp.iteration == it0 + 2 + 4 * 2 and smp.prior_weight != w0
        Y, s, Q, n = smp.cov_sketch()
        assert n == 3 == smp.moments()[2]
        for g, w in zip(host((Y, s, Q)), before):
            np.testing.assert_array_equal(g, w)
        smp.step(1)                                                                                    # and they take samples again afterwards
        assert smp.cov_sketch()[3] == 6
        smp.reset_moments()
        assert lib.lmc_sampler_set_cov_sketch(smp._h, 0, None, None) == 0                              # off again
        refused(lib.lmc_sampler_get_cov_sketch(smp._h, None, None, None, None, None), E_INVALID)
        smp.cov_k = None
        with pytest.raises(ValueError):
            smp.cov_sketch()
        smp.step(1)                                                                                    # and the sampler goes on without it
        assert smp.moments()[2] == 3
    finally:
        smp.close()
        off.close()


def test_end_to_end_region_fluxes_of_a_deconvolution(la):
    """32 x 48, 64 chains, blur + TV, two rectangles as probes about the observation as centre: cov_tt of the result is the covariance matrix of the two
    region sums over the kept states, which the callback gathers.  The yardstick is the fp32 restatement on the same states: it may be FACTOR times
    closer to the float64 covariance than the device."""
    shape, C_, burn, thin, niter = (32, 48), 64, 5, 2, 25
    rng = np.random.default_rng(3)
    y, pf, pg = BM.blur_problem(la, shape, rng, "tv", level=100.0)
    P = np.zeros((2,) + shape, dtype=np.float32)
    P[0, 4:12, 6:20] = 1.0
    P[1, 10:30, 16:40] = 1.0           # overlaps the first
    m = y.astype(np.float32)
    x0 = (100.0 + rng.normal(0, 1.0, (C_,) + shape)).astype(np.float32)
    kept, seen = [], [0]

    def gather(state):
        it = seen[0]
        seen[0] += 1
        if it >= burn and (it - burn) % thin == 0:
            kept.append(state.cpu().numpy().copy())

    res = la.MoreauYosidaUnadjustedLangevin(pf, pg, x0, tau=TAU, gamma=GAMMA, niter=niter, seed=11, n_chains=C_, burn_in=burn, thin=thin, dims=shape,
                                            callback=gather, cov_probes=P, cov_center=m)
    cs = res.cov_sketch
    assert len(kept) == 10 and cs.n == res.count == 10 * C_
    assert cs.cov_xt.shape == (2,) + shape and cs.cov_tt.shape == (2, 2) and cs.t_mean.shape == (2,)
    X = np.concatenate(kept).reshape(cs.n, -1)
    sums = X.astype(np.float64) @ P.reshape(2, -1).astype(np.float64).T
    want = np.cov(sums.T, bias=True)
    s1 = X.astype(np.float64).sum(axis=0)
    r32 = R.sketch_fp32(X, P, m)
    e32 = np.abs(la.cov_from_sketch(r32[0], r32[1], r32[2], cs.n, s1, m).cov_tt - want).max()
    err = np.abs(cs.cov_tt - want).max()
    print(f"cov sketch end to end: cov_tt {cs.cov_tt.tolist()} np.cov {want.tolist()} err {err:.3e} fp32 restatement {e32:.3e} ratio {err / e32:.3f}")
    assert e32 > 0 and err <= FACTOR * e32
    assert want[0, 0] > 0 and want[1, 1] > 0
    # the correlation of a region with its own pixels is positive on average, and the map is in [-1, 1]
    corr = cs.corr(res.var.cpu().numpy())
    assert np.isfinite(corr).all() and np.abs(corr).max() <= 1 + 1e-6 and corr[0][P[0] > 0].mean() > 0
    plain = la.MoreauYosidaUnadjustedLangevin(pf, pg, x0[:4], tau=TAU, gamma=GAMMA, niter=2, seed=11, n_chains=4, dims=shape)
    assert plain.cov_sketch is None


def test_the_other_entry_points_return_the_sketch(la):
    shape = (16, 64)
    rng = np.random.default_rng(5)
    y, pf, pg = BM.blur_problem(la, shape, rng)
    P = la.random_probes(4, shape, seed=1)
    kw = dict(cov_probes=P, cov_center=y)

    def shown(res, n):
        cs = res.cov_sketch
        assert cs.n == n == res.count and cs.cov_xt.shape == (4,) + shape and np.isfinite(cs.cov_xt).all()
        assert (np.diag(cs.cov_tt) > 0).all()

    shown(la.UnadjustedLangevinPrimalDual(pf, la.L21(sigma=0.3), la.Gradient(shape), y.ravel(), 0.95 * GAMMA, 1.0, niter=5, seed=2, gfirst=False,
                                          n_chains=4, burn_in=1, **kw), 16)
    shown(la.MoreauYosidaMetropolisAdjustedLangevin(pf, pg, y.ravel(), tau=0.01 * GAMMA, gamma=GAMMA, niter=5, seed=2, n_chains=4, burn_in=1, **kw), 16)
    shown(la.StabilisedLangevin(pf, pg, y.ravel(), tau=TAU, gamma=GAMMA, niter=5, n_stages=3, seed=2, n_chains=4, burn_in=1, **kw), 16)

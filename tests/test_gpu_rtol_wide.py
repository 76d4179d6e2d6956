"""The per-chain early exit of the TV prox (pyproximal.TV's rtol = 1e-4, decided on the device: DESIGN 3.0r) on every width the fixed-count pipeline
covers: rows that are not 16-byte aligned (the last image column anywhere inside a lane) and images wider than 512 columns (column strips of
480 written columns with recomputed halos; a chain is then several workgroups that add their share of every objective).  The reference's second
image, `einstein`, is 667 x 877: two strips, unaligned rows.

Built like tests/test_gpu_rtol.py: the same image generator, the same checker (oracle.lmc_oracle_c.tv_prox_fgp(..., rtol=1e-4, return_passes=True)),
the same tolerances.  The pass every chain leaves in is compared for EVERY chain; that is a fair demand only when no chain sits on the threshold, so
each case first computes, on the CPU in float64, the smallest |rel_j - rtol| / rtol over all chains and tested passes and asserts that it is >= 1e-3
(the device's objective is fp32 per lane and row folded into fp64: its relative error is orders below that)."""
import numpy as np
import pytest

from oracle import lmc_oracle as O
from oracle import lmc_oracle_c as OC

pytestmark = pytest.mark.gpu

SIGMA = 0.75
GAMMA, TAU = SIGMA ** 2, 0.2 * SIGMA ** 2
RTOL = 1e-4
MIN_MARGIN = 1e-3
STRIP = 480           # columns a strip writes at 8 pixels per lane: 512 - 2 x 16


def rel(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


@pytest.fixture(scope="module")
def la():
    import torch
    assert torch.cuda.is_available()
    import lmc_atomi_amd as la
    return la


def images(shape, n, seed):
    """n images that leave a 10-pass prox in different passes: flat / piecewise constant / textured at several noise levels (tests/test_gpu_rtol.py)"""
    rng = np.random.default_rng(seed)
    base = np.zeros(shape)
    base[shape[0] // 5:shape[0] // 2, shape[1] // 6:2 * shape[1] // 3] = 160.0
    base[shape[0] // 2:, shape[1] // 2:] = 70.0
    base += np.linspace(0, 25, shape[1])[None, :]
    out = np.empty((n,) + shape)
    for c in range(n):
        out[c] = base * (0.2 + 0.4 * (c % 4)) + rng.normal(0, [0.05, 0.6, 3.0, 12.0, 40.0][c % 5], shape)
    out[0] = 0.0            # x0 = 0 (prox_lmc_deconv.py:135): every objective is zero, the prox runs out of passes
    return out


def exit_margins(x, gam, niter, rtol=RTOL):
    """The checker's loop (oracle/lmc_oracle.py: tv_prox_fgp, float64) image by image, keeping the relative change of the objective at every pass
    that is tested: -> (pass each image leaves in, smallest |rel_j - rtol| / rtol over all images and tested passes)."""
    betas = O.fgp_betas(niter, "unlocbox")
    passes, margin = [], np.inf
    for img in np.asarray(x, dtype=np.float64):
        rr = np.zeros_like(img); ss = np.zeros_like(img); p = np.zeros_like(img); q = np.zeros_like(img)
        c, prev, left = 0.125 / gam, None, niter
        for k in range(niter):
            sol = img - gam * O.div2d(rr, ss)
            obj = 0.5 * float(np.sum((img - sol) ** 2)) + gam * float(O.tv_value(sol))
            if prev is not None and obj > 0:
                r_ = abs(obj - prev) / obj
                margin = min(margin, abs(r_ - rtol) / rtol)
                if r_ < rtol:
                    left = k
                    break
            prev = obj
            dr, dc = O.grad2d(sol)
            r = rr - c * dr
            s = ss - c * dc
            w = np.maximum(1.0, np.sqrt(r * r + s * s))
            pn, qn = r / w, s / w
            rr = pn + betas[k] * (pn - p)
            ss = qn + betas[k] * (qn - q)
            p, q = pn, qn
        passes.append(left)
    return np.array(passes, dtype=np.int32), margin


def check_margin(x, gam, K, passes):
    mine, margin = exit_margins(x, gam, K)
    print(f"exit passes {passes.tolist()} smallest margin {margin:.3g}")
    np.testing.assert_array_equal(mine, passes)            # the helper above IS the checker's loop
    assert margin >= MIN_MARGIN, margin


def prox_twice(la, x, shape, K, gam):
    """The prox alone through a sampler, twice (test_gpu_rtol.py): -> the checker's prox and passes; asserts iterates, passes and re-run counts."""
    n = x.shape[0]
    pg = la.TV(shape, sigma=gam / GAMMA, niter=K, rtol=RTOL)
    smp = la.MYULASampler(None, pg, shape, n_chains=n, tau=TAU, gamma=GAMMA, noise="none")
    ref, passes = OC.tv_prox_fgp(x, gam, K, rtol=RTOL, return_passes=True)
    check_margin(x, gam, K, passes)
    want = (1 - TAU / GAMMA) * x + (TAU / GAMMA) * ref
    got = None
    for call in range(2):
        smp.set_state(x)
        smp.step(1)
        assert "per-chain exit" in smp.kernel_name, smp.kernel_name
        got = smp.get_state().cpu().numpy()
        ps, reruns = smp.tv_exit_stats("prior")
        print(f"call {call}: device passes {ps.cpu().numpy().tolist()} reruns {list(reruns)} worst rel-L2 {max(rel(got[c], want[c]) for c in range(n)):.3g}")
        np.testing.assert_array_equal(ps.cpu().numpy(), passes)
        for c in range(n):
            assert rel(got[c], want[c]) < 2e-6, (call, c, rel(got[c], want[c]))
        assert reruns[3] == 0
        if call == 0:
            first = list(reruns)
            assert first[0] == int(np.sum(passes < K)) and first[1] == 0 and first[2] == 0      # the chains that left early ran again with their count, once
        else:
            assert list(reruns) == first                                      # nothing to repeat: every prediction held
    smp.close()
    return pg, ref, passes, got, want


# two unaligned strips, two aligned strips, three strips, four strips, one unaligned strip above / below 256 columns; caps 10 and 7; gam 0.17 and 2.0
@pytest.mark.parametrize("shape,K,gam", [((20, 877), 10, 0.17), ((24, 520), 10, 0.17), ((18, 1100), 10, 0.17), ((19, 1544), 10, 0.17), ((26, 301), 10, 0.17),
                                         ((21, 877), 10, 2.0), ((22, 667), 7, 0.17), ((27, 203), 10, 0.17), ((27, 203), 7, 0.17)])
def test_prox_and_exit_pass_equal_the_checkers_chain_by_chain(la, shape, K, gam):
    n = 10
    x = images(shape, n, K)
    pg, ref, passes, _, _ = prox_twice(la, x, shape, K, gam)
    assert len(set(passes.tolist())) >= 3, passes
    # the stateless prox (lmc_fused_eval) takes the same path
    px = pg.prox(x[3].ravel(), GAMMA).reshape(shape)
    assert rel(px, ref[3]) < 2e-6


# Column-wise error of ONE prox evaluation against the float64 checker.  tests/test_gpu_wide.py allows 2e-3 after three fused iterations with noise.  The bound
# here comes from the device path that exists since round 3 at H x 512 (one strip, aligned rows: kernels this change does not touch), the first case below: it shows
# 2.9e-5 on these images (values up to ~290: one fp32 ulp there is 3e-5); 1e-4 is that with room for other columns' rounding, and nothing at the seams or in
# the last columns may stand out against the rest of the image.
COL_BOUND = 1e-4


@pytest.mark.parametrize("shape", [(24, 512), (20, 877), (24, 520), (18, 1100), (19, 1544)])
def test_nothing_at_the_strip_seams(la, shape):
    n = 10
    x = images(shape, n, 10)
    x[:, :, -3:] += 40.0                                   # structure right at the last columns
    x[0] = 0.0
    _, _, _, got, want = prox_twice(la, x, shape, 10, 0.17)
    colerr = np.abs(got - want).max(axis=(0, 1))
    W = shape[1]
    near = np.zeros(W, dtype=bool)
    for b in range(STRIP, W, STRIP):
        near[max(b - 3, 0):b + 3] = True
    near[-4:] = True
    print(f"W = {W}: column-wise max error {colerr.max():.3g} at column {int(colerr.argmax())}; at seams / last columns {colerr[near].max():.3g}, "
          f"elsewhere {colerr[~near].max():.3g}")
    assert colerr.max() < COL_BOUND, (int(colerr.argmax()), float(colerr.max()))
    assert colerr[near].max() <= 2.0 * colerr[~near].max(), (colerr[near].max(), colerr[~near].max())


@pytest.mark.parametrize("edge", [480, 481])
@pytest.mark.parametrize("W", [877, 1100])
def test_step_edge_on_a_strip_boundary(la, W, edge):
    """Images with a step exactly on the first strip boundary (between columns 479 | 480, and 480 | 481): a halo counted twice or a difference
    dropped at the seam moves the objective by a relative amount far above 1e-4 there, and the chains would leave in other passes."""
    shape, n = (20, W), 10
    rng = np.random.default_rng(edge)
    x = np.empty((n,) + shape)
    for c in range(n):
        x[c] = rng.normal(0, [0.05, 0.6, 3.0, 12.0, 40.0][c % 5], shape)
        x[c, :, edge:] += 40.0 * (1 + c % 4)
    _, _, passes, _, _ = prox_twice(la, x, shape, 10, 0.17)
    assert len(set(passes.tolist())) >= 3, passes


@pytest.mark.parametrize("shape,k", [((24, 877), 5), ((22, 877), 7), ((26, 301), 5), ((25, 301), 7)])
def test_fused_step_with_the_exit_follows_the_checker_over_iterations(la, shape, k):
    """The whole MYULA update with the exit inside the fused launch (blur gradient, injected noise), 8 iterations: states against the checker's
    rtol branch; the pass-by-pass path (exit_path='passes') gives the same states and the same pass counts."""
    rng = np.random.default_rng(k)
    img = images(shape, 2, 1)[1]
    h = np.ones((k, k)) / (k * k)
    y = O.blur(img, h, (k // 2, k // 2)) + rng.normal(0, SIGMA, shape)
    C_, nit = 5, 8
    x0 = img[None] + rng.normal(0, 8, (C_,) + shape)
    x0[0] = 0.0
    noise = rng.standard_normal((nit, C_) + shape)
    pf = la.L2(Op=la.Convolve2D(shape, h, offset=(k // 2, k // 2)), b=y, sigma=1 / SIGMA ** 2)
    outs = {}
    for path in ("device", "passes"):
        smp = la.MYULASampler(pf, la.TV(shape, sigma=0.3, niter=10, rtol=RTOL, exit_path=path), shape, n_chains=C_, tau=TAU, gamma=GAMMA, noise="injected")
        smp.set_state(x0)
        smp.step(nit, noise=noise)
        outs[path] = smp.get_state().cpu().numpy()
        if path == "device":
            assert "per-chain exit" in smp.kernel_name, smp.kernel_name
            ps, reruns = smp.tv_exit_stats()
            assert reruns[3] == 0
        else:
            assert "per-chain exit" not in smp.kernel_name
        smp.close()
    pri = {"kind": "tv", "sigma": 0.3, "niter": 10, "t": GAMMA, "rtol": RTOL}
    x = x0.copy()
    last = np.zeros(C_, dtype=np.int32)
    for i in range(nit):
        x = OC.myula_step(x, y, h, (k // 2, k // 2), 1 / SIGMA ** 2, TAU, GAMMA, pri, noise[i], passes=last)
    print(f"device vs checker {rel(outs['device'], x):.3g}, device vs passes {rel(outs['device'], outs['passes']):.3g}, passes {last.tolist()}")
    assert rel(outs["device"], x) < 5e-5, rel(outs["device"], x)
    assert rel(outs["device"], outs["passes"]) < 3e-6, rel(outs["device"], outs["passes"])
    np.testing.assert_array_equal(ps.cpu().numpy(), last)            # the passes of the last iteration


@pytest.mark.parametrize("shape", [(24, 877), (20, 520)])
@pytest.mark.parametrize("niter", [14, 20, 50])
def test_chained_inner_prox_leaves_where_the_checkers_does(la, shape, niter):
    """The chained inner prox of the ME-TV term (links of 10 that hand the dual state over in HBM, across strips): through the gradient of the term
    against the checker's rtol branch (1e-4), the pass counts through a sampler."""
    n = 6
    x = images(shape, n, niter)[:n] + 40.0
    rng = np.random.default_rng(niter)
    h = np.ones((5, 5)) / 25.0
    y = O.blur(x[1], h, (2, 2)) + rng.normal(0, SIGMA, shape)
    lam, gam = 0.3, 15.0
    me = la.L2_ncvx_tv(dims=shape, Op=la.Convolve2D(shape, h, offset=(2, 2)), b=y.ravel(), sigma=1 / SIGMA ** 2, lamda=lam, gamma=gam, isotropic=True,
                       niter=niter, rtol=RTOL)
    got = me.grad(x.reshape(n, -1)).reshape((n,) + shape)
    prox, passes = OC.tv_prox_fgp(x, gam, niter, rtol=RTOL, return_passes=True)
    check_margin(x, gam, niter, passes)
    for c in range(n):
        gl2 = (1 / SIGMA ** 2) * O.blur_adjoint(O.blur(x[c], h, (2, 2)) - y, h, (2, 2))
        want = gl2 - lam * (x[c] - prox[c]) / gam
        assert rel(got[c], want) < 1e-4, (c, passes[c], rel(got[c], want))
    smp = la.MYULASampler(me, None, shape, n_chains=n, tau=TAU, gamma=GAMMA, noise="none")
    smp.set_state(x)
    smp.step(1)
    ps, reruns = smp.tv_exit_stats("ncvx")
    print(f"device passes {ps.cpu().numpy().tolist()} reruns {list(reruns)}")
    np.testing.assert_array_equal(ps.cpu().numpy(), passes)
    assert reruns[3] == 0
    smp.close()


def test_myula_with_the_me_tv_term_on_a_wide_image(la):
    """MYULA whose data term carries the ME-TV term with rtol = 1e-4 (models M3 / M6 / M9) and the TV prior with rtol = 1e-4, 24 x 877, injected noise."""
    shape = (24, 877)
    rng = np.random.default_rng(3)
    img = images(shape, 2, 1)[1]
    h = np.ones((5, 5)) / 25.0
    y = O.blur(img, h, (2, 2)) + rng.normal(0, SIGMA, shape)
    C_, nit = 2, 2
    x0 = img[None] + rng.normal(0, 8, (C_,) + shape)
    noise = rng.standard_normal((nit, C_) + shape)
    kw = dict(dims=shape, b=y.ravel(), sigma=1 / SIGMA ** 2, lamda=0.3, gamma=15.0, isotropic=True, niter=50)
    pf = la.L2_ncvx_tv(Op=la.Convolve2D(shape, h, offset=(2, 2)), rtol=RTOL, **kw)
    smp = la.MYULASampler(pf, la.TV(shape, sigma=0.3, niter=10, rtol=RTOL), shape, n_chains=C_, tau=TAU, gamma=GAMMA, noise="injected")
    smp.set_state(x0)
    smp.step(nit, noise=noise)
    assert "per-chain exit" in smp.kernel_name, smp.kernel_name
    got = smp.get_state().cpu().numpy()
    for which in ("prior", "ncvx"):
        assert smp.tv_exit_stats(which)[1][3] == 0
    smp.close()
    opf = O.L2NcvxTV(Op=O.Convolve2D(shape, h, (2, 2)), tv_kwargs={"rtol": RTOL}, **kw)
    otv = O.TV(shape, sigma=0.3, niter=10, rtol=RTOL)
    ref = np.stack([O.myula(opf, otv, x0[c].ravel(), TAU, GAMMA, niter=nit, noise=[noise[i, c].ravel() for i in range(nit)])[-1].reshape(shape)
                    for c in range(C_)])
    assert rel(got, ref) < 1e-4, rel(got, ref)


def test_ulpda_with_the_me_tv_term_on_a_wide_image(la):
    """ULPDA with the ME-TV term as the reference configures it (tests/test_gpu_rtol.py's case at 20 x 877)."""
    shape = (20, 877)
    rng = np.random.default_rng(21)
    img = np.zeros(shape); img[5:16, 20:700] = 170.0
    img += np.linspace(0, 30, shape[1])[None, :]
    h = np.ones((5, 5)) / 25
    y = O.blur(img, h, (2, 2)) + rng.normal(0, SIGMA, shape)
    n = shape[0] * shape[1]
    nit = 4
    tau0, mu0 = 0.95 * SIGMA ** 2, 0.99 / (0.95 * SIGMA ** 2 * 8)
    kw = dict(dims=shape, b=y.ravel(), sigma=1 / SIGMA ** 2, lamda=0.3, gamma=15.0, isotropic=True, niter=50)
    pf = la.L2_ncvx_tv(Op=la.Convolve2D(shape, h, offset=(2, 2)), warm=True, rtol=RTOL, **kw)
    of = O.L2NcvxTV(Op=O.Convolve2D(shape, h, (2, 2)), tv_kwargs={"rtol": RTOL}, **kw)
    xs = la.UnadjustedLangevinPrimalDual(pf, la.L21(ndim=2, sigma=0.3), la.Gradient(shape), tau=tau0, mu=mu0, theta=1.0, x0=np.zeros(n), gfirst=False,
                                         niter=nit, seed=4, rng="pcg64")
    ref = O.ulpda(of, O.L21(ndim=2, sigma=0.3), O.Gradient(shape), np.zeros(n), tau0, mu0, theta=1.0, niter=nit, seed=4, gfirst=False)
    assert rel(xs, ref) < 2e-4, rel(xs, ref)


def test_a_step_is_one_launch_as_at_512_columns(la):
    """With event timing on, a steady-state step() call of the sampler at H x 877 reports what the same sampler reports at H x 512 (the device path that
    exists since round 3): one fused launch per iteration, nothing per pass."""
    counts = {}
    for W in (512, 877):
        shape = (32, W)
        rng = np.random.default_rng(W)
        img = images(shape, 2, 1)[1]
        h = np.ones((5, 5)) / 25.0
        y = O.blur(img, h, (2, 2)) + rng.normal(0, SIGMA, shape)
        pf = la.L2(Op=la.Convolve2D(shape, h, offset=(2, 2)), b=y, sigma=1 / SIGMA ** 2)
        smp = la.MYULASampler(pf, la.TV(shape, sigma=0.3, niter=10, rtol=RTOL), shape, n_chains=4, tau=TAU, gamma=GAMMA, seed=1)
        smp.step(6)
        smp.enable_timing(True)
        smp.step(3)
        ms, counts[W] = smp.last_step_timing()
        assert "per-chain exit" in smp.kernel_name, (W, smp.kernel_name)
        assert ms > 0
        smp.close()
    assert counts[877] == counts[512] == 3, counts


def test_the_reference_image_size_once(la):
    """667 x 877 (`einstein`), 3 chains, 5 x 5 blur + TV(niter = 10, rtol = 1e-4), 4 iterations with Philox noise; one chain replayed by the checker."""
    shape = (667, 877)
    rng = np.random.default_rng(0)
    img = images(shape, 2, 1)[1]
    h = np.ones((5, 5)) / 25.0
    y = O.blur(img, h, (2, 2)) + rng.normal(0, SIGMA, shape)
    C_, nit, seed, cho = 3, 4, 11, 2
    pf = la.L2(Op=la.Convolve2D(shape, h, offset=(2, 2)), b=y, sigma=1 / SIGMA ** 2)
    smp = la.MYULASampler(pf, la.TV(shape, sigma=0.3, niter=10, rtol=RTOL), shape, n_chains=C_, tau=TAU, gamma=GAMMA, seed=seed, chain_offset=cho)
    smp.step(nit)
    assert "per-chain exit" in smp.kernel_name, smp.kernel_name
    got = smp.get_state().cpu().numpy()
    ps, reruns = smp.tv_exit_stats()
    assert reruns[3] == 0
    smp.close()
    c = 1
    pri = {"kind": "tv", "sigma": 0.3, "niter": 10, "t": GAMMA, "rtol": RTOL}
    x = np.zeros((1,) + shape)
    last = np.zeros(1, dtype=np.int32)
    for i in range(nit):
        xi = O.philox_normals(seed, i, np.arange(cho + c, cho + c + 1), *shape).astype(np.float64)
        x = OC.myula_step(x, y, h, (2, 2), 1 / SIGMA ** 2, TAU, GAMMA, pri, xi, passes=last)
    print(f"chain {c}: rel-L2 {rel(got[c], x[0]):.3g}, passes device {int(ps[c])} checker {int(last[0])}")
    assert rel(got[c], x[0]) < 5e-5, rel(got[c], x[0])
    assert int(ps[c]) == int(last[0])


def test_a_narrow_image_warns_once_and_the_forced_path_stays_silent(la, monkeypatch):
    """96 columns: below what the pipeline covers, so rtol > 0 lands on the pass-by-pass path -- a RuntimeWarning unless exit_path='passes' asked for it."""
    import warnings
    from lmc_atomi_amd import proximal as P
    shape = (20, 96)
    x = images(shape, 2, 1)[1]
    monkeypatch.setattr(P, "_warned_pass_by_pass", False)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        la.TV(shape, sigma=0.3, niter=10, rtol=RTOL, exit_path="passes").prox(x.ravel(), GAMMA)          # silent
        la.TV((20, 301), sigma=0.3, niter=10, rtol=RTOL).prox(images((20, 301), 2, 1)[1].ravel(), GAMMA)  # on the device: silent
    with pytest.warns(RuntimeWarning, match="pass by pass"):
        px = la.TV(shape, sigma=0.3, niter=10, rtol=RTOL).prox(x.ravel(), GAMMA).reshape(shape)
    assert rel(px, O.tv_prox_fgp(x, 0.3 * GAMMA, 10, rtol=RTOL)) < 5e-6
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        la.TV(shape, sigma=0.3, niter=10, rtol=RTOL).prox(x.ravel(), GAMMA)                               # once per process

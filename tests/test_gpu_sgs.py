"""The split Gibbs sampler on the device (la.SplitGibbsSampler, lmc_sgs_*) against tests/_sgs_ref.py: one iteration per pixel on both planes within
`max(3 e32, 2 ulp32)` of the float64 reference for every case (injected noise), the x-step without noise against L2.prox, Philox against injected
noise bit for bit, a five-iteration trajectory with its energies, the moments, sharding, the Gaussian-prior statistical check and the C-ABI refusals."""
import ctypes as C

import numpy as np
import pytest

import _fourier_ref as F
import _pixel as X
import _poisson_ref as P
import _sgs_ref as S

pytestmark = pytest.mark.gpu

STEP_TOL = 1e-5          # the project's trajectory and energy tolerances (tests/test_gpu_fourier.py)
ENERGY_RTOL = 5e-5


@pytest.fixture(scope="module")
def la():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import lmc_atomi_amd as la
    return la


def f64(a):
    return None if a is None else np.array(a, dtype=np.float64)


def case(name):
    return S.CASES[S.IDS.index(name)]


def device_terms(la, c, m):
    shape = c.shape
    if c.kind == "spectral":
        if c.term == "mask":
            pf = la.L2(Op=la.FourierSampling(shape, m.mask2), b=m.y, sigma=m.sigma_f)
        else:
            pf = la.L2(Op=la.PeriodicConvolve2D(shape, m.h, offset=m.offset), b=m.y, sigma=m.sigma_f)
    elif c.term == "mask":
        pf = la.L2(Op=la.Diagonal(f64(m.m), dims=shape), b=f64(m.b_img), sigma=m.sigma_f, dims=shape)
    else:
        pf = la.L2(b=f64(m.b_img), sigma=m.sigma_f, weights=f64(m.w), dims=shape)
    if c.prior in ("tv", "aniso"):
        pg = la.TV(shape, sigma=m.weight, niter=10, isotropic=c.prior == "tv", bounds=c.box)
    elif c.prior == "l1":
        pg = la.L1(sigma=m.weight)
    elif c.prior == "wavelet":
        pg = la.WaveletL1(shape, sigma=m.weight, levels=S.WAVELET[2], wavelet=S.WAVELET[0])
    else:
        pg = la.TGV(shape, sigma=m.weight, alpha0=S.TGV_ALPHA0, niter=S.TGV_K)
    return pf, pg


def sampler(la, c, m, **kw):
    pf, pg = device_terms(la, c, m)
    args = dict(n_chains=S.n_chains(c), rho=m.rho, tau=m.tau, gamma=m.gamma, n_inner=c.n_inner)
    args.update(kw)
    return la.SplitGibbsSampler(pf, pg, c.shape, **args)


def within(what, got, ref64, bound, e32):
    err, where = F.worst(got, ref64)
    print(f"pixel {what}: err {err:.3e} at {where}, e32 {e32:.3e}, bound {bound:.3e}, err / bound {err / bound:.2f}")
    assert err <= bound, (what, err, bound, where)


# ------------------------------------------------------------------ 1. one iteration, both planes, every case
@pytest.mark.parametrize("name", S.IDS)
def test_one_iteration_per_pixel(la, name):
    c = case(name)
    m, r = S.problem(c), S.reference(c)
    with sampler(la, c, m, noise="injected") as smp:
        smp.set_state(m.x0, m.z0)
        smp.step(1, noise=m.noise[None])
        x, z = smp.state.cpu().numpy(), smp.aux.cpu().numpy()
        kernel = smp.kernel_name
    within(f"{name} x ({kernel})", x, r.x64, r.bx, r.ex)
    within(f"{name} z ({kernel})", z, r.z64, r.bz, r.ez)
    assert ("sgs_cols_gibbs_kernel" if c.kind == "spectral" else "sgs_xdiag") in kernel and "sgs_couple_kernel" in kernel, kernel
    if c.kind == "diag":
        assert ("sgs_xdiag4_kernel" if c.shape[1] % 4 == 0 else "sgs_xdiag1_kernel") in kernel, kernel


# ------------------------------------------------------------------ 2. the draw without noise is prox_{rho^2 f}(z)
@pytest.mark.parametrize("name", ["spectral-16x8-mask-tv", "spectral-64x128-periodic-tv", "spectral-128x32-mask-tv", "diag-33x70-identity-tv",
                                  "diag-64x136-mask-tv"])
def test_draw_without_noise_is_the_l2_prox(la, name):
    c = case(name)
    m = S.problem(c)
    pf, _ = device_terms(la, c, m)
    if c.kind == "spectral":
        want = F.prox_folded(m.z0.astype(np.float64), m.G, m.b, m.sigma_f, m.rho ** 2)
        reps = [S.xdraw_spectral(m.z0, None, *S.tables(m.G, m.b, np.float32), m.sigma_f, m.rho, np.float32, order) for order in ("definition", "kernel")]
    else:
        want = S.xdraw_diag(m.z0, None, m.b_img, m.w, m.m, m.sigma_f, m.rho, np.float64)
        reps = [S.xdraw_diag(m.z0, None, m.b_img, m.w, m.m, m.sigma_f, m.rho, np.float32, order) for order in ("definition", "kernel")]
    e32, bound = min((X.bound_of(want, r) for r in reps), key=lambda eb: eb[0])
    mean = la.sgs_xstep(pf, m.z0, m.rho, dims=c.shape)
    prox = np.asarray(pf.prox(m.z0, float(np.float32(m.rho) * np.float32(m.rho)))).reshape(m.z0.shape)
    assert mean.shape == m.z0.shape and mean.dtype == np.float32
    within(f"mean {name}", mean, want, bound, e32)
    within(f"prox {name}", prox, want, bound, e32)
    within(f"mean against prox {name}", mean, prox.astype(np.float64), bound, e32)
    noise = np.zeros_like(m.z0)
    within(f"zero noise {name}", la.sgs_xstep(pf, m.z0, m.rho, noise=noise, dims=c.shape), want, bound, e32)


def test_no_data_term_draws_around_z(la):
    """LMC_DATA_NONE: q = 1 / rho^2, x = z + rho xi up to rounding."""
    c = case("diag-5x7-identity-tv")
    m = S.problem(c)
    want = S.xdraw_diag(m.z0, m.noise[0], None, None, None, 0.0, m.rho, np.float64)
    r32 = S.xdraw_diag(m.z0, m.noise[0], None, None, None, 0.0, m.rho, np.float32, "kernel")
    e32, bound = X.bound_of(want, r32)
    assert np.max(np.abs(want - (m.z0 + np.float64(np.float32(m.rho)) * m.noise[0]))) < 1e-4
    within("no data term", la.sgs_xstep(None, m.z0, m.rho, noise=m.noise[0], dims=c.shape), want, bound, e32)


# ------------------------------------------------------------------ 3. Philox mode = injected mode fed with the sampler's own fields
@pytest.mark.parametrize("name", ["spectral-8x64-periodic-tv-inner3", "diag-33x70-mask-tv", "diag-64x136-weights-tv", "diag-33x72-mask-tv"])
def test_philox_mode_equals_injected_mode_bit_for_bit(la, name):
    import torch
    c = case(name)
    m = S.problem(c)
    seed, nit, off = X.SEED_P, 2, 3
    with sampler(la, c, m, seed=seed, chain_offset=off) as a, sampler(la, c, m, noise="injected", seed=seed, chain_offset=off) as b:
        a.set_state(m.x0, m.z0)
        b.set_state(m.x0, m.z0)
        a.step(nit)
        fields = torch.stack([torch.stack([a.noise(it, p) for p in range(1 + c.n_inner)]) for it in range(nit)])
        assert torch.isfinite(fields).all() and not torch.equal(fields[0, 0], fields[0, 1]) and not torch.equal(fields[0, 1], fields[1, 1])
        b.step(nit, noise=fields)
        np.testing.assert_array_equal(a.state.cpu().numpy(), b.state.cpu().numpy())
        np.testing.assert_array_equal(a.aux.cpu().numpy(), b.aux.cpu().numpy())
        kernel = a.kernel_name
    if c.kind == "diag":
        assert ("sgs_xdiag_philox4_kernel" if c.shape[1] % 4 == 0 else "sgs_xdiag_philox1_kernel") in kernel, kernel
    # plane 1 is the field of a grey sampler of the seed (seed + (1 << 32)) mod 2^64: the convention of the multi-channel sampler
    from oracle import lmc_oracle as O
    want = O.philox_normals((seed + (1 << 32)) % (1 << 64), 1 * c.n_inner, np.arange(off, off + S.n_chains(c)), *c.shape)
    assert np.max(np.abs(fields[1, 1].cpu().numpy() - want)) <= X.NOISE_TOL
    want0 = O.philox_normals(seed, 1, np.arange(off, off + S.n_chains(c)), *c.shape)
    assert np.max(np.abs(fields[1, 0].cpu().numpy() - want0)) <= X.NOISE_TOL


# ------------------------------------------------------------------ 4. five iterations against float64, with the energies
def f_value(c, m, x):
    if c.kind == "spectral":
        return F.SpectralRef(m.G, m.b, m.sigma_f).value(x)
    w = np.ones(c.shape) if m.w is None else m.w.astype(np.float64)
    mk = np.ones(c.shape) if m.m is None else m.m.astype(np.float64)
    return 0.5 * m.sigma_f * np.sum(w * (mk * x - m.b_img.astype(np.float64)) ** 2, axis=(-2, -1))


@pytest.mark.parametrize("name", ["spectral-64x128-mask-tv", "diag-33x70-weights-tv"])
def test_five_iteration_trajectory_and_energies(la, name):
    c = case(name)
    m = S.problem(c)
    nit = 5
    rng = np.random.default_rng(17)
    noise = X.f32(rng.standard_normal((nit, 1 + c.n_inner) + m.z0.shape))
    x, z = m.x0.astype(np.float64), m.z0.astype(np.float64)
    with sampler(la, c, m, noise="injected") as smp:
        smp.set_state(m.x0, m.z0)
        worst = 0.0
        for it in range(nit):
            smp.step(1, noise=noise[it:it + 1])
            x, z = S.iteration(c, m, x, z, noise[it], np.float64)
            ex, ez = X.rel(smp.state.cpu().numpy(), x), X.rel(smp.aux.cpu().numpy(), z)
            worst = max(worst, ex, ez)
            print(f"trajectory {name} iteration {it + 1}: rel-L2 x {ex:.3e} z {ez:.3e}")
            assert ex <= STEP_TOL * (it + 1) and ez <= STEP_TOL * (it + 1), (it, ex, ez)
        f, g, k = (t.cpu().numpy() for t in smp.energies())
        f2, g2, k2 = (t.cpu().numpy() for t in smp.energies())
    want_f = f_value(c, m, x)
    want_g = m.weight * P.TVRef(c.shape, m.weight, 10).value(z)
    want_k = np.sum((x - z) ** 2, axis=(-2, -1)) / (2 * m.rho ** 2)
    rels = [float(np.max(np.abs(a - b) / np.abs(b))) for a, b in ((f, want_f), (g, want_g), (k, want_k))]
    print(f"trajectory {name}: worst rel-L2 {worst:.3e}; energies rel f {rels[0]:.2e} g {rels[1]:.2e} coupling {rels[2]:.2e}")
    assert max(rels) < ENERGY_RTOL, rels
    # the coupling is this sampler's own fixed-order sum; f and g are the values of lmc_energies, whose sums are not pinned to bits for every term
    assert np.array_equal(k, k2), "two evaluations of the coupling energy differ"
    assert np.max(np.abs(g - g2) / np.abs(g)) < 1e-12 and np.max(np.abs(f - f2) / np.abs(f)) < 1e-12


# ------------------------------------------------------------------ 5. moments and chain-group moments of the kept x
def test_moments_and_group_moments_are_the_sums_of_the_kept_states(la):
    c = case("diag-33x70-mask-tv")
    m = S.problem(c)
    nit, burn, thin, G, C_, off = 6, 1, 2, 2, 3, 5
    z0 = np.concatenate([m.z0, m.z0[:1] + 1.0])
    with sampler(la, c, m, n_chains=C_, seed=7, burn_in=burn, thin=thin, chain_groups=G, chain_offset=off) as smp:
        smp.set_state(z0)
        kept = []
        for it in range(nit):
            smp.step(1)
            if it >= burn and (it - burn) % thin == 0:
                kept.append(smp.state.cpu().numpy().astype(np.float64))
        s1, s2, cnt = smp.moments()
        S1, S2, counts = smp.group_moments()
        kept = np.stack(kept)
        assert cnt == kept.shape[0] * C_ == 3 * C_
        tol = lambda a: 1e-12 * np.max(np.abs(a))
        assert np.max(np.abs(s1.cpu().numpy() - kept.sum(axis=(0, 1)))) <= tol(kept.sum(axis=(0, 1)))
        assert np.max(np.abs(s2.cpu().numpy() - (kept ** 2).sum(axis=(0, 1)))) <= tol((kept ** 2).sum(axis=(0, 1)))
        for g in range(G):
            sel = [ch for ch in range(C_) if (off + ch) % G == g]
            assert int(counts[g]) == kept.shape[0] * len(sel)
            assert np.max(np.abs(S1[g].cpu().numpy() - kept[:, sel].sum(axis=(0, 1)))) <= tol(kept[:, sel].sum(axis=(0, 1)))
            assert np.max(np.abs(S2[g].cpu().numpy() - (kept[:, sel] ** 2).sum(axis=(0, 1)))) <= tol((kept[:, sel] ** 2).sum(axis=(0, 1)))
        smp.reset_moments()
        assert smp.moments()[2] == 0 and not smp.moments()[0].any()
    pf, pg = device_terms(la, c, m)
    res = la.SplitGibbs(pf, pg, z0, m.rho, m.tau, m.gamma, nit, n_chains=C_, seed=7, burn_in=burn, thin=thin, chain_groups=G, chain_offset=off, dims=c.shape)
    assert res.count == 3 * C_ and res.mcse_mean.shape == c.shape and res.ess.shape == c.shape
    np.testing.assert_array_equal(res.mean.cpu().numpy(), (s1 / cnt).cpu().numpy())      # x = z = x0 and the same seed: the same run
    assert res.state.shape == res.aux.shape == (C_,) + c.shape
    assert all(t.shape == (C_,) for t in (res.energy_f, res.energy_g, res.energy_coupling))


# ------------------------------------------------------------------ 6. sharding
@pytest.mark.parametrize("name", ["spectral-16x8-mask-tv", "diag-33x70-weights-tv"])
def test_chains_split_two_and_one_equal_the_unsplit_run(la, name):
    c = case(name)
    m = S.problem(c)
    z0 = np.concatenate([m.z0, m.z0[:1] + 1.0])[:3]
    with sampler(la, c, m, n_chains=3, seed=9) as whole:
        whole.set_state(z0)
        whole.step(3)
        want_x, want_z = whole.state.cpu().numpy(), whole.aux.cpu().numpy()
    assert np.isfinite(want_x).all() and not np.array_equal(want_x, z0)
    for off, n in ((0, 2), (2, 1)):
        with sampler(la, c, m, n_chains=n, seed=9, chain_offset=off) as part:
            part.set_state(z0[off:off + n])
            part.step(3)
            np.testing.assert_array_equal(part.state.cpu().numpy(), want_x[off:off + n])
            np.testing.assert_array_equal(part.aux.cpu().numpy(), want_z[off:off + n])


# ------------------------------------------------------------------ 7. exactness under a Gaussian prior: the twin of tests/test_sgs_reference.py
def test_gaussian_prior_marginal_variance_per_frequency(la):
    """g = theta / 2 ||z||^2, same N and the same condition as the CPU test, with the z-step by MYULA: 16 inner steps of tau = 0.9 sgs_step_bound at
    gamma theta = 0.05.  The z-step's own bias -- the envelope's theta / (1 + gamma theta) in place of theta (5 %) and the discretisation's
    tau (1 / rho^2 + theta) / 2 (2 % of the conditional variance of z) -- is well inside the 5 standard errors = 15.8 % of the check; the curvature of
    the z-potential is 1 / rho^2 + theta, far below the bound's 1 / gamma, so one iteration renews z only in part and the chain runs 80 iterations, not
    40 (a float64 simulation of this recursion passes the check at 2.8 and 3.3 standard errors for two seeds)."""
    mask, transfer, G, y = S.gauss_problem()
    shape = S.GAUSS_SHAPE
    gamma = 0.05 / S.GAUSS_THETA
    tau = 0.9 * la.sgs_step_bound(S.GAUSS_RHO, gamma)
    pf = la.L2(Op=la.FourierSampling(shape, mask, transfer=transfer), b=y, sigma=S.GAUSS_SIGMA_F)
    pg = la.L2(sigma=S.GAUSS_THETA, dims=shape)
    with la.SplitGibbsSampler(pf, pg, shape, S.GAUSS_N, S.GAUSS_RHO, tau, gamma, n_inner=16, seed=5, moments=False) as smp:
        smp.step(2 * S.GAUSS_ITERS)
        x = smp.state.cpu().numpy()
    assert x.shape == (S.GAUSS_N,) + shape and np.isfinite(x).all()
    assert S.gauss_check(x, G, "device chain") <= S.GAUSS_SE


# ------------------------------------------------------------------ 8. the C-ABI refusals, with their messages
def test_c_abi_refusals(la):
    import torch
    from lmc_atomi_amd import _dev
    import _sgs_cases as A
    buf = torch.zeros(4 * 16 * 16, dtype=torch.float32, device="cuda")
    for fields, word in A.UNSUPPORTED:
        fields = {k: (buf.data_ptr() if v == A.FAKE else v) for k, v in fields.items()}
        cfg = A.sgs_config(**fields)
        cfg.problem.y_dev = buf.data_ptr()
        rc, msg = A.create(cfg)
        print(f"refused {fields}: {msg}")
        assert rc == A.LMC_E_UNSUPPORTED and word in msg, (rc, msg)
    for fields in A.INVALID:
        cfg = A.sgs_config(**fields)
        cfg.problem.y_dev = buf.data_ptr()
        rc, msg = A.create(cfg)
        assert rc == A.LMC_E_INVALID and msg, (fields, rc, msg)
    cfg = A.sgs_config()      # and the configuration they vary is accepted
    cfg.problem.y_dev = buf.data_ptr()
    h = C.c_void_p()
    assert _dev.lib().lmc_sgs_create(C.byref(cfg), C.byref(h)) == 0 and h.value
    assert _dev.lib().lmc_sgs_step(h, 1, buf.data_ptr(), None) == A.LMC_E_INVALID      # noise given, noise_mode is PHILOX
    assert _dev.lib().lmc_sgs_noise(h, 0, 2, buf.data_ptr(), None) == A.LMC_E_INVALID   # plane_and_inner outside 0 .. n_inner
    _dev.lib().lmc_sgs_destroy(h)

"""MYMALA's Metropolis target over the models: log alpha = U(x) - U(x') - (||x - m(x')||^2 - ||x' - m(x)||^2) / (4 tau) with U = f + epsg g, for
every data term x prior x non-log-concave term x image shape of tests/_mala_ref.py::CASES, against the float64 reference built there from the
checker's classes.  MYMALA is the one sampler that is only right if the energies are: a wrong U neither crashes nor shows in an image, it samples
another distribution.  tests/test_mala_reference.py shows (on the CPU) that on every one of these problems a missing f, a missing g or a wrongly
weighted g moves log alpha by 20 to 100 times the tolerance and more.

Six chains, three iterations, injected noise, one iteration per call; the device's accept counts are read after each.  Where a chain's decision is
within the tolerance of log u the device may decide the other way: the reference is then replayed with the device's own decisions on those chains, so
log alpha is compared at every chain and iteration.  Tolerances are those of tests/test_gpu_mymala.py (log alpha: 2e-6 max|U(x0)| + 2e-3; state:
rel-L2 2e-5 on the clear-cut chains) and tests/test_gpu_poisson.py (energies: 5e-5 relative)."""
import ctypes as C

import numpy as np
import pytest

from oracle import lmc_oracle as O
from tests import _mala_ref as R

pytestmark = pytest.mark.gpu

ENERGY_RTOL = 5e-5
STATE_TOL = 2e-5
LMC_E_UNSUPPORTED = -2


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


def device_terms(la, m):
    """The device's data term and prior of the problem ``m`` (a ``_mala_ref.Model``), from the arrays the checker's were built from."""
    case, shape = m.case, m.shape
    n = shape[0] * shape[1]
    y = m.y.ravel().copy()           # (the reference's arrays are read-only)
    if case.data in R.BLURS:
        Op = la.Convolve2D(shape, m.h, offset=m.offset)
    elif case.data == "identity":
        Op = None
    else:
        Op = la.Diagonal(m.mask, dims=shape)
    if case.ncvx == "none":
        pf = la.L2(Op=Op, b=y, sigma=1 / R.SIG ** 2, dims=shape)
    else:
        kw = dict(dims=shape, b=y, Op=Op if Op is not None else la.Identity(n), **R.NCVX_KW)
        if case.ncvx in ("mc", "mc_aniso"):
            pf = la.L2_ncvx_tv(Op2=la.Gradient(shape), isotropic=case.ncvx == "mc", **kw)
        else:
            pf = la.L2_ncvx_tv(isotropic=True, rtol=1e-4 if case.ncvx == "me_rtol" else 0.0, **kw)
    if case.prior in R.TV_PRIORS:
        niter, lagged = R.TV_PRIORS[case.prior]
        pg = la.TV(shape, sigma=0.3, niter=niter, lagged_output=lagged)
    elif case.prior == "aniso":
        pg = la.TV(shape, sigma=0.3, niter=10, isotropic=False)
    elif case.prior == "l2":
        pg = la.L2(sigma=0.05, dims=shape)
    elif case.prior == "l1":
        pg = la.L1(sigma=0.8)
    elif case.prior == "haar":
        pg = la.WaveletL1(shape, sigma=0.3)
    else:
        pg = None
    return pf, pg


def expected_kernel(case):
    """The step kernel that forms m(x'), by the order in which the library's dispatch (``launch_step``, variant auto) tries its kernels:

    1. register blocks: a pointwise data term on an image whose sides are multiples of 8, a prior local to 8 x 8 blocks (l1, l2, Haar, none), no
       non-convex term or MC-TV (added by a stencil pass of its own);
    2. row streaming: a centred separable blur with such a prior (the Haar prox as a launch of its own before it), no MC-TV term -- the ME-TV
       term reaches every kernel as a ready-made gradient array;
    3. the full-width pipeline: TV on more than 128 columns -- isotropic with 6, 9 or 10 dual iterations (rows that are not 16-byte aligned: 10
       only), anisotropic with 10 -- a centred separable blur, or a pointwise data term without an MC-TV term;
    4. the split pipeline: up to 512 columns, any prior but the anisotropic TV, any separable blur (every dual-iteration count of the matrix fits
       its LDS budget at these widths);
    5. the LDS-tiled kernel: what is left -- the anisotropic TV up to 128 columns and TV with 5 dual iterations on the 520-column image.

    So with the Metropolis energies from the energy kernels, m(x') comes from the tiled kernel in eight cases of the matrix and in the forced-variant
    tests below."""
    (H, W), blur = case.shape, case.data in R.BLURS
    centred = case.data in R.CENTRED
    block_local = case.prior in ("l1", "l2", "haar", "none")
    if not blur and block_local and H % 8 == 0 and W % 8 == 0 and case.ncvx in ("none", "mc"):
        return "myula_step_block_kernel"
    if centred and block_local and case.ncvx in ("none", "me", "me_rtol"):
        return "myula_step_rows_kernel"
    if not block_local and W > 128:
        if case.prior == "aniso":
            K, aligned = 10, True
        else:
            K = R.TV_PRIORS[case.prior][0] - R.TV_PRIORS[case.prior][1]
            aligned = K == 10 or W % (8 if W > 256 else 4) == 0
        if K in (6, 9, 10) and aligned and (K == 10 or case.prior != "aniso") and (centred if blur else case.ncvx not in ("mc", "mc_aniso")):
            return "myula_step_pipe_aniso_kernel" if case.prior == "aniso" else "myula_step_pipe_kernel"
    if W <= 512 and case.prior != "aniso":
        return "myula_step_split_kernel"
    return "myula_step_tile_kernel"


_RUNS, _LEFT_OUT, _USED = {}, {}, {}


def run(la, case, variant=None):
    """The device run of ``case``, once per process: log alpha and the accept decisions per iteration, the final state, its energies as the
    sampler reports them, the kernel name.  None where the create call refuses the model (kept in ``_LEFT_OUT``)."""
    key = (case, variant)
    if key in _RUNS:
        return _RUNS[key]
    m = R.reference(case).model
    pf, pg = device_terms(la, m)
    try:
        smp = la.MYMALASampler(pf, pg, m.shape, n_chains=R.N_CHAINS, tau=m.tau, gamma=m.gamma, epsg=m.epsg, noise="injected", seed=R.SEED,
                               chain_offset=R.CHAIN_OFFSET, variant=variant)
    except NotImplementedError as err:
        _LEFT_OUT[key] = str(err)
        _RUNS[key] = None
        return None
    try:
        smp.set_state(m.x0.copy())
        las, accs = [], []
        for k in range(R.N_ITERS):
            smp.step(1, noise=m.noise[k:k + 1].copy())
            acc, la_d = smp.acceptance()
            las.append(la_d.cpu().numpy())
            accs.append(acc.cpu().numpy())
        f, g = smp.energies()
        out = {"log_alpha": np.array(las), "accepted": accs[-1], "decisions": np.diff(np.array([np.zeros_like(accs[0])] + accs), axis=0),
               "state": smp.get_state().cpu().numpy(), "f": f.cpu().numpy(), "g": g.cpu().numpy(), "kernel": smp.kernel_name,
               "iteration": smp.iteration}
    finally:
        smp.close()
    _RUNS[key] = out
    return out


def against_reference(case, out, label=""):
    """The assertions every run shares.  Returns the largest |log alpha error| / bound."""
    r = R.reference(case)
    m = r.model
    dec_d, dec_r = out["decisions"], (np.log(m.uniforms) <= r.log_alpha).astype(np.int64)
    assert set(np.unique(dec_d)) <= {0, 1}, dec_d
    x_ref, acc_ref, la_ref = r.x, r.accepted, r.log_alpha
    if (dec_d != dec_r)[:, ~r.safe].any():     # a borderline decision went the other way: the reference follows the device on the chains that have one
        x_ref, acc_ref, la_ref, _, _ = m.run(decisions=np.where(r.safe[None, :], -1, dec_d))
        dec_r = np.where(r.safe[None, :], dec_r, dec_d)
    # history agrees: every earlier decision of the chain is the reference's
    agree = np.vstack([np.ones((1, R.N_CHAINS), dtype=bool), np.cumprod(dec_d == dec_r, axis=0).astype(bool)[:-1]])
    err = np.abs(out["log_alpha"] - la_ref)
    used = float((err / r.bound)[agree].max())
    print(f"{case.id}{label}: {out['kernel']}; bound {r.bound:.3e}, max |log alpha error| / bound {used:.3f}; safe {int(r.safe.sum())}/{R.N_CHAINS}; "
          f"accepted {out['accepted'].tolist()} (reference {acc_ref.tolist()})")
    assert (err[agree] < r.bound).all(), (case.id, label, out["kernel"], "log alpha", out["log_alpha"], la_ref, r.bound)
    assert (out["accepted"][r.safe] == acc_ref[r.safe]).all(), (case.id, label, out["accepted"], acc_ref, r.safe)
    e = rel(out["state"][r.safe], x_ref[r.safe])
    assert e < STATE_TOL, (case.id, label, "state", e)
    assert out["iteration"] == R.N_ITERS
    return used


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.id)
def test_log_alpha_accept_counts_and_state(la, case):
    out = run(la, case)
    assert out is not None, f"{case.id}: the create call refuses a model of the matrix: {_LEFT_OUT[(case, None)]}"
    _USED[case] = against_reference(case, out)
    assert out["kernel"] == expected_kernel(case), (case.id, out["kernel"], expected_kernel(case))


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.id)
def test_energies_of_the_final_state(la, case):
    """``smp.energies()`` after the run against the checker's f and g of that state (the device's own final state, in float64)."""
    out = run(la, case)
    assert out is not None, f"{case.id}: the create call refuses a model of the matrix"
    m = R.reference(case).model
    x = out["state"].astype(np.float64)
    f, g = m.f(x), m.g(x)
    ef = np.max(np.abs(out["f"] - f) / np.abs(f))
    print(f"{case.id}: f rel {ef:.2e}", end="")
    assert ef < ENERGY_RTOL, (case.id, "f", out["f"], f)
    if case.prior != "none":
        eg = np.max(np.abs(out["g"] - g) / np.abs(g))
        print(f", g rel {eg:.2e}")
        assert eg < ENERGY_RTOL, (case.id, "g", out["g"], g)
    else:
        assert (out["g"] == 0).all()


def test_how_much_of_the_bound_the_matrix_uses(la):
    """The largest |log alpha error| / bound over the matrix, for the next reader of the bound (the runs are shared with the tests above)."""
    used = {case: _USED[case] if case in _USED else against_reference(case, run(la, case)) for case in R.CASES if run(la, case) is not None}
    assert len(used) == len(R.CASES), sorted(c.id for c in R.CASES if c not in used)      # no model of the matrix is one MYMALA refuses
    worst = max(used, key=used.get)
    tiled = [c.id for c in R.CASES if run(la, c)["kernel"] == "myula_step_tile_kernel"]
    print(f"largest |log alpha error| / bound over {len(used)} cases: {used[worst]:.3f} ({worst.id}); m(x') from the tiled kernel: {tiled}")
    assert used[worst] < 1.0


# ---- the pipeline's by-product energies against the energy kernels ---------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [R.PIPE, R.UNALIGNED], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("data", ["blur5", "blur7"])
def test_forced_tile_variant_against_auto(la, shape, data):
    """The same inputs through ``variant='tile'`` (f, g from the energy kernels) and ``'auto'`` (the pipeline, f and g as by-products of the
    update): each log alpha within the bound of the reference, so within twice the bound of the other."""
    case = R.Case(shape, data, "tv10")
    auto, tile = run(la, case), run(la, case, variant="tile")
    assert auto is not None and tile is not None
    against_reference(case, auto, " auto")
    against_reference(case, tile, " tile")
    assert auto["kernel"] == "myula_step_pipe_kernel" and "tile" in tile["kernel"], (auto["kernel"], tile["kernel"])
    r = R.reference(case)
    same = (np.cumsum(auto["decisions"] != tile["decisions"], axis=0) - (auto["decisions"] != tile["decisions"])) == 0     # same history so far
    assert (np.abs(auto["log_alpha"] - tile["log_alpha"])[same] < 2 * r.bound).all()


@pytest.mark.parametrize("data,prior", [("blur5", "tv10"), ("mask", "tv10"), ("blur7", "tv5"), ("identity", "l1")])
def test_forced_tile_variant_on_the_odd_image(la, data, prior):
    """``variant='tile'`` at 17 x 67, where auto takes the split pipeline: the tiled kernel's m(x') with the isotropic TV and a closed-form prior on
    an odd pixel count, against the reference."""
    case = R.Case(R.ODD, data, prior)
    tile = run(la, case, variant="tile")
    assert tile is not None
    against_reference(case, tile, " tile")
    assert tile["kernel"] == "myula_step_tile_kernel", tile["kernel"]


# ---- Philox mode on an image whose rows do not fill the proposal kernel's quads -------------------------------------------------------------

def test_philox_proposals_on_a_partial_row_quad(la, shape=R.ODD):
    """noise='philox' at 17 x 67: the proposal kernel draws quads of 4 rows, the last quad has one.  The reference runs on ``O.philox_normals``,
    which the device's normals match to 2e-5 (hardware log2 / sqrt / sin / cos: tests/test_gpu_parity.py).  That difference dxi enters log alpha
    through ||x' - m(x)||^2 / (4 tau) = sum xi^2 / 2, by at most 2e-5 sum |xi| per chain and iteration, and through x' = m(x) + sqrt(2 tau) xi,
    by 2.1e-5 per pixel -- the size of the fp32 rounding of x' itself (ulp(150) = 1.5e-5), which the bound allows for once already.  Hence
    tol = 2 bound + 2e-5 sum |xi|.  One wrong normal (an error of order 1) moves sum xi dxi by order 1, fifty times this."""
    case = R.Case(shape, "blur5", "tv10")
    m = R.reference(case).model
    H, W = m.shape
    chains = R.CHAIN_OFFSET + np.arange(R.N_CHAINS)
    xi = np.stack([O.philox_normals(R.SEED, k, chains, H, W).astype(np.float64) for k in range(R.N_ITERS)])
    x_ref, acc_ref, la_ref, _, _ = m.run(noise=xi)
    tol = 2 * R.bound_of(m.U(m.x0)) + 2e-5 * np.abs(xi).sum(axis=(-2, -1))
    safe = (np.abs(np.log(m.uniforms) - la_ref) > 10 * tol).all(axis=0)
    assert safe.sum() >= R.N_CHAINS // 2, "test problem too borderline"
    pf, pg = device_terms(la, m)
    smp = la.MYMALASampler(pf, pg, m.shape, n_chains=R.N_CHAINS, tau=m.tau, gamma=m.gamma, seed=R.SEED, chain_offset=R.CHAIN_OFFSET)
    try:
        smp.set_state(m.x0.copy())
        las, accs = [], []
        for k in range(R.N_ITERS):
            smp.step(1)
            acc, la_d = smp.acceptance()
            las.append(la_d.cpu().numpy())
            accs.append(acc.cpu().numpy())
        got = smp.get_state().cpu().numpy()
    finally:
        smp.close()
    dec_d = np.diff(np.array([np.zeros_like(accs[0])] + accs), axis=0)
    dec_r = (np.log(m.uniforms) <= la_ref).astype(np.int64)
    if (dec_d != dec_r)[:, ~safe].any():
        x_ref, acc_ref, la_ref, _, _ = m.run(noise=xi, decisions=np.where(safe[None, :], -1, dec_d))
        dec_r = np.where(safe[None, :], dec_r, dec_d)
    agree = np.vstack([np.ones((1, R.N_CHAINS), dtype=bool), np.cumprod(dec_d == dec_r, axis=0).astype(bool)[:-1]])
    err = np.abs(np.array(las) - la_ref)
    print(f"philox {case.id}: max |log alpha error| / tol {(err / tol)[agree].max():.3f}; tol {tol.min():.3e}..{tol.max():.3e}; accepted {accs[-1].tolist()}")
    assert (err[agree] < tol[agree]).all(), (err, tol)
    assert (accs[-1][safe] == acc_ref[safe]).all(), (accs[-1], acc_ref, safe)
    assert rel(got[safe], x_ref[safe]) < STATE_TOL


@pytest.mark.parametrize("shape", [(5, 7), (9, 130)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_philox_proposals_on_other_partial_quads(la, shape):
    """The same at 5 x 7 (two row-groups, the last of one row, fewer columns than a wave) and at 9 x 130 (three row-groups, columns past two waves):
    the proposal kernel's quad index is (i >> 2) W + j, and 17 x 67 alone leaves the other widths and a last group behind two full ones unchecked."""
    test_philox_proposals_on_a_partial_row_quad(la, shape)


# ---- the stateless energies at the edges of the separable energy kernel's 32 x 64 tile ---------------------------------------------------

EDGE_DATA = ["blur5", "blur7", "blur6", "mask"]
EDGE_PRIORS = ["tv", "aniso", "l1", "l2"]


@pytest.mark.parametrize("H", [1, 31, 33])
@pytest.mark.parametrize("W", [3, 63, 65, 129])
def test_stateless_energies_at_tile_edges(la, H, W):
    """``lmc_energies`` (through ``_Problem.energies``) on three images per call against float64.  The states are the image plus noise of 10, 20
    and 30 grey levels: residuals of order 10, so that the fp32 rounding of a blurred value near 150 (a few 1e-5) is a few 1e-6 of them."""
    from lmc_atomi_amd.proximal import _Problem
    from tests._tv_aniso_ref import tv_aniso_value
    shape = (H, W)
    rng = np.random.default_rng(1000 * H + W)
    img = np.zeros(shape)
    img[H // 4:H // 2 + 1, W // 4:3 * W // 4] = 150.0
    img += np.linspace(0, 30, W)[None, :]
    x = np.stack([img + rng.normal(0, s, shape) for s in (10.0, 20.0, 30.0)])
    sf = 1 / R.SIG ** 2
    priors = {"tv": (la.TV(shape, sigma=0.3, niter=10), lambda v: 0.3 * np.array([O.tv_value(vc) for vc in v])),
              "aniso": (la.TV(shape, sigma=0.3, niter=10, isotropic=False), lambda v: 0.3 * tv_aniso_value(v)),
              "l1": (la.L1(sigma=0.8), lambda v: 0.8 * np.abs(v).sum(axis=(-2, -1))),
              "l2": (la.L2(sigma=0.05, dims=shape), lambda v: 0.5 * 0.05 * (v * v).sum(axis=(-2, -1)))}
    bad = []
    for data in EDGE_DATA:
        if data == "mask":
            mask = (rng.uniform(size=shape) < 0.5).astype(np.float64)
            mask.flat[0] = 1.0
            y = mask * (img + rng.normal(0, R.SIG, shape))
            pf = la.L2(Op=la.Diagonal(mask, dims=shape), b=y.ravel(), sigma=sf, dims=shape)
            f_ref = 0.5 * sf * ((mask * x - y) ** 2).sum(axis=(-2, -1))
        else:
            k, off = R.BLURS[data]
            h = np.ones((k, k)) / k ** 2
            y = O.blur(img, h, off) + rng.normal(0, R.SIG, shape)
            pf = la.L2(Op=la.Convolve2D(shape, h, offset=off), b=y.ravel(), sigma=sf, dims=shape)
            f_ref = 0.5 * sf * ((O.blur(x, h, off) - y) ** 2).sum(axis=(-2, -1))
        for prior in EDGE_PRIORS:
            pg, g_of = priors[prior]
            g_ref = g_of(x)
            prob = _Problem(shape, pf.descriptor(), pg.prior_descriptor())
            f, g = prob.energies(x)
            f, g = f.cpu().numpy(), g.cpu().numpy()
            ef, eg = np.max(np.abs(f - f_ref) / np.abs(f_ref)), np.max(np.abs(g - g_ref) / np.abs(g_ref))
            print(f"{H}x{W} {data} {prior}: f rel {ef:.2e} g rel {eg:.2e}")
            if not (ef < ENERGY_RTOL and eg < ENERGY_RTOL):
                bad.append((data, prior, ef, eg))
    assert not bad, bad


# ---- priors without a value -------------------------------------------------------------------------------------------------------------------

def _eprox_models(la, shape):
    rng = np.random.default_rng(3)
    y = rng.normal(100, 20, shape)
    pf = la.L2(b=y.ravel(), sigma=1 / R.SIG ** 2, dims=shape)
    return pf, [la.Laplace(1.5), la.Huber(1.0, 0.5), la.GenGaussian(3, 0.2)]


def test_mymala_refuses_closed_form_priors(la):
    """A closed-form prior of prox.py has a prox and no value: MYULA runs it, MYMALA has no target to test against."""
    shape = (16, 64)
    pf, priors = _eprox_models(la, shape)
    for pg in priors:
        with pytest.raises(NotImplementedError, match="MYMALA"):
            la.MYMALASampler(pf, pg, shape, n_chains=2, tau=0.1, gamma=R.GAM)
        with pytest.raises(NotImplementedError, match="MYMALA"):
            la.MoreauYosidaMetropolisAdjustedLangevin(pf, pg, np.zeros(shape), tau=0.1, gamma=R.GAM, niter=2, n_chains=2, dims=shape)
        la.MYULASampler(pf, pg, shape, n_chains=2, tau=0.1, gamma=R.GAM).close()


def test_c_abi_refuses_mymala_with_a_closed_form_prior(la):
    from lmc_atomi_amd import _capi, _dev
    from lmc_atomi_amd.proximal import _Problem
    shape = (16, 64)
    pf, priors = _eprox_models(la, shape)
    lib = _dev.lib()
    for pg in priors:
        prob = _Problem(shape, pf.descriptor(), pg.prior_descriptor())
        assert prob.c.prior_kind == _capi.PRIOR_EPROX
        cfg = _capi.lmc_myula_config()
        cfg.struct_size = C.sizeof(_capi.lmc_myula_config)
        cfg.problem = prob.c
        cfg.n_chains = 2
        cfg.tau, cfg.gamma, cfg.epsg = 0.1, R.GAM, 1.0
        cfg.noise_mode = _capi.NOISE_PHILOX
        cfg.thin = 1
        hnd = C.c_void_p()
        rc = lib.lmc_mymala_create(C.byref(cfg), C.byref(hnd))
        msg = lib.lmc_last_error().decode()
        print(rc, msg)
        assert rc == LMC_E_UNSUPPORTED and not hnd.value, (rc, msg)
        assert "MYMALA" in msg and "value" in msg, msg
        assert lib.lmc_myula_create(C.byref(cfg), C.byref(hnd)) == 0 and hnd.value      # the same problem is MYULA's to run
        lib.lmc_sampler_destroy(hnd)

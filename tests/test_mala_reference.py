"""The float64 MYMALA reference of tests/_mala_ref.py, checked on the CPU: it reproduces the checker's ``O.mymala_batched``, and every problem of
the matrix of tests/test_gpu_mymala_matrix.py is one on which a wrong Metropolis target shows.  The second part states conditions on the test INPUTS,
from the reference alone: they are what makes a missing f, a missing g or a wrong weight of g fail the GPU comparison of log alpha instead of
passing inside its tolerance ``bound = 2e-6 max|U(x0)| + 2e-3`` (tests/test_gpu_mymala.py)."""
import numpy as np
import pytest

from oracle import lmc_oracle as O
from tests import _mala_ref as R


@pytest.mark.parametrize("kind,epsg", [("tv", 1.0), ("tv", 2.5), ("haar", 1.0)])
def test_reference_reproduces_the_checkers_mymala(kind, epsg):
    """Callables built from the checker's classes against ``O.mymala_batched`` with its dict-described prior: 5 x 5 blur + TV, mask + Haar."""
    shape, sigma, C, nit = (32, 32), 0.75, 4, 4
    gamma, tau = sigma ** 2, sigma ** 2
    rng = np.random.default_rng(5)
    img = np.zeros(shape)
    img[8:16, 8:24] = 150.0
    img += np.linspace(0, 30, shape[1])[None, :]
    if kind == "tv":
        h, off, mask = np.ones((5, 5)) / 25, (2, 2), None
        y = O.blur(img, h, off) + rng.normal(0, sigma, shape)
        of, og = O.L2(Op=O.Convolve2D(shape, h, off), b=y.ravel(), sigma=1 / sigma ** 2), O.TV(shape, sigma=0.3, niter=5)
        prior = {"kind": "tv", "sigma": 0.3, "niter": 5, "t": epsg * gamma}
    else:
        h, off, mask = None, None, (rng.uniform(size=shape) < 0.6).astype(np.float64)
        y = mask * (img + rng.normal(0, sigma, shape))
        of, og = O.L2(Op=O.Diagonal(mask), b=y.ravel(), sigma=1 / sigma ** 2), O.WaveletL1(shape, sigma=2.0)
        prior = {"kind": "haar", "sigma": 2.0, "t": epsg * gamma}
    x0 = img[None] + rng.normal(0, 3, (C,) + shape)
    noise = rng.standard_normal((nit, C) + shape)
    us = rng.uniform(size=(nit, C))

    def mean(v):
        return np.stack([O.myula(of, og, vc.ravel(), tau, gamma, epsg=epsg, niter=1, noise=[0.0])[-1].reshape(shape) for vc in v])

    def g(v):
        return np.array([og(vc.ravel()) for vc in v])

    def U(v):
        return np.array([of(vc.ravel()) for vc in v]) + epsg * g(v)

    xo, acc_o, la_o = O.mymala_batched(x0, y, h, off, 1 / sigma ** 2, tau, gamma, prior, nit, lambda k: noise[k], lambda k: us[k], mask=mask, epsg=epsg)
    x, acc, las, dU, dg = R.mymala(mean, U, x0, tau, noise, us, g=g)
    if kind == "haar":      # (the blurred problem accepts everything at this step; its rejections are the forced ones below)
        assert 0 < acc_o.sum() < nit * C, "the comparison needs both outcomes"
    np.testing.assert_array_equal(acc, acc_o)
    np.testing.assert_allclose(las, la_o, rtol=1e-12, atol=0)
    np.testing.assert_allclose(x, xo, rtol=1e-12, atol=1e-12 * np.abs(xo).max())
    # dU, dg: the changes the log alpha above was formed from
    f0, g0 = O.energies(x0, y, h, off, 1 / sigma ** 2, prior, mask=mask)
    xp = mean(x0) + np.sqrt(2 * tau) * noise[0]
    f1, g1 = O.energies(xp, y, h, off, 1 / sigma ** 2, prior, mask=mask)
    np.testing.assert_allclose(dg[0], g1 - g0, rtol=1e-10)
    np.testing.assert_allclose(dU[0], (f1 + epsg * g1) - (f0 + epsg * g0), rtol=1e-10)
    # forced decisions: the opposite outcome everywhere changes every count, and a negative entry leaves the rule in charge
    flip = (np.log(us[:1]) > la_o[:1]).astype(int)
    x_f, acc_f, las_f, _, _ = R.mymala(mean, U, x0, tau, noise[:1], us[:1], g=g, decisions=flip)
    np.testing.assert_allclose(las_f[0], la_o[0], rtol=1e-12)
    np.testing.assert_array_equal(acc_f, flip[0])
    np.testing.assert_array_equal(x_f, np.where(flip[0][:, None, None] > 0, xp, x0))
    _, acc_n, las_n, _, _ = R.mymala(mean, U, x0, tau, noise, us, g=g, decisions=-np.ones((nit, C), dtype=int))
    np.testing.assert_array_equal(acc_n, acc_o)
    np.testing.assert_array_equal(las_n, las)


def test_every_problem_of_the_matrix_shows_a_wrong_target(capsys):
    """Per case: at least half the chains have every decision clear-cut, |log u - log alpha| > 10 bound; the first iteration changes U by at least
    100 bound and epsg g by at least 20 bound on every chain (so a missing f or g, or g with the wrong weight, moves log alpha far outside the
    bound).  Over the matrix, both outcomes occur among the clear-cut chains."""
    bad, accepted, rejected = [], 0, 0
    lines = []
    for case in R.CASES:
        r = R.reference(case)
        n_safe = int(r.safe.sum())
        dU = float(np.min(np.abs(r.dU[0]))) / r.bound
        dg = float(np.min(np.abs(case.epsg * r.dg[0]))) / r.bound
        lines.append(f"{case.id:44s} safe {n_safe}/{R.N_CHAINS}  accepted {r.accepted.tolist()}  min|dU|/bound {dU:9.1f}  min|epsg dg|/bound {dg:9.1f}  "
                     f"bound {r.bound:.3e}")
        if n_safe < R.N_CHAINS // 2:
            bad.append((case.id, "safe chains", n_safe))
        if dU < 100:
            bad.append((case.id, "|dU| / bound", dU))
        if case.prior != "none" and dg < 20:
            bad.append((case.id, "|epsg dg| / bound", dg))
        accepted += int(r.accepted[r.safe].sum())
        rejected += int((R.N_ITERS - r.accepted[r.safe]).sum())
    with capsys.disabled():
        print("\n" + "\n".join(lines))
        print(f"{len(R.CASES)} cases; over their clear-cut chains {accepted} proposals accepted, {rejected} rejected")
    assert not bad, "\n".join(str(b) for b in bad)
    assert accepted > 0 and rejected > 0


def test_matrix_covers_what_it_is_there_for():
    """The shapes, data terms, priors and non-convex terms the matrix exists to cross (a case dropped by mistake shows here, not as a quiet gap)."""
    cs = R.CASES
    assert {c.shape for c in cs} == {(17, 67), (24, 136), (20, 150), (16, 520)}
    assert (17 * 67) % 2 == 1 and 17 % 4 and 150 % 4 and 520 > 512
    for shape in R.SHAPES:
        here = [c for c in cs if c.shape == shape]
        assert {c.data for c in here} >= {"blur5", "blur7", "blur6", "identity", "mask"}
        assert {c.prior for c in here} >= {"tv10", "tv5", "aniso", "l1", "l2", "none"}
    assert {c.prior for c in cs if c.shape == R.PIPE and c.data.startswith("blur")} >= {"tv6", "tv11lag", "tv10lag", "haar"}
    for shape in (R.PIPE, R.ODD):
        assert {c.ncvx for c in cs if c.shape == shape} == {"none", "mc", "me", "me_rtol", "mc_aniso"}
    assert all(c.ncvx == "none" for c in cs if c.shape in (R.UNALIGNED, R.STRIPS))
    eps = [c for c in cs if c.epsg == 2.5]
    assert len(eps) >= 3 and any(c.data == "mask" and c.prior == "tv10" and c.shape[1] > 128 for c in eps)
    assert all(c.prior != "haar" or (c.shape[0] % 8 == 0 and c.shape[1] % 8 == 0) for c in cs)


def test_mymala_refuses_a_prior_without_a_value_before_any_device_call():
    """A closed-form prior of prox.py has a prox and no value g(x): MYMALA's target exp(-f - epsg g) is undefined with it.  The Python classes say so
    before they build a problem (no device here: anything later would raise RuntimeError)."""
    import lmc_atomi_amd as la
    shape = (16, 64)
    pf = la.L2(b=np.zeros(shape), sigma=1.0, dims=shape)
    for pg in (la.Laplace(1.5), la.Huber(1.0, 0.5), la.GenGaussian(3, 0.2)):
        with pytest.raises(NotImplementedError, match="MYMALA.*closed-form prior"):
            la.MYMALASampler(pf, pg, shape, n_chains=2, tau=0.1, gamma=0.5)
        with pytest.raises(NotImplementedError, match="MYMALA.*closed-form prior"):
            la.MoreauYosidaMetropolisAdjustedLangevin(pf, pg, np.zeros(shape), tau=0.1, gamma=0.5, niter=2, n_chains=2, dims=shape)

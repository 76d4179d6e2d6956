"""Chain-group moments (lmc_group_moments / lmc_sampler_set_chain_groups / lmc_sampler_get_group_moments / lmc_allreduce_group_moments): per pixel and
chain group -- global chain id mod G -- the float64 sums of x and x^2 over the kept samples, and the Monte-Carlo error maps made of them.

The reference forms the same sums in np.longdouble from the fp32 states.  The tolerance of an entry that received n terms is (n - 1) 2^-53 sum |term|, the
float64 summation bound for any order: derived, not tuned.  The states are 100 + N(0, 1) -- a mean 100 times the spread, as in the images -- where an fp32
accumulator misses that bound by orders of magnitude.  An entry of one term is exact and an entry of none is exactly zero."""
import functools

import numpy as np
import pytest

from tests import test_gpu_block_moments as BM

pytestmark = pytest.mark.gpu

TAU, GAMMA = BM.TAU, BM.GAMMA
U = 2.0 ** -53
E_INVALID, E_STATE = -1, -5


@pytest.fixture(scope="module")
def la():
    import torch
    assert torch.cuda.is_available()
    import lmc_atomi_amd as la
    return la


def reference(xs, G, chain_offset=0):
    """kept states (a list of [C, H, W] fp32 arrays) -> S1, S2 (longdouble [G, H, W]), their tolerances, counts [G]"""
    shape = xs[0].shape[1:]
    S1, S2, A1 = (np.zeros((G,) + shape, dtype=np.longdouble) for _ in range(3))
    n = np.zeros(G, dtype=np.int64)
    for x in xs:
        assert x.dtype == np.float32
        xl = x.astype(np.longdouble)
        for c in range(x.shape[0]):
            g = (chain_offset + c) % G
            S1[g] += xl[c]
            A1[g] += np.abs(xl[c])
            S2[g] += xl[c] * xl[c]
            n[g] += 1
    terms = np.maximum(n - 1, 0).astype(np.longdouble).reshape((G,) + (1,) * len(shape))
    return S1, S2, terms * U * A1, terms * U * S2, n


def check(got1, got2, ref, tag="", slack=1):
    S1, S2, tol1, tol2, n = ref
    g1, g2 = got1.cpu().numpy(), got2.cpu().numpy()
    assert g1.dtype == np.float64 and g1.shape == S1.shape and g2.shape == S2.shape
    e1, e2 = np.abs(g1.astype(np.longdouble) - S1), np.abs(g2.astype(np.longdouble) - S2)
    with np.errstate(divide="ignore", invalid="ignore"):
        print(f"{tag}: worst error / tolerance S1 {np.nanmax(np.where(tol1 > 0, e1 / tol1, np.nan)) if (tol1 > 0).any() else 0:.3g}"
              f" S2 {np.nanmax(np.where(tol2 > 0, e2 / tol2, np.nan)) if (tol2 > 0).any() else 0:.3g}")
    assert (e1 <= slack * tol1).all(), (tag, "S1", float((e1 - slack * tol1).max()))
    assert (e2 <= slack * tol2).all(), (tag, "S2", float((e2 - slack * tol2).max()))
    for g in np.flatnonzero(n == 0):
        assert not g1[g].any() and not g2[g].any(), (tag, "an empty group is not zero", g)


@functools.lru_cache(maxsize=None)
def states(shape, C_):
    x = (100.0 + np.random.default_rng(shape[1] + C_).standard_normal((C_,) + shape)).astype(np.float32)
    return x


@functools.lru_cache(maxsize=None)
def states_reference(shape, C_, G, off):
    return reference([states(shape, C_)], G, off)


# (9, 7): 63 pixels, less than one wave, H W % 4 != 0: the scalar form; (5, 7): the same, smaller; (16, 64): the vector form, whole workgroups at every G;
# (19, 203): odd, the scalar form over several workgroups; (33, 520): the vector form with a partial last workgroup.  3 chains: fewer chains than groups at
# G = 16 and 64 (empty groups) and only the tail of the chain loop; 37: the unrolled loop at G = 2 and 3 (19 and 13 chains per group), its tail at 16.
@pytest.mark.parametrize("off", [0, 5])
@pytest.mark.parametrize("G", [2, 3, 16, 64])
@pytest.mark.parametrize("C_", [3, 37])
@pytest.mark.parametrize("shape", [(9, 7), (5, 7), (16, 64), (19, 203), (33, 520)])
def test_stateless_pass_matches_the_long_double_reference(la, shape, C_, G, off):
    import torch
    x = states(shape, C_)
    ref = states_reference(shape, C_, G, off)
    if C_ < G:
        assert (ref[4] == 0).sum() == G - C_
    xd = torch.from_numpy(x).cuda()
    S1, S2 = la.group_moments(xd, G, chain_offset=off)
    assert S1.dtype == torch.float64 and tuple(S1.shape) == (G,) + shape and S1.is_cuda and S2.is_cuda
    check(S1, S2, ref, f"{shape} C={C_} G={G} off={off}")
    T1, T2 = la.group_moments(xd, G, chain_offset=off)                  # fresh outputs: equal bits
    np.testing.assert_array_equal(T1.cpu().numpy(), S1.cpu().numpy())
    np.testing.assert_array_equal(T2.cpu().numpy(), S2.cpu().numpy())
    first = S1.cpu().numpy().copy(), S2.cpu().numpy().copy()
    again = la.group_moments(xd, G, chain_offset=off, out=(S1, S2))     # ADDS: twice the sums, exactly (s + s)
    assert again[0] is S1 and again[1] is S2
    np.testing.assert_array_equal(S1.cpu().numpy(), 2 * first[0])
    np.testing.assert_array_equal(S2.cpu().numpy(), 2 * first[1])


def test_more_chains_than_a_16_bit_index_holds(la):
    import torch
    C_, shape, G = 65537, (2, 4), 3
    x = (100.0 + np.random.default_rng(1).standard_normal((C_,) + shape)).astype(np.float32)
    ref = reference([x], G, 0)
    assert ref[4].tolist() == [21846, 21846, 21845]
    S1, S2 = la.group_moments(torch.from_numpy(x).cuda(), G)
    check(S1, S2, ref, "65537 chains")


def test_a_view_one_float_into_a_buffer_takes_the_scalar_form_and_is_right(la):
    """(16, 64) is the vector form's shape, but the array starts 4 bytes past a 16-byte boundary, where the launcher falls back to the scalar form.  What
    the test shows is that such an array is summed right; it cannot tell which form ran, since both walk the chains of a (group, pixel) in the same
    order and so give the sums of the aligned array bit for bit."""
    import torch
    shape, C_, G = (16, 64), 37, 3
    x = states(shape, C_)
    buf = torch.zeros(x.size + 4, dtype=torch.float32, device="cuda")
    view = buf[1:1 + x.size].view((C_,) + shape)
    view.copy_(torch.from_numpy(x))
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    S1, S2 = la.group_moments(view, G, chain_offset=5)
    check(S1, S2, states_reference(shape, C_, G, 5), "misaligned view")
    A1, A2 = la.group_moments(torch.from_numpy(x).cuda(), G, chain_offset=5)
    np.testing.assert_array_equal(S1.cpu().numpy(), A1.cpu().numpy())
    np.testing.assert_array_equal(S2.cpu().numpy(), A2.cpu().numpy())


def test_stateless_pass_refuses_what_it_cannot_group(la):
    import torch
    x = torch.zeros((3, 4, 4), dtype=torch.float32, device="cuda")
    for bad in (1, 65):
        with pytest.raises(ValueError):
            la.group_moments(x, bad)
    with pytest.raises(ValueError):
        la.group_moments(x, 2, out=(torch.zeros((2, 4, 4), device="cuda"), torch.zeros((2, 4, 4), device="cuda")))      # fp32 outputs
    same = torch.zeros((2, 4, 4), dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match="DISTINCT"):
        la.group_moments(x, 2, out=(same, same))
    lib = la._dev.lib()
    out = torch.zeros((2, 4, 4), dtype=torch.float64, device="cuda")
    p = la._dev.ptr
    assert lib.lmc_group_moments(p(x), 3, 0, 4, 4, 1, p(out), p(out), None) == E_INVALID
    assert lib.lmc_group_moments(p(x), 3, 0, 4, 4, 65, p(out), p(out), None) == E_INVALID
    assert lib.lmc_group_moments(p(x), 3, 0, 4, 4, 2, None, p(out), None) == E_INVALID
    assert lib.lmc_group_moments(p(x), 3, -1, 4, 4, 2, p(out), p(out), None) == E_INVALID


# ---- samplers: the sampler under test runs all iterations in ONE step call; a twin with the same seed steps `stride` iterations at a time and records
# get_state() at the kept iterations (burn_in = 3, thin = 2: the iterations 3, 5, 7, ... counted from 0)
BURN, THIN, NIT = 3, 2, 14


def mymala_problem(la, shape, rng):
    img = np.zeros(shape)
    img[6:12, 24:72] = 150.0
    img += np.linspace(0, 30, shape[1])[None, :]
    h = np.ones((5, 5)) / 25.0
    pf = la.L2(Op=la.Convolve2D(shape, h, offset=(2, 2)), b=img + rng.normal(0, BM.SIGMA, shape), sigma=1 / BM.SIGMA ** 2)
    return img, pf, la.TV(shape, sigma=0.3, niter=5)


def sampler_case(la, kind, C_):
    """-> (make(**extra) -> sampler, x0, shape, stride of the twin, kernel the sampler must report or None)"""
    rng = np.random.default_rng(7)
    stride, kernel = 1, None
    if kind == "myula_tv":
        shape = (16, 136)
        y, pf, pg = BM.blur_problem(la, shape, rng, "tv", level=100.0)
        make = lambda **kw: la.MYULASampler(pf, pg, shape, n_chains=C_, tau=TAU, gamma=GAMMA, seed=5, **kw)
        kernel = "pipe"
    elif kind.startswith("myula_l2_pair"):
        # two iterations per launch: the states of a pair launch equal those of single launches to fp32 rounding only (tests/test_gpu_rows_pair.py), so the
        # twin steps a PAIR at a time -- the same launches -- and the kept iterations 3, 5, ... are the second of their pairs, which get_state() returns
        shape = (40, 64)
        y, pf, pg = BM.blur_problem(la, shape, rng, "l2", level=100.0)
        pol = {"iterations_per_launch": 2, "moments_overlap": 1 if kind.endswith("side") else -1}
        make = lambda **kw: la.MYULASampler(pf, pg, shape, n_chains=C_, tau=TAU, gamma=GAMMA, seed=5, policy=pol, **kw)
        stride, kernel = 2, "rows_pair"
    elif kind == "mymala":
        shape = (24, 96)
        img, pf, pg = mymala_problem(la, shape, rng)
        # a step at which about two proposals in three are accepted (at 0.01 gamma none is): kept iterates that moved and kept iterates that stayed
        make = lambda **kw: la.MYMALASampler(pf, pg, shape, n_chains=C_, tau=0.0003 * GAMMA, gamma=GAMMA, seed=9, **kw)
        return make, np.broadcast_to(img.astype(np.float32), (C_,) + shape).copy(), shape, 1, None
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
    return make, x0, shape, stride, kernel


def twin_states(make, x0, stride, nit=NIT):
    kept, stayed = [], 0
    twin = make()
    try:
        twin.set_state(x0)
        prev = x0
        for done in range(stride, nit + 1, stride):
            twin.step(stride)
            it = done - 1
            if it >= BURN and (it - BURN) % THIN == 0:
                x = twin.get_state().cpu().numpy()
                stayed += int((x.reshape(len(x), -1) == prev.reshape(len(x), -1)).all(axis=1).sum())
                kept.append(x)
            prev = twin.get_state().cpu().numpy()
        return kept, prev, stayed
    finally:
        twin.close()


@pytest.mark.parametrize("C_", [12, 10])
@pytest.mark.parametrize("kind", ["myula_tv", "myula_l2_pair_inline", "myula_l2_pair_side", "mymala", "skrock", "ulpda"])
def test_sampler_group_moments_match_the_states_of_a_stepping_twin(la, kind, C_):
    G = 4
    make, x0, shape, stride, kernel = sampler_case(la, kind, C_)
    kept, final, stayed = twin_states(make, x0, stride)
    assert len(kept) == 6
    ref = reference(kept, G, 0)
    assert ref[4].tolist() == ([18] * 4 if C_ == 12 else [18, 18, 12, 12])
    smp = make(moments=True, burn_in=BURN, thin=THIN, chain_groups=G)
    try:
        assert smp.chain_groups == G
        smp.set_state(x0)
        smp.step(NIT)
        if kernel:
            assert kernel in smp.kernel_name, smp.kernel_name
        np.testing.assert_array_equal(smp.get_state().cpu().numpy(), final)
        S1, S2, counts = smp.group_moments()
        s1, s2, count = smp.moments()
        T1, T2, tcounts = smp.allreduce_group_moments(None)              # NULL communicator: a plain copy
        U1, U2, ucounts = la.allreduce_sampler_group_moments(smp)        # no process group
    finally:
        smp.close()
    import torch
    assert counts.dtype == torch.int64 and not counts.is_cuda and tuple(counts.shape) == (G,)
    assert counts.tolist() == ref[4].tolist() and int(counts.sum()) == count == 6 * C_
    check(S1, S2, ref, f"{kind} x {C_}")
    for a, b in ((T1, S1), (T2, S2), (U1, S1), (U2, S2)):
        np.testing.assert_array_equal(a.cpu().numpy(), b.cpu().numpy())
    assert tcounts.tolist() == counts.tolist() == ucounts.tolist()
    # the pixel moments hold the same 6 C terms per pixel in another order: both lie within (6 C - 1) 2^-53 sum |term| of the exact sum
    whole = reference(kept, 1, 0)
    for got, acc, exact, tol in ((S1, s1, whole[0][0], whole[2][0]), (S2, s2, whole[1][0], whole[3][0])):
        total = got.cpu().numpy().sum(axis=0).astype(np.longdouble)
        assert (np.abs(total - exact) <= tol).all()
        assert (np.abs(total - acc.cpu().numpy().astype(np.longdouble)) <= 2 * tol).all()
    if kind == "mymala":
        print("chains that stayed at a kept iteration:", stayed)
        assert 0 < stayed < 6 * C_, "expected rejections and acceptances among the kept iterations at this step size"


def test_pair_launches_that_keep_the_iterate_in_between_give_equal_bits_on_both_streams(la):
    """thin = 1 under two iterations per launch: the first iterate of every pair is kept too -- on the side stream it is reduced out of an array of its own.
    No step(1) replay reproduces these states, so the two routes are compared with each other -- one owner per entry and ordered launches mean equal bits --
    and each with the pixel moments of its own handle, which another kernel forms from the same iterates: sum_g S_g and s are two float64 sums of the same
    n = 9 x 10 terms per pixel, each within (n - 1) 2^-53 sum |term| of the exact sum, and with states near 100 every term is positive, so sum |term| is the
    sum itself."""
    G, C_ = 4, 10
    out = []
    for kind in ("myula_l2_pair_inline", "myula_l2_pair_side"):
        make, x0, shape, _, kernel = sampler_case(la, kind, C_)
        smp = make(moments=True, burn_in=1, thin=1, chain_groups=G)
        try:
            smp.set_state(x0)
            smp.step(10)
            assert kernel in smp.kernel_name, smp.kernel_name
            S1, S2, counts = smp.group_moments()
            s1, s2, count = smp.moments()
            assert count == 90 == int(counts.sum())
            for S, acc in ((S1, s1), (S2, s2)):
                total, acc = S.cpu().numpy().sum(axis=0), acc.cpu().numpy()
                assert acc.min() > 0
                assert (np.abs(total - acc) <= 2 * (count - 1) * U * acc).all(), (kind, float(np.abs(total - acc).max()))
            out.append((S1.cpu().numpy(), S2.cpu().numpy(), counts.tolist(), smp.get_state().cpu().numpy()))
        finally:
            smp.close()
    assert out[0][2] == out[1][2] == [27, 27, 18, 18]
    for a, b in zip(out[0], out[1]):
        np.testing.assert_array_equal(a, b)
    assert out[0][0].min() > 0


def test_two_handles_of_7_and_5_chains_together_equal_one_of_12(la):
    G, nit = 4, 5
    rng = np.random.default_rng(31)
    shape = (16, 136)
    y, pf, pg = BM.blur_problem(la, shape, rng, "tv", level=100.0)
    x0 = (100.0 + rng.normal(0, 1.0, (12,) + shape)).astype(np.float32)
    kw = dict(tau=TAU, gamma=GAMMA, seed=7, moments=True, chain_groups=G)
    got, kept = [], []
    for off, n in ((0, 12), (0, 7), (7, 5)):
        smp = la.MYULASampler(pf, pg, shape, n_chains=n, chain_offset=off, **kw)
        try:
            smp.set_state(x0[off:off + n])
            if n == 12:                                    # the whole job steps one iteration at a time and shows its states
                for _ in range(nit):
                    smp.step(1)
                    kept.append(smp.get_state().cpu().numpy())
            else:
                smp.step(nit)
            S1, S2, counts = smp.group_moments()
            got.append((S1.cpu().numpy(), S2.cpu().numpy(), counts.numpy()))
        finally:
            smp.close()
    ref = reference(kept, G, 0)
    whole, first, second = got
    assert whole[2].tolist() == [3 * nit] * 4
    assert first[2].tolist() == [2 * nit, 2 * nit, 2 * nit, nit] and second[2].tolist() == [nit, nit, nit, 2 * nit]
    import torch
    check(torch.from_numpy(whole[0]), torch.from_numpy(whole[1]), ref, "one handle of 12")
    check(torch.from_numpy(first[0] + second[0]), torch.from_numpy(first[1] + second[1]), ref, "7 + 5")
    check(torch.from_numpy(first[0]), torch.from_numpy(first[1]), reference([x[:7] for x in kept], G, 0), "the handle of 7")
    check(torch.from_numpy(second[0]), torch.from_numpy(second[1]), reference([x[7:] for x in kept], G, 7), "the handle of 5")


def test_reset_refusals_empty_groups_and_a_sapg_call(la):
    import torch
    shape = (16, 32)
    rng = np.random.default_rng(41)
    y, pf, pg = BM.blur_problem(la, shape, rng, level=100.0)
    lib = la._dev.lib()

    def refused(rc, code):
        assert rc == code, (rc, code)
        assert lib.lmc_last_error(), "lmc_last_error() is empty"

    kw = dict(n_chains=3, tau=TAU, gamma=GAMMA, seed=1)
    smp = la.MYULASampler(pf, pg, shape, moments=True, **kw)
    off = la.MYULASampler(pf, pg, shape, **kw)
    try:
        smp.set_state(np.full(shape, 100.0, dtype=np.float32))
        refused(lib.lmc_sampler_get_group_moments(smp._h, None, None, None, None), E_INVALID)         # get without set
        refused(lib.lmc_allreduce_group_moments(smp._h, None, None, None, None, None), E_INVALID)
        with pytest.raises(ValueError):
            smp.group_moments()
        for bad in (1, 65, -1):
            refused(lib.lmc_sampler_set_chain_groups(smp._h, bad), E_INVALID)
        refused(lib.lmc_sampler_set_chain_groups(off._h, 4), E_STATE)                                  # moments = 0
        assert lib.lmc_sampler_set_chain_groups(smp._h, 64) == 0                                       # more groups than chains: empty groups
        smp.chain_groups = 64
        assert lib.lmc_sampler_get_group_moments(smp._h, None, None, None, None) == 0                  # every output is nullable
        smp.step(2)
        S1, S2, counts = smp.group_moments()
        assert counts.tolist() == [2, 2, 2] + [0] * 61 and smp.moments()[2] == 6
        assert not S1[3:].any() and not S2[3:].any() and bool((S1[:3] > 0).all())
        refused(lib.lmc_sampler_set_chain_groups(smp._h, 8), E_STATE)                                  # after a kept sample
        refused(lib.lmc_sampler_set_chain_groups(smp._h, 0), E_STATE)
        smp.reset_moments()
        S1, S2, counts = smp.group_moments()
        assert counts.tolist() == [0] * 64 and not S1.any() and not S2.any()
        assert lib.lmc_sampler_set_chain_groups(smp._h, 2) == 0                                        # empty again: the groups may change
        smp.chain_groups = 2
        smp.step(1)
        x = smp.get_state().cpu().numpy()
        S1, S2, counts = smp.group_moments()
        assert counts.tolist() == [2, 1]
        check(S1, S2, reference([x], 2, 0), "after a reset")
        # lmc_sampler_sapg: the accumulators take nothing, the counts stay, the iteration counter advances
        before = S1.cpu().numpy(), S2.cpu().numpy()
        it0 = smp.iteration
        smp.estimate_prior_weight(4, (1e-3, 1e2), theta0=0.3, warmup=2, iters_per_update=2)
        assert smp.iteration == it0 + 2 + 4 * 2
        S1, S2, counts = smp.group_moments()
        assert counts.tolist() == [2, 1] and smp.moments()[2] == 3
        np.testing.assert_array_equal(S1.cpu().numpy(), before[0])
        np.testing.assert_array_equal(S2.cpu().numpy(), before[1])
        smp.step(1)                                                                                    # and they take samples again afterwards
        assert smp.group_moments()[2].tolist() == [4, 2]
        smp.reset_moments()
        assert lib.lmc_sampler_set_chain_groups(smp._h, 0) == 0                                        # off again
        refused(lib.lmc_sampler_get_group_moments(smp._h, None, None, None, None), E_INVALID)
        smp.chain_groups = None
        smp.step(1)                                                                                    # and the sampler goes on without them
        assert smp.moments()[2] == 3
    finally:
        smp.close()
        off.close()


def test_end_to_end_on_a_chain_with_a_known_answer(la):
    """MYULA with f = |x - y|^2 / 2, g = |x|^2 / 2, gamma = 1, tau = 1/3 is x' = x / 2 + y / 3 + sqrt(2/3) xi: the AR(1) process with rho = 0.5 and
    stationary variance (2/3) / (1 - 1/4) = 8/9, whose mean of N samples has variance (8/9) 3 / N and effective sample size N / 3.  64 chains, 32 groups,
    400 kept iterations at 9 x 7: the medians over the pixels scatter by about 2 % (simulated: mcse 0.951 .. 1.011, ess 0.98 .. 1.11 of the targets)."""
    shape, C_, G, burn, kept = (9, 7), 64, 32, 50, 400
    rng = np.random.default_rng(3)
    y = 3.0 + rng.standard_normal(shape)
    pf, pg = la.L2(b=y, sigma=1.0, dims=shape), la.L2(sigma=1.0)
    res = la.MoreauYosidaUnadjustedLangevin(pf, pg, y.ravel(), tau=1.0 / 3.0, gamma=1.0, niter=burn + kept, seed=11, n_chains=C_, burn_in=burn,
                                            dims=shape, chain_groups=G)
    N = C_ * kept
    assert res.count == N and res.group_counts.tolist() == [2 * kept] * G
    for m in (res.mcse_mean, res.mcse_var, res.ess):
        assert tuple(m.shape) == shape and m.dtype.is_floating_point and m.is_cuda
    var = float(np.median(res.var.cpu().numpy()))
    mcse = float(np.median(res.mcse_mean.cpu().numpy()))
    ess = float(np.median(res.ess.cpu().numpy()))
    print(f"median var / (8/9) = {var / (8 / 9):.4f}  median mcse_mean / sqrt((8/9) 3 / N) = {mcse / np.sqrt((8 / 9) * 3 / N):.4f}"
          f"  median ess / (N / 3) = {ess / (N / 3):.4f}")
    np.testing.assert_allclose(res.mean.cpu().numpy(), 2.0 * y / 3.0, rtol=0, atol=6 * np.sqrt((8 / 9) * 3 / N))
    assert abs(var / (8 / 9) - 1) <= 0.02, var
    assert abs(mcse / np.sqrt((8 / 9) * 3 / N) - 1) <= 0.15, mcse
    assert abs(ess / (N / 3) - 1) <= 0.25, ess
    plain = la.MoreauYosidaUnadjustedLangevin(pf, pg, y.ravel(), tau=1.0 / 3.0, gamma=1.0, niter=2, seed=11, n_chains=4, dims=shape)
    assert plain.mcse_mean is None and plain.mcse_var is None and plain.ess is None and plain.group_counts is None


def test_the_other_entry_points_return_the_error_maps(la):
    shape = (16, 64)
    rng = np.random.default_rng(5)
    y, pf, pg = BM.blur_problem(la, shape, rng)

    def shown(res, n):
        assert res.group_counts.tolist() == [n // 2, n // 2] and res.count == n
        for m in (res.mcse_mean, res.mcse_var, res.ess):
            assert tuple(m.shape) == shape
        assert bool((res.mcse_mean > 0).all()) and bool((res.ess > 0).all())

    shown(la.UnadjustedLangevinPrimalDual(pf, la.L21(sigma=0.3), la.Gradient(shape), y.ravel(), 0.95 * GAMMA, 1.0, niter=5, seed=2, gfirst=False,
                                          n_chains=4, burn_in=1, chain_groups=2), 16)
    shown(la.MoreauYosidaMetropolisAdjustedLangevin(pf, pg, y.ravel(), tau=0.01 * GAMMA, gamma=GAMMA, niter=5, seed=2, n_chains=4, burn_in=1,
                                                    chain_groups=2), 16)
    shown(la.StabilisedLangevin(pf, pg, y.ravel(), tau=TAU, gamma=GAMMA, niter=5, n_stages=3, seed=2, n_chains=4, burn_in=1, chain_groups=2), 16)
    out = la.sharded_myula(pf, pg, shape, 4, y, TAU, GAMMA, niter=5, seed=2, burn_in=1, chain_groups=2)
    assert len(out) == 4 and out.group_counts.tolist() == [8, 8] and tuple(out.mcse_mean.shape) == shape and out.hist is None
    res = la.MoreauYosidaUnadjustedLangevin(pf, pg, y.ravel(), tau=TAU, gamma=GAMMA, niter=5, seed=2, n_chains=4, burn_in=1, chain_groups=2)
    np.testing.assert_array_equal(out.mcse_mean.cpu().numpy(), res.mcse_mean.cpu().numpy())
    np.testing.assert_array_equal(out.ess.cpu().numpy(), res.ess.cpu().numpy())

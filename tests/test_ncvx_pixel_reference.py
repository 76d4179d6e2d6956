"""The per-pixel harness of the non-convex data terms (tests/_ncvx_pixel.py) checked on itself, on the CPU, for every case of the GPU file
(tests/test_gpu_ncvx_pixel.py imports the same lists): the three conditions on the inputs, the agreement of the dtype-generic restatement with
`O.L2NcvxTV` in float64, the independence of the replay order, both float32 replays inside the bound -- and five faults of the stencil planted on the
launch-form replay, each reported in bounds and in rel-L2 of the state against the 5e-5 the norm tests assert:

  1. the term's last row scaled by 1 - 5e-3;
  2. vy of the column left of a declared seam (64 in the tile, split and point kernels, a block boundary at 8, a lane-group boundary at 128 and the strip
     boundary at 512 in the pipe kernel) taken as zero at that one column;
  3. the isotropic weight used on one row of an anisotropic case;
  4. the (i, j-1) neighbour's dx formed as if a row existed below the last row;
  5. ME-TV: the inner prox one dual iteration short along one tile's top row (the fault of DESIGN section 4, named risk 2).

The bound rejects 1 to 4 at both weightings and 5 at the prominent one; the norm accepts 1 on every chosen case (`test_planted_faults` prints the rest)."""
import numpy as np
import pytest

from oracle import lmc_oracle as O
import _ncvx_pixel as N
import _pixel as X


def test_the_matrix_has_every_family_and_unique_ids():
    assert {n.base.family for n in N.CASES} == set(N.FAMILIES)
    assert len(set(N.IDS)) == len(N.IDS) and len(N.CASES) >= 150
    for n in N.CASES:
        H, W = n.base.shape
        assert all(0 < s < H for s in n.base.seam_rows) and all(0 < s < W for s in n.base.seam_cols), N.case_id(n)
        assert n.weight in ("cfg", "prom") and n.nc in ("mc", "mca", "me") and (n.niter > 0) == (n.nc == "me")
    for fam in N.FAMILIES:       # every family at both weightings
        assert {n.weight for n in N.CASES if n.base.family == fam} == {"cfg", "prom"}, fam
    assert abs(N.lam_of(N.CASES[1]) * X.TAU - 1) < 1e-6 and N.lam_of(N.CASES[0]) == float(np.float32(0.3))


def _check_conditions(tag, n, x0, stage):
    share, flat = N.conditions(n, x0)
    H = x0.shape[-2]
    assert 0.2 <= share <= 0.8, (tag, share)
    assert flat >= (4 if H >= 3 else 2), (tag, flat)           # 2 x 2 pixels with |grad x| = 0 exactly (1 x 2 on a single row)
    r0, r1, c0, c1 = N.flat_block(x0.shape[-2:])
    assert np.all(x0[:, r0:r1, c0:c1] == np.float32(N.FLAT_LEVEL))
    if n.weight == "prom":
        med = float(np.median(stage.contrib)) / stage.bound
        assert med >= 1e3, (tag, med)


@pytest.mark.parametrize("n", N.CASES, ids=N.IDS)
def test_conditions_on_the_inputs(n):
    _check_conditions(N.case_id(n), n, N.problem(n).x0, N.reference(n)[0])


@pytest.mark.parametrize("c", N.P_CASES, ids=N.P_IDS)
def test_conditions_on_the_inputs_of_the_prox_cases(c):
    _check_conditions(X.case_id(c), c, N.p_problem(c).x0, N.p_reference(c))


def _oracle_term(shape, nc, niter, lam, Op, b, sigma):
    kw = dict(dims=shape, Op=Op, b=b.ravel(), sigma=sigma, lamda=lam, gamma=N.CFG_GAMMA)
    if nc == "me":
        return O.L2NcvxTV(isotropic=True, niter=niter, **kw)
    return O.L2NcvxTV(Op2=O.Gradient(shape), isotropic=nc == "mc", **kw)


def _close(a, b, tag):
    d = float(np.max(np.abs(a - b)))
    assert d <= 1e-12 * max(1.0, float(np.max(np.abs(b)))), (tag, d)


@pytest.mark.parametrize("n", N.CASES, ids=N.IDS)
def test_float64_restatement_equals_the_checkers_class(n):
    c, m, shape = n.base, N.problem(n), n.base.shape
    if m.h is not None:
        Op = O.Convolve2D(shape, m.h.astype(np.float64), m.offset)
    elif m.mask is not None:
        Op = O.Diagonal(m.mask.astype(np.float64).ravel())
    else:
        Op = O.Identity(shape[0] * shape[1])
    step = N.Step(n, np.float64)
    of = _oracle_term(shape, n.nc, n.niter, step.lam, Op, m.y.astype(np.float64), m.sigma_f)
    x = m.x0.astype(np.float64)
    mine_m, mine_g = step.term(x), step.grad(x)
    for ch in range(N.N_CHAINS):
        _close(mine_m[ch].ravel(), of.grad_moreau(x[ch].ravel().copy()), "grad_moreau")
        _close(mine_g[ch].ravel(), of.grad(x[ch].ravel().copy()), "grad")
    if c.mode == "restart" and c.prior in ("tv", "l1", "l2", "none"):      # ... and the step the checker's own loop (`O.myula`)
        og = {"tv": O.TV(shape, sigma=X.weight(c), niter=c.K), "l1": O.L1(sigma=X.weight(c)), "l2": O.L2(sigma=X.weight(c)), "none": None}[c.prior]
        if og is not None:
            want = O.myula(of, og, x[0].ravel(), m.tau, m.gamma, niter=1, noise=[m.noise[0, 0].astype(np.float64).ravel()])[-1].reshape(shape)
            _close(N.reference(n)[0].ref64[0], want, "myula")


@pytest.mark.parametrize("c", N.P_CASES, ids=N.P_IDS)
def test_float64_prox_equals_the_checkers_class(c):
    """The pre-step and the closed-form solve against `O.L2NcvxTV.prox` (CG on a system with at most two eigenvalues: converged to round-off)."""
    m, shape = N.p_problem(c), c.shape
    Op = O.Diagonal(m.mask.astype(np.float64).ravel()) if m.mask is not None else O.Identity(shape[0] * shape[1])
    x = m.x0.astype(np.float64)
    ref = N.p_reference(c).ref64
    for ch in range(N.N_CHAINS):
        of = _oracle_term(shape, c.nc, c.niter, N.p_lam(c), Op, m.b.astype(np.float64), N.P_SIGMA)
        of.niter = 50
        want = of.prox(x[ch].ravel(), N.P_TAU).reshape(shape)
        assert np.max(np.abs(ref[ch] - want)) <= 1e-9 * np.max(np.abs(want)), X.case_id(c)


@pytest.mark.parametrize("n", N.CASES, ids=N.IDS)
def test_replays_inside_the_bound_and_independent_of_their_order(n):
    stages = N.reference(n)
    again = N._reference(n, order=(2, 1, 0))
    assert len(stages) == n.base.iters == len(again)
    for it, (st, ag) in enumerate(zip(stages, again)):
        for a, b in ((st.ref64, ag.ref64), (st.ref32, ag.ref32), (st.alt32, ag.alt32)):
            assert np.array_equal(a, b), (N.case_id(n), it)
        assert np.isfinite(st.e32) and st.e32 > 0 and np.isfinite(st.ref64).all()
        assert st.bound == max(X.FACTOR * st.e32, 2 * X.ulp32(np.abs(st.ref64).max()))
        for r in (st.ref32, st.alt32):
            v = X.check(n.base, it, r, st)
            assert v.ok and v.err <= st.e32 and v.err <= st.bound / X.FACTOR, v.message


@pytest.mark.parametrize("c", N.P_CASES, ids=N.P_IDS)
def test_prox_replays_inside_the_bound(c):
    st = N.p_reference(c)
    assert np.isfinite(st.e32) and st.e32 > 0
    for r in (st.ref32, st.alt32):
        v = X.check(c, 0, r, st)
        assert v.ok and v.err <= st.bound / X.FACTOR, v.message


@pytest.mark.parametrize("c", N.E_CASES, ids=N.E_IDS)
def test_value_reference_equals_the_checkers_class(c):
    h, off, y, x0 = N.e_problem(c.shape)
    of = _oracle_term(c.shape, c.nc, 0, N.e_lam(), O.Convolve2D(c.shape, h.astype(np.float64), off), y.astype(np.float64), 1 / X.SIGMA ** 2)
    want, tol, _ = N.e_reference(c)
    for ch in range(N.N_CHAINS):
        v = of(x0[ch].astype(np.float64).ravel())
        assert abs(v - want[ch]) <= 1e-12 * abs(v), (c.tag, v, want[ch])
    assert np.all(tol >= N.E_FLOOR * np.abs(want))


@pytest.mark.parametrize("c", N.S_CASES, ids=N.S_IDS)
def test_blur_prox_and_sampler_references(c):
    """The conditions, the truncation condition of tests/_ulpda_pixel.py (float64 CG two iterations short within e32 / 10 of the solution), both float32
    replays inside the bounds of the state and of the dual, and the float64 iteration equal to the checker's own loop (`O.ulpda`) where the solve is
    closed form."""
    m, stages = N.s_problem(c), N.s_reference(c)
    assert len(stages) == (1 if c.entry == "prox" else 2)
    share, flat = N.conditions(c, m.x0)
    assert 0.2 <= share <= 0.8 and flat >= 4, (share, flat)
    for it, st in enumerate(stages):
        if c.weight == "prom":
            assert float(np.median(st.contrib)) >= 1e3 * st.x.bound
        assert (st.trunc is None) == (m.h is None)
        if st.trunc is not None:
            assert st.trunc <= st.x.e32 / 10, (st.trunc, st.x.e32)
        for r in (st.x,) + (st.y or ()):
            assert np.isfinite(r.e32) and r.e32 > 0
            for rep in (r.ref32, r.alt32):
                v = X.check(c, it, rep, r)
                assert v.ok and v.err <= r.bound / X.FACTOR, v.message
    if c.entry == "sampler" and m.h is None:
        class _F:
            def prox(self, v, tau):
                return N.SProx(c, "exact")(v.reshape((1,) + c.shape)).ravel()
        st = stages[0]
        for ch in range(N.N_CHAINS):
            xs, ys = O.ulpda(_F(), O.L21(ndim=2, sigma=N.U.RADIUS), O.Gradient(c.shape), m.x0[ch].astype(np.float64).ravel(), N.S_TAU, N.S_MU,
                             y0=m.y0[ch].astype(np.float64).ravel(), theta=N.S_THETA, niter=1, gfirst=False, returny=True,
                             noise=[m.noise[0, ch].astype(np.float64).ravel()])
            _close(st.x.ref64[ch].ravel(), xs[0], "ulpda x")
            _close(np.stack([st.y[0].ref64[ch], st.y[1].ref64[ch]]).ravel(), ys[0], "ulpda y")


# ------------------------------------------------------------------ planted faults
def _find(family, shape, nc, tag, niter=0):
    """The case at both weightings."""
    out = []
    for w in ("cfg", "prom"):
        got = [n for n in N.CASES if (n.base.family, n.base.shape, n.weight) == (family, shape, w) and n.base.tag == f"{nc}{niter or ''}-{tag}-{w}"]
        assert len(got) == 1, (family, shape, nc, tag, w, len(got))
        out.append(got[0])
    return out


# (family, shape, tag, seam column of fault 2, row of fault 3)
MC_REPS = [("tile", (66, 67), "tv10-A", 64, 64), ("split", (6, 257), "tv10-A", 64, 3), ("point", (34, 130), "l1-A", 64, 32), ("block", (16, 72), "haar-identity", 8, 8),
           ("pipe", (6, 264), "tv10-A", 128, 3), ("pipe", (6, 513), "tv10-A-strips", 512, 3)]
# (family, shape, tag, niter, (row, first column, end column) of fault 5: the top row of one tile / band / the middle of the pipeline)
ME_REPS = [("tile", (66, 67), "tv10-A", 50, (64, 0, 64)), ("tile", (66, 67), "tv10-A", 17, (64, 0, 64)), ("split", (5, 129), "tv10-A", 10, (2, 64, 128)),
           ("rows", (17, 67), "l1-A", 10, (16, 0, 67)), ("pipe", (6, 264), "tv10-A", 50, (3, 0, 264))]


def _planted(n, fault):
    """(err in bounds, rel-L2 of the state) of the launch-form replay with `fault`, first iteration."""
    m, st = N.problem(n), N.reference(n)[0]
    got = N.Step(n, np.float32, fault).launch(m.x0, m.noise[0])
    clean = N.Step(n, np.float32).launch(m.x0, m.noise[0])
    assert np.array_equal(clean, st.alt32) and not np.array_equal(got, clean), (N.case_id(n), fault)
    v = X.check(n.base, 0, got, st)
    return v, v.err / st.bound, N.rel(got, st.ref64)


def test_planted_faults():
    rows = []
    for fam, shape, tag, seam, row in MC_REPS:
        for n in _find(fam, shape, "mc", tag):
            for name, fault in (("1 last row", ("last-row",)), ("2 seam vy", ("seam-vy", seam)), ("4 row below", ("row-below",))):
                v, nb, r = _planted(n, fault)
                rows.append((name, N.case_id(n), nb, r, v.region))
                assert not v.ok and nb > 1, (name, v.message)
                if name[0] == "1":
                    assert r < N.NORM_RTOL, (N.case_id(n), r)          # the norm accepts it
                    assert v.region in ("last row", "corner"), v.message
        if (fam, shape) == ("pipe", (6, 513)):
            continue       # (the strip boundary has an isotropic case of its own only for fault 2)
        for n in _find(fam, shape, "mca", tag):
            for name, fault in (("1 last row", ("last-row",)), ("3 iso weight", ("iso-row", row))):
                v, nb, r = _planted(n, fault)
                rows.append((name, N.case_id(n), nb, r, v.region))
                assert not v.ok and nb > 1, (name, v.message)
                if name[0] == "1":
                    assert r < N.NORM_RTOL, (N.case_id(n), r)
    for fam, shape, tag, niter, where in ME_REPS:
        for n in _find(fam, shape, "me", tag, niter):
            v, nb, r = _planted(n, ("short-row",) + where)
            rows.append(("5 short prox", N.case_id(n), nb, r, v.region))
            if n.weight == "prom":
                assert not v.ok and nb > 1, v.message
    for name, cid, nb, r, reg in rows:
        print(f"planted {name:14s} {cid:44s} {nb:10.1f} bounds  rel-L2 {r:.2e} ({'accepted' if r < N.NORM_RTOL else 'rejected'} by the norm)  [{reg}]")
    under = [(cid, nb) for name, cid, nb, r, reg in rows if name[0] == "5" and nb <= 1]
    print("fault 5 under one bound at the configured weight:", under or "none")

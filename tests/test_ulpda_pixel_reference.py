"""The per-pixel harness of tests/_ulpda_pixel.py checked on itself, on the CPU, for every case of tests/test_gpu_ulpda_pixel.py: the float32 replay
passes its own bound, the dtypes are right, the truncation conditions of the solves hold on the reference alone, every region class of a case has a
pixel -- and four planted faults, each rejected by the harness by at least three bounds and accepted by the three criteria the ULPDA tests had
(tests/test_gpu_ulpda.py: rel-L2 < 2e-4, 2e-3 for the dual; |r| <= 3e-6 |rhs| for the solve; a row maximum below 0.05), with both sides printed."""
import numpy as np
import pytest

from oracle import lmc_oracle as O
import _pixel as X
import _ulpda_pixel as U

OLD_X, OLD_Y, OLD_RES, OLD_ROW = 2e-4, 2e-3, 3e-6, 0.05


def test_the_matrix_covers_the_axes_the_shapes_and_the_paths():
    rs = [c for c in U.A_CASES if c.mode == "restart"]
    for shape in U.A_SHAPES4 + U.A_SHAPES1:
        mine = [c for c in rs if c.shape == shape]
        assert {c.gfirst for c in mine} == {True, False} and {c.prior for c in mine} == {"l21", "l1"} and {c.theta for c in mine} == {1.0, 0.5}, shape
        assert {c.z for c in mine} == {True, False} and {c.data for c in mine} == {"identity", "mask", "none"}, shape
    for shape in U.A_FULL:
        assert len({c[2:7] for c in rs if c.shape == shape}) == 48
    ph = [c for c in U.A_CASES if c.mode == "philox"]
    assert {c.shape[0] for c in ph} == {16, 17, 3, 5, 6, 7} and {c.shape[1] % 4 == 0 for c in ph} == {True, False}
    # the draw is four columns per thread and four rows per quad: every remainder of both
    assert {c.shape[0] % 4 for c in ph} == {0, 1, 2, 3} and {c.shape[1] % 4 for c in ph} == {0, 1, 2, 3}
    assert {c.family for c in U.B_CASES} == {"cheb", "cheb-uni", "cheb-pairs", "cg-rows", "cg-general"}
    for fam in ("cheb", "cheb-uni", "cheb-pairs"):
        assert any(c.family == fam and c.mode == "warm" for c in U.B_CASES), fam
    for c in U.B_CASES:
        assert U.expected_path(c) == c.family, (U.case_id(c), U.expected_path(c))
        H, W = c.shape
        assert all(0 < s < H for s in c.seam_rows) and all(0 < s < W for s in c.seam_cols), U.case_id(c)
    # the taps the dispatch tells apart: centred windows of 5 and 7, the even box in 7, and the two the row kernel refuses
    kt = {k: U.centred_taps(U.f32(h), off) for k, (h, off) in U.B_BLURS.items()}
    assert (kt["A"], kt["B"], kt["D"], kt["E"], kt["G"], kt["A0"]) == (5, 5, 7, 7, 0, 0), kt
    # ts = 1.74, sum |h| = 1, tolerance CHEB_TOL: the a-priori count is far below the cap of 50, so the Chebyshev path is kept
    plan = U.cheb_plan(U.b_ts(np.float32), U.f32(U.BLURS["A"][0]))
    assert plan is not None and plan.adaptive and plan.kmax <= 20, plan
    assert U.cheb_plan(U.b_ts(np.float32), U.f32(U.BLURS["A"][0]), cap=plan.kmax - 3) is None


def _regions_ok(c):
    regions = X.region_pixels(c)
    H, W = c.shape
    assert "corner" in regions
    if H >= 3 and W >= 3:
        assert {"first row", "last row", "first column", "last column", "interior"} <= set(regions), regions
    assert {f"row seam {s}" for s in c.seam_rows} | {f"column seam {s}" for s in c.seam_cols} <= set(regions), (regions, c.seam_rows, c.seam_cols)
    return regions


def _replay_ok(c, it, ref, regions, move=True):
    assert np.isfinite(ref.e32) and ref.e32 >= 0 and np.isfinite(ref.bound) and ref.bound > 0
    assert ref.ref64.dtype == np.float64 and ref.ref32.dtype == np.float32
    v = X.check(c, it, ref.ref32, ref)
    assert v.ok and v.err <= ref.e32 and ref.bound >= U.FACTOR * ref.e32, v.message
    if ref.alt32 is not None:       # the second replay: e32 is the larger of the two errors
        w = X.check(c, f"{it} (fma form)", ref.alt32, ref)
        assert w.ok and w.err <= ref.e32 == max(v.err, w.err), w.message
    if move:
        for reg, (i, j) in regions.items():
            moved = ref.ref64.copy()
            moved[U.N_CHAINS - 1, i, j] += 1.5 * ref.bound
            v = X.check(c, it, moved, ref)
            assert not v.ok and v.where == (U.N_CHAINS - 1, i, j) and v.region == reg, v.message


@pytest.mark.parametrize("c", U.A_CASES, ids=U.A_IDS)
def test_part_a_replay_passes_its_own_bound(c):
    stages = U.a_reference(c)
    assert len(stages) == c.iters
    regions = _regions_ok(c)
    iso = c.prior == "l21"
    for it, st in enumerate(stages):
        extra = (it + 1) * U.PHILOX_DXI * np.sqrt(2 * U.A_TAU) if c.mode == "philox" else 0.0
        assert st.x.bound == max(U.FACTOR * st.x.e32, 2 * U.ulp32(np.abs(st.x.ref64).max())) + extra
        assert st.x.e32 > 0
        _replay_ok(c, f"{it} x", st.x, regions, move=st.compare)
        for k in range(2):
            assert st.y[k].bound == max(U.FACTOR * st.y[k].e32, (6 if iso else 2) * U.ulp32(U.RADIUS)) + U.A_MU * 2 * (1 + c.theta) * extra
            _replay_ok(c, f"{it} y{k}", st.y[k], regions, move=st.compare)
            assert np.abs(st.y[k].ref64).max() <= U.RADIUS * (1 + 1e-12)
    # the first dual update meets both branches of the projection: gradients outside the ball and inside it
    if c.shape[0] * c.shape[1] >= 100:
        y = np.stack([r.ref64 for r in stages[0].y], axis=1)
        size = np.sqrt((y ** 2).sum(axis=1)) if iso else np.abs(y).max(axis=1)
        inside = size < U.RADIUS * (1 - 1e-6)
        assert 0.02 < inside.mean() < 0.98, inside.mean()


@pytest.mark.parametrize("c", U.B_CASES, ids=U.B_IDS)
def test_part_b_replay_passes_its_own_bound_and_truncation_is_out(c):
    stages = U.b_reference(c)
    assert len(stages) == c.iters
    regions = _regions_ok(c)
    for it, st in enumerate(stages):
        assert st.x.e32 > 0 and st.res.e32 > 0
        _replay_ok(c, f"{it} x", st.x, regions)
        # the condition that keeps a lower device count from looking like an error: the float64 replay two iterations short is within e32 / 10 of u*
        print(f"trunc {U.case_id(c)} it {it}: K {st.K} (float64 replay {st.K64}), |u64[K-2] - u*| {st.trunc:.3e}, e32 {st.x.e32:.3e}, "
              f"residual e32 {st.res.e32:.3e}")
        assert st.trunc <= st.x.e32 / 10, (st.trunc, st.x.e32)
        assert st.K >= 4 and st.K % 2 == 0
        # the replay's own residual passes the residual bound, the reference's is far below it
        v = X.check(c, f"{it} residual", U.residual(c, st.x.ref32, st), st.res)
        assert v.ok and v.err <= st.res.e32 * (1 + 1e-12), v.message
        assert np.abs(U.residual(c, st.x.ref64, st)).max() < st.res.e32 / 10
        if st.y is not None:
            for k in range(2):
                _replay_ok(c, f"{it} y{k}", st.y[k], regions)


def test_the_batched_loop_is_the_checkers_ulpda():
    c = next(c for c in U.B_CASES if c.mode == "warm" and c.family == "cheb")
    m = U.b_problem(c)
    ex = U.Solver(c, np.float64, "exact")
    xs, ys = U.ulpda_batched(ex.prox, m.x0, m.noise[:2], np.float64)

    class One:      # the same exact solve, one chain, flat vectors
        def prox(self, v, tau):
            return U.exact_solve((v.reshape(c.shape) + ex.ts * ex.htb)[None], ex.h, m.offset, ex.ts)[0].ravel()
    for ch in range(U.N_CHAINS):
        a, d = O.ulpda(One(), O.L21(ndim=2, sigma=U.RADIUS), O.Gradient(c.shape), m.x0[ch].astype(np.float64).ravel(), U.B_TAU, U.B_MU, theta=U.B_THETA,
                       niter=2, gfirst=False, returny=True, noise=m.noise[:2, ch].astype(np.float64).reshape(2, -1))
        for it in range(2):
            assert np.array_equal(a[it].reshape(c.shape), xs[it][ch]) and np.array_equal(d[it].reshape((2,) + c.shape), ys[it][ch])


# ---------------------------------------------------------------------------------------------------------------- planted faults
def _old_criteria(name, got_x, ref_x, got_y=None, ref_y=None, res=None, rhs=None):
    """The three criteria of tests/test_gpu_ulpda.py on a faulty result: all must hold (the fault passes the old suite)."""
    relx = X.rel(got_x, ref_x)
    rowmax = float(np.abs(got_x - ref_x).max(axis=-1).max())
    rely = X.rel(got_y, ref_y) if got_y is not None else 0.0
    rr = max(np.linalg.norm(res[ch]) / np.linalg.norm(rhs[ch]) for ch in range(res.shape[0])) if res is not None else 0.0
    print(f"fault {name}: old criteria rel-L2 {relx:.2e} (< {OLD_X:g}), dual rel-L2 {rely:.2e} (< {OLD_Y:g}), |r|/|rhs| {rr:.2e} (<= {OLD_RES:g}), "
          f"row maximum {rowmax:.2e} (< {OLD_ROW:g})")
    assert relx < OLD_X and rely < OLD_Y and rr <= OLD_RES and rowmax < OLD_ROW


def _caught(name, verdicts):
    v = U.worst([v for v in verdicts if not v.ok] or verdicts)
    print(f"fault {name}: harness err {v.err:.3e} against bound {v.bound:.3e} ({v.err / v.bound:.1f} bounds) at {v.where} [{v.region}]")
    assert not v.ok and v.err >= 3 * v.bound, v.message


def test_fault_a_seam_row_of_the_operator_scaled():
    """The operator with blurred row 32 (a seam of the pairs at LMC_PAIR_BAND=32) scaled by 1 - 5e-5, at (72, 128)."""
    c = next(c for c in U.B_CASES if c.family == "cheb-pairs" and c.shape == (72, 128) and c.mode == "cold")
    m, st = U.b_problem(c), U.b_reference(c)[0]
    h, ts = m.h.astype(np.float64), float(U.b_ts(np.float32))
    d = np.ones(c.shape)
    d[32] = 1 - 5e-5

    def faulty(v):
        return v + ts * O.blur_adjoint(d * O.blur(v, h, m.offset), h, m.offset)
    u = np.stack([O.cg_solve(faulty, st.rhs[ch], np.zeros(c.shape), 300, tol=(1e-13 * np.linalg.norm(st.rhs[ch])) ** 2) for ch in range(U.N_CHAINS)])
    _caught("seam row", U.check_b(c, 0, u, None, st)[:1])
    res = U.residual(c, u, st)
    v = X.check(c, "0 residual", res, st.res)
    rows = np.nonzero(np.abs(res).max(axis=(0, 2)) > st.res.bound)[0]
    print(f"fault seam row: residual over its bound on rows {rows.min()}..{rows.max()}")
    assert not v.ok and rows.min() >= 32 - 4 and rows.max() <= 32 + 4        # the residual map names the rows: H^T of row 32 reaches two rows either way
    _old_criteria("seam row", u, st.x.ref64, res=res, rhs=st.rhs)


def _a_case(**kw):
    want = dict(shape=(17, 64), gfirst=False, prior="l21", theta=1.0, z=True, data="identity", mode="restart")
    want.update(kw)
    return next(c for c in U.A_CASES if all(getattr(c, k) == v for k, v in want.items()))


def _step64(c, fault=None):
    """One iteration of `O.ulpda` (L21, identity, either order) written out in float64 on [C][H][W], with one planted fault; fault=None is the checker's."""
    m = U.a_problem(c)
    x, y, b, z, xi = (a.astype(np.float64) for a in (m.x0, m.y0, m.b, m.z, m.noise[0]))

    def dual(y, xhat):
        radius = np.full(c.shape, U.RADIUS)
        if fault == "dual":       # one row projected onto a ball 1e-4 too large
            radius[8] += 1e-4
        a = y + U.A_MU * np.stack(O.grad2d(xhat), axis=1)
        return a / np.maximum(1.0, np.sqrt(np.sum(a * a, axis=1, keepdims=True)) / radius)
    if c.gfirst:
        y = dual(y, x)
    aty = -O.div2d(y[:, 0], y[:, 1])
    if fault == "rhs":        # the divergence term of the last column left out: + yc[p - 1] there
        aty[:, :, -1] -= y[:, 1, :, -2]
    aty = aty + z
    ts = U.A_TAU * U.SIGMA_F
    xn = ((x - U.A_TAU * aty) + ts * b) / (1.0 + ts) + np.sqrt(2 * U.A_TAU) * xi
    xold = x.copy()
    where = None
    if fault == "finish":     # x_old of the other chain at one pixel: a low-noise pixel, where the chains differ by hundredths of a grey level
        cand = np.abs(np.abs(x[0] - x[1]) - 0.01) + 1e3 * ~m.low
        cand[0] = cand[-1] = cand[:, 0] = cand[:, -1] = 1e6
        where = np.unravel_index(int(np.argmin(cand)), cand.shape)
        xold[0][where] = x[1][where]
    if not c.gfirst:
        y = dual(y, xn + c.theta * (xn - xold))
    return xn, y, where


def test_the_written_out_step_is_the_checkers():
    for gfirst in (False, True):
        c = _a_case(gfirst=gfirst)
        st = U.a_reference(c)[0]
        x, y, _ = _step64(c)
        assert np.abs(x - st.x.ref64).max() <= 1e-12 and max(np.abs(y[:, k] - st.y[k].ref64).max() for k in range(2)) <= 1e-13


@pytest.mark.parametrize("fault", ["rhs", "dual", "finish"])
def test_fault_in_a_kernel_around_the_solve(fault):
    """The right-hand side without the divergence term at the last column; the dual projected to a radius 1e-4 too large on one row; xhat built from
    x_old of the wrong chain at one pixel.  The old residual criterion sees the solve alone, which these faults leave exact.  The first two are planted
    where the dual comes first (gfirst: it is formed from xhat = x, exact on both sides, and its bound is the floor of 6 ulp32(radius)); formed last it
    inherits the rounding of xhat and a bound of 1e-4, which the same fault reaches only once."""
    c = _a_case(gfirst=fault != "finish")
    st = U.a_reference(c)[0]
    x, y, where = _step64(c, fault)
    verdicts = U.check_stage(c, 0, x, y, st)
    _caught(fault, verdicts)
    bad = [v for v in verdicts if not v.ok]
    if fault == "rhs":
        assert all(v.where[2] == c.shape[1] - 1 for v in bad)
    if fault == "dual":
        assert all(v.where[1] in (7, 8) for v in bad)      # (row 7 of the state through the divergence)
    if fault == "finish":
        assert all(abs(v.where[1] - where[0]) + abs(v.where[2] - where[1]) <= 1 for v in bad), (where, [v.where for v in bad])
    _old_criteria(fault, x, st.x.ref64, y, np.stack([r.ref64 for r in st.y], axis=1))

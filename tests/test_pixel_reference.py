"""The per-pixel harness of tests/_pixel.py checked on itself, on the CPU, for every case of the GPU matrix (tests/test_gpu_pixel_parity.py imports the
same list): the float32 replay of the checker passes its own bound with the ratio 1 / FACTOR, the rounding scale is finite and positive, ONE pixel of the
float64 result moved by 1.5 bounds fails in every region class the case has (corner, each edge, each declared seam, interior) -- and the same state passes
the criterion the suite had, rel-L2 < 2e-6, which is the gap the per-pixel file closes."""
import numpy as np
import pytest

import _pixel as X

OLD_RTOL = 2e-6       # tests/test_gpu_pipe.py and its siblings: rel(got, want) < 2e-6 * (it + 1)


def test_the_matrix_has_every_family_and_unique_ids():
    fam = {c.family for c in X.CASES}
    assert fam == {"tile", "split", "point", "rows", "block", "rows_pair", "block_fused", "pipe", "pipe2", "pois", "wl2"}, fam
    assert len(X.CASES) >= 150 and len(set(X.IDS)) == len(X.IDS)
    assert len(X.LAYOUT_PAIRS) == 4, [(X.case_id(a), X.case_id(b)) for a, b in X.LAYOUT_PAIRS]
    for c in X.CASES:
        H, W = c.shape
        assert all(0 < s < H for s in c.seam_rows) and all(0 < s < W for s in c.seam_cols), X.case_id(c)


@pytest.mark.parametrize("c", X.CASES, ids=X.IDS)
def test_bound_accepts_the_float32_replay_and_rejects_one_moved_pixel(c):
    stages = X.reference(c)
    assert len(stages) == (1 if c.mode == "prox" else c.iters)
    regions = X.region_pixels(c)
    assert "corner" in regions and (c.shape[0] < 3 or {"first row", "last row"} <= set(regions))
    assert {f"row seam {s}" for s in c.seam_rows} | {f"column seam {s}" for s in c.seam_cols} <= set(regions), (regions, c.seam_rows, c.seam_cols)
    for it, st in enumerate(stages):
        if not st.compare:
            continue
        assert np.isfinite(st.e32) and st.e32 > 0, st.e32
        assert np.isfinite(st.ref64).all() and np.isfinite(st.bound)
        floor = 2 * X.ulp32(np.abs(st.ref64).max())
        assert st.bound == max(X.FACTOR * st.e32, floor)
        v = X.check(c, it, st.ref32, st)
        assert v.ok and v.err == st.e32 and v.err <= st.bound / X.FACTOR, v.message
        for reg, (i, j) in regions.items():
            for chain, sign in ((0, 1.0), (X.N_CHAINS - 1, -1.0)):
                moved = st.ref64.copy()
                moved[chain, i, j] += sign * 1.5 * st.bound
                v = X.check(c, it, moved, st)
                assert not v.ok and v.where == (chain, i, j) and v.region == reg, v.message
                old = X.rel(moved, st.ref64)
                print(f"moved {X.case_id(c)} it {it} [{reg}] by {1.5 * st.bound:.3e}: rejected; rel-L2 {old:.2e}")
                if c.shape[0] >= 17 and c.shape[1] >= 67:
                    assert old < OLD_RTOL, (reg, old)       # the norm averages it away


def test_the_old_norm_accepts_what_the_issue_measured():
    """0.05 added at two corner pixels of the (40, 512) state passes the third-iteration bound of the rel-L2 tests (6e-6): a missing tap of H^T there."""
    rng = np.random.default_rng(21)
    x = X.step_image((40, 512))[None] + rng.normal(0, 10, (2, 40, 512))
    moved = x.copy()
    moved[:, 0, 0] += 0.05
    assert X.rel(moved, x) < 3 * OLD_RTOL
    assert 0.05 > 1000 * X.ulp32(np.abs(x).max())

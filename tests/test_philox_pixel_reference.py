"""The Philox cases of tests/_pixel.py checked on themselves, on the CPU: what tests/test_gpu_pixel_parity.py asks of the kernels' own draw, and the proof
that its bound sees a fault in a kernel's counter arithmetic.

For every Philox case: the inputs (the field included) are float32 numbers; the float32 replay of the checker lies within the bound of the float64 one;
q, the coefficient of xi, is what the checker's step gives (step(x, 1) - step(x, 0)); and the noise term q NOISE_TOL of the bound is below
3 e32 + 2 ulp32, so the bound stays a rounding bound and the 2e-5 a device deviate may be off by does not dominate it.

Planted faults: the launch-form float32 replay of the case (`_pixel.replay32`) is run with the field a faulty draw would produce, and every compared
stage must fall outside its bound, on EVERY case the fault applies to:

    1  the last, partial quad row-group takes the field of the group above it          (H % 4 != 0, two groups or more)
    2  the columns from the first column seam on -- the second strip, the second team, the columns right of column 64 in the tile / split / point
       kernels -- take the field one column to the left                                 (cases with a column seam)
    3  the sine and cosine deviates of a Box-Muller pair swapped on one row: row 0 takes the deviate of row 1   (H >= 2)
    4  one row-group, the last, drawn at iteration + 1                                  (every case)
    5  one pixel of chain 0, the last one, with the deviate of chain 1                  (every case)
    6  the noise added in two links of a chained launch: + q xi once more              (K beyond one launch: 10 dual iterations, 8 in the tile kernel)
    7  the slab half not switched: row-group g carries the field of group g - 2        (three groups or more)

`test_what_the_norm_accepts` prints the table DESIGN section 4.1 holds: per fault, the pairs (case, fault) planted, how many the per-pixel bound rejects
(all) and how many the rel-L2 criterion of the trajectory tests (5e-5 per iteration) accepts; `test_faults_at_full_size` the rel-L2 of faults 1 and 5 on a
full-size image; and the smallest |q dxi| / bound -- the chance argument: a wrong deviate passes only if it lies within bound / q of the right one."""
import collections
import functools

import numpy as np
import pytest

import _pixel as X
from oracle import lmc_oracle as O

TRAJECTORY_RTOL = 5e-5       # tests/test_gpu_parity.py::test_philox_trajectory_matches_oracle_with_same_counters and its siblings: rel-L2 <= 5e-5 it
FAULTS = {1: "last partial row-group from the group above", 2: "columns past the first seam from one column to the left", 3: "sine / cosine swapped on row 0",
          4: "last row-group at iteration + 1", 5: "one pixel from chain c + 1", 6: "noise added in two links", 7: "row-group g from group g - 2"}


def chained(c):
    """Whether the case's prox runs as more than one launch: the pipe kernels chain launches of 10 dual iterations, the tile kernel chunks of 8."""
    return c.K > (8 if c.variant == "tile" else 10)


def faulty_noise(c, k, noise=None):
    """The field of case `c` ([iters, chains, H, W]) under fault `k`; None where the fault does not apply."""
    xi = X.problem(c).noise if noise is None else noise
    (H, W), out = c.shape, np.array(xi)
    last = 4 * ((H + 3) // 4 - 1)       # first row of the last row-group
    if k == 1:
        if H % 4 == 0 or last == 0:
            return None
        out[..., last:, :] = xi[..., last - 4:H - 4, :]
    elif k == 2:
        if not c.seam_cols:
            return None
        s = c.seam_cols[0]
        out[..., s:] = xi[..., s - 1:W - 1]
    elif k == 3:
        if H < 2:
            return None
        out[..., 0, :] = xi[..., 1, :]
    elif k == 4:
        for it in range(c.iters):
            out[it][:, last:] = O.philox_normals(X.seed_of(c), c.it0 + it + 1, np.arange(X.CHAIN_OFFSET, X.CHAIN_OFFSET + X.N_CHAINS), H, W)[:, last:]
    elif k == 5:
        out[:, 0, H - 1, W - 1] = xi[:, 1, H - 1, W - 1]
    elif k == 6:
        if not chained(c):
            return None
        out *= np.float32(2.0)
    elif k == 7:
        if last < 8:
            return None
        out[..., 8:, :] = xi[..., :H - 8, :]
    return out


Planted = collections.namedtuple("Planted", "fault it rejected rel accepted_by_norm ratio pixels pixels_within message")


@functools.lru_cache(maxsize=None)
def planted(c):
    """Every fault that applies to `c`, replayed: one `Planted` per fault and compared stage.  ratio: the largest |q dxi| / bound over the pixels the
    fault changed; pixels_within: how many of them changed by no more than the bound."""
    stages, xi, q, out = X.reference(c), X.problem(c).noise, X.noise_gain(c), []
    for k in FAULTS:
        bad = faulty_noise(c, k)
        if bad is None:
            continue
        states = X.replay32(c, bad)
        for it, st in enumerate(stages):
            if not st.compare:
                continue
            v = X.check(c, it, states[it], st)
            rel = X.rel(states[it], st.ref64)
            carried = it + 1 if st.start is None or c.mode == "philox_warm" else 1
            d = q * np.abs(bad[it].astype(np.float64) - xi[it])
            out.append(Planted(k, it, not v.ok, rel, rel <= TRAJECTORY_RTOL * carried, float(d.max() / st.bound), int((d > 0).sum()),
                               int(((d > 0) & (d <= st.bound)).sum()), v.message))
    return tuple(out)


def test_the_philox_matrix():
    fam = {c.family for c in X.PHILOX_CASES}
    assert fam == {"tile", "split", "point", "rows", "block", "rows_pair", "block_fused", "pipe", "pipe2", "pois", "wl2"}, fam
    assert X.SEED_P >> 32 and X.SEED_P & 0xFFFFFFFF and X.SEED_P >> 32 != X.SEED_P & 0xFFFFFFFF
    assert len(X.PHILOX_LAYOUT_PAIRS) == 3, [(X.case_id(a), X.case_id(b)) for a, b in X.PHILOX_LAYOUT_PAIRS]
    assert X.NOISE_TOL == 2e-5
    for c in X.PHILOX_CASES:
        assert c.mode in X.PHILOX_MODES + ("fused",) and c.kernel, X.case_id(c)
        assert c.shape[0] * c.shape[1] <= max(66 * 130, 13 * 1544) and c.it0 + c.iters <= 0xFFFFFFFF, X.case_id(c)
        if c.mode != "fused":       # a Philox case differs from an injected-noise case in the noise source only
            twin = [b for b in X.CASES if b._replace(mode="", tag="", shape=(), seam_rows=(), seam_cols=()) ==
                    c._replace(mode="", tag="", shape=(), seam_rows=(), seam_cols=(), it0=0) and b.mode in ("restart", "warm")]
            assert twin, X.case_id(c)
            same = [b for b in twin if b.shape == c.shape]
            for b in same:
                assert (b.seam_rows, b.seam_cols) == (c.seam_rows, c.seam_cols), (X.case_id(c), X.case_id(b))
                for name in ("h", "mask", "aux", "y", "x0"):
                    assert np.array_equal(getattr(X.problem(b), name), getattr(X.problem(c), name)), (X.case_id(c), name)


def test_the_oracle_takes_the_top_of_the_counter():
    """Iterations up to 0xFFFFFFFF are counter words like any other: the field is finite, differs from iteration 0 and from its neighbour, and does not
    depend on how the iteration is passed (int or uint32)."""
    ids = np.arange(X.CHAIN_OFFSET, X.CHAIN_OFFSET + X.N_CHAINS)
    f0 = O.philox_normals(X.SEED_P, 0, ids, 6, 264)
    seen = [f0]
    for it in (X.IT_TOP_FUSED, X.IT_TOP, X.IT_TOP + 1, 0xFFFFFFFF, 2 ** 31):
        f = O.philox_normals(X.SEED_P, it, ids, 6, 264)
        assert f.dtype == np.float32 and np.isfinite(f).all()
        assert np.array_equal(f, O.philox_normals(X.SEED_P, np.uint32(it), ids, 6, 264))
        for g in seen:
            assert np.mean(f == g) < 1e-3 and abs(np.corrcoef(f.ravel(), g.ravel())[0, 1]) < 5 / np.sqrt(f.size)
        seen.append(f)


@pytest.mark.parametrize("c", X.PHILOX_CASES, ids=X.PHILOX_IDS)
def test_philox_case_is_exact_in_float32_and_its_bound_is_a_rounding_bound(c):
    m, stages, q = X.problem(c), X.reference(c), X.noise_gain(c)
    assert len(stages) == c.iters
    for a in (m.h, m.mask, m.aux, m.y, m.x0, m.noise):
        assert a is None or a.dtype == np.float32
    for it in range(c.iters):
        assert np.array_equal(m.noise[it], X.philox_field(c, it)) and np.isfinite(m.noise[it]).all()
        assert np.array_equal(m.noise[it], O.philox_normals(X.seed_of(c), c.it0 + it, X.CHAIN_OFFSET + np.arange(X.N_CHAINS), *c.shape))
    # q from the checker: two fresh replays (the warm dual is carried in the object), one with xi = 1 and one with xi = 0
    one, zero = (X.Stepper(c, np.float64).step(m.x0, np.full(m.x0.shape, v)) for v in (1.0, 0.0))
    got_q = (one - zero)[0, c.shape[0] // 2, c.shape[1] // 2]
    assert abs(got_q - np.sqrt(2 * m.tau)) <= 1e-12 * np.abs(one).max() and abs(q - got_q) <= 2.0 ** -23 * q, (got_q, q, np.sqrt(2 * m.tau))
    for it, st in enumerate(stages):
        if not st.compare:
            continue
        floor = 2 * X.ulp32(np.abs(st.ref64).max())
        rounding = max(X.FACTOR * st.e32, floor)
        if c.mode == "fused":
            assert not hasattr(st, "noise_term") and st.bound == rounding
        else:
            carried = it + 1 if c.mode == "philox_warm" else 1
            assert st.noise_term == carried * q * X.NOISE_TOL and st.bound == rounding + st.noise_term
            assert st.start is not None or c.mode == "philox_warm"
            # the noise term does not dominate (per carried iteration; for the warm dual both parts grow with the iteration)
            assert q * X.NOISE_TOL < X.FACTOR * st.e32 + floor, (q * X.NOISE_TOL, st.e32, floor)
        assert np.isfinite(st.e32) and st.e32 > 0 and np.isfinite(st.ref64).all()
        v = X.check(c, it, st.ref32, st)
        assert v.ok and v.err == st.e32 and v.err <= st.bound / X.FACTOR, v.message


@pytest.mark.parametrize("c", X.PHILOX_CASES, ids=X.PHILOX_IDS)
def test_every_planted_fault_is_rejected(c):
    got = planted(c)
    ks = {p.fault for p in got}
    assert {4, 5} <= ks, ks
    H = c.shape[0]
    assert (1 in ks) == (H % 4 != 0 and H > 4) and (2 in ks) == bool(c.seam_cols) and (3 in ks) == (H >= 2) and (6 in ks) == chained(c) and (7 in ks) == (H > 8)
    for p in got:
        print(f"fault {p.fault} {X.case_id(c)} it {p.it}: rejected {p.rejected}; rel-L2 {p.rel:.2e} (the trajectory tests allow {TRAJECTORY_RTOL:.0e} per "
              f"iteration: {'accepted' if p.accepted_by_norm else 'rejected'}); largest |q dxi| / bound {p.ratio:.3g}")
        assert p.rejected, (FAULTS[p.fault], p.message)


def test_what_the_norm_accepts(capsys):
    """The table of DESIGN section 4.1."""
    rows, lines = [p for c in X.PHILOX_CASES for p in planted(c)], []
    pairs = {k: {(X.case_id(c)) for c in X.PHILOX_CASES for p in planted(c) if p.fault == k} for k in FAULTS}
    accepted = {k: {(X.case_id(c)) for c in X.PHILOX_CASES for p in planted(c) if p.fault == k and p.accepted_by_norm} for k in FAULTS}
    for k in FAULTS:
        rk = [p for p in rows if p.fault == k]
        assert rk and all(p.rejected for p in rk)
        lines.append(f"fault {k} ({FAULTS[k]}): {len(pairs[k])} cases, {len(rk)} stages, all rejected by the bound; the norm accepts {len(accepted[k])} cases; "
                     f"rel-L2 {min(p.rel for p in rk):.1e} .. {max(p.rel for p in rk):.1e}; smallest per-stage max |q dxi| / bound {min(p.ratio for p in rk):.3g}")
    n_pairs, n_acc = sum(len(v) for v in pairs.values()), sum(len(v) for v in accepted.values())
    pix, within = sum(p.pixels for p in rows), sum(p.pixels_within for p in rows)
    lines.append(f"(case, fault) pairs: {n_pairs}; the per-pixel bound rejects {n_pairs}, rel-L2 <= {TRAJECTORY_RTOL:.0e} per iteration accepts {n_acc}")
    lines.append(f"smallest |q dxi| / bound over the stages: {min(p.ratio for p in rows):.3g}; of {pix} planted pixels {within} moved by no more than the bound "
                 f"({within / pix:.1e})")
    with capsys.disabled():
        print("\n" + "\n".join(lines))
    assert min(p.ratio for p in rows) > 1.0


def test_faults_at_full_size():
    """The flagship size, replayed on the CPU after one step of a 510 x 512 image (rows 508, 509: a partial quad).  Fault 1 moves each of the 1024 pixels
    per chain of the last row-group by a deviate's worth (q |dxi| ~ 0.5): tens of thousands of bounds.  Fault 5 moves one pixel.  Both rel-L2 figures are
    printed next to the 5e-5 per iteration of the trajectory tests (DESIGN section 4.1 holds them); the per-pixel bound rejects both."""
    base = next(c for c in X.PHILOX_CASES if X.case_id(c) == "rows-17x67-l1-A-philox")
    c = base._replace(shape=(510, 512), seam_rows=(), seam_cols=(), iters=1, tag="l1-A-philox-full")
    st = X.reference(c)[0]
    for k in (1, 5):
        got = X.replay32(c, faulty_noise(c, k))[0]
        v = X.check(c, 0, got, st)
        rel = X.rel(got, st.ref64)
        print(f"fault {k} at 510 x 512: rel-L2 {rel:.2e} after one step (the trajectory tests allow {TRAJECTORY_RTOL:.0e} per iteration); err {v.err:.3g}, "
              f"bound {st.bound:.3g}")
        assert not v.ok and v.err > 100 * st.bound, v.message

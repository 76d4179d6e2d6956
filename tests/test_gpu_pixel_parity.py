"""Per-pixel parity of every MYULA step kernel against the float64 checker: max |got - ref64| over EVERY chain and pixel within
max(3 e32, 2 ulp32(max |ref64|)), where e32 = max |ref32 - ref64| is the checker's own float32 rounding for the case (tests/_pixel.py: how the inputs are
rounded once, the two replays, the restart from ref64 after the first iteration, the regions).  The rel-L2 tests average the places where step kernels go
wrong -- first and last rows, the last partly filled lane, tile, band, strip and team seams, the corner of H^T -- away (tests/test_pixel_reference.py
shows on the CPU, for each case, a pixel the bound rejects and the norm accepts); tests/test_gpu_pipe_pairs.py and tests/test_gpu_pipe_uni.py pin the
pipe kernels no worse than a parent commit, this file pins every family against the reference alone.

The cases are `_pixel.CASES` (family, shape, data term, prior, blur taps, K): the tile, split, point, rows, block kernels with `variant=` forced, the two-
and four-iteration launches, the pipe kernel in both layouts outside what the two files above pin (K = 2, 6, 8, 9, other taps, pointwise and no data term,
unaligned widths, column strips, chained launches, the warm dual, anisotropic TV, the box), the Poisson and weighted Gaussian instantiations.  Every case
asserts `kernel_name` exactly, so a fallback cannot pass as coverage; a variant that does not cover its case must refuse (LMC_E_UNSUPPORTED), never skip.

The launches of two and four iterations (Philox noise, driven on the checker's side by `O.philox_normals`) and the warm dual cannot restart from ref64
in between -- the iterations are inside one launch, and `set_state` zeroes the carried dual -- so both replays run the same iterations from x0 and are
compared after the launch (after every iteration for the warm dual); `TV.prox` alone has no sampler and so no kernel name to read.

Measured on an MI355X (all 192 cases and the 4 layout pairs pass; the whole file takes 3 s): the largest err / e32 of each family over its cases and
iterations, and where it sat.  The bound is at ratio 3; no family needed another factor, and no case has its worst pixel at an edge or seam with a ratio
apart from the interior's (the largest off-interior ratio is given last).

    family        stages  largest err / e32   case, region                                     largest off the interior
    tile              62  0.82                (3, 5) tv10-E, first row (err 9.4e-6)            0.82 first row
    split             36  0.50                (5, 64) tv10-A, interior                         0.42 first and last row
    point             28  0.46                (33, 65) l2-D, interior                          0.43 column seam 64
    rows              80  0.66                (9, 4) l1-B, interior                            0.48 last column
    block             24  1.83                (8, 8) haar-identity, interior (err 2.5e-5)      1.00 row seam 8
    rows_pair          4  0.45                (40, 132) l1-A, interior                         (no edge pixel was the worst)
    block_fused        4  0.74                (16, 72) haar-identity 2 iterations, interior    0.71 row seam 8
    pipe             109  1.00                (6, 136) TV.prox, interior (err 8.9e-6)          0.91 first and last row
    pipe2              8  0.45                (6, 264) tv10box-A, column seam 132              0.45 column seam 132
    pois              12  0.70                (17, 67) tile-tv10-A, column seam 64             0.70 column seam 64
    wl2               12  0.52                (17, 67) tile-tv10box-A, column seam 64          0.52 column seam 64

(block: 1.83 e32 = 2.5e-5 is 1.6 ulp of a state of 200, inside its bound of 3 e32 = 4.1e-5, and its worst pixel is interior.)  One-team and two-team layouts were bit-equal on all four pairs.

The noise a kernel draws itself.  The cases above inject their noise, apart from the six fused launches.  `_pixel.PHILOX_CASES` are injected-noise cases
with the noise source changed and nothing else (mode "philox": the restart mode with the field O.philox_normals(SEED_P, it0 + it, global chain ids, H, W)
as the noise of iteration it; "philox_warm": the warm mode with it): a sampler with seed SEED_P and chain offset CHAIN_OFFSET, policy
iterations_per_launch = 1 for the rows and block families, and before every iteration `set_state(start)`, `smp.iteration = it0 + it`, `step(1)`.  The
bound gains q NOISE_TOL (q = sqrt(2 tau), NOISE_TOL = 2e-5: the reference's field is exact arithmetic rounded once, the device's is hardware log2 / sqrt /
sin / cos).  The rtol > 0 instantiations are left out: their pass count is discontinuous, and their Philox code is the same template code.  Measured on
an MI355X (all 104 cases and the 3 layout pairs pass; these tests take 2.3 s): stages, largest err / e32, where, largest off the interior.

    family        stages  largest err / e32   case, region                                     largest off the interior
    tile              16  0.55                (3, 5) tv10-A, interior (err 1.1e-5)             0.41 column seam 64
    split             12  0.50                (1, 300) tv10-A, first and last row              0.50 first and last row
    point              6  0.40                (34, 130) l2-A, interior                         (no edge pixel was the worst)
    rows              14  0.52                (9, 4) l1-A, interior                            (no edge pixel was the worst)
    block             16  1.01                (16, 72) haar-mask, interior (err 2.1e-5)        0.61 row seam 8
    pipe              99  0.54                (4, 136) tv10-A, first row (err 1.2e-5)          0.54 first row
    pipe2              6  0.45                (6, 264) tv10box-A, interior                     0.41 column seam 132
    pois               8  0.58                (6, 136) pipe-tv10-A, interior (err 1.6e-6)      0.48 column seam 64
    wl2                8  0.71                (6, 136) pipe-tv10-A, interior (err 9.3e-6)      0.58 column seam 64
    counter's top     10  1.10                block (16, 72) haar-mask, row seam 8 (err 2.7e-5, bound 8.2e-5); tile, split, rows, pipe 0.33 to 0.55
    fused, top         8  0.81                block (16, 72) haar-identity 2 iterations, column seam 32; rows_pair 0.45 (bounds without the noise term)

The pipe rows hold H in {1, 2, 3, 4, 5, 7, 8, 9, 13} at 264 and 136 columns (the last, partial quad row-group; both halves of the Philox slab), the
unaligned widths, two to four column strips, K = 2, 6, 8, 9, the chained launches (the noise added once), the anisotropic and box instantiations and the
warm dual; none stands apart from the interior.  One-team and two-team layouts drew bit-equal states on all three pairs.  No kernel was wrong.
"""
import numpy as np
import pytest

import _pixel as X

pytestmark = pytest.mark.gpu
LMC_E_UNSUPPORTED = -2


@pytest.fixture(scope="module")
def la():
    import torch
    assert torch.cuda.is_available()
    import lmc_atomi_amd as la
    return la


def f64(a):
    return None if a is None else np.array(a, dtype=np.float64)      # (the same numbers; the reference's arrays are read-only)


def device_terms(la, c):
    """The library's data term and prior of case `c`, from the float32 numbers of `_pixel.problem`."""
    m, shape = X.problem(c), c.shape
    if m.h is not None:
        Op = la.Convolve2D(shape, f64(m.h), offset=m.offset)
    elif m.mask is not None:
        Op = la.Diagonal(f64(m.mask), dims=shape)
    else:
        Op = None
    if c.term == "pois":
        pf = la.Poisson(Op if Op is not None else la.Identity(shape[0] * shape[1]), f64(m.y), f64(m.aux), sigma=m.sigma_f)
    elif c.term == "wl2":
        pf = la.L2(Op=Op, b=f64(m.y), sigma=m.sigma_f, weights=f64(m.aux), dims=shape)
    elif c.data == "none":
        pf = None
    else:
        pf = la.L2(Op=Op, b=f64(m.y), sigma=m.sigma_f, dims=shape)
    w = X.weight(c)
    if c.prior in ("tv", "aniso"):
        pg = la.TV(shape, sigma=w, niter=c.K + (1 if c.lagged else 0), lagged_output=c.lagged, warm=c.mode in ("warm", "philox_warm"), isotropic=c.prior == "tv", bounds=c.box)
    elif c.prior == "l1":
        pg = la.L1(sigma=w)
    elif c.prior == "l2":
        pg = la.L2(sigma=w, dims=shape)
    elif c.prior == "haar":
        pg = la.WaveletL1(shape, sigma=w)
    elif c.prior == "eprox":
        pg = la.UncenteredLaplace(w, X.EPROX_MU)
    else:
        pg = None
    return pf, pg


_RUNS = {}


def run(la, c):
    """The device run of case `c`, once per process: {"states": the state after each compared iteration, "kernel": its name} or {"refused": status}."""
    key = X.case_id(c)
    if key in _RUNS:
        return _RUNS[key]
    m, stages = X.problem(c), X.reference(c)
    pf, pg = device_terms(la, c)
    if c.mode == "prox":
        got = np.stack([np.asarray(pg.prox(f64(m.x0[i]).ravel(), X.PROX_T)).reshape(c.shape) for i in range(X.N_CHAINS)])
        _RUNS[key] = {"states": [got], "kernel": ""}
        return _RUNS[key]
    kw = dict(n_chains=X.N_CHAINS, tau=m.tau, gamma=m.gamma, variant=c.variant)
    if c.mode == "fused":
        smp = la.MYULASampler(pf, pg, c.shape, seed=X.SEED, chain_offset=X.CHAIN_OFFSET, policy={"iterations_per_launch": 2}, **kw)
    elif c.mode in X.PHILOX_MODES:      # the rows and block families would fuse iterations: hold them to single launches
        policy = {"iterations_per_launch": 1} if c.variant in ("rows", "block") else None
        smp = la.MYULASampler(pf, pg, c.shape, seed=X.SEED_P, chain_offset=X.CHAIN_OFFSET, policy=policy, **kw)
    else:
        smp = la.MYULASampler(pf, pg, c.shape, noise="injected", **kw)
    states = []
    try:
        if c.mode == "fused":
            smp.set_state(f64(m.x0))
            if c.it0:
                smp.iteration = c.it0
            smp.step(c.iters)
            assert smp.iteration == c.it0 + c.iters
            states.append(smp.get_state().cpu().numpy())
        elif c.mode in X.PHILOX_MODES:      # the kernel draws the noise itself, at the counter set before every launch
            for it, st in enumerate(stages):
                if st.start is not None:
                    smp.set_state(f64(st.start))
                smp.iteration = c.it0 + it
                smp.step(1)
                assert smp.iteration == c.it0 + it + 1
                states.append(smp.get_state().cpu().numpy())
        else:
            for it, st in enumerate(stages):
                if st.start is not None:
                    smp.set_state(f64(st.start))
                smp.step(1, noise=f64(m.noise[it:it + 1]))
                states.append(smp.get_state().cpu().numpy())
        out = {"states": states, "kernel": smp.kernel_name}
    except la.LMCError as err:
        out = {"refused": err.code, "message": str(err)}
    finally:
        smp.close()
    _RUNS[key] = out
    return out


@pytest.mark.parametrize("c", X.CASES, ids=X.IDS)
def test_every_pixel_within_the_reference_bound(la, c):
    out = run(la, c)
    if c.kernel is None:
        assert out.get("refused") == LMC_E_UNSUPPORTED, out
        return
    assert "refused" not in out, out
    assert out["kernel"] == c.kernel, (out["kernel"], c.kernel)
    compared = [(it, st) for it, st in enumerate(X.reference(c)) if st.compare]
    assert len(compared) == len(out["states"])
    verdicts = [X.check(c, it, got, st) for (it, st), got in zip(compared, out["states"])]
    bad = [v.message for v in verdicts if not v.ok]
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("c", X.PHILOX_CASES, ids=X.PHILOX_IDS)
def test_every_pixel_within_the_reference_bound_with_the_noise_the_kernel_draws(la, c):
    """The Philox cases (tests/_pixel.py): the bound is max(3 e32, 2 ulp32) + q NOISE_TOL -- the reference's field is exact arithmetic rounded once, the
    device's is hardware log2 / sqrt / sin / cos, stated to within NOISE_TOL = 2e-5 per deviate, and the deviate enters the state as q xi (the launches of
    two and four iterations at the top of the counter keep the bound of their twins at iteration 0, without that term).  A deviate from the wrong quad,
    row, chain or iteration is off by thousands of bounds (tests/test_philox_pixel_reference.py plants them).  The rows family at every shape of the
    list is held to single launches by policy iterations_per_launch = 1, so none of them runs in "fused" form."""
    test_every_pixel_within_the_reference_bound(la, c)


@pytest.mark.parametrize("a,b", X.PHILOX_LAYOUT_PAIRS, ids=[X.case_id(b) for _, b in X.PHILOX_LAYOUT_PAIRS])
def test_one_team_and_two_team_layouts_draw_the_same_noise(la, a, b):
    test_one_team_and_two_team_layouts_are_bit_equal(la, a, b)


@pytest.mark.parametrize("a,b", X.LAYOUT_PAIRS, ids=[X.case_id(b) for _, b in X.LAYOUT_PAIRS])
def test_one_team_and_two_team_layouts_are_bit_equal(la, a, b):
    ra, rb = run(la, a), run(la, b)
    assert "refused" not in ra and "refused" not in rb, (ra, rb)
    for it, (sa, sb) in enumerate(zip(ra["states"], rb["states"])):
        d = np.abs(sa.astype(np.float64) - sb)
        assert np.array_equal(sa, sb), (it, float(d.max()), np.unravel_index(int(np.argmax(d)), d.shape))

"""The helpers of tests/_many.py, checked without a device: what the many-image GPU tests take for granted about their own reference."""
import numpy as np

from tests import _many as M
from oracle import lmc_oracle as O


def test_tiled_expectation_equals_the_checker_on_a_real_tiled_batch():
    """blur, TV prox and one MYULA step of 3 * 7 + 2 images built by tiling == the checker's results on the 7 patterns, tiled"""
    shape, n = (6, 10), 3 * M.P + 2
    base = M.patterns(shape, 1)
    batch = M.tile(base, n)
    assert batch.shape == (n,) + shape and np.array_equal(batch[M.P + 2], base[2]) and not np.array_equal(base[0], base[1])
    h, off, y = M.blur_problem(shape, 3)
    for fn in (lambda v: O.blur(v, h, (0, 2)), lambda v: O.tv_prox_fgp(v, 0.17, 10), lambda v: M.tv_prox_aniso(v, 0.17, 10)):
        assert M.per_image_rel(fn(batch), fn(base)).max() < 1e-14
    noise = np.random.default_rng(2).standard_normal((M.P,) + shape)
    for prior in ({"kind": "tv", "sigma": M.TAU_REG, "niter": 10, "t": M.GAMMA}, {"kind": "tv_aniso", "sigma": M.TAU_REG, "niter": 10, "t": M.GAMMA}):
        full = M.myula_step_ref(batch, y, h, off, M.TAU, M.GAMMA, prior, M.tile(noise, n))
        assert M.per_image_rel(full, M.myula_step_ref(base, y, h, off, M.TAU, M.GAMMA, prior, noise)).max() < 1e-14
    # the anisotropic step assembled in _many is the checker's own one-chain loop with that prox
    class Aniso:
        def prox(self, x, t):
            return M.tv_prox_aniso(np.asarray(x).reshape(shape), M.TAU_REG * t, 10).ravel()
    one = O.myula(O.L2(Op=O.Convolve2D(shape, h, off), b=y.ravel(), sigma=1 / M.SIGMA ** 2), Aniso(), base[4].ravel(), M.TAU, M.GAMMA, niter=1, noise=[noise[4].ravel()])
    assert M.global_rel(M.myula_step_ref(base, y, h, off, M.TAU, M.GAMMA, prior, noise)[4].ravel(), one[0]) < 1e-13


def test_chunk_phase_and_windows():
    assert M.CHUNK % M.P == 1 and M.N_OPS == 131077 and M.C_SMP == 65543
    # the chunks start at different phases of the pattern: an output that lost its chunk offset holds another pattern
    assert len({(k * M.CHUNK) % M.P for k in range(3)}) == 3
    w = M.windows(M.C_SMP)
    assert {0, 3, M.CHUNK - 1, M.CHUNK, M.C_SMP - 1} <= set(w.tolist()) and w.max() < M.C_SMP and len(set(w.tolist())) == len(w)


def test_per_image_error_sees_one_image_a_global_norm_does_not():
    shape = (5, 7)
    base = M.patterns(shape, 4)
    got = M.tile(base, M.N_OPS).astype(np.float32)
    ref = M.tile(base, M.N_OPS)
    bad = M.CHUNK + 11
    got[bad] *= np.float32(1 + 1e-4)
    errs = M.per_image_rel(got, base)
    e, i = M.worst(errs)
    assert i == bad and 0.9e-4 < e < 1.1e-4
    assert M.global_rel(got, ref) < M.STEP_TOL < e            # the global norm passes the batch, the per-image error does not
    try:
        M.check_per_image(got, base, M.STEP_TOL, "one image off")
    except AssertionError as err:
        assert f"image {bad} (index 11 of chunk 1" in str(err)
    else:
        raise AssertionError("check_per_image let a wrong image through")
    got[bad] = np.nan
    assert M.worst(M.per_image_rel(got, base))[1] == bad
    # explicit per-image references and per-image scalars
    assert M.per_image_rel(ref[:20], ref[:20]).max() == 0.0
    assert M.per_image_rel(np.arange(1.0, 15.0), np.arange(1.0, 15.0) * (1 + 1e-3)).max() < 1.1e-3


def test_rtol_patterns_leave_in_three_distinct_passes():
    for shape in ((6, 10), (2, 136)):
        x7 = M.rtol_patterns(shape)
        sol, passes = M.rtol_reference(x7)
        print(shape, passes)
        assert len(set(passes.tolist())) >= 3, passes
        assert passes[0] == M.RTOL_K                  # the zero image runs out of passes
        seen = 0
        for c in range(M.P):                          # the helper is the checker's rtol branch, with the pass it left in
            assert np.array_equal(sol[c], O.tv_prox_fgp(x7[c], M.RTOL_GAM, M.RTOL_K, rtol=M.RTOL))
            seen += passes[c] < M.RTOL_K and M.global_rel(sol[c], O.tv_prox_fgp(x7[c], M.RTOL_GAM, M.RTOL_K)) > 10 * M.STEP_TOL
        assert seen >= 2                              # ... and an exit is visible in the result: a prox that ignored it would miss STEP_TOL


def test_mymala_scene_is_clear_cut_for_nearly_every_chain():
    """At least 95 % of the 65543 chains decide with a margin the fp32 energies cannot cross, and both outcomes occur among them"""
    la_o, logu, ok, safe, xp, x0, bound = M.mala_reference(np.arange(M.C_SMP))
    print(f"log alpha {la_o}; safe {safe.mean():.4f}, accepted {ok.mean():.4f}")
    assert safe.mean() >= 0.95
    assert ok[safe].any() and (~ok[safe]).any()
    # the log acceptance ratio assembled in _many is the checker's own
    y, h, off, prior, _, noise = M.mala_scene()
    _, acc, las = O.mymala_batched(x0, y, h, off, 1 / M.SIGMA ** 2, M.MALA_TAU, M.GAMMA, prior, 1, lambda k: noise, lambda k: np.exp(logu[:M.P]))
    assert np.allclose(las[0], la_o, rtol=0, atol=1e-9) and np.array_equal(acc.astype(bool), ok[:M.P])


def test_philox_reference_accepts_the_top_chain_ids():
    ids = np.array([2 ** 32 - 1 - M.C_SMP, 2 ** 32 - 2, 2 ** 32 - 1], dtype=np.uint64)
    a = O.philox_normals(7, 0, ids, 4, 6)
    assert a.shape == (3, 4, 6) and np.isfinite(a).all() and not np.array_equal(a[1], a[2])
    assert np.array_equal(a[2], O.philox_normals(7, 0, np.array([2 ** 32 - 1], dtype=np.uint64), 4, 6)[0])

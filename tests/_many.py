"""Helpers shared by tests/test_gpu_many_images.py, tests/test_gpu_thin_images.py and tests/test_many_images_reference.py.

A batch far larger than the checker could replay is built from P = 7 distinct patterns: image c is base[c % 7].  The launchers that split the
image axis do so in chunks of 65535, and 65535 % 7 == 1: every chunk starts at another phase of the pattern, so an output whose pointer forgot
its chunk offset holds the wrong pattern from image 65535 on.  The checker runs on the 7 patterns; the expectation for image c is ref[c % 7].

Errors are taken per image (one partly wrong image in 131077 vanishes in a norm over the batch) and the worst image is named together with its
index inside its chunk."""
import numpy as np

from oracle import lmc_oracle as O

P = 7
CHUNK = 65535                  # gridDim.y / gridDim.z limit the launchers split at
N_OPS = 2 * CHUNK + 7          # stateless operators: three chunks, the last one short
C_SMP = CHUNK + 8              # samplers: two chunks
STEP_TOL = 1e-5                # one operator / one step, rel-L2 (tests/test_gpu_parity.py)
SIGMA, TAU_REG = 0.75, 0.3
GAMMA, TAU = SIGMA ** 2, 0.2 * SIGMA ** 2
assert CHUNK % P == 1


def tile_index(n):
    return np.arange(n) % P


def tile(base, n):
    """[P, ...] -> [n, ...]: image c is base[c % P]"""
    base = np.asarray(base)
    assert base.shape[0] == P
    return base[tile_index(n)]


def tile_dev(base, n, device="cuda"):
    """the same batch as an fp32 tensor in HBM, formed there"""
    import torch
    b = torch.from_numpy(np.ascontiguousarray(base, dtype=np.float32)).to(device)
    return b[torch.arange(n, device=device) % P].contiguous()


def per_image_rel(got, ref, block=8192):
    """Relative L2 error of every image: got [N, ...]; ref [N, ...] or the P patterns [P, ...] (then image c is compared with ref[c % P]).
    float64, block by block (the full batch is never held twice).  Scalars per image (energies) count as one-pixel images."""
    ref = np.asarray(ref, dtype=np.float64)
    n = got.shape[0]
    tiled = ref.shape[0] == P and n != P
    assert tiled or ref.shape[0] == n, (got.shape, ref.shape)
    assert tuple(got.shape[1:]) == tuple(ref.shape[1:]) or int(np.prod(got.shape[1:])) == int(np.prod(ref.shape[1:])), (got.shape, ref.shape)
    ref = ref.reshape(ref.shape[0], -1)
    out = np.empty(n)
    for a in range(0, n, block):
        b = min(a + block, n)
        g = np.asarray(got[a:b].cpu() if hasattr(got, "cpu") else got[a:b], dtype=np.float64).reshape(b - a, -1)
        r = ref[np.arange(a, b) % P] if tiled else ref[a:b]
        out[a:b] = np.linalg.norm(g - r, axis=1) / np.maximum(np.linalg.norm(r, axis=1), 1e-30)
    return out


def worst(errs):
    """(largest error, its image)"""
    errs = np.where(np.isfinite(errs), errs, np.inf)
    i = int(np.argmax(errs))
    return float(errs[i]), i


def check_per_image(got, ref, tol, what):
    """assert every image within `tol`; the message names the worst image, and the worst one of every chunk of 65535 with the number that miss"""
    errs = per_image_rel(got, ref)
    e, i = worst(errs)
    print(f"{what}: worst image {i} (index {i % CHUNK} of chunk {i // CHUNK}, pattern {i % P}) rel {e:.3e}, bound {tol:.1e}")
    if not e < tol:
        per_chunk = []
        for k in range(0, len(errs), CHUNK):
            ek, ik = worst(errs[k:k + CHUNK])
            per_chunk.append(f"chunk {k // CHUNK}: {int(np.sum(~(errs[k:k + CHUNK] < tol)))} images miss, worst image {k + ik} rel {ek:.3e}")
        raise AssertionError(f"{what}: image {i} (index {i % CHUNK} of chunk {i // CHUNK}, pattern {i % P}) is off by rel {e:.3e} >= {tol:.1e}; " + "; ".join(per_chunk))
    return e


def global_rel(got, ref):
    """one norm over the whole batch (what the per-image error replaces)"""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    return np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-30)


def windows(C):
    """chains the checker replays one by one in Philox mode: the first four, both sides of the chunk seam, the last four"""
    w = list(range(0, 4)) + list(range(CHUNK - 4, min(CHUNK + 5, C))) + list(range(max(C - 4, 0), C))
    return np.array(sorted(set(c for c in w if 0 <= c < C)), dtype=np.int64)


def patterns(shape, seed=0, noise=6.0):
    """P distinct images: blocks and a ramp, another contrast, offset and noise realisation per pattern"""
    rng = np.random.default_rng(seed)
    H, W = shape
    out = np.empty((P,) + tuple(shape))
    for k in range(P):
        img = np.full(shape, 30.0 + 9.0 * k)
        for _ in range(3):
            i0, j0 = rng.integers(0, H), rng.integers(0, W)
            i1, j1 = rng.integers(i0 + 1, H + 1), rng.integers(j0 + 1, W + 1)
            img[i0:i1, j0:j1] = rng.uniform(20, 235)
        img += np.linspace(0, 20, W)[None, :] * (1 + 0.25 * k)
        out[k] = img + rng.normal(0, noise, shape)
    return out


def blur_problem(shape, k=5, seed=0, box=True):
    """(h, offset, y): a k x k blur (the uniform box, or a separable non-uniform one) of a scene plus noise"""
    rng = np.random.default_rng(seed + 100)
    if box:
        h = np.ones((k, k)) / (k * k)
    else:
        u = np.linspace(1.0, 2.0, k)
        u = u + u[::-1]
        h = np.outer(u, u) / np.sum(np.outer(u, u))
    off = (k // 2, k // 2)
    img = patterns(shape, seed + 1, noise=0.0)[3]
    y = O.blur(img, h, off) + rng.normal(0, SIGMA, shape)
    return h, off, y


H3_NONSEP = np.array([[0.02, 0.11, 0.05], [0.13, 0.34, 0.09], [0.04, 0.15, 0.07]])      # rank 3: no separable kernel covers it


# ---------------------------------------------------------------- the TV prox with upstream's early exit, and the pass it leaves in
def tv_prox_exit(x, gamma, niter, rtol):
    """(prox, pass) of ONE image: the checker's tv_prox_fgp(rtol=...) with the index of the loop pass it returned from (niter: it ran out of
    passes) -- the number the device reports through tv_exit_stats."""
    x = np.asarray(x, dtype=np.float64)
    c = 0.125 / gamma
    betas = O.fgp_betas(niter)
    rr, ss, p, q = (np.zeros_like(x) for _ in range(4))
    prev = None
    for k in range(niter):
        sol = x - gamma * O.div2d(rr, ss)
        obj = 0.5 * float(np.sum((x - sol) ** 2)) + gamma * float(O.tv_value(sol))
        rel = abs(obj - prev) / obj if (prev is not None and obj > 0) else 2 * rtol
        prev = obj
        if rel < rtol:
            return sol, k
        dr, dc = O.grad2d(sol)
        r, s = rr - c * dr, ss - c * dc
        w = np.maximum(1.0, np.sqrt(r * r + s * s))
        pn, qn = r / w, s / w
        rr, ss = pn + betas[k] * (pn - p), qn + betas[k] * (qn - q)
        p, q = pn, qn
    return x - gamma * O.div2d(rr, ss), niter


def rtol_patterns(shape, seed=3):
    """P images that leave a 10-pass prox (gamma = 0.17, rtol = 1e-4) in at least three different passes: the recipe of tests/test_gpu_rtol.py --
    one scene at several contrasts and noise levels, and the zero image, whose objectives are all zero and which runs out of passes."""
    rng = np.random.default_rng(seed)
    H, W = shape
    base = np.zeros(shape)
    base[H // 5:max(H // 2, H // 5 + 1), W // 6:2 * W // 3] = 160.0
    base[H // 2:, W // 2:] = 70.0
    base += np.linspace(0, 25, W)[None, :]
    out = np.empty((P,) + tuple(shape))
    for c in range(P):
        out[c] = base * (0.2 + 0.4 * (c % 4)) + rng.normal(0, [0.05, 0.6, 3.0, 12.0, 40.0][c % 5], shape)
    out[0] = 0.0
    return out


RTOL, RTOL_GAM, RTOL_K = 1e-4, 0.17, 10


def rtol_reference(x7, gam=RTOL_GAM, niter=RTOL_K, rtol=RTOL):
    res = [tv_prox_exit(x, gam, niter, rtol) for x in x7]
    return np.stack([r[0] for r in res]), np.array([r[1] for r in res], dtype=np.int32)


# ---------------------------------------------------------------- anisotropic TV (the checker has the isotropic prox only; tests/test_gpu_tv_aniso.py)
def tv_prox_aniso(x, gamma, niter, step=0.125):
    """prox_{gamma TV_aniso}(x): tv_prox_fgp with the dual clipped to [-1, 1] per component; images on the last two axes"""
    x = np.asarray(x, dtype=np.float64)
    c = step / gamma
    betas = O.fgp_betas(niter)
    rr, ss, p, q = (np.zeros_like(x) for _ in range(4))
    for k in range(niter):
        dr, dc = O.grad2d(x - gamma * O.div2d(rr, ss))
        pn, qn = np.clip(rr - c * dr, -1.0, 1.0), np.clip(ss - c * dc, -1.0, 1.0)
        rr, ss = pn + betas[k] * (pn - p), qn + betas[k] * (qn - q)
        p, q = pn, qn
    return x - gamma * O.div2d(rr, ss)


def tv_aniso_value(x):
    dr, dc = O.grad2d(x)
    return np.sum(np.abs(dr) + np.abs(dc), axis=(-2, -1))


def myula_step_ref(x, y, h, off, tau, gamma, prior, xi, mask=None):
    """O.myula_step, plus the anisotropic TV prior ({'kind': 'tv_aniso', ...}) assembled from the checker's own gradient"""
    x = np.asarray(x, dtype=np.float64)
    if prior["kind"] != "tv_aniso":
        return O.myula_step(x, y, h, off, 1 / SIGMA ** 2, tau, gamma, prior, xi, mask=mask)
    none = O.myula_step(x, y, h, off, 1 / SIGMA ** 2, tau, gamma, {"kind": "none"}, xi, mask=mask)       # a x - tau grad f + b x + s xi
    return none + (tau / gamma) * (tv_prox_aniso(x, prior["t"] * prior["sigma"], prior["niter"]) - x)


# ---------------------------------------------------------------- the MYMALA scene
MALA_SHAPE, MALA_SEED, MALA_TAU = (8, 8), 1234, SIGMA ** 2


def mala_scene():
    """8 x 8, 5 x 5 box blur, TV prior with 10 dual iterations, tau = sigma^2: (y, h, off, prior, x0[P], noise[P]).  The P starting states sit near
    the scene the data came from (noise of 0.5 grey levels): log alpha between -2.2 and 0.1, so a good part of the chains reject."""
    h, off = np.ones((5, 5)) / 25, (2, 2)
    img = patterns(MALA_SHAPE, 10, noise=0.0)[3]
    y = O.blur(img, h, off) + np.random.default_rng(109).normal(0, SIGMA, MALA_SHAPE)
    rng = np.random.default_rng(17)
    x0 = img[None] + rng.normal(0, 0.5, (P,) + MALA_SHAPE)
    noise = rng.standard_normal((P,) + MALA_SHAPE)
    prior = {"kind": "tv", "sigma": TAU_REG, "niter": 10, "t": GAMMA}
    return y, h, off, prior, x0, noise


def mala_reference(chain_ids, tau=MALA_TAU):
    """One MYMALA iteration of the tiled scene with the uniforms of `chain_ids`, from the checker alone:
    (log alpha [P], log u [C], accept [C], safe [C], proposals [P], x0 [P], bound) -- a chain is `safe` when |log u - log alpha| exceeds the margin
    of tests/test_gpu_mymala.py, 10 (1e-6 scale + 1e-3): the fp32 energies cannot flip its decision."""
    y, h, off, prior, x0, noise = mala_scene()
    sf = 1 / SIGMA ** 2
    zero = np.zeros_like(x0)
    mean = lambda v: O.myula_step(v, y, h, off, sf, tau, GAMMA, prior, zero)
    U = lambda v: np.add(*O.energies(v, y, h, off, sf, prior))
    mx = mean(x0)
    xp = mx + np.sqrt(2 * tau) * noise
    mxp = mean(xp)
    la_o = (U(x0) - U(xp)) - (np.sum((x0 - mxp) ** 2, axis=(-2, -1)) - np.sum((xp - mx) ** 2, axis=(-2, -1))) / (4 * tau)
    scale = np.abs(U(x0)).max()
    logu = np.log(O.philox_uniforms(MALA_SEED, 0, chain_ids))
    la_c = la_o[tile_index(len(chain_ids))]
    safe = np.abs(logu - la_c) > 10 * (1e-6 * scale + 1e-3)
    return la_o, logu, logu <= la_c, safe, xp, x0, 2e-6 * scale + 2e-3

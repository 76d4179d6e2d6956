"""Per-pixel parity of the MYULA step kernels against the checker (oracle/lmc_oracle.py): the case list, the references and the bound.  numpy only;
tests/test_pixel_reference.py (CPU) checks this harness on every case, tests/test_gpu_pixel_parity.py runs the kernels against it.  A new step kernel
adds its cases to `_build_cases` below, so both files see them.

For one case (kernel family, shape, data term, prior, blur taps, K, noise):

* every input -- x0, y, h, mask / weights / background, the injected noise -- is rounded to float32 ONCE; the library gets those numbers as they are and
  the checker gets them cast back to float64, so both sides start from the same numbers;
* the checker's step is replayed twice, in float64 (`ref64`) and in float32 (`ref32`: "every routine computes in the dtype of its input");
* `e32 = max |ref32 - ref64|` over chains and pixels is the size of float32 rounding for this operation at this shape, measured on the reference and never
  on a kernel;
* `bound = max(FACTOR * e32, 2 ulp32(max |ref64|))`.  FACTOR = 3 is a margin over the reference (a kernel may associate sums differently, contract to fma,
  use a reciprocal or rsqrt where the checker divides); it is not fitted to what a kernel achieves.  The floor: the combine a x - tau g + b prox + s xi has
  four terms and rounds at most four times in any association, each time by at most half an ulp of the largest magnitude;
* a result `got` passes if `max |got - ref64| <= bound` over EVERY chain and pixel; `check` reports the worst pixel, its region (corner, first / last row
  or column, near a declared seam of the kernel's decomposition, interior) and err / e32.

Modes.  "restart" (injected noise, 2 iterations): after the first iteration both sides restart from `ref64` rounded to float32, so the second measures
one step and not drift, and a first-step edge error cannot hide in it.  "fused" (Philox noise; two or four iterations inside one launch) and "warm" (the
TV dual carried from one iteration to the next; `set_state` would zero it) cannot restart in between: both replays run the same iterations from x0 and
the float32 replay carries its own drift, as the kernel does.  "prox": `TV.prox` alone, one evaluation.  "philox" and "philox_warm" (`PHILOX_CASES`,
below): "restart" and "warm" with the noise the kernel draws itself; their bound gains q NOISE_TOL for the device's deviates (`philox_bound_of`), and
tests/test_philox_pixel_reference.py checks them on the CPU and plants the faults of a draw that the bound has to reject.

The early exit of the TV prox (rtol > 0) is left out: its pass count is a discontinuous function of the state and is pinned by the pass-count tests.
The non-convex terms of L2_ncvx_tv (`ncvx_kind != NONE`) have cases of their own, on this file's problem recipe, bound and `check`: tests/_ncvx_pixel.py."""
import functools
from collections import namedtuple

import numpy as np

from oracle import lmc_oracle as O
import _poisson_ref as P
import _tv_aniso_ref as A
import _wl2_ref as W

SIGMA, TAU_REG = 0.75, 0.3
GAMMA, TAU = SIGMA ** 2, 0.2 * SIGMA ** 2
N_CHAINS = 2
FACTOR = 3.0
SEED, CHAIN_OFFSET = 13, 4          # Philox field of the fused launches
L1_WEIGHT, L2_WEIGHT, HAAR_WEIGHT = 0.8, 0.02, 0.3
EPROX_WEIGHT, EPROX_MU = 0.8, 100.0        # the closed-form prior: prox_uncentered_laplace(x, tau * weight, mu), la.UncenteredLaplace
POIS_GAMMA, POIS_TV, POIS_BOX = 0.02, 5.0, (0.5, 40.0)      # as tests/test_gpu_poisson.py
WL2_BOX = (0.0, 255.0)                                       # (gamma, weights and sigma_f: tests/_wl2_ref.py)
BOX = (0.0, 255.0)


def _gauss(k, s):
    t = np.exp(-0.5 * ((np.arange(k) - k // 2) / s) ** 2)
    return np.outer(t, t) / np.sum(np.outer(t, t))


BLURS = {   # name -> (taps, origin)
    "A": (np.ones((5, 5)) / 25.0, (2, 2)),
    "B": (np.outer([1.0, 2.0, 4.0, 3.0, 0.5], [0.2, 1.0, 3.0, 0.7, 0.1]) / 66.0, (2, 2)),     # asymmetric: conv vs corr, rows vs columns
    "C": (np.ones((3, 3)) / 9.0, (1, 1)),
    "D": (_gauss(7, 1.5), (3, 3)),
    "E": (np.ones((6, 6)) / 36.0, (3, 3)),                                                     # even: off-centre
    "F": (np.outer([1.0, 2.0, 4.0], [3.0, 1.0, 0.5, 0.25]) / 33.25, (0, 3)),
    "G": (np.array([[0.0, 1, 0], [1, 4, 1], [0, 1, 2]]) / 10.0, (1, 1)),                       # rank 2: the tile kernel only
}

# family, shape, term ('l2' | 'pois' | 'wl2'), data (a BLURS key | 'identity' | 'mask' | 'none'), prior ('tv' | 'aniso' | 'l1' | 'l2' | 'none' | 'haar' |
# 'eprox'), K (dual iterations the prox runs), lagged (TV(niter=K + 1, lagged_output=True)), box (None | (lo, hi)), variant, kernel (the exact
# `kernel_name`; None: the variant must refuse), mode ('restart' | 'fused' | 'warm' | 'prox' | 'philox' | 'philox_warm'), iters, seam rows, seam columns,
# tag, it0 (the iteration counter the run starts at: the Philox modes and "fused")
Case = namedtuple("Case", "family shape term data prior K lagged box variant kernel mode iters seam_rows seam_cols tag it0", defaults=(0,))


def case_id(c):
    return f"{c.family}-{c.shape[0]}x{c.shape[1]}-{c.tag}"


def _mult(step, n):
    return tuple(range(step, n, step))


def _build_cases():
    out = []

    def add(family, shape, tag, data="A", prior="tv", K=10, term="l2", lagged=False, box=None, variant=None, kernel=None, mode="restart", iters=2,
            rows=(), cols=()):
        out.append(Case(family, shape, term, data, prior, K if prior in ("tv", "aniso") else 0, lagged, box, variant or family, kernel, mode, iters,
                        tuple(rows), tuple(cols), tag))

    # ---- tile: output tiles of at most 64 x 64 with halo
    def tile(shape, tag, kernel="myula_step_tile_kernel", **kw):
        add("tile", shape, tag, kernel=kernel, rows=_mult(64, shape[0]), cols=_mult(64, shape[1]), **kw)
    for b in "ABEG":
        for s in [(3, 5), (17, 67), (66, 67), (65, 130)]:
            tile(s, f"tv10-{b}", data=b)
    for b in "CDF":
        for s in [(17, 67), (66, 67)]:
            tile(s, f"tv10-{b}", data=b)
    for d in ("identity", "mask"):
        tile((66, 67), f"tv10-{d}", data=d)
    for p in ("l1", "l2", "none"):
        tile((66, 67), f"{p}-A", prior=p)
    tile((66, 67), "tv20-A", K=20)                                                        # chunked launches of 8 + 8 + 4
    for s in [(17, 67), (66, 67)]:
        tile(s, "aniso10-A", prior="aniso")
    tile((66, 67), "tv10box-A", box=BOX, kernel="myula_step_tile_box_kernel")

    # ---- split: one wave per 64 columns, wave-count classes W <= 64, 128, 256, 512
    def split(shape, tag, **kw):
        add("split", shape, tag, kernel="myula_step_split_kernel", cols=_mult(64, shape[1]), **kw)
    for s in [(5, 64), (5, 65), (5, 128), (5, 129), (6, 256), (6, 257), (1, 300)]:
        split(s, "tv10-A")
    for K in (5, 12):
        for b in "AB":
            for s in [(5, 65), (6, 257)]:
                split(s, f"tv{K}-{b}", data=b, K=K)
    split((5, 129), "tv10-D", data="D")
    for d in ("identity", "mask"):
        split((5, 65), f"tv10-{d}", data=d)

    # ---- point: tiles of 32 rows x 64 columns
    def point(shape, tag, **kw):
        add("point", shape, tag, kernel="myula_step_point_kernel", rows=_mult(32, shape[0]), cols=_mult(64, shape[1]), **kw)
    for s in [(33, 65), (34, 130)]:
        for p in ("l1", "l2"):
            for b in "ABD":
                point(s, f"{p}-{b}", data=b, prior=p)
    point((33, 65), "eprox-B", data="B", prior="eprox")
    point((33, 65), "l1-identity", data="identity", prior="l1")

    # ---- rows: one wave per band of >= 16 rows, column strips of 496 past 512 columns
    def rows(shape, tag, kernel="myula_step_rows_kernel", **kw):
        add("rows", shape, tag, kernel=kernel, rows=_mult(16, shape[0]), cols=_mult(496, shape[1]) if shape[1] > 512 else (), **kw)
    for s in [(9, 4), (17, 67), (9, 512), (9, 516), (9, 513)]:
        for p in ("none", "l1", "l2"):
            for b in "AB":
                rows(s, f"{p}-{b}", data=b, prior=p)
    for b in "CDEF":
        for s in [(17, 67), (9, 516)]:
            rows(s, f"l1-{b}", data=b, prior="l1")
    rows((9, 512), "eprox-A", prior="eprox")
    # the closed-form instantiations need aligned rows in one strip: two strips fall to the point kernel
    rows((9, 516), "eprox-A-auto", prior="eprox", variant="auto", kernel="myula_step_point_kernel")

    # ---- block: 8 x 8 register blocks
    for s in [(8, 8), (16, 72)]:
        for p in ("haar", "l1", "l2"):
            for d in ("identity", "mask"):
                add("block", s, f"{p}-{d}", data=d, prior=p, kernel="myula_step_block_kernel", rows=_mult(8, s[0]), cols=_mult(8, s[1]))

    # ---- two and four iterations per launch (Philox noise only)
    for s in [(16, 264), (40, 132)]:
        for p in ("l2", "l1"):
            add("rows_pair", s, f"{p}-A-2it", prior=p, variant="rows", kernel="myula_step_rows_pair_kernel", mode="fused", iters=2)
    for d in ("identity", "mask"):
        add("block_fused", (16, 72), f"haar-{d}-2it", data=d, prior="haar", variant="block", kernel="myula_step_block_kernel(2 iterations)", mode="fused",
            iters=2, rows=(8,), cols=_mult(8, 72))
        add("block_fused", (16, 72), f"haar-{d}-4it", data=d, prior="haar", variant="block", kernel="myula_step_block_kernel(4 iterations)", mode="fused",
            iters=4, rows=(8,), cols=_mult(8, 72))

    # ---- pipe (one team) and pipe2 (two teams: a seam in the middle), column strips of 512
    def pipe(shape, tag, kernel="myula_step_pipe_kernel", variant="pipe", **kw):
        cols = _mult(512, shape[1]) if shape[1] > 512 else ((shape[1] // 2,) if variant == "pipe2" else ())
        add("pipe2" if variant == "pipe2" else "pipe", shape, tag, variant=variant, kernel=kernel, cols=cols, **kw)
    for s in [(6, 132), (6, 264)]:
        for K in (2, 6, 8):
            pipe(s, f"tv{K}-A", K=K)
        pipe(s, "tv9lagged-A", K=9, lagged=True)
    for b in "BCDEF":
        for s in [(6, 264), (6, 260)]:
            pipe(s, f"tv10-{b}", data=b)
    for b in "BC":
        pipe((6, 264), f"tv10-{b}", data=b, variant="pipe2")
    for s in [(6, 136), (6, 264), (1, 256)]:
        for d in ("identity", "mask", "none"):
            pipe(s, f"tv10-{d}", data=d)
        pipe(s, "tv10-prox", data="none", mode="prox", iters=1, variant="auto", kernel="")       # TV.prox: no sampler, no kernel name to read
    for s in [(6, 129), (6, 133), (6, 257), (6, 261)]:
        pipe(s, "tv10-A-unaligned")
    for s in [(6, 513), (6, 1024), (6, 1026)]:
        pipe(s, "tv10-A-strips")
    for s, K in [((6, 264), 20), ((6, 264), 29), ((6, 264), 60), ((6, 132), 30)]:
        pipe(s, f"tv{K}-A-chained", K=K, lagged=K == 29)
    for s in [(6, 264), (6, 132)]:
        for K in (1, 2, 3):
            pipe(s, f"tv{K}-A-warm", K=K, mode="warm", iters=3, variant="auto", kernel="myula_step_pipe_kernel(warm)")
    for s in [(6, 264), (6, 520)]:
        pipe(s, "aniso10-A", prior="aniso", kernel="myula_step_pipe_aniso_kernel")
    pipe((6, 264), "aniso10-A", prior="aniso", variant="pipe2", kernel="myula_step_pipe_aniso_kernel")
    for s in [(6, 264), (6, 132)]:
        for K in (10, 20):
            pipe(s, f"tv{K}box-A", K=K, box=BOX, kernel="myula_step_pipe_box_kernel")
    pipe((6, 264), "tv10box-A", box=BOX, variant="pipe2", kernel="myula_step_pipe_box2_kernel")

    # ---- Poisson and weighted Gaussian data terms: the pipe and tile instantiations of their own
    for term, box in (("pois", POIS_BOX), ("wl2", WL2_BOX)):
        for s in [(6, 264), (6, 136)]:
            add(term, s, "pipe-tv10-A", term=term, variant="pipe", kernel=f"myula_step_pipe_{term}_kernel")
        add(term, (6, 264), "pipe-tv10box-A", term=term, box=box, variant="pipe", kernel=f"myula_step_pipe_{term}_box_kernel")
        for s in [(17, 67), (66, 67)]:
            add(term, s, "tile-tv10-A", term=term, variant="tile", kernel=f"myula_step_tile_{term}_kernel", rows=_mult(64, s[0]), cols=_mult(64, s[1]))
        add(term, (17, 67), "tile-tv10box-A", term=term, box=box, variant="tile", kernel=f"myula_step_tile_{term}_box_kernel", cols=(64,))
    return out


CASES = _build_cases()
IDS = [case_id(c) for c in CASES]
assert len(set(IDS)) == len(IDS), "case ids must be unique"

# pairs (one team, two teams) that cover the same case: their states must also be bit-equal
LAYOUT_PAIRS = [(a, b) for a in CASES for b in CASES if a.family == "pipe" and b.family == "pipe2" and a._replace(family="", variant="", kernel="", seam_cols=())
                == b._replace(family="", variant="", kernel="", seam_cols=())]


# ------------------------------------------------------------------ the Philox cases: the noise the step kernel draws itself
# Every case above but the six fused launches injects its noise, so the counter arithmetic of a kernel's own draw -- (quad, iteration, global chain,
# stream), the quad q = (i >> 2) W + j -- is held per pixel nowhere else.  A Philox case is an injected-noise case with the noise source changed and
# nothing else: same family, shape, terms, kernel.  Mode "philox" is "restart" with the noise of iteration `it` taken from the field
# O.philox_normals(SEED_P, it0 + it, CHAIN_OFFSET + arange(N_CHAINS), H, W); "philox_warm" is "warm" with that field.  The device side sets the counter
# (`smp.iteration = it0 + it`) before every single-iteration launch.  Left out: the rtol > 0 instantiations -- their pass count is discontinuous, and their
# Philox code is the same template code.
SEED_P = 0x9E3779B185EBCA87            # both 32-bit halves non-zero and distinct: key0 and key1 swapped or one of them dropped shows
NOISE_TOL = 2e-5                       # the project's stated error of a device deviate (lmc_device.h, rung R3); not fitted here
IT_TOP, IT_TOP_FUSED = 0xFFFFFFFD, 0xFFFFFFFB      # the library allows iteration + n <= 0xFFFFFFFF: two single launches, one launch of four
PHILOX_MODES = ("philox", "philox_warm")


def _seams(variant, shape):
    H, W = shape
    rows = {"tile": 64, "point": 32, "rows": 16, "block": 8}.get(variant)
    if variant in ("tile", "split", "point", "block"):
        cols = _mult(8 if variant == "block" else 64, W)
    elif variant == "rows":
        cols = _mult(496, W) if W > 512 else ()
    else:
        cols = _mult(512, W) if W > 512 else ((W // 2,) if variant == "pipe2" else ())
    return (_mult(rows, H) if rows else ()), cols


def _build_philox_cases():
    by_key = {}
    for c in CASES:
        by_key.setdefault((c.family, c.tag), []).append(c)
    out = []

    def twin(family, shape, tag, it0=0, mode="philox", suffix="", name=None):
        """The injected-noise case (family, tag) at `shape` -- the one of CASES where it has that shape, else its recipe at the new shape -- with the
        noise source changed."""
        base = next((c for c in by_key[(family, tag)] if c.shape == shape), by_key[(family, tag)][0])
        assert base.mode in ("restart", "warm", "fused"), case_id(base)
        rows, cols = _seams(base.variant if base.variant != "auto" else "pipe", shape)
        out.append(base._replace(shape=shape, seam_rows=rows, seam_cols=cols, mode=mode, tag=f"{name or tag}-philox{suffix}", it0=it0))

    for s in [(3, 5), (17, 67), (66, 67), (65, 130)]:
        twin("tile", s, "tv10-A")
    for tag in ("tv20-A", "tv10box-A", "l1-A"):                # tv20: chunks of 8 + 8 + 4 dual iterations, the noise added once
        twin("tile", (66, 67), tag)
    twin("tile", (17, 67), "aniso10-A")
    for s in [(5, 64), (5, 65), (5, 129), (6, 257), (1, 300)]:
        twin("split", s, "tv10-A")
    twin("split", (5, 65), "tv5-B")
    twin("point", (33, 65), "l1-B")
    twin("point", (34, 130), "l2-A")
    twin("point", (33, 65), "eprox-B")
    for s in [(9, 4), (17, 67), (9, 512), (9, 513), (9, 516)]:     # (one iteration per launch: policy iterations_per_launch = 1)
        twin("rows", s, "l1-A")
    twin("rows", (17, 67), "none-B")
    twin("rows", (9, 512), "eprox-A")
    for s in [(8, 8), (16, 72)]:
        for p in ("haar", "l1"):
            for d in ("identity", "mask"):
                twin("block", s, f"{p}-{d}")
    # pipe.  Quad boundaries: H on either side of 4, 8, 12 at PXL = 8 (W = 264) and PXL = 4 (W = 136); three row-groups (H = 9, 13) exercise both halves
    # of the double-buffered slab and a partial last quad.  The recipe of the K = 10, blur A launch is that of "tv10-A-unaligned".
    for W in (264, 136):
        for H in (1, 2, 3, 4, 5, 7, 8, 9, 13):
            twin("pipe", (H, W), "tv10-A-unaligned", name="tv10-A")
    for s in [(6, 129), (6, 132), (6, 133), (6, 257), (6, 260), (6, 261)]:
        twin("pipe", s, "tv10-A-unaligned", name="tv10-A")
    for s in [(6, 513), (6, 1024), (6, 1026), (5, 1544)]:
        twin("pipe", s, "tv10-A-strips", name="tv10-A")
    for tag in ("tv10-B", "tv10-D", "tv2-A", "tv6-A", "tv8-A", "tv9lagged-A", "tv20-A-chained", "tv29-A-chained", "tv60-A-chained", "tv10box-A", "tv20box-A"):
        twin("pipe", (6, 264), tag)
    twin("pipe", (6, 132), "tv30-A-chained")
    for d in ("identity", "mask", "none"):
        twin("pipe", (6, 136), f"tv10-{d}")
    for s in [(6, 264), (6, 520)]:
        twin("pipe", s, "aniso10-A")
    for tag in ("tv10-B", "aniso10-A", "tv10box-A"):
        twin("pipe2", (6, 264), tag)
    for term in ("pois", "wl2"):
        for s in [(6, 264), (6, 136)]:
            twin(term, s, "pipe-tv10-A")
        twin(term, (6, 264), "pipe-tv10box-A")
        twin(term, (17, 67), "tile-tv10-A")
    for K in (1, 2, 3):        # the warm dual cannot restart: the field as the noise of three carried iterations
        twin("pipe", (6, 264), f"tv{K}-A-warm", mode="philox_warm")
    # the counter's top: iterations 0xFFFFFFFD and 0xFFFFFFFE in single launches, 0xFFFFFFFB .. 0xFFFFFFFE inside the launches of two and four
    twin("tile", (17, 67), "tv10-A", it0=IT_TOP, suffix="-top")
    twin("split", (5, 65), "tv10-A", it0=IT_TOP, suffix="-top")
    twin("rows", (17, 67), "l1-A", it0=IT_TOP, suffix="-top")
    twin("block", (16, 72), "haar-mask", it0=IT_TOP, suffix="-top")
    twin("pipe", (6, 264), "tv10-B", it0=IT_TOP, suffix="-top")
    for c in CASES:
        if c.mode == "fused":
            out.append(c._replace(tag=c.tag + "-top", it0=IT_TOP_FUSED))
    return out


PHILOX_CASES = _build_philox_cases()
PHILOX_IDS = [case_id(c) for c in PHILOX_CASES]
assert len(set(PHILOX_IDS + IDS)) == len(PHILOX_IDS) + len(IDS), "case ids must be unique"
PHILOX_LAYOUT_PAIRS = [(a, b) for a in PHILOX_CASES for b in PHILOX_CASES if a.family == "pipe" and b.family == "pipe2" and a.it0 == b.it0
                       and a._replace(family="", variant="", kernel="", seam_cols=()) == b._replace(family="", variant="", kernel="", seam_cols=())]


def seed_of(c):
    return SEED_P if c.mode in PHILOX_MODES else SEED


def philox_field(c, it):
    """The noise of iteration `it` of a Philox case, as the "fused" mode computes it."""
    return O.philox_normals(seed_of(c), c.it0 + it, np.arange(CHAIN_OFFSET, CHAIN_OFFSET + N_CHAINS), *c.shape)


def noise_gain(c):
    """q, the coefficient of xi in the case's step: sqrt(2 tau) in the step's float32 (tests/test_philox_pixel_reference.py checks it against the
    checker: step(x, 1) - step(x, 0))."""
    return float(np.sqrt(np.float32(2.0 * problem(c).tau)))


# ------------------------------------------------------------------ the problem of a case: float32 numbers, made once
def f32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32))


def step_image(shape, level=190.0):
    """The image of tests/test_gpu_pipe.py: a block of `level` on a ramp, so that edges and flat areas both occur."""
    img = np.zeros(shape)
    img[shape[0] // 5:shape[0] // 2 + 1, shape[1] // 4:shape[1] // 2 + 2] = level
    img += np.linspace(0, 30, shape[1])[None, :]
    return img


Problem = namedtuple("Problem", "h offset mask aux y x0 noise tau gamma sigma_f")      # aux: the background (pois) or the weights (wl2)


@functools.lru_cache(maxsize=None)
def problem(c):
    rng = np.random.default_rng(1000 * c.shape[0] + c.shape[1])
    shape = c.shape
    h, off = (f32(BLURS[c.data][0]), BLURS[c.data][1]) if c.data in BLURS else (None, None)
    mask = f32(rng.uniform(size=shape) < 0.6) if c.data == "mask" else None
    op = P.Op("blur", h.astype(np.float64), off) if h is not None else (P.Op("mask", mask.astype(np.float64)) if mask is not None else P.Op("identity"))
    aux = None
    if c.term == "pois":
        aux = f32(P.ramp_background(shape))
        _, _, y, _, x0 = P.recipe(shape, n_chains=N_CHAINS, seed=shape[1], op=op, beta=aux.astype(np.float64))
        y, x0 = f32(y), f32(x0)
        gamma, sigma_f = POIS_GAMMA, 1.0
        tau = 0.5 / (P.PoissonRef(op, y, aux, sigma_f).grad_lipschitz() + 1.0 / gamma)
    elif c.term == "wl2":
        _, _, y, w, x0 = W.recipe(shape, n_chains=N_CHAINS, seed=shape[1], op=op)
        w[0, :] = 0.0       # a zero row at the top and a zero column at the right edge: a weight row or column read one off shows
        w[:, -1] = 0.0
        aux, y, x0 = f32(w), f32(y), f32(x0)
        gamma, sigma_f = W.GAMMA, W.SIGMA_F
        tau = W.step_size(W.WL2Ref(op, y, aux, sigma_f))
    else:
        img = step_image(shape, 250.0 if c.box else 190.0)       # with a box: the block at 250, so that the clamp at 255 acts
        y = f32(op.fwd(img) + rng.normal(0, SIGMA, shape) * (mask if mask is not None else 1.0))
        x0 = f32(img[None] + rng.normal(0, 10, (N_CHAINS,) + shape))
        gamma, sigma_f, tau = GAMMA, 1 / SIGMA ** 2, TAU
    if c.mode == "fused" or c.mode in PHILOX_MODES:
        noise = np.stack([philox_field(c, i) for i in range(c.iters)])
        assert noise.dtype == np.float32
    else:
        noise = f32(rng.standard_normal((c.iters, N_CHAINS) + shape))
    for a in (h, mask, aux, y, x0, noise):
        if a is not None:
            a.setflags(write=False)
    return Problem(h, off, mask, aux, y, x0, noise, tau, gamma, sigma_f)


# ------------------------------------------------------------------ the checker's step of a case, in the dtype handed in
class _Data:
    """sigma_f Op^T (Op x - y), or nothing: the plain Gaussian data term over `_poisson_ref.Op`, in `dtype`."""

    def __init__(self, op, y, sigma_f, dtype):
        self.op, self.y, self.sigma_f = op, (None if y is None else np.asarray(y, dtype=dtype)), np.dtype(dtype).type(sigma_f)

    def grad(self, x):
        return np.zeros_like(x) if self.op is None else self.sigma_f * self.op.adj(self.op.fwd(x) - self.y)


class _Prox:
    def __init__(self, fn):
        self.prox = fn


def weight(c):
    return {"tv": POIS_TV if c.term == "pois" else TAU_REG, "aniso": TAU_REG, "l1": L1_WEIGHT, "l2": L2_WEIGHT, "haar": HAAR_WEIGHT, "eprox": EPROX_WEIGHT,
            "none": 0.0}[c.prior]


class Stepper:
    """One replay of the checker in `dtype`; `step(x, xi)` -> the next state.  The warm mode carries the TV dual in the object."""

    def __init__(self, c, dtype):
        self.c, self.m, self.dtype = c, problem(c), np.dtype(dtype)
        m = self.m
        self.standard = c.term == "l2" and c.data != "none" and c.box is None and c.prior in ("tv", "l1", "l2", "none", "haar")
        cast = lambda a: None if a is None else a.astype(dtype)
        self.h, self.mask, self.y = cast(m.h), cast(m.mask), cast(m.y)
        if self.standard:       # the checker's own step, as the rel-L2 tests call it
            self.prior = {"kind": c.prior, "sigma": weight(c), "niter": c.K, "t": m.gamma}
            if c.mode in ("warm", "philox_warm"):
                self.prior["warm"] = True
            return
        op = P.Op("blur", self.h, m.offset) if m.h is not None else (P.Op("mask", self.mask) if m.mask is not None else P.Op("identity"))
        if c.term == "pois":
            self.pf = P.PoissonRef(op, m.y, m.aux, m.sigma_f, dtype=dtype)
        elif c.term == "wl2":
            self.pf = W.WL2Ref(op, m.y, m.aux, m.sigma_f, dtype=dtype)
        else:
            self.pf = _Data(None if c.data == "none" else op, None if c.data == "none" else m.y, m.sigma_f, dtype)
        wgt = weight(c)
        if c.box is not None:       # the recipe of tests/_poisson_ref.py: the primal iterate clipped inside every dual iteration
            self.pg = P.TVRef(c.shape, wgt, c.K, c.box, aniso=c.prior == "aniso", dtype=dtype)
        elif c.prior == "tv":
            self.pg = _Prox(lambda x, t: O.tv_prox_fgp(x, wgt * t, c.K))
        elif c.prior == "aniso":
            self.pg = _Prox(lambda x, t: A.tv_prox_aniso(x, wgt * t, c.K))
        elif c.prior == "eprox":
            self.pg = _Prox(lambda x, t: O.prox_uncentered_laplace(x, wgt * t, EPROX_MU))
        else:
            raise ValueError(c.prior)

    def _step(self, x, tau, xi):
        c, m = self.c, self.m
        x, xi = np.asarray(x, dtype=self.dtype), np.asarray(xi, dtype=self.dtype)
        if self.standard:
            out = O.myula_step(x, self.y, self.h, m.offset, m.sigma_f, tau, m.gamma, self.prior, xi, mask=self.mask)
        else:
            out = P.myula_step(self.pf, self.pg, x, tau, m.gamma, xi, dtype=self.dtype)
        assert out.dtype == self.dtype, (case_id(c), out.dtype)
        return out

    def step(self, x, xi):
        return self._step(x, self.m.tau, xi)

    def advance(self, x, t):
        """v + t drift(v), drift(v) = -grad f(v) - (v - prox(v)) / gamma: the checker's step with tau = t and xi = 0 (what the stages of SK-ROCK are made
        of; tests/_skrock_pixel.py)."""
        return self._step(x, t, 0.0)

    def prox(self, x, t):
        return O.tv_prox_fgp(np.asarray(x, dtype=self.dtype), weight(self.c) * t, self.c.K)


def replay32(c, noise):
    """The launch-form float32 replay of case `c` with `noise` ([iters, chains, H, W]) in place of its own: the float32 state after every iteration, from
    the starts of `reference(c)` ("restart", "philox") or carried from x0.  What a kernel with a fault in its draw would hold."""
    s32, out, x = Stepper(c, np.float32), [], problem(c).x0
    for it, st in enumerate(reference(c)):
        x = s32.step(st.start if st.start is not None else x, f32(noise[it]))
        out.append(x)
    return out


def ulp32(v):
    return float(np.spacing(np.float32(abs(v))))


def bound_of(ref64, ref32, factor=FACTOR):
    e32 = float(np.max(np.abs(ref32.astype(np.float64) - ref64)))
    return e32, max(factor * e32, 2.0 * ulp32(np.max(np.abs(ref64))))


PROX_T = 2.5       # the prox parameter of the "prox" mode: TV.prox(x, PROX_T), as tests/test_gpu_pipe.py

# start: the float32 state both sides start the comparison's iteration(s) from (None: they carry their own); compare: whether the device state is compared
# after this iteration
# after this iteration
Stage = namedtuple("Stage", "start ref64 ref32 e32 bound compare")
# a stage of the Philox modes; noise_term: the part of `bound` that is not rounding, q NOISE_TOL per carried iteration
PStage = namedtuple("PStage", Stage._fields + ("noise_term",))


def philox_bound_of(c, ref64, ref32, carried=1):
    """The bound of a Philox stage: max(3 e32, 2 ulp32) + carried q NOISE_TOL.  The second term is there because the reference's field is exact
    arithmetic (float64 log / sqrt / sin / cos, rounded once) and the device's is hardware log2 / sqrt / sin / cos, which lmc_device.h states to within
    NOISE_TOL per deviate; the deviate enters the state as q xi.  `carried`: the iterations since both sides last started from the same state (the warm
    dual cannot restart) -- the step without its noise does not expand a difference (tau is below the stability limit), so the terms add."""
    e32, rounding = bound_of(ref64, ref32)
    term = carried * noise_gain(c) * NOISE_TOL
    return e32, rounding + term, term


@functools.lru_cache(maxsize=None)
def reference(c):
    """The stages of case `c`, computed once: a tuple of `Stage`, one per iteration."""
    m = problem(c)
    s64, s32 = Stepper(c, np.float64), Stepper(c, np.float32)
    stages = []
    if c.mode == "prox":
        r64, r32 = s64.prox(m.x0, PROX_T), s32.prox(m.x0, PROX_T)
        stages.append(Stage(m.x0, r64, r32, *bound_of(r64, r32), True))
    elif c.mode in ("restart", "philox"):
        start = m.x0
        for it in range(c.iters):
            r64, r32 = s64.step(start, m.noise[it]), s32.step(start, m.noise[it])
            if c.mode == "philox":
                e32, bound, term = philox_bound_of(c, r64, r32)
                stages.append(PStage(start, r64, r32, e32, bound, True, term))
            else:
                stages.append(Stage(start, r64, r32, *bound_of(r64, r32), True))
            start = f32(r64)
    elif c.mode == "philox_warm":
        x64, x32 = m.x0.astype(np.float64), m.x0
        for it in range(c.iters):
            x64, x32 = s64.step(x64, m.noise[it]), s32.step(x32, m.noise[it])
            e32, bound, term = philox_bound_of(c, x64, x32, carried=it + 1)
            stages.append(PStage(m.x0 if it == 0 else None, x64, x32, e32, bound, True, term))
    else:       # fused, warm: no restart in between
        x64, x32 = m.x0.astype(np.float64), m.x0
        for it in range(c.iters):
            x64, x32 = s64.step(x64, m.noise[it]), s32.step(x32, m.noise[it])
            stages.append(Stage(m.x0 if it == 0 else None, x64, x32, *bound_of(x64, x32), c.mode == "warm" or it == c.iters - 1))
    for st in stages:
        for a in (st.ref64, st.ref32):
            a.setflags(write=False)
        assert st.ref64.dtype == np.float64 and st.ref32.dtype == np.float32
    return tuple(stages)


# ------------------------------------------------------------------ regions and the check
def taps_of(c):
    return max(BLURS[c.data][0].shape) if c.data in BLURS else 1


def reach_of(c):
    """How far from a seam an error of the seam's handling can sit: the halo of the stencils, taps - 1 for the blur and its adjoint, one pixel per dual
    iteration of a launch (at most 10 per launch in every kernel) for the TV prox; at least the two pixels that touch the seam."""
    return max(taps_of(c) - 1, min(c.K, 10), 1)


def region(c, i, j):
    H, W = c.shape
    top, bottom, left, right = i == 0, i == H - 1, j == 0, j == W - 1
    if (top or bottom) and (left or right):
        return "corner"
    d = reach_of(c)
    if H <= 2:      # every pixel is on the first or the last row: the column seams are the finer class
        for s in c.seam_cols:
            if not (left or right) and s - d <= j < s + d:
                return f"column seam {s}"
    if top or bottom:
        return ("first row" if top else "last row") if H > 1 else "first and last row"
    if left or right:
        return "first column" if left else "last column"
    for s in c.seam_rows:
        if s - d <= i < s + d:
            return f"row seam {s}"
    for s in c.seam_cols:
        if s - d <= j < s + d:
            return f"column seam {s}"
    return "interior"


def region_pixels(c):
    """One pixel per region class the case has: {region: (i, j)}; a seam by a pixel that touches it, away from the other seams and the edges."""
    H, W = c.shape
    mi, mj = min(H - 1, max(1, H // 2)), min(W - 1, max(1, W // 2))
    by_mid = lambda n, m: sorted(range(n), key=lambda v: abs(v - m))
    cand = [(0, 0), (H - 1, W - 1), (0, mj), (H - 1, mj), (mi, 0), (mi, W - 1)]
    cand += [(i, j) for s in c.seam_rows for j in by_mid(W, mj) for i in (s, s - 1) if region(c, i, j) == f"row seam {s}"][:len(c.seam_rows) * 2 * W]
    cand += [(i, j) for s in c.seam_cols for i in by_mid(H, mi) for j in (s, s - 1) if region(c, i, j) == f"column seam {s}"]
    cand += [(i, j) for i in by_mid(H, mi) for j in by_mid(W, mj) if region(c, i, j) == "interior"][:1]
    out = {}
    for i, j in cand:
        out.setdefault(region(c, i, j), (i, j))
    return out


Verdict = namedtuple("Verdict", "ok err bound e32 ratio where region message")


def check(c, it, got, stage):
    """max |got - ref64| over every chain and pixel against the stage's bound; prints `pixel <case>: err ... e32 ... ratio ...`."""
    got = np.asarray(got)
    assert got.shape == stage.ref64.shape, (got.shape, stage.ref64.shape)
    d = np.abs(got.astype(np.float64) - stage.ref64)
    if not np.isfinite(d).all():
        d = np.where(np.isfinite(d), d, np.inf)
    k = np.unravel_index(int(np.argmax(d)), d.shape)
    err = float(d[k])
    reg = region(c, int(k[1]), int(k[2]))
    ratio = err / stage.e32 if stage.e32 > 0 else float("inf")
    interior = [d[:, i, j].max() for i in range(d.shape[1]) for j in range(d.shape[2]) if region(c, i, j) == "interior"] if err > stage.bound else []
    msg = (f"pixel {case_id(c)} it {it}: err {err:.3e} at chain {k[0]} pixel ({k[1]}, {k[2]}) [{reg}], e32 {stage.e32:.3e}, ratio {ratio:.2f}, "
           f"bound {stage.bound:.3e}" + (f", worst interior pixel {max(interior):.3e}" if interior else ""))
    print(msg)
    return Verdict(err <= stage.bound, err, stage.bound, stage.e32, ratio, tuple(int(v) for v in k), reg, msg)


def rel(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)

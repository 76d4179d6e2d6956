"""CPU checks of the lattice harness (tests/_lattice.py) on itself: the expectation table is total, every combination runs on some shape, the float64
reference of every running cell differs from each of its lattice neighbours by far more than the bound the GPU comparison uses, and the check that
tests/test_gpu_lattice.py applies to a device state rejects every neighbour put in its place.  No GPU, no library."""
import numpy as np
import pytest

import _lattice as T
import _poisson_ref as P

SHAPE_IDS = [f"{h}x{w}" for h, w in T.SHAPES]
PAIRS = [(s, k) for s in T.SHAPES for k in T.KINDS]
PAIR_IDS = [f"{s[0]}x{s[1]}-{T.KIND_NAMES[k]}" for s, k in PAIRS]
MARGIN = 10.0          # a neighbour is at least this many bounds away at some pixel


def left_out_by_rule(shape):
    """The number of cells the three shape preconditions forbid, counted from the rules and not from the cells: 26 combinations per data kind, 40 cells
    of each wavelet prior (20 kinds, box or not), two of which a spectral kind holds."""
    H, W = shape
    spectral = 0 if (T.power_of_two(H) and T.power_of_two(W)) else 1
    haar = 1 if (H % 8 or W % 8) else 0
    db2 = 1 if (H % 4 or W % 4 or min(H, W) // 2 < 4) else 0
    return 26 * spectral + (40 - 2 * spectral) * (haar + db2)


@pytest.mark.parametrize("shape", T.SHAPES, ids=SHAPE_IDS)
def test_the_table_is_total(shape):
    every = T.all_cells(shape)
    assert len(every) == 520 and len(set(every)) == 520
    out = [c for c in every if T.left_out(c) is not None]
    assert len(out) == left_out_by_rule(shape), (len(out), left_out_by_rule(shape))
    counts = {}
    for sampler in T.SAMPLERS:
        run = refused = 0
        for c in T.cells(shape):
            e = T.expected(c, sampler)
            if e == "runs":
                run += 1
            else:
                status, phrases = e
                assert status == T.LMC_E_UNSUPPORTED and phrases and all(isinstance(p, str) and p for p in phrases), (T.cell_id(c), e)
                refused += 1
        assert run + refused + len(out) == 520
        counts[sampler] = (run, refused)
    print(f"lattice {shape}: {counts['myula'][0]} cells run and {counts['myula'][1]} are refused under MYULA, {counts['skrock'][0]} and {counts['skrock'][1]} "
          f"under SK-ROCK, {len(out)} left out")


def test_every_combination_runs_on_some_shape():
    seen = {tuple(c[1:]) for s in T.SHAPES for c in T.cells(s)}
    missing = [c for c in T.combinations() if c not in seen]
    print(f"combinations never exercised: {len(missing)} of {len(T.combinations())}")
    assert not missing
    assert all(T.left_out(c) is None for c in T.all_cells((16, 64))), "(16, 64) satisfies every precondition"


def test_the_table_by_hand():
    """A few rows spelled out from include/lmc_atomi.h."""
    s = (16, 64)
    E = lambda k, p, b, e, smp: T.expected(T.Cell(s, k, p, b, e), smp)       # noqa: E731
    for k in T.KINDS:
        assert E(k, "tv10", T.BOX, "scalar", "myula") == "runs"
        assert E(k, "db2", None, "scalar", "skrock") == "runs"
        assert E(k, "l1", T.BOX, "array", "myula") == "runs"
        assert E(k, "l1", None, "array", "skrock")[1] == ("epsg",)
        assert E(k, "aniso10", T.BOX, "scalar", "skrock")[1] == ("box",)
        assert E(k, "vtv", None, "scalar", "myula") == (T.LMC_E_UNSUPPORTED, ("VTV",))
        assert (E(k, "haar", None, "scalar", "myula") == "runs") == (k not in (4, 5, 6, 7, 8, 13, 14))
        assert E(k, "db2", T.BOX, "scalar", "myula")[1] == ("box",)


@pytest.mark.parametrize("shape", T.SHAPES, ids=SHAPE_IDS)
def test_start_states_and_data_reach_every_branch(shape):
    for k in T.KINDS:
        if T.OPERATOR[k] == "spectral" and not (T.power_of_two(shape[0]) and T.power_of_two(shape[1])):
            continue
        m = T.problem(shape, k)
        assert (m.x0 < 0).mean() > 0.01 and (m.x0 > 255).mean() > 0.01, T.KIND_NAMES[k]
        if T.TERM[k] == "hub":          # residuals on both sides of the thresholds, both special thresholds present
            r = np.abs(T.operator_of(m, np.float64).fwd(m.x0.astype(np.float64)) - m.y)
            inside = float((r <= m.aux).mean())
            assert 0.1 < inside < 0.9 and (m.aux == 0).any() and np.isinf(m.aux).any(), (T.KIND_NAMES[k], inside)
        if T.TERM[k] == "pois":         # both branches of phi', counts at and near the background
            u = T.operator_of(m, np.float64).fwd(m.x0.astype(np.float64))
            assert (u < 0).any() and (u > 0).any() and (np.abs(m.y - m.aux) <= 2.0 * np.sqrt(m.aux) + 1).mean() > 0.05, T.KIND_NAMES[k]
        if T.TERM[k] == "wl2":
            assert (m.aux == 0).mean() > 0.1


@pytest.mark.parametrize("shape,kind", PAIRS, ids=PAIR_IDS)
def test_the_reference_tells_a_cell_from_its_neighbours(shape, kind):
    """For every running cell the float64 iterate differs from each neighbour's -- the prior dropped, the box dropped, the clamp on the state instead of
    the prox, the plain Gaussian term, epsg by its mean -- by more than 10 bounds at some pixel, and the GPU-side check rejects the neighbour (rounded to
    float32, as a device would hold it) in the place of the device state."""
    todo = [c for c in T.cells(shape) if c.kind == kind and T.runs(c, "myula")]
    if not todo:
        assert T.OPERATOR[kind] == "spectral"
        return
    m = T.problem(shape, kind)
    weak, worst = [], (np.inf, "")
    for c in todo:
        st = T.reference(c, "myula")[0]
        own = T.check(T.cell_id(c), T.f32(st.ref64), st)
        assert own.ok, own.message
        for name, (applies, wrong) in T.NEIGHBOURS.items():
            if not applies(c):
                continue
            other = T.myula(c, m.x0, m.noise[0], np.float64, **wrong)
            d = float(np.max(np.abs(other - st.ref64))) / st.bound
            if T.same_by_construction(c, name):
                assert d == 0.0, (T.cell_id(c), name, d)
                continue
            if d < worst[0]:
                worst = (d, f"{T.cell_id(c)} / {name}")
            if not d > MARGIN or T.check(name, T.f32(other), st).ok:
                weak.append(f"{T.cell_id(c)} / {name}: {d:.2f} bounds")
    print(f"{shape} {T.KIND_NAMES[kind]}: {len(todo)} running cells, nearest neighbour {worst[0]:.1f} bounds away ({worst[1]})")
    assert not weak, "\n".join(weak)


@pytest.mark.parametrize("kind", [0, 5, 12, 15, 18], ids=lambda k: T.KIND_NAMES[k])
def test_skrock_reference_is_the_recursion_of_the_header(kind):
    """The composed SK-ROCK iterate against the recursion restated from the text of lmc_skrock_create (tests/_poisson_ref.py), float64; and its two
    float32 replays stay inside the bound they define."""
    shape = (16, 64)
    for prior in ("none", "l1", "tv10", "db2"):
        c = T.Cell(shape, kind, prior, None, "scalar")
        m, pf, pg = T.terms(c, np.float64)
        st = T.reference(c, "skrock")[0]
        want = P.skrock_iteration(pf, pg, m.x0.astype(np.float64), m.Z[0].astype(np.float64), m.delta, m.gamma, T.SK_STAGES, T.SK_ETA)
        assert np.max(np.abs(want - st.ref64)) <= 1e-9 * np.max(np.abs(want)), T.cell_id(c)
        assert 3.0 * st.e32 <= st.bound and st.e32 > 0
        assert not T.check("start", m.x0, st).ok, "an iterate that did not move is rejected"

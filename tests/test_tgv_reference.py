"""CPU only: the numpy restatement of the TGV prior (tests/_tgv_ref.py) is checked on its own before a kernel is measured against it -- the adjoint
identity of its operators, the norm bound behind the default step, what the prior is for (a ramp survives where TV flattens it), that the loop
descends to the energy of a long run, that the box form is not clip-afterwards, and that the bound of tests/_pixel.py rejects every planted fault.

The case list crosses alpha0 in {0.1, 0.5, 2.0} with lam in {0.75, 2.5, 40}: with alpha0 = 2 the second-order ball is not active within 23 iterations
on these inputs, so a fault in its norm (e12 counted once) changes nothing there; it shows from K = 5 at alpha0 = 0.1 and 0.5."""
import numpy as np
import pytest

import _pixel as PX
import _tgv_ref as T
from oracle import lmc_oracle as O

SMALL = [(4, 4), (5, 7), (16, 24)]


def test_adjoint_identity():
    rng = np.random.default_rng(1)
    for shape in [(1, 9), (9, 1), (5, 7), (13, 17)]:
        u, w1, w2, p1, p2, q11, q22, q12 = (rng.normal(size=shape) for _ in range(8))
        # <E w, q>_F = -<w, div2 q>
        e11, e22, e12 = T.sym_grad(w1, w2)
        d1, d2 = T.div2(q11, q22, q12)
        lhs, rhs = np.sum(e11 * q11 + e22 * q22 + 2 * e12 * q12), -np.sum(w1 * d1 + w2 * d2)
        assert abs(lhs - rhs) <= 1e-12 * max(1.0, abs(lhs)), (shape, lhs, rhs)
        # <K (u, w), (p, q)> = <(u, w), K^T (p, q)>
        k = T.operator_K(u, w1, w2)
        kt = T.operator_Kt(p1, p2, q11, q22, q12)
        lhs = np.sum(k[0] * p1 + k[1] * p2 + k[2] * q11 + k[3] * q22 + 2 * k[4] * q12)
        rhs = np.sum(kt[0] * u + kt[1] * w1 + kt[2] * w2)
        assert abs(lhs - rhs) <= 1e-12 * max(1.0, abs(lhs)), (shape, lhs, rhs)


def test_operator_norm_is_below_twelve():
    """Power iteration on K^T K in the Frobenius inner product (the q12 component counts twice), 64 x 64."""
    rng = np.random.default_rng(2)
    x = [rng.normal(size=(64, 64)) for _ in range(3)]
    lam = 0.0
    for _ in range(300):
        k = T.operator_K(*x)
        y = T.operator_Kt(*k)
        lam = np.sqrt(sum(np.sum(a * a) for a in y) / sum(np.sum(a * a) for a in x))
        nrm = np.sqrt(sum(np.sum(a * a) for a in y))
        x = [a / nrm for a in y]
    print(f"||K||^2 on 64 x 64: {lam:.3f}; 12 s^2 = {12 * float(T.STEP) ** 2:.7f}")
    assert 8.0 < lam < 12.0
    assert float(T.STEP) ** 2 * lam < 1.0


def test_a_ramp_survives_where_tv_flattens_it():
    ramp = T.facets((32, 48))
    tv = np.max(np.abs(O.tv_prox_fgp(ramp, 5.0, 200) - ramp))
    tgv = np.max(np.abs(T.tgv_prox(ramp, 5.0, 2.0, 200) - ramp))
    print(f"clean two-facet ramp, lam = 5, 200 iterations: TV moves it by {tv:.2f}, TGV by {tgv:.2f}")
    assert tgv < 0.25 * tv


def test_the_primal_energy_descends_to_that_of_a_long_run():
    shape, lam, alpha0 = (16, 24), 5.0, 2.0
    v = T.images(shape)[:1].astype(np.float64)
    u, w = T.tgv_prox(v, lam, alpha0, 20000, return_w=True)
    e_inf = float(T.primal_energy(u, w, v, lam, alpha0)[0])
    gaps = []
    for K in (10, 40, 160, 640, 2560):
        u, w = T.tgv_prox(v, lam, alpha0, K, return_w=True)
        gaps.append(float(T.primal_energy(u, w, v, lam, alpha0)[0]) - e_inf)
    print("primal energy above the 20000-iteration run at 10, 40, 160, 640, 2560 iterations:", " ".join(f"{g:.3e}" for g in gaps), f"(of {e_inf:.3e})")
    assert all(g > -1e-9 * e_inf for g in gaps), "the long run has the lowest energy"
    assert all(a > b for a, b in zip(gaps, gaps[1:])), "the energy decreases with the count"
    assert gaps[-1] < 1e-3 * gaps[0]


def test_the_box_form_is_not_clip_afterwards():
    shape, lam, alpha0, K, box = (16, 24), 2.5, 2.0, 40, (80.0, 200.0)
    v = T.images(shape).astype(np.float64)
    inside = T.tgv_prox(v, lam, alpha0, K, bounds=box)
    after = np.clip(T.tgv_prox(v, lam, alpha0, K), *box)
    d = float(np.max(np.abs(inside - after)))
    print(f"box inside the loop vs clip afterwards: {d:.2f} grey levels")
    assert inside.min() >= box[0] and inside.max() <= box[1]
    assert d > 0.5


def test_the_two_forms_agree_within_float32_rounding_and_float64_exactly():
    for shape in SMALL:
        x = T.images(shape)
        a = T.tgv_prox(x.astype(np.float64), 2.5, 0.5, 19)
        b = T.tgv_prox(x.astype(np.float64), 2.5, 0.5, 19, form="kernel")
        assert np.max(np.abs(a - b)) < 1e-10
        (u64, e32, bound), (w64, ew, bw) = T.prox_reference(shape, 2.5, 0.5, 19)
        assert 0 < e32 < 5e-4 and bound >= 3 * e32 and 0 < ew and bw >= 3 * ew


@pytest.mark.parametrize("planted", T.PLANTED)
def test_planted_faults_exceed_the_bound(planted):
    """Each fault, in the kernel's float32 arithmetic, is outside the bound on at least one case of the list (and e12_once on none with alpha0 = 2,
    K = 8: the condition the case list answers)."""
    box = (80.0, 200.0) if planted == "clip_after" else None
    worst, quiet = 0.0, []
    for shape in SMALL:
        x = T.images(shape)
        for alpha0 in T.ALPHAS:
            for lam in T.PROX_PARAMS:
                for K in (8, 19):
                    (u64, e32, bound), _ = T.prox_reference(shape, lam, alpha0, K, box)
                    good = T.tgv_prox(x, lam, alpha0, K, bounds=box, form="kernel")
                    assert np.max(np.abs(good - u64)) <= bound, "the faultless replay is inside its own bound"
                    r = float(np.max(np.abs(T.tgv_prox(x, lam, alpha0, K, bounds=box, form="kernel", planted=planted) - u64))) / bound
                    worst = max(worst, r)
                    if r <= 1.0:
                        quiet.append((shape, alpha0, lam, K))
    print(f"{planted}: worst err / bound {worst:.1f}; inside the bound on {len(quiet)} cases")
    assert worst > 1.0
    if planted == "e12_once":
        assert quiet and all(a == 2.0 for _, a, _, _ in quiet), quiet
        assert not [c for c in quiet if c[1] in (0.1, 0.5)]
    else:
        assert not quiet, quiet

"""Per-pixel parity of SK-ROCK against the float64 checker: max |got - ref64| over EVERY chain and pixel within max(3 e32, 2 ulp32(max |ref64|)) (plus
q 2e-5 for the device's Philox deviates), e32 the larger float32 rounding of two replays of the reference -- the definition in float32 and the launch form
`skrock_step` runs (tests/_skrock_pixel.py: the cases, the replays, the modes; tests/test_skrock_pixel_reference.py shows on the CPU which planted faults
of the stage coefficients, the perturbation and the buffer rotation the bound rejects and the rel-L2 criteria of tests/test_gpu_skrock.py accept).

Part A: every restart case of tests/_pixel.py without a box at s = 5, each with its variant and exact kernel name; the box refused before a handle
exists.  B: one case per family at s = 2, 3, 4 (the residues of the three-array rotation), 10 and 15.  C: no noise.  D: Philox noise on the shapes that
pick each form of the perturbation kernel and its edges; the stage launches of a Philox handle must be the single-iteration kernels.  E: six `step(1)`
calls with moments, the state held to a pixel after each, `set_state(get_state())` a no-op on the rotated arrays, the moment sums the float64 sums of
the states read back, `step(6)` the same bits.  F: more than 8192 x 256 units in each of the four perturbation kernels, by the closed form of a linear
drift.

Measured on an MI355X (229 tests pass; the whole file takes 8 s): 470 verdicts in parts A to E, the largest err / e32 1.30 (block kernel, (8, 8) l2 mask,
interior; the bound is at 3), 0.99 next; by stage count 0.81 / 0.99 / 0.77 / 1.30 / 0.82 / 0.98 at s = 2 / 3 / 4 / 5 / 10 / 15; part F 0.74 to 0.78 with
the second stride at 0.46 to 0.72; the moment sums equal the float64 sums of the states exactly.  No edge, seam, tail row or stride stands apart from the
interior.  DESIGN section 4.1 has the table per part and family."""
import numpy as np
import pytest

import _skrock_pixel as S
from test_gpu_pixel_parity import device_terms, f64

pytestmark = pytest.mark.gpu
LMC_E_UNSUPPORTED = -2
PAIR_POLICY = {"iterations_per_launch": 2}      # what makes a Philox MYULA handle on these shapes run two iterations per launch (tests/_pixel.py)


@pytest.fixture(scope="module")
def la():
    import torch
    assert torch.cuda.is_available()
    import lmc_atomi_amd as la
    return la


def make_sampler(la, sc, **kw):
    c, m = sc.base, S.problem(sc.base)
    pf, pg = device_terms(la, c)
    if sc.noise == "philox":
        kw.update(seed=S.SEED, chain_offset=S.CHAIN_OFFSET)
        if c.tag.endswith("2it") or c.family == "block":
            kw.setdefault("policy", PAIR_POLICY)
    else:
        kw.update(noise=sc.noise)
    return la.SKROCKSampler(pf, pg, c.shape, n_stages=sc.s, eta=S.ETA, n_chains=S.N_CHAINS, tau=S.delta_of(sc), gamma=m.gamma, variant=c.variant, **kw)


_RUNS = {}


def run(la, sc):
    """The device run of case `sc`, once per process: {"states": {iteration: state}, "kernel": its name} or {"refused": status}."""
    key = S.case_id(sc)
    if key in _RUNS:
        return _RUNS[key]
    m, stages = S.problem(sc.base), S.reference(sc)
    states, names = {}, set()
    try:
        if sc.mode == "restart":
            with make_sampler(la, sc) as smp:
                for it, st in enumerate(stages):
                    smp.set_state(f64(st.start))
                    smp.step(1, noise=f64(m.noise[it:it + 1]))
                    states[it] = smp.get_state().cpu().numpy()
                    assert smp.iteration == it + 1
                names.add(smp.kernel_name)
        else:       # carried: step(n) in one call compared after the last iteration, a second handle compared after the first
            for n in (sc.iters, 1):
                with make_sampler(la, sc) as smp:
                    smp.set_state(f64(m.x0))
                    smp.step(n)
                    states[n - 1] = smp.get_state().cpu().numpy()
                    assert smp.iteration == n
                    names.add(smp.kernel_name)
        out = {"states": states, "kernel": names}
    except la.LMCError as err:
        out = {"refused": err.code, "message": str(err)}
    except NotImplementedError as err:
        out = {"refused": LMC_E_UNSUPPORTED, "message": str(err)}
    _RUNS[key] = out
    return out


def _fail_on(verdicts):
    bad = [v.message for v in verdicts if not v.ok]
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("sc", S.CASES, ids=S.IDS)
def test_every_pixel_within_the_reference_bound(la, sc):
    out = run(la, sc)
    if sc.base.kernel is None:
        assert out.get("refused") == LMC_E_UNSUPPORTED, out
        return
    assert "refused" not in out, out
    assert out["kernel"] == {sc.base.kernel}, (out["kernel"], sc.base.kernel)
    stages = S.reference(sc)
    assert sorted(out["states"]) == ([0, 1] if sc.iters == 2 else sorted({0, sc.iters - 1}))
    verdicts = []
    for it, got in sorted(out["states"].items()):
        v = S.check(S.label(sc), it, got, stages[it])
        if sc.noise == "philox":
            print(f"    bound {stages[it].bound:.3e} = rounding {stages[it].rounding:.3e} + philox {stages[it].philox:.3e}")
        verdicts.append(v)
    _fail_on(verdicts)


@pytest.mark.parametrize("c", S.BOX_CASES, ids=[S.X.case_id(c) for c in S.BOX_CASES])
def test_a_box_is_refused_before_a_handle_exists(la, c, monkeypatch):
    created = []
    real = la.SKROCKSampler._create
    monkeypatch.setattr(la.SKROCKSampler, "_create", lambda self, cfg: created.append(1) or real(self, cfg))
    pf, pg = device_terms(la, c)
    m = S.problem(c)
    with pytest.raises(NotImplementedError, match="bounds"):
        la.SKROCKSampler(pf, pg, c.shape, n_stages=5, eta=S.ETA, n_chains=S.N_CHAINS, tau=m.tau, gamma=m.gamma, variant=c.variant, noise="injected")
    assert not created


# ------------------------------------------------------------------ E: rotation and reductions
@pytest.mark.parametrize("sc", S.E_CASES, ids=S.E_IDS)
def test_rotation_state_round_trip_and_moment_sums(la, sc):
    m, stages = S.problem(sc.base), S.reference(sc)
    H, W = sc.base.shape
    kw = dict(moments=True, burn_in=S.E_BURN_IN, thin=S.E_THIN)
    s1, s2, kept, verdicts = np.zeros((H, W)), np.zeros((H, W)), 0, []
    with make_sampler(la, sc, **kw) as one:
        one.set_state(f64(m.x0))
        for k in range(S.E_ITERS):
            one.step(1)
            got = one.get_state().cpu().numpy()
            verdicts.append(S.check(S.label(sc), k, got, stages[k]))
            one.set_state(got)                      # writes the array the rotation left the state in: a no-op
            again = one.get_state().cpu().numpy()
            assert got.tobytes() == again.tobytes(), k
            if k >= S.E_BURN_IN and (k - S.E_BURN_IN) % S.E_THIN == 0:
                x = got.astype(np.float64)
                s1 += x.sum(axis=0)
                s2 += (x * x).sum(axis=0)
                kept += 1
        assert one.kernel_name == sc.base.kernel and one.iteration == S.E_ITERS
        d1, d2, cnt = one.moments()
        d1, d2 = d1.cpu().numpy(), d2.cpu().numpy()
    assert kept == 3 and cnt == S.N_CHAINS * kept
    # the accumulators are float64 sums of float32 numbers and of their (exact) squares: their definition, at every pixel
    r1, r2 = np.abs(d1 - s1) / np.abs(s1), np.abs(d2 - s2) / s2
    print(f"moments {S.case_id(sc)}: max relative difference {r1.max():.2e} (sum), {r2.max():.2e} (sum of squares)")
    assert r1.max() <= 1e-12 and r2.max() <= 1e-12, (r1.max(), r2.max())
    with make_sampler(la, sc, **kw) as whole:
        whole.set_state(f64(m.x0))
        whole.step(S.E_ITERS)
        assert whole.get_state().cpu().numpy().tobytes() == got.tobytes()
        w1, w2, wcnt = whole.moments()
        assert wcnt == cnt
        assert np.abs(w1.cpu().numpy() - s1).max() <= 1e-12 * np.abs(s1).max() and np.abs(w2.cpu().numpy() - s2).max() <= 1e-12 * s2.max()
    _fail_on(verdicts)


# ------------------------------------------------------------------ F: the strided part of the perturbation grid
@pytest.mark.parametrize("fc", S.F_CASES, ids=S.F_IDS)
def test_perturbation_grid_past_its_cap(la, fc):
    import torch
    assert S.f_form_expected(fc) == fc.form and S.f_units(fc) > S.PERTURB_STRIDE and S.f_units(fc) % 256
    m = S.f_problem(fc)
    st = S.f_reference(fc, m)
    pf = la.L2(Op=None, b=np.zeros(fc.shape), sigma=S.F_ELL, dims=fc.shape)
    kw = dict(seed=S.SEED, chain_offset=S.CHAIN_OFFSET) if fc.noise == "philox" else dict(noise="injected")
    smp = la.SKROCKSampler(pf, la.L2(sigma=S.F_SP), fc.shape, n_stages=S.F_S, eta=S.ETA, n_chains=fc.chains, tau=S.f_delta(), gamma=S.F_GAMMA,
                           variant="point", **kw)
    try:
        smp.set_state(m.x0)
        if fc.noise == "philox":
            smp.step(1)
        else:
            smp.step(1, noise=m.Z[None])
        got = smp.get_state().cpu().numpy()
        assert smp.kernel_name == S.F_KERNEL, smp.kernel_name
    finally:
        smp.close()         # the handle's arrays are free before the next case opens
        torch.cuda.empty_cache()
    _fail_on([S.f_check(fc, got, st)])

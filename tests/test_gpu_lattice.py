"""Every data kind crossed with every prior, the box, array-valued epsg and two samplers (MYULA, SK-ROCK with three stages) against float64: the cells,
the table of what each must do and the reference are tests/_lattice.py's (held to themselves on the CPU by tests/test_lattice_reference.py).  The samplers
are created through the C ABI itself (lmc_myula_create / lmc_skrock_create on an lmc_problem), so the refusals seen are the library's and not the Python
surface's.  Per (shape, data kind): two chains, two iterations with injected noise, each restarted from the rounded float64 state (the "restart" mode of
tests/_pixel.py), `step_variant` 0.  A cell's creation does what the table says; a handle that was created steps; every pixel of every chain is inside
max(3 e32, 2 ulp32); the energies at the final state match float64 to 5e-5.  Failures are collected and reported together, each with its kernel name.
Once per (shape, data kind): the Philox iteration is the injected one on the sampler's own field, and lmc_fused_eval follows a change of the operator
(PSF taps, Radon angles, sampling mask of the same size: the cached tables of the shared scratch) from call to call."""
import ctypes as C

import numpy as np
import pytest

import _lattice as T
from oracle import lmc_oracle as O

pytestmark = pytest.mark.gpu

PAIRS = [(s, k) for s in T.SHAPES for k in T.KINDS]
PAIR_IDS = [f"{s[0]}x{s[1]}-{T.KIND_NAMES[k]}" for s, k in PAIRS]
LMC_E_HIP = -3
WORST = {}          # (axis, name) -> (err / bound, cell, sampler, kernel): filled by the cell tests, printed by the last test


@pytest.fixture(scope="module")
def la():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import lmc_atomi_amd as la
    return la


# ------------------------------------------------------------------ a cell as an lmc_problem
def data_descriptor(m):
    from lmc_atomi_amd.operators import spectral_tables
    opk = T.OPERATOR[m.kind]
    d = {"data_kind": m.kind, "sigma_f": m.sigma_f}
    if opk == "none":
        return d
    if opk == "spectral":
        d["y"] = spectral_tables(m.G, m.b)
        return d
    d["y"] = m.y if m.aux is None else np.stack([m.y, m.aux])
    if opk in ("blur", "psf"):
        d["h"], d["offset"] = m.h, m.offset
    if opk == "mask":
        d["mask"] = m.mask
    if opk == "radon":
        d["angles"], d["n_det"] = m.angles, m.n_det
    return d


def prior_descriptor(c):
    w = T.weight(c)
    tv = lambda kind, K: {"prior_kind": kind, "prior_sigma": w, "tv_niter": K, "tv_step": 0.125, "tv_betas": O.fgp_betas(K, "unlocbox")}       # noqa: E731
    d = {"none": {"prior_kind": 0}, "l2": {"prior_kind": 1, "prior_sigma": w}, "l1": {"prior_kind": 2, "prior_sigma": w},
         "laplace": {"prior_kind": 6, "eprox_kind": 0, "eprox_p0": w, "eprox_p1": 0.0, "eprox_scale_mask": 1},
         "tv10": tv(3, 10), "tv20": tv(3, 20), "aniso10": tv(4, 10), "haar": {"prior_kind": 5, "prior_sigma": w},
         "db2": {"prior_kind": 7, "prior_sigma": w, "wavelet_p": T.DB2[0], "wavelet_levels": T.DB2[1]},
         "vtv": tv(3, 10)}[c.prior]      # (LMC_PRIOR_VTV: the kind is set on the struct below; the Python surface refuses the descriptor itself)
    if c.box:
        d["box"] = c.box
    return d


def problem_of(c, alt=0):
    from lmc_atomi_amd import _dev
    from lmc_atomi_amd.proximal import _Problem
    opts = {}
    if c.epsg == "array":
        opts["prox_scale"] = (_dev.to_dev(T.epsg_array(c.shape).ravel()), 0, 1)
    prob = _Problem(c.shape, data_descriptor(T.problem(c.shape, c.kind, alt)), prior_descriptor(c), options=opts)
    if c.prior == "vtv":
        prob.c.prior_kind = 8
    return prob


def last_error():
    from lmc_atomi_amd import _dev
    return (_dev.lib().lmc_last_error() or b"").decode()


class Handle:
    """A sampler of a cell through the C ABI: `rc` and `msg` of its creation, then set_state / step / get_state / energies / noise on the handle."""

    def __init__(self, c, sampler, noise="injected", seed=0, chain_offset=0):
        from lmc_atomi_amd import _capi, _dev
        self.lib, self.dev, self.c = _dev.lib(), _dev, c
        m = T.problem(c.shape, c.kind)
        self.prob = problem_of(c)
        cfg = _capi.lmc_myula_config()
        cfg.struct_size = C.sizeof(_capi.lmc_myula_config)
        cfg.problem = self.prob.c
        cfg.n_chains, cfg.chain_offset = T.N_CHAINS, chain_offset
        cfg.tau, cfg.gamma, cfg.epsg = (m.tau if sampler == "myula" else m.delta), m.gamma, 1.0
        cfg.seed = seed
        cfg.noise_mode = _capi.NOISE_INJECTED if noise == "injected" else _capi.NOISE_PHILOX
        cfg.thin = 1
        self.h = C.c_void_p()
        if sampler == "myula":
            self.rc = self.lib.lmc_myula_create(C.byref(cfg), C.byref(self.h))
        else:
            self.rc = self.lib.lmc_skrock_create(C.byref(cfg), T.SK_STAGES, T.SK_ETA, C.byref(self.h))
        self.msg = last_error() if self.rc else ""
        self.shape = (T.N_CHAINS,) + c.shape

    def _call(self, fn, *args):
        rc = getattr(self.lib, fn)(self.h, *args, self.dev.stream_ptr())
        msg = last_error() if rc else ""
        if rc == LMC_E_HIP:
            pytest.exit(f"{T.cell_id(self.c)}: {fn} returned a HIP error ({msg}); nothing more is started on the GPU", returncode=3)
        return rc, msg

    def set_state(self, x):
        import torch
        t = self.dev.to_dev(x)
        rc, msg = self._call("lmc_sampler_set_state", self.dev.ptr(t))
        torch.cuda.current_stream().synchronize()
        assert rc == 0, msg

    def step(self, noise=None):
        import torch
        t = None if noise is None else self.dev.to_dev(noise)
        out = self._call("lmc_sampler_step", 1, self.dev.ptr(t))
        torch.cuda.current_stream().synchronize()
        return out

    def get_state(self):
        import torch
        out = torch.empty(self.shape, dtype=torch.float32, device="cuda")
        rc, msg = self._call("lmc_sampler_get_state", self.dev.ptr(out))
        assert rc == 0, msg
        return out.cpu().numpy()

    def energies(self):
        import torch
        f = torch.empty(T.N_CHAINS, dtype=torch.float64, device="cuda")
        g = torch.empty_like(f)
        rc, msg = self._call("lmc_sampler_energies", self.dev.ptr(f), self.dev.ptr(g))
        return rc, msg, f.cpu().numpy(), g.cpu().numpy()

    def noise_field(self, it):
        import torch
        out = torch.empty(self.shape, dtype=torch.float32, device="cuda")
        rc, msg = self._call("lmc_sampler_noise", it, self.dev.ptr(out))
        assert rc == 0, msg
        return out.cpu().numpy()

    @property
    def kernel_name(self):
        return self.lib.lmc_sampler_kernel_name(self.h).decode() if self.h.value else "(no handle)"

    def close(self):
        if self.h.value:
            self.lib.lmc_sampler_destroy(self.h)
            self.h = C.c_void_p()


def record(c, sampler, kernel, ratio):
    for key in (("kind", T.KIND_NAMES[c.kind]), ("prior", c.prior + ("+box" if c.box else "") + ("+epsg[]" if c.epsg == "array" else ""))):
        if ratio > WORST.get(key, (-1.0,))[0]:
            WORST[key] = (ratio, T.cell_id(c), sampler, kernel)


def close_to(got, want):
    return np.all(np.abs(got - want) <= T.ENERGY_RTOL * np.abs(want))


def run_cell(c, sampler, bad):
    who = f"{T.cell_id(c)} [{sampler}]"
    exp = T.expected(c, sampler)
    h = Handle(c, sampler)
    try:
        if exp != "runs":
            status, phrases = exp
            if h.rc == 0:
                bad.append(f"{who}: created, the table says {status} ({' / '.join(phrases)})")
            elif h.rc != status or not any(p.lower() in h.msg.lower() for p in phrases):
                bad.append(f"{who}: creation gave {h.rc} '{h.msg}', the table says {status} naming {' / '.join(phrases)}")
            return
        if h.rc != 0:
            bad.append(f"{who}: creation failed with {h.rc} '{h.msg}', the table says it runs")
            return
        m = T.problem(c.shape, c.kind)
        noise = m.noise if sampler == "myula" else m.Z
        got = None
        for it, st in enumerate(T.reference(c, sampler)):
            h.set_state(st.start)
            rc, msg = h.step(noise[it:it + 1])
            if rc != 0:      # a handle that was created must step: LMC_E_UNSUPPORTED from step under the auto variant is a failure
                bad.append(f"{who} it {it}: step failed with {rc} '{msg}' ({h.kernel_name})")
                return
            got = h.get_state()
            v = T.check(f"{who} it {it} ({h.kernel_name})", got, st)
            print(v.message)
            record(c, sampler, h.kernel_name, v.ratio)
            if not v.ok:
                bad.append(v.message)
        has_f, has_g = T.energies_exist(c)
        rc, msg, f, g = h.energies()
        if rc != 0:
            bad.append(f"{who}: lmc_sampler_energies failed with {rc} '{msg}' ({h.kernel_name})")
            return
        want_f, want_g = T.f_value(m, got), T.g_value(c, got)
        if has_f and not close_to(f, want_f):
            bad.append(f"{who}: f {f} against float64 {want_f} ({h.kernel_name})")
        if has_g and not close_to(g, want_g):
            bad.append(f"{who}: g {g} against float64 {want_g} ({h.kernel_name})")
    finally:
        h.close()


def run_cells(shape, kind):
    bad = []
    for c in T.cells(shape):
        if c.kind == kind:
            for sampler in T.SAMPLERS:
                run_cell(c, sampler, bad)
    return bad


@pytest.mark.parametrize("shape,kind", PAIRS, ids=PAIR_IDS)
def test_every_cell_does_what_the_table_says(la, shape, kind):
    bad = run_cells(shape, kind)
    assert not bad, f"{len(bad)} failures\n" + "\n".join(bad)


PHILOX_PRIORS = [("none", None), ("l1", T.BOX), ("tv10", None), ("db2", None)]       # one prior of each route: in the kernel, the elementwise launch, TV, the transforms


@pytest.mark.parametrize("shape,kind", PAIRS, ids=PAIR_IDS)
def test_philox_iteration_is_the_injected_one_on_the_samplers_field(la, shape, kind):
    bad = []
    for prior, box in PHILOX_PRIORS:
        c = T.Cell(shape, kind, prior, box, "scalar")
        if T.left_out(c) is not None:
            continue
        m = T.problem(shape, kind)
        a, b = Handle(c, "myula", noise="philox", seed=7, chain_offset=3), Handle(c, "myula")
        try:
            assert a.rc == 0 and b.rc == 0, (T.cell_id(c), a.msg, b.msg)
            a.set_state(m.x0)
            field = a.noise_field(0)
            rc_a, msg_a = a.step()
            b.set_state(m.x0)
            rc_b, msg_b = b.step(field[None])
            assert rc_a == 0 and rc_b == 0, (T.cell_id(c), msg_a, msg_b)
            ga, gb = a.get_state(), b.get_state()
            # the same arithmetic on the same field: equal up to the rounding of one fma (two ulps of the largest state) and the 2e-5 per deviate that lmc_device.h
            # states for the device's transcendentals, times sqrt(2 tau)
            d, lim = np.max(np.abs(ga - gb)), 2e-5 * np.sqrt(2 * m.tau) + 2 * np.spacing(np.float32(np.abs(ga).max()))
            if not (abs(field.std() - 1.0) < 0.1 and d <= lim and not np.array_equal(ga, m.x0)):
                bad.append(f"{T.cell_id(c)}: Philox against injected {d:.3e} (limit {lim:.3e}), field std {field.std():.3f} ({a.kernel_name} / {b.kernel_name})")
        finally:
            a.close()
            b.close()
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("shape,kind", PAIRS, ids=PAIR_IDS)
def test_stateless_update_follows_the_operator(la, shape, kind):
    """lmc_fused_eval, the noise-free update, over the running cells with one number for epsg: each on operator instance A, then on B where the kind has
    tables the shared scratch caches (bind_psf, bind_radon, bind_fft) -- consecutive calls change the operator, and a stale table gives a plausible image."""
    alts = (0, 1) if T.OPERATOR[kind] in ("psf", "radon", "spectral") else (0,)
    bad = []
    for c in T.cells(shape):
        if c.kind != kind or c.epsg != "scalar" or not T.runs(c, "myula"):
            continue
        for alt in alts:
            m = T.problem(shape, kind, alt)
            who = f"{T.cell_id(c)} lmc_fused_eval, operator {'AB'[alt]}"
            try:
                got = problem_of(c, alt).eval(m.x0, *T.coefficients(m))
            except (la.LMCError, NotImplementedError) as err:
                if getattr(err, "code", 0) == LMC_E_HIP:
                    pytest.exit(f"{who}: HIP error ({err}); nothing more is started on the GPU", returncode=3)
                bad.append(f"{who}: {err}")
                continue
            v = T.check(who, got, T.stateless_reference(c, alt))
            print(v.message)
            if not v.ok:
                bad.append(v.message)
    assert not bad, f"{len(bad)} failures\n" + "\n".join(bad)


def test_worst_ratio_per_data_kind_and_prior(la):
    """Prints the largest err / bound per data kind and per prior over the cells this session ran (all of (16, 64) when it ran none), with the kernel."""
    if not WORST:
        for kind in T.KINDS:
            bad = run_cells((16, 64), kind)
            assert not bad, "\n".join(bad)
    for axis in ("kind", "prior"):
        for (ax, name), (ratio, cell, sampler, kernel) in sorted(WORST.items()):
            if ax == axis:
                print(f"lattice worst by {axis} {name}: err / bound {ratio:.3f} at {cell} [{sampler}] ({kernel})")
    top = max(WORST.values())
    print(f"lattice worst overall: err / bound {top[0]:.3f} at {top[1]} [{top[2]}] ({top[3]})")
    assert top[0] <= 1.0

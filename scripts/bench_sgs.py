"""The split Gibbs sampler beside MYULA and SK-ROCK(10) on one problem, in one process: a 30 % k-space mask (`FourierSampling`), the TV prior at K = 10.

  - event-timed milliseconds per SGS iteration, per x-step alone (`lmc_sgs_xstep` with a noise field: rows forward twice, the column kernel, rows
    inverse) against its byte count at the copy rate `lmc_hbm_copy_probe` measures in this process, per MYULA iteration and per SK-ROCK(10) iteration;
  - from `chain_groups=32` the median per-pixel effective sample size of the mean (`mcse_from_group_moments`) per second of event time, for SGS at
    rho^2 = sigma^2 and 4 sigma^2 with tau = 0.8 sgs_step_bound, for MYULA at tau = 1 / (L_f + 1 / gamma) and for SK-ROCK(10) at 0.8 of its bound.
Nothing is asserted.  One JSON line per configuration, then one with all of them.

    python scripts/bench_sgs.py [--size 512x512x1024] [--steps 40] [--warmup 10]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIGMA, TAU_REG = 0.75, 0.3
GAMMA = SIGMA ** 2
GROUPS = 32


def timed(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="512x512x1024")
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    import torch
    import lmc_atomi_amd as la
    from lmc_atomi_amd import _dev
    ny, nx, C_ = (int(v) for v in a.size.split("x"))
    shape, wh = (ny, nx), nx // 2 + 1
    rng = np.random.default_rng(0)
    img = np.zeros(shape)
    img[ny // 5:ny // 2, nx // 4:nx // 2] = 190.0
    img += np.linspace(0, 30, nx)[None, :]
    x0 = torch.from_numpy(img.astype(np.float32)).cuda()[None].repeat(C_, 1, 1) + 5.0 * torch.randn((C_, ny, nx), device="cuda")
    results = []

    def emit(r):
        print(json.dumps(r), flush=True)
        results.append(r)

    gbs = C.c_float()
    lib = _dev.lib()
    rc = lib.lmc_hbm_copy_probe(C.c_size_t(1 << 30), 3, C.byref(gbs), _dev.stream_ptr())
    assert rc == 0, lib.lmc_last_error()
    emit({"config": "hbm-copy-probe", "gb_per_s": round(gbs.value, 1)})

    mask = (rng.uniform(size=shape) < 0.3).astype(np.float64)
    mask[:2, :2] = mask[:2, -2:] = mask[-2:, :2] = mask[-2:, -2:] = 1.0
    y_k = mask * np.fft.fft2(img, norm="ortho") + SIGMA * (rng.normal(size=shape) + 1j * rng.normal(size=shape))
    pf = la.L2(Op=la.FourierSampling(shape, mask), b=y_k, sigma=1 / SIGMA ** 2)
    pg = la.TV(shape, sigma=TAU_REG, niter=10)
    L = pf.grad_lipschitz() + 1 / GAMMA

    def run(label, smp, extra):
        """warm up, reset the accumulators, time `steps` iterations as one event-bracketed call, read the chain-group ESS"""
        with smp:
            smp.set_state(x0)
            smp.step(a.warmup)
            smp.reset_moments()
            ms = timed(torch, lambda: smp.step(a.steps))
            S1, S2, counts = smp.group_moments()
            ess = float(np.median(np.asarray(la.mcse_from_group_moments(S1, S2, counts).ess.cpu())))
            emit({"config": label, "size": a.size, "ms_per_iteration": round(ms / a.steps, 4), "median_pixel_ess": round(ess, 1),
                  "median_pixel_ess_per_s": round(ess / (ms * 1e-3), 1), "kept_samples": int(counts.sum()), "kernels": smp.kernel_name, **extra})

    for mult in (1.0, 4.0):
        rho = float(np.sqrt(mult)) * SIGMA
        tau = 0.8 * la.sgs_step_bound(rho, GAMMA)
        run(f"sgs-rho2={mult:g}sigma2", la.SplitGibbsSampler(pf, pg, shape, C_, rho, tau, GAMMA, seed=1, chain_groups=GROUPS), {"rho": rho, "tau": tau})
    run("myula", la.MYULASampler(pf, pg, shape, n_chains=C_, tau=1 / L, gamma=GAMMA, seed=1, moments=True, chain_groups=GROUPS,
                                 policy={"iterations_per_launch": 1}), {"tau": 1 / L})
    dk = 0.8 * la.skrock_step_bound(L, 10)
    run("skrock10", la.SKROCKSampler(pf, pg, shape, n_stages=10, n_chains=C_, tau=dk, gamma=GAMMA, seed=1, moments=True, chain_groups=GROUPS), {"tau": dk})

    # the x-step alone against its bytes: z and xi read (4 + 4), two row spectra written (8 + 8 per half-plane bin), both read and one written by the column
    # kernel (8 + 8 + 8), one read by the row inverse (8), x written (4)
    # (the entry point itself on a problem and an output made beforehand: nothing but its four launches is inside the event pair)
    from lmc_atomi_amd.proximal import _Problem
    z = x0
    xi = torch.randn_like(x0)
    out = torch.empty_like(x0)
    prob = _Problem(shape, pf.descriptor(), None)
    stream = _dev.stream_ptr()

    def xstep():
        rc = lib.lmc_sgs_xstep(C.byref(prob.c), _dev.ptr(z), _dev.ptr(xi), _dev.ptr(out), C_, SIGMA, stream)
        assert rc == 0, lib.lmc_last_error()

    xstep()
    torch.cuda.synchronize()
    ms = min(timed(torch, xstep) for _ in range(5))
    nbytes = C_ * ny * (3 * nx * 4 + 6 * wh * 8)
    floor = nbytes / (gbs.value * 1e9) * 1e3
    emit({"config": "sgs-xstep-alone", "size": a.size, "ms_best": round(ms, 4), "bytes": nbytes, "bytes_per_pixel": round(nbytes / (C_ * ny * nx), 2),
          "ms_at_copy_rate": round(floor, 4), "ratio_to_copy_rate": round(ms / floor, 2)})
    print(json.dumps({"bench": "sgs", "size": a.size, "steps": a.steps, "results": results}))


if __name__ == "__main__":
    main()

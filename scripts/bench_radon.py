"""The Radon operator in one process: event-timed forward projection alone, back-projection alone and whole MYULA iterations (all three launches;
lmc_sampler_last_step_timing: HIP events around each iteration's step launches, the moment reductions outside) with the TV prior at K = 10 and
bounds = (0, inf), for the Poisson and the plain Gaussian term, 180 angles over [0, pi).  Beside each time: the byte floor -- state read and write,
sinogram write and read -- at the copy rate lmc_hbm_copy_probe gives in this process, the weight evaluations per second, and the time of the data-free
step of the same prior (the middle launch).  One JSON line per configuration, then one with all of them.

    python scripts/bench_radon.py [--sizes 256x256x256,512x512x1024] [--angles 180] [--steps 5] [--warmup 2] [--repeats 3]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TAU_REG, GAMMA = 0.3, 0.5


def timed(torch, fn, repeats):
    fn()
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return float(np.min(out)), float(np.median(out))


def step_ms(torch, la, pf, shape, C_, x0, tau, steps, warmup, repeats):
    pg = la.TV(shape, sigma=TAU_REG, niter=10, bounds=(0.0, float("inf")))
    smp = la.MYULASampler(pf, pg, shape, n_chains=C_, tau=tau, gamma=GAMMA, seed=1, policy={"iterations_per_launch": 1})
    try:
        smp.set_state(x0)
        smp.step(warmup)
        smp.enable_timing(True)
        ms = []
        for _ in range(repeats):
            smp.step(steps)
            t, n = smp.last_step_timing()
            ms.append(t / steps)
        smp.enable_timing(False)
        torch.cuda.synchronize()
        return float(np.min(ms)), float(np.median(ms)), smp.kernel_name
    finally:
        smp.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256x256x256,512x512x1024")
    ap.add_argument("--angles", type=int, default=180)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    import torch
    import lmc_atomi_amd as la
    from lmc_atomi_amd import _dev
    gbs = C.c_float()
    la._capi.check(_dev.lib().lmc_hbm_copy_probe(1 << 30, 3, C.byref(gbs), _dev.stream_ptr()))
    copy_gbs = float(gbs.value)
    floor_ms = lambda nbytes: nbytes / (copy_gbs * 1e9) * 1e3
    results = []
    for size in a.sizes.split(","):
        ny, nx, C_ = (int(v) for v in size.split("x"))
        shape = (ny, nx)
        op = la.Radon(shape, np.linspace(0.0, np.pi, a.angles, endpoint=False))
        na, nd = op.sino_shape
        rng = np.random.default_rng(0)
        img = np.zeros(shape)
        img[ny // 5:ny // 2, nx // 4:nx // 2] = 4.0
        img += np.linspace(0, 1, nx)[None, :]
        x0 = (torch.from_numpy(img.astype(np.float32)).cuda()[None].repeat(C_, 1, 1) + 0.2 * torch.randn((C_, ny, nx), device="cuda")).contiguous()
        sino = np.asarray(op.matvec(img.astype(np.float32)), dtype=np.float64).reshape(op.sino_shape)
        r0 = torch.randn((C_, na * nd), device="cuda")
        state_b, sino_b = 4.0 * C_ * ny * nx, 4.0 * C_ * na * nd
        fwd_best, fwd_med = timed(torch, lambda: op.matvec(x0), a.repeats)
        adj_best, adj_med = timed(torch, lambda: op.rmatvec(r0), a.repeats)
        # what the kernels evaluate: forward, four candidates per (angle, line, bin) -- every bin of the 256-wide tiles; adjoint, two per (angle, pixel)
        n_row = int(np.sum(np.abs(np.cos(op.angles.astype(np.float64))) >= np.abs(np.sin(op.angles.astype(np.float64)))))
        bins = (nd + 255) // 256 * 256
        fwd_evals = 4.0 * C_ * bins * (n_row * ny + (na - n_row) * nx)
        adj_evals = 2.0 * C_ * na * ny * nx
        base = {"size": size, "angles": na, "n_det": nd, "hbm_copy_GBps": round(copy_gbs, 1)}
        r = dict(base, config="forward", ms_best=round(fwd_best, 4), ms_median=round(fwd_med, 4), byte_floor_ms=round(floor_ms(state_b + sino_b), 4),
                 weight_evals_per_s=float(f"{fwd_evals / (fwd_best * 1e-3):.4g}"))
        print(json.dumps(r), flush=True)
        results.append(r)
        r = dict(base, config="adjoint", ms_best=round(adj_best, 4), ms_median=round(adj_med, 4), byte_floor_ms=round(floor_ms(state_b + sino_b), 4),
                 weight_evals_per_s=float(f"{adj_evals / (adj_best * 1e-3):.4g}"))
        print(json.dumps(r), flush=True)
        results.append(r)
        free_best, free_med, free_kernel = step_ms(torch, la, None, shape, C_, x0, 1e-3, a.steps, a.warmup, a.repeats)
        for term in ("poisson", "gaussian"):
            if term == "poisson":
                pf = la.Poisson(op, rng.poisson(sino + 0.5), 0.5)
            else:
                pf = la.L2(Op=op, b=sino + rng.normal(0, 1.0, sino.shape), sigma=1.0)
            tau = 0.5 / (pf.grad_lipschitz() + 1.0 / GAMMA)
            best, med, kernel = step_ms(torch, la, pf, shape, C_, x0, tau, a.steps, a.warmup, a.repeats)
            # residual launch: state read, sinogram written; middle launch: state read and written; adjoint launch: sinogram read, state read and written
            nbytes = (state_b + sino_b) + 2 * state_b + (sino_b + 2 * state_b)
            r = dict(base, config=f"myula-{term}", ms_per_iteration_best=round(best, 4), ms_per_iteration_median=round(med, 4),
                     byte_floor_ms=round(floor_ms(nbytes), 4), weight_evals_per_s=float(f"{(fwd_evals + adj_evals) / (best * 1e-3):.4g}"),
                     data_free_step_ms_best=round(free_best, 4), data_free_step_ms_median=round(free_med, 4), middle_launch_kernel=kernel,
                     data_free_kernel=free_kernel)
            print(json.dumps(r), flush=True)
            results.append(r)
        del x0, r0
        torch.cuda.empty_cache()
    print(json.dumps({"bench": "radon", "steps": a.steps, "results": results}))


if __name__ == "__main__":
    main()

"""Large PSFs beside the fused kernels, in one process: event-timed MYULA iterations (lmc_sampler_last_step_timing: HIP events around each iteration's
step launches, the moment reductions outside) with the TV prior at K = 10.

  - `PSF` 15 x 15 and 31 x 31, a Gaussian (sigma = 2.5 / 5) in the separable two-pass form and the same taps in the general 2-D form;
  - what the three-launch decomposition costs against code that exists: `PSF` and `Convolve2D` on the same 7 x 7 separable box (the fused pipe kernel)
    and on the same 9 x 9 non-separable kernel (the fused tile kernel);
  - the operator alone (`PSF.matvec`), per call.
One JSON line per configuration, then one with all of them.

    python scripts/bench_psf.py [--size 512x512x1024] [--steps 10] [--warmup 3] [--repeats 3]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIGMA, TAU_REG = 0.75, 0.3
GAMMA, TAU = SIGMA ** 2, 0.2 * SIGMA ** 2


def gauss(k, s):
    t = np.exp(-0.5 * ((np.arange(k) - k // 2) / s) ** 2)
    return np.outer(t, t) / np.sum(np.outer(t, t))


def nonseparable(k):
    """A rotated anisotropic Gaussian: rank > 1."""
    i, j = np.meshgrid(np.arange(k) - k // 2, np.arange(k) - k // 2, indexing="ij")
    u, v = (i + j) / np.sqrt(2), (i - j) / np.sqrt(2)
    h = np.exp(-0.5 * ((u / (0.35 * k)) ** 2 + (v / (0.12 * k)) ** 2))
    return h / h.sum()


def step_ms(torch, la, pf, shape, C_, x0, steps, warmup, repeats):
    """(best and median event-timed ms per iteration, the kernel name of the prior launch)"""
    pg = la.TV(shape, sigma=TAU_REG, niter=10)
    smp = la.MYULASampler(pf, pg, shape, n_chains=C_, tau=TAU, gamma=GAMMA, seed=1, policy={"iterations_per_launch": 1})
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


def apply_ms(torch, op, x, repeats):
    out = []
    op.matvec(x)
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        op.matvec(x)
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return float(np.min(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="512x512x1024")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    import torch
    import lmc_atomi_amd as la
    ny, nx, C_ = (int(v) for v in a.size.split("x"))
    shape = (ny, nx)
    rng = np.random.default_rng(0)
    img = np.zeros(shape)
    img[ny // 5:ny // 2, nx // 4:nx // 2] = 190.0
    img += np.linspace(0, 30, nx)[None, :]
    y = img + rng.normal(0, SIGMA, shape)
    x0 = torch.from_numpy(img.astype(np.float32)).cuda()[None].repeat(C_, 1, 1) + 5.0 * torch.randn((C_, ny, nx), device="cuda")
    results = []

    def run(label, op, note):
        pf = la.L2(Op=op, b=y, sigma=1 / SIGMA ** 2)
        best, med, kernel = step_ms(torch, la, pf, shape, C_, x0, a.steps, a.warmup, a.repeats)
        r = {"config": label, "size": a.size, "taps": list(op.h.shape), "form": note, "ms_per_iteration_best": round(best, 4),
             "ms_per_iteration_median": round(med, 4), "prior_launch_kernel": kernel}
        if isinstance(op, la.PSF):
            r["matvec_ms"] = round(apply_ms(torch, op, x0, a.repeats), 4)
            r["gflop_per_iteration"] = round(2 * 2.0 * op.h.size * ny * nx * C_ / 1e9, 1) if op.factors is None else None
        print(json.dumps(r), flush=True)
        results.append(r)

    for k, s in ((15, 2.5), (31, 5.0)):
        h = gauss(k, s)
        run(f"psf{k}-gauss-separable", la.PSF(shape, h), "separable")
        run(f"psf{k}-gauss-general", la.PSF(shape, h, separable=False), "general")
    box7 = np.ones((7, 7)) / 49.0
    run("box7-psf-separable", la.PSF(shape, box7), "separable")
    run("box7-psf-general", la.PSF(shape, box7, separable=False), "general")
    run("box7-convolve2d", la.Convolve2D(shape, box7, offset=(3, 3)), "fused")
    ns9 = nonseparable(9)
    run("nonsep9-psf", la.PSF(shape, ns9), "general")
    run("nonsep9-convolve2d", la.Convolve2D(shape, ns9, offset=(4, 4)), "fused")
    print(json.dumps({"bench": "psf", "size": a.size, "steps": a.steps, "results": results}))


if __name__ == "__main__":
    main()

"""The Poisson data term beside the Gaussian one in one process: ms per step-kernel launch (HIP events around each launch,
lmc_sampler_enable_timing / lmc_sampler_last_step_timing) for 5 x 5 box blur + TV (K = 10) with bounds = (0, inf):

  (a) the Gaussian term, variant 'pipe' (myula_step_pipe_box_kernel): the yardstick -- its code is what it was before the Poisson term
  (b) the Poisson term, the full-width pipeline (variant 'pipe': myula_step_pipe_pois_box_kernel)
  (c) the Poisson term, the tiled kernel (variant 'tile': myula_step_tile_pois_box_kernel)
  and what 'auto' picks for the Poisson term.

The legs are interleaved `--repeats` times so that a drift of the clocks hits all of them.  One JSON line at the end.

    python scripts/bench_poisson.py [--size 512x512x1024] [--steps 30] [--warmup 5] [--repeats 5]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="512x512x1024", help="HxWxchains")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    import lmc_atomi_amd as la

    H, W, C = (int(v) for v in args.size.split("x"))
    rng = np.random.default_rng(0)
    img = np.zeros((H, W), dtype=np.float32)
    img[H // 5:H // 2, W // 6:2 * W // 3] = 20.0
    img += np.linspace(0, 5, W, dtype=np.float32)[None, :]
    h = np.ones((5, 5)) / 25.0
    Op = la.Convolve2D((H, W), h, offset=(2, 2))
    beta = 0.5
    hx = np.asarray(Op.matvec(img.ravel())).reshape(H, W).astype(np.float64)
    y = rng.poisson(hx + beta).astype(np.float64)
    pg = la.TV((H, W), sigma=5.0, niter=10, bounds=(0.0, float("inf")))
    pois = la.Poisson(Op, y, beta)
    gauss = la.L2(Op=Op, b=y, sigma=1.0)
    gamma = 0.02
    tau = 0.5 / (pois.grad_lipschitz() + 1.0 / gamma)
    legs = {"gaussian_pipe": (gauss, "pipe"), "poisson_pipe": (pois, "pipe"), "poisson_tile": (pois, "tile"), "poisson_auto": (pois, "auto")}
    smps, ms = {}, {k: [] for k in legs}
    for name, (pf, variant) in legs.items():
        smp = la.MYULASampler(pf, pg, (H, W), n_chains=C, tau=tau, gamma=gamma, seed=1, variant=variant, policy={"iterations_per_launch": 1})
        smp.set_state(np.maximum(y, 0.5))
        smp.step(args.warmup)
        smp.enable_timing(True)
        smps[name] = smp
    for _ in range(args.repeats):
        for name, smp in smps.items():
            smp.step(args.steps)
            t, n = smp.last_step_timing()
            assert n == args.steps, (name, n)
            ms[name].append(t / n)
    res = {"config": f"{args.size} blur5x5 + TV K=10 bounds=(0, inf)", "tau": tau, "gamma": gamma}
    for name, smp in smps.items():
        v = np.asarray(ms[name])
        finite = bool(np.isfinite(smp.get_state().cpu().numpy()).all())
        res[name] = {"kernel": smp.kernel_name, "launch_ms_median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "finite": finite}
        print(f"{name:14s} {smp.kernel_name:36s} {np.median(v):.4f} ms per launch ({v.min():.4f} .. {v.max():.4f}); state finite: {finite}", flush=True)
        smp.close()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()

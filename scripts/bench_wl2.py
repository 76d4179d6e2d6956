"""The weighted Gaussian data term (L2 with per-pixel weights, LMC_DATA_WL2_*) beside the unweighted one in one process: ms per step-kernel launch (HIP
events around each launch, lmc_sampler_enable_timing / lmc_sampler_last_step_timing) for 5 x 5 box blur + TV (K = 10) with bounds = (0, 255):

  (a) the unweighted term, variant 'pipe' (myula_step_pipe_box_kernel): the yardstick -- its code is what it was before the weighted term
  (b) the weighted term, the full-width pipeline (variant 'pipe': myula_step_pipe_wl2_box_kernel)
  (c) the weighted term, the tiled kernel (variant 'tile': myula_step_tile_wl2_box_kernel)
  (d) what 'auto' picks for the weighted term.

The legs are interleaved `--repeats` times so that a drift of the clocks hits all of them.  One JSON line at the end.

    python scripts/bench_wl2.py [--size 512x512x1024] [--steps 30] [--warmup 5] [--repeats 5]
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
    img[H // 5:H // 2, W // 6:2 * W // 3] = 150.0
    img += np.linspace(0, 30, W, dtype=np.float32)[None, :]
    h = np.ones((5, 5)) / 25.0
    Op = la.Convolve2D((H, W), h, offset=(2, 2))
    hx = np.asarray(Op.matvec(img.ravel())).reshape(H, W).astype(np.float64)
    y = hx + rng.normal(0, 5.0, (H, W))
    # a noise map, log-uniform on [0.25, 4], with 20 % of the pixels unobserved
    w = np.exp(rng.uniform(np.log(0.25), np.log(4.0), (H, W)))
    w[rng.uniform(size=(H, W)) < 0.2] = 0.0
    pg = la.TV((H, W), sigma=0.3, niter=10, bounds=(0.0, 255.0))
    weighted = la.L2(Op=Op, b=y, sigma=1.0 / 25.0, weights=w)
    plain = la.L2(Op=Op, b=y, sigma=1.0 / 25.0)
    gamma = 25.0
    tau = 0.5 / (weighted.grad_lipschitz() + 1.0 / gamma)
    legs = {"unweighted_pipe": (plain, "pipe"), "weighted_pipe": (weighted, "pipe"), "weighted_tile": (weighted, "tile"), "weighted_auto": (weighted, "auto")}
    smps, ms = {}, {k: [] for k in legs}
    for name, (pf, variant) in legs.items():
        smp = la.MYULASampler(pf, pg, (H, W), n_chains=C, tau=tau, gamma=gamma, seed=1, variant=variant, policy={"iterations_per_launch": 1})
        smp.set_state(np.clip(y, 0.0, 255.0))
        smp.step(args.warmup)
        smp.enable_timing(True)
        smps[name] = smp
    for _ in range(args.repeats):
        for name, smp in smps.items():
            smp.step(args.steps)
            t, n = smp.last_step_timing()
            assert n == args.steps, (name, n)
            ms[name].append(t / n)
    res = {"config": f"{args.size} blur5x5 + TV K=10 bounds=(0, 255)", "tau": tau, "gamma": gamma}
    for name, smp in smps.items():
        v = np.asarray(ms[name])
        finite = bool(np.isfinite(smp.get_state().cpu().numpy()).all())
        res[name] = {"kernel": smp.kernel_name, "launch_ms_median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "finite": finite}
        print(f"{name:16s} {smp.kernel_name:36s} {np.median(v):.4f} ms per launch ({v.min():.4f} .. {v.max():.4f}); state finite: {finite}", flush=True)
        smp.close()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()

"""The Huber data term (`la.HuberLoss`, LMC_DATA_HUBER_*) beside the plain and the weighted Gaussian terms in one process: ms per step-kernel launch (HIP
events around each launch, lmc_sampler_enable_timing / lmc_sampler_last_step_timing) for 5 x 5 box blur + TV (K = 10) with bounds = (0, 255):

  (a) the plain term, variant 'pipe' (myula_step_pipe_box_kernel): the yardstick -- its code is what it was before the Huber term
  (b) the weighted term, variant 'pipe' (myula_step_pipe_wl2_box_kernel): the sibling in the same kernel family, likewise unchanged
  (c) the Huber term, the full-width pipeline (variant 'pipe': myula_step_pipe_hub_box_kernel)
  (d) the Huber term, the tiled kernel (variant 'tile': myula_step_tile_hub_box_kernel)
  (e) what 'auto' picks for the Huber term.

Every leg is warmed up at the timed shape; the legs are interleaved `--repeats` times so that a drift of the clocks hits all of them, and the spread of
a leg over the repeats (min .. max of the per-launch means) is printed beside its median.  One JSON line at the end.

    python scripts/bench_huber.py [--size 512x512x1024] [--steps 30] [--warmup 5] [--repeats 5]
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
    # outliers of +-U(50, 150) on 10 % of the pixels; thresholds log-uniform on [3, 12], 10 % unobserved (0) and 10 % plain (+inf)
    hit = rng.uniform(size=(H, W)) < 0.1
    y = y + np.where(hit, rng.uniform(50.0, 150.0, (H, W)) * rng.choice([-1.0, 1.0], (H, W)), 0.0)
    delta = np.exp(rng.uniform(np.log(3.0), np.log(12.0), (H, W)))
    u = rng.uniform(size=(H, W))
    delta[u < 0.1] = 0.0
    delta[(u >= 0.1) & (u < 0.2)] = np.inf
    w = np.exp(rng.uniform(np.log(0.25), np.log(1.0), (H, W)))      # (max 1: the three terms share one step size)
    w[u < 0.2] = 0.0
    pg = la.TV((H, W), sigma=0.3, niter=10, bounds=(0.0, 255.0))
    huber = la.HuberLoss(Op, y, delta, sigma=1.0 / 25.0)
    weighted = la.L2(Op=Op, b=y, sigma=1.0 / 25.0, weights=w)
    plain = la.L2(Op=Op, b=y, sigma=1.0 / 25.0)
    gamma = 25.0
    tau = 0.5 / (huber.grad_lipschitz() + 1.0 / gamma)
    legs = {"plain_pipe": (plain, "pipe"), "weighted_pipe": (weighted, "pipe"), "huber_pipe": (huber, "pipe"), "huber_tile": (huber, "tile"),
            "huber_auto": (huber, "auto")}
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
    res = {"config": f"{args.size} blur5x5 + TV K=10 bounds=(0, 255)", "tau": tau, "gamma": gamma, "steps": args.steps, "repeats": args.repeats}
    for name, smp in smps.items():
        v = np.asarray(ms[name])
        finite = bool(np.isfinite(smp.get_state().cpu().numpy()).all())
        res[name] = {"kernel": smp.kernel_name, "launch_ms_median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "finite": finite}
        print(f"{name:16s} {smp.kernel_name:36s} {np.median(v):.4f} ms per launch ({v.min():.4f} .. {v.max():.4f}); state finite: {finite}", flush=True)
        smp.close()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()

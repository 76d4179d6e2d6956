"""What the multi-scale moments cost: ms per MYULA step without scales, with scales (2, 4, 8, 16) reduced on the side stream, and with them
reduced in line (moments_overlap = -1), in ONE process on the same problem -- the comparison is the row without scales of the same run.

Blur 5 x 5 + TV (K = 10), thin = 1, Philox noise.  Each figure: median (min - max) over --steps single step() calls of --chunk iterations, host clock
around a device synchronise, after --warmup iterations.  Then the event-timed duration of one in-line fused reduction beside one in-line
moments4_kernel launch on the same state: a sampler that keeps every iterate, step(1) with and without scales, minus the step kernel's own time.

    python scripts/bench_block_moments.py [--size 512x512x1024] [--steps 100] [--warmup 30] [--chunk 10]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="512x512x1024", help="HxWxchains")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--chunk", type=int, default=10, help="iterations per timed step() call (reductions overlap only inside a call)")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    import lmc_atomi_amd as la

    H, W, C = (int(v) for v in args.size.split("x"))
    sigma, tau_reg = 0.75, 0.3
    gamma, tau = sigma ** 2, 0.2 * sigma ** 2
    rng = np.random.default_rng(0)
    img = np.zeros((H, W), dtype=np.float32)
    img[H // 5:H // 2, W // 6:2 * W // 3] = 160.0
    img += np.linspace(0, 25, W, dtype=np.float32)[None, :]
    y = img + rng.normal(0, sigma, (H, W)).astype(np.float32)
    pf = la.L2(Op=la.Convolve2D((H, W), np.ones((5, 5)) / 25.0, offset=(2, 2)), b=y, sigma=1 / sigma ** 2)
    pg = la.TV((H, W), sigma=tau_reg, niter=10)
    scales = (2, 4, 8, 16)
    rows = [("no scales (overlapped)", None, None), ("scales 2..16, overlapped", scales, None), ("scales 2..16, in line", scales, {"moments_overlap": -1}),
            ("no scales, in line", None, {"moments_overlap": -1})]
    for label, sc, policy in rows:
        smp = la.MYULASampler(pf, pg, (H, W), n_chains=C, tau=tau, gamma=gamma, seed=1, moments=True, thin=1, moment_scales=sc, policy=policy)
        smp.set_state(img)
        smp.step(args.warmup)
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.steps):
            t0 = time.perf_counter()
            smp.step(args.chunk)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3 / args.chunk)
        ms = np.asarray(ms)
        print(f"{args.size:>16} {label:<26} median {np.median(ms):.4f} ms/step  ({ms.min():.4f} - {ms.max():.4f})  ({smp.kernel_name})", flush=True)
        smp.close()

    # one in-line reduction, event-timed: step(1) is the step kernel plus ONE in-line reduction; the step kernel's own time comes from the sampler's timing
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for label, sc in (("moments4_kernel", None), ("moments_ms_kernel (2..16)", scales)):
        smp = la.MYULASampler(pf, pg, (H, W), n_chains=C, tau=tau, gamma=gamma, seed=1, moments=True, thin=1, moment_scales=sc)
        smp.set_state(img)
        smp.step(args.warmup)
        smp.enable_timing(True)
        red = []
        for _ in range(args.steps):
            start.record()
            smp.step(1)
            stop.record()
            stop.synchronize()
            red.append(start.elapsed_time(stop) - smp.last_step_timing()[0])
        red = np.asarray(red)
        print(f"{args.size:>16} in-line reduction, {label:<26} median {np.median(red):.4f} ms  ({red.min():.4f} - {red.max():.4f})", flush=True)
        smp.close()


if __name__ == "__main__":
    main()

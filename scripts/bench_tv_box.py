"""Step-kernel time of the box-constrained TV prior, `TV(bounds=(lo, hi))`, beside its unconstrained isotropic twin of the same build, in one process.

Per size: the box kernel (library's choice), its two-team and one-team forms (variants 'pipe2' / 'pipe'), and the unconstrained kernels in the same
three forms.  Each figure is the median over --launches event-timed launches (lmc_sampler_enable_timing / lmc_sampler_last_step_timing: the step
kernel alone, moment reductions outside the brackets) after --warmup launches; min and max show the run-to-run spread.  5 x 5 box blur, K = 10 dual
iterations, Philox noise, bounds (0, 255).

    python scripts/bench_tv_box.py [--launches 100] [--warmup 30] [--sizes 512x512x1024,256x256x4096,667x877x512]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--sizes", default="512x512x1024,256x256x4096,667x877x512", help="HxWxchains, comma separated")
    ap.add_argument("--bounds", default="0,255", help="lo,hi")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    import lmc_atomi_amd as la

    bounds = tuple(float(v) for v in args.bounds.split(","))
    sigma, tau_reg = 0.75, 0.3
    gamma, tau = sigma ** 2, 0.2 * sigma ** 2
    for size in args.sizes.split(","):
        H, W, C = (int(v) for v in size.split("x"))
        rng = np.random.default_rng(0)
        img = np.zeros((H, W), dtype=np.float32)
        img[H // 5:H // 2, W // 6:2 * W // 3] = 160.0
        img += np.linspace(0, 25, W, dtype=np.float32)[None, :]
        h = np.ones((5, 5)) / 25.0
        y = img + rng.normal(0, sigma, (H, W)).astype(np.float32)
        pf = la.L2(Op=la.Convolve2D((H, W), h, offset=(2, 2)), b=y, sigma=1 / sigma ** 2)
        rows = [("box (library's choice)", bounds, None), ("box two-team (pipe2)", bounds, "pipe2"), ("box one-team (pipe)", bounds, "pipe"),
                ("free (library's choice)", None, None), ("free two-team (pipe2)", None, "pipe2"), ("free one-team (pipe)", None, "pipe")]
        for label, b, variant in rows:
            pg = la.TV((H, W), sigma=tau_reg, niter=10, bounds=b)
            smp = la.MYULASampler(pf, pg, (H, W), n_chains=C, tau=tau, gamma=gamma, seed=1, variant=variant)
            smp.set_state(img)
            try:
                smp.step(args.warmup)
            except la.LMCError as err:
                print(f"{size:>16} {label:<26} not covered ({err.code})", flush=True)
                smp.close()
                continue
            smp.enable_timing(True)
            ms = []
            for _ in range(args.launches):
                smp.step(1)
                t, n = smp.last_step_timing()
                ms.append(t / n)
            ms = np.asarray(ms)
            print(f"{size:>16} {label:<26} median {np.median(ms):.4f} ms  min {ms.min():.4f}  max {ms.max():.4f}  ({smp.kernel_name})", flush=True)
            smp.close()


if __name__ == "__main__":
    main()

"""What the covariance sketch costs.

1. Per kept iterate, in line: the event-timed duration of one lmc_cov_sketch call (projection, finish twice, update) on a state x[C][H][W] for k = 8 and
   32 probes, beside the floor -- the time to read the state twice at the copy peak lmc_hbm_copy_probe reports here.  The passes read x twice (8 C H W
   bytes) and compute 4 x 32 C H W FLOP whatever k is (k is padded to 32 probe rows).
2. Whole iterations: event-timed step(n) of a MYULA blur + TV sampler that keeps every iterate (thin = 1) or every tenth (thin = 10), with and without
   the sketch, the reductions beside the step kernels (moments_overlap = 1) and in line (-1): milliseconds per iteration and the difference the sketch
   makes.

    python scripts/bench_cov_sketch.py [--size 512x512x1024] [--steps 40] [--warmup 10] [--probes 8,32]

Reported, not gated.
"""
import argparse
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="512x512x1024", help="HxWxchains")
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--probes", default="8,32")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    import lmc_atomi_amd as la

    H, W, C = (int(v) for v in args.size.split("x"))
    ks = [int(v) for v in args.probes.split(",")]
    sigma = 0.75
    gamma, tau = sigma ** 2, 0.2 * sigma ** 2
    rng = np.random.default_rng(0)
    y = (100.0 + rng.normal(0, sigma, (H, W))).astype(np.float32)
    pf = la.L2(Op=la.Convolve2D((H, W), np.ones((5, 5)) / 25.0, offset=(2, 2)), b=y, sigma=1 / sigma ** 2)
    pg = la.TV((H, W), sigma=0.3, niter=10)

    g = ctypes.c_float()
    la._capi.check(la._dev.lib().lmc_hbm_copy_probe(1 << 30, 3, ctypes.byref(g), None))
    peak = float(g.value)
    floor_ms = 2 * 4.0 * H * W * C / (peak * 1e9) * 1e3
    print(f"{args.size:>16} copy peak {peak:.0f} GB/s: two reads of the state take {floor_ms:.4f} ms", flush=True)

    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    lib, st, p = la._dev.lib(), la._dev.stream_ptr(), la._dev.ptr
    x = torch.from_numpy(y).cuda().expand(C, H, W).contiguous()
    x += torch.randn_like(x)
    center = torch.from_numpy(y).cuda()
    for k in ks:
        P = torch.from_numpy(la.random_probes(k, (H, W), seed=1)).cuda()
        Y = torch.zeros((k, H, W), dtype=torch.float64, device=x.device)
        s, Q = torch.zeros(k, dtype=torch.float64, device=x.device), torch.zeros((k, k), dtype=torch.float64, device=x.device)
        ws = torch.empty(int(lib.lmc_cov_sketch_workspace_bytes(C, H, W, k)), dtype=torch.uint8, device=x.device)
        ms = []
        for i in range(args.steps + 3):
            start.record()
            la._capi.check(lib.lmc_cov_sketch(p(x), C, H, W, k, p(P), p(center), p(Y), p(s), p(Q), p(ws), st))
            stop.record()
            stop.synchronize()
            if i >= 3:
                ms.append(start.elapsed_time(stop))
        ms = np.asarray(ms)
        med = float(np.median(ms))
        print(f"{args.size:>16} cov sketch in line, k = {k:<2}      median {med:.4f} ms  ({ms.min():.4f} - {ms.max():.4f})"
              f"  = {med / floor_ms:.2f} x two reads of the state, {4.0 * 32 * C * H * W / med / 1e9:.1f} TFLOP/s of the padded product", flush=True)
        del P, Y, s, Q, ws
    del x

    def per_iteration(thin, overlap, k):
        kw = {}
        if k:
            kw = dict(cov_probes=la.random_probes(k, (H, W), seed=1), cov_center=y)
        smp = la.MYULASampler(pf, pg, (H, W), n_chains=C, tau=tau, gamma=gamma, seed=1, moments=True, thin=thin, policy={"moments_overlap": overlap}, **kw)
        try:
            smp.set_state(y)
            smp.step(args.warmup)
            torch.cuda.synchronize()
            start.record()
            smp.step(args.steps)
            stop.record()
            stop.synchronize()
            return start.elapsed_time(stop) / args.steps, smp.kernel_name
        finally:
            smp.close()

    for thin in (1, 10):
        for overlap, how in ((1, "beside the step kernels"), (-1, "in line")):
            base, name = per_iteration(thin, overlap, 0)
            line = f"{args.size:>16} {name} thin = {thin:<2} reductions {how:<23}: {base:.4f} ms / iteration without the sketch"
            for k in ks:
                with_k, _ = per_iteration(thin, overlap, k)
                line += f"; k = {k}: {with_k:.4f} (+{with_k - base:.4f}, +{(with_k - base) * thin:.4f} per kept iterate)"
            print(line, flush=True)


if __name__ == "__main__":
    main()

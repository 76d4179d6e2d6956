"""What the chain-group moments cost per kept iterate: the event-timed duration of one lmc_group_moments launch on a state x[C][H][W] for G = 8, 32 and 64,
beside one launch of the pixel-moment reduction (launch_moments) on the same state in the same process -- step(1) of a sampler that keeps every iterate,
event-timed, minus the step kernel's own time -- and beside the floor: the time to read the state once at the copy peak lmc_hbm_copy_probe reports here.
The pass moves 4 C H W bytes of reads plus 32 G H W bytes of accumulator traffic; the table gives both as a rate.

    python scripts/bench_group_moments.py [--size 512x512x1024] [--steps 100] [--warmup 10]
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
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--groups", default="8,32,64")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    import lmc_atomi_amd as la

    H, W, C = (int(v) for v in args.size.split("x"))
    sigma = 0.75
    gamma, tau = sigma ** 2, 0.2 * sigma ** 2
    rng = np.random.default_rng(0)
    y = (100.0 + rng.normal(0, sigma, (H, W))).astype(np.float32)
    pf = la.L2(Op=la.Convolve2D((H, W), np.ones((5, 5)) / 25.0, offset=(2, 2)), b=y, sigma=1 / sigma ** 2)
    pg = la.L2(sigma=0.05)

    g = ctypes.c_float()
    la._capi.check(la._dev.lib().lmc_hbm_copy_probe(1 << 30, 3, ctypes.byref(g), None))
    peak = float(g.value)
    read_bytes = 4.0 * H * W * C
    floor_ms = read_bytes / (peak * 1e9) * 1e3
    print(f"{args.size:>16} copy peak {peak:.0f} GB/s: one read of the state takes {floor_ms:.4f} ms", flush=True)

    # the pixel-moment reduction alone: an in-line step(1) that keeps its iterate, minus the event-timed step kernel
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    smp = la.MYULASampler(pf, pg, (H, W), n_chains=C, tau=tau, gamma=gamma, seed=1, moments=True, thin=1)
    smp.set_state(y)
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
    print(f"{args.size:>16} launch_moments alone          median {np.median(red):.4f} ms  ({red.min():.4f} - {red.max():.4f})"
          f"  = {np.median(red) / floor_ms:.2f} x one read of the state", flush=True)
    x = smp.get_state()
    smp.close()

    lib, st = la._dev.lib(), la._dev.stream_ptr()
    for G in (int(v) for v in args.groups.split(",")):
        S1 = torch.zeros((G, H, W), dtype=torch.float64, device=x.device)
        S2 = torch.zeros_like(S1)
        ms = []
        for k in range(args.steps + 3):
            start.record()
            la._capi.check(lib.lmc_group_moments(la._dev.ptr(x), C, 0, H, W, G, la._dev.ptr(S1), la._dev.ptr(S2), st))
            stop.record()
            stop.synchronize()
            if k >= 3:
                ms.append(start.elapsed_time(stop))
        ms = np.asarray(ms)
        moved = read_bytes + 32.0 * G * H * W
        med = float(np.median(ms))
        print(f"{args.size:>16} group moments, G = {G:<2}          median {med:.4f} ms  ({ms.min():.4f} - {ms.max():.4f})"
              f"  = {med / floor_ms:.2f} x one read of the state, {moved / med / 1e6:.0f} GB/s of {moved / 2 ** 20:.0f} MiB moved", flush=True)
        del S1, S2


if __name__ == "__main__":
    main()

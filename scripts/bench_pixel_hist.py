"""What the pixel histogram costs: ms per MYULA step without a histogram, with it on the side stream, and with it in line (moments_overlap = -1), in
ONE process on the same problem -- the comparison is the row without a histogram of the same run.

Blur 5 x 5 + TV (K = 10), thin = 1, Philox noise, 62 bins over mean -+ 5 std per pixel of a pilot run (the intended use).  Each figure: median
(min - max) over --steps single step() calls of --chunk iterations, host clock around a device synchronise, after --warmup iterations.  Then the
event-timed duration of one histogram launch (lmc_pixel_histogram on the sampler's state; the library's segment length, then fixed ones) beside one
in-line moments4_kernel launch on the same state (step(1) of a sampler that keeps every iterate, minus the step kernel's own time), and the floor: the time to read the state once at the copy peak
lmc_hbm_copy_probe reports in this process.

    python scripts/bench_pixel_hist.py [--size 512x512x1024] [--steps 100] [--warmup 30] [--chunk 10] [--bins 62] [--pilot 100]
"""
import argparse
import ctypes
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
    ap.add_argument("--bins", type=int, default=62)
    ap.add_argument("--pilot", type=int, default=100, help="kept iterations of the pilot run that sets the range (after as many of burn-in)")
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
    kw = dict(n_chains=C, tau=tau, gamma=gamma, seed=1, moments=True, thin=1)

    # pilot run: the range of every pixel is its mean -+ 5 std
    smp = la.MYULASampler(pf, pg, (H, W), burn_in=args.pilot, **kw)
    smp.set_state(img)
    smp.step(2 * args.pilot)
    s1, s2, n = smp.moments()
    smp.close()
    mean, var = la.mean_var_from_moments(s1, s2, n)
    std = var.clamp_min(1e-6).sqrt()
    hist = dict(hist_bins=args.bins, hist_range=(mean - 5 * std, mean + 5 * std))

    g = ctypes.c_float()
    la._capi.check(la._dev.lib().lmc_hbm_copy_probe(1 << 30, 3, ctypes.byref(g), None))
    floor_ms = 4.0 * H * W * C / (float(g.value) * 1e9) * 1e3
    print(f"{args.size:>16} copy peak {float(g.value):.0f} GB/s: one read of the state takes {floor_ms:.4f} ms", flush=True)

    rows = [("no histogram (overlapped)", {}, None), ("histogram, side stream", hist, None), ("histogram, in line", hist, {"moments_overlap": -1}),
            ("no histogram, in line", {}, {"moments_overlap": -1})]
    for label, hk, policy in rows:
        smp = la.MYULASampler(pf, pg, (H, W), policy=policy, **hk, **kw)
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
        if hk:
            counts, cnt = smp.histogram()
            filled = float((counts > 0).sum()) / (H * W)
            tails = float(counts[0].sum() + counts[-1].sum()) / max(float(counts.sum()), 1.0)
            print(f"{'':>16} {'':<26} {filled:.1f} non-empty rows per pixel, {tails:.2e} of the samples in the tail rows", flush=True)
            del counts
        smp.close()

    # one launch of each reduction on the same state, event-timed
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    smp = la.MYULASampler(pf, pg, (H, W), **kw)
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
    print(f"{args.size:>16} in-line reduction, {'moments4_kernel':<26} median {np.median(red):.4f} ms  ({red.min():.4f} - {red.max():.4f})", flush=True)
    x = smp.get_state()
    smp.close()
    B, lo32, sc32 = la.algs._hist_arrays(args.bins, *hist["hist_range"], (H, W))
    lo_d, sc_d = la._dev.to_dev(lo32), la._dev.to_dev(sc32)
    counts = torch.zeros((B + 2, H, W), dtype=torch.int64, device=x.device)
    lib, st = la._dev.lib(), la._dev.stream_ptr()
    # the library's own choice of the segment length first, then fixed lengths (LMC_HIST_SEG, read at every launch): a shorter segment means more
    # workgroups and more atomics (one per non-empty row, pixel and segment), a longer one fewer of both
    ref = None
    for seg in (None, 128, 256, 512, 1024, 2040):
        if seg is None:
            os.environ.pop("LMC_HIST_SEG", None)
        else:
            os.environ["LMC_HIST_SEG"] = str(seg)
        counts.zero_()
        la._capi.check(lib.lmc_pixel_histogram(la._dev.ptr(x), C, H, W, B, la._dev.ptr(lo_d), la._dev.ptr(sc_d), la._dev.ptr(counts), st))
        if ref is None:
            ref = counts.clone()
        assert torch.equal(counts, ref), "the counts depend on the segment length"
        red = []
        for k in range(args.steps + 3):
            start.record()
            la._capi.check(lib.lmc_pixel_histogram(la._dev.ptr(x), C, H, W, B, la._dev.ptr(lo_d), la._dev.ptr(sc_d), la._dev.ptr(counts), st))
            stop.record()
            stop.synchronize()
            if k >= 3:
                red.append(start.elapsed_time(stop))
        red = np.asarray(red)
        label = "library default" if seg is None else f"{-(-C // seg)} segment(s) of <= {seg}"
        print(f"{args.size:>16} one launch, pixel_hist_kernel, {label:<28} median {np.median(red):.4f} ms  ({red.min():.4f} - {red.max():.4f})"
              f"  = {np.median(red) / floor_ms:.2f} x one read of the state", flush=True)
    os.environ.pop("LMC_HIST_SEG", None)
    print(f"{'':>16} {float((ref > 0).sum()) / (H * W):.1f} non-empty rows per pixel in one iterate", flush=True)

if __name__ == "__main__":
    main()

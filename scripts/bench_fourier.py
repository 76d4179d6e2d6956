"""The Fourier-domain data term beside what exists, in one process: event-timed MYULA iterations (lmc_sampler_last_step_timing: HIP events around each
iteration's step launches, the moment reductions outside) with the TV prior at K = 10.

  - `FourierSampling` with a 30 % mask (a fully sampled centre plus random frequencies);
  - `PeriodicConvolve2D` with a 31 x 31 Gaussian (sigma = 5), and the zero-padded `PSF` of the same taps (the three-launch pixel-space step);
  - the three FFT launches alone (`L2.grad`: rows forward, columns with the functor, rows inverse in the overwrite form) against their byte count at the
    copy rate `lmc_hbm_copy_probe` measures in this process;
  - the same gradient composed from `torch.fft.rfft2` / `irfft2` (rocFFT) and two elementwise operations.
One JSON line per configuration, then one with all of them.

    python scripts/bench_fourier.py [--size 512x512x1024] [--steps 10] [--warmup 3] [--repeats 3]
"""
import argparse
import ctypes as C
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


def event_ms(torch, fn, repeats):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="512x512x1024")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    import torch
    import lmc_atomi_amd as la
    from lmc_atomi_amd import _dev
    ny, nx, C_ = (int(v) for v in a.size.split("x"))
    shape, wh = (ny, nx), nx // 2 + 1
    rng = np.random.default_rng(0)
    img = np.zeros(shape)
    img[ny // 5:ny // 2, nx // 4:nx // 2] = 190.0
    img += np.linspace(0, 30, nx)[None, :]
    x0 = torch.from_numpy(img.astype(np.float32)).cuda()[None].repeat(C_, 1, 1) + 5.0 * torch.randn((C_, ny, nx), device="cuda")
    results = []

    def emit(r):
        print(json.dumps(r), flush=True)
        results.append(r)

    def run(label, pf):
        best, med, kernel = step_ms(torch, la, pf, shape, C_, x0, a.steps, a.warmup, a.repeats)
        emit({"config": label, "size": a.size, "ms_per_iteration_best": round(best, 4), "ms_per_iteration_median": round(med, 4), "prior_launch_kernel": kernel})

    gbs = C.c_float()
    lib = _dev.lib()
    rc = lib.lmc_hbm_copy_probe(C.c_size_t(1 << 30), 3, C.byref(gbs), _dev.stream_ptr())
    assert rc == 0, lib.lmc_last_error()
    emit({"config": "hbm-copy-probe", "gb_per_s": round(gbs.value, 1)})

    mask = (rng.uniform(size=shape) < 0.3).astype(np.float64)
    mask[:2, :2] = mask[:2, -2:] = mask[-2:, :2] = mask[-2:, -2:] = 1.0
    y_k = mask * np.fft.fft2(img, norm="ortho") + SIGMA * (rng.normal(size=shape) + 1j * rng.normal(size=shape))
    pf_mask = la.L2(Op=la.FourierSampling(shape, mask), b=y_k, sigma=1 / SIGMA ** 2)
    run("fourier-mask30", pf_mask)

    h31 = gauss(31, 5.0)
    per = la.PeriodicConvolve2D(shape, h31)
    y_b = np.fft.ifft2(per.gain() * np.fft.fft2(img)).real + rng.normal(0, SIGMA, shape)
    run("periodic31-gauss", la.L2(Op=per, b=y_b, sigma=1 / SIGMA ** 2))
    run("psf31-gauss-separable", la.L2(Op=la.PSF(shape, h31), b=y_b, sigma=1 / SIGMA ** 2))

    # the three launches alone, against their byte count at the measured copy rate
    nbytes = C_ * ny * (nx * 4 + wh * 8 + 2 * wh * 8 + wh * 8 + nx * 4 + nx * 4)
    best, med = event_ms(torch, lambda: pf_mask.grad(x0), a.repeats)
    floor = nbytes / (gbs.value * 1e9) * 1e3
    emit({"config": "fft-gradient-three-launches", "size": a.size, "ms_best": round(best, 4), "ms_median": round(med, 4), "bytes": nbytes,
          "bytes_per_pixel": round(nbytes / (C_ * ny * nx), 2), "ms_at_copy_rate": round(floor, 4), "ratio_to_copy_rate": round(best / floor, 2)})

    # the same gradient from rocFFT through torch.fft
    tab = torch.from_numpy(pf_mask._spectral["tab"][:3]).cuda()
    A_, B_ = tab[0], torch.complex(tab[1], tab[2])
    sig = float(pf_mask.sigma)
    best_t, med_t = event_ms(torch, lambda: sig * torch.fft.irfft2(A_ * torch.fft.rfft2(x0, norm="ortho") - B_, s=shape, norm="ortho"), a.repeats)
    emit({"config": "torch-fft-gradient", "size": a.size, "ms_best": round(best_t, 4), "ms_median": round(med_t, 4), "ratio_to_three_launches": round(best_t / best, 2)})
    print(json.dumps({"bench": "fourier", "size": a.size, "steps": a.steps, "results": results}))


if __name__ == "__main__":
    main()

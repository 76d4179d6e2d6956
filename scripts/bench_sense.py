"""The multi-coil SENSE data term beside what exists, in one process: event-timed MYULA iterations (lmc_sampler_last_step_timing: HIP events around each
iteration's step launches, the moment reductions outside) with the TV prior at K = 10.

  - `MultiCoilFourierSampling` with 8 coils (smooth Gaussian magnitudes times phase ramps) and a 30 % mask;
  - the gradient alone (`L2.grad`: per coil rows forward, columns with the functor, rows inverse; then the elementwise overwrite form), in ms and ms per coil,
    against its byte count at the copy rate `lmc_hbm_copy_probe` measures in this process: per coil and pixel 4 + 8 (rows forward: x in, spectrum out)
    + 16 (columns: spectrum in and out) + 8 + 8 (rows inverse: spectrum in, g read and written; coil 0 only writes: 4 B less), plus 8 B for step 3;
  - n_coils x the single-coil spectral gradient (`FourierSampling`, the half plane: half the bytes per coil) -- the honest comparison;
  - the same gradient composed from `torch.fft.fft2` / `ifft2` (rocFFT) and elementwise operations, coil by coil.
One JSON line per configuration, then one with all of them.

    python scripts/bench_sense.py [--size 512x512x1024] [--coils 8] [--steps 10] [--warmup 3] [--repeats 3]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_fourier import GAMMA, SIGMA, TAU, event_ms, step_ms      # noqa: E402


def coil_maps(shape, n_coils):
    H, W = shape
    i, j = np.meshgrid(np.arange(H) / H - 0.5, np.arange(W) / W - 0.5, indexing="ij")
    out = np.empty((n_coils, H, W), dtype=np.complex64)
    for c in range(n_coils):
        ang = 2 * np.pi * (c + 0.25) / n_coils
        mag = 0.2 + np.exp(-((i - 0.45 * np.sin(ang)) ** 2 + (j - 0.45 * np.cos(ang)) ** 2) / (2 * 0.6 ** 2))
        out[c] = mag * np.exp(1j * (2 * np.pi * ((0.7 + 0.3 * c) * i - (0.4 + 0.2 * c) * j) + 0.9 * c))
    return out / np.sqrt(np.max(np.sum(np.abs(out) ** 2, axis=0)))      # sum_c |S_c|^2 <= 1: the step size of the other scripts stays stable


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="512x512x1024")
    ap.add_argument("--coils", type=int, default=8)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    import torch
    import lmc_atomi_amd as la
    from lmc_atomi_amd import _dev
    ny, nx, C_ = (int(v) for v in a.size.split("x"))
    shape, nc = (ny, nx), a.coils
    rng = np.random.default_rng(0)
    img = np.zeros(shape)
    img[ny // 5:ny // 2, nx // 4:nx // 2] = 190.0
    img += np.linspace(0, 30, nx)[None, :]
    x0 = torch.from_numpy(img.astype(np.float32)).cuda()[None].repeat(C_, 1, 1) + 5.0 * torch.randn((C_, ny, nx), device="cuda")
    results = []

    def emit(r):
        print(json.dumps(r), flush=True)
        results.append(r)

    gbs = C.c_float()
    lib = _dev.lib()
    rc = lib.lmc_hbm_copy_probe(C.c_size_t(1 << 30), 3, C.byref(gbs), _dev.stream_ptr())
    assert rc == 0, lib.lmc_last_error()
    emit({"config": "hbm-copy-probe", "gb_per_s": round(gbs.value, 1)})

    mask = (rng.uniform(size=shape) < 0.3).astype(np.float64)
    mask[:2, :2] = mask[:2, -2:] = mask[-2:, :2] = mask[-2:, -2:] = 1.0
    maps = coil_maps(shape, nc)
    ksp = mask * np.fft.fft2(maps * img, norm="ortho") + SIGMA * (rng.normal(size=(nc,) + shape) + 1j * rng.normal(size=(nc,) + shape))
    pf = la.L2(Op=la.MultiCoilFourierSampling(shape, maps, mask), b=ksp, sigma=1 / SIGMA ** 2)
    assert TAU < 1.0 / (pf.grad_lipschitz() + 1.0 / GAMMA)
    best, med, kernel = step_ms(torch, la, pf, shape, C_, x0, a.steps, a.warmup, a.repeats)
    emit({"config": f"sense-{nc}coils-mask30", "size": a.size, "ms_per_iteration_best": round(best, 4), "ms_per_iteration_median": round(med, 4),
          "prior_launch_kernel": kernel})

    # the gradient alone, against its byte count at the measured copy rate
    per_pixel = nc * (4 + 8 + 16 + 8 + 8) - 4 + 8
    nbytes = C_ * ny * nx * per_pixel
    g_best, g_med = event_ms(torch, lambda: pf.grad(x0), a.repeats)
    floor = nbytes / (gbs.value * 1e9) * 1e3
    emit({"config": "sense-gradient", "size": a.size, "coils": nc, "ms_best": round(g_best, 4), "ms_median": round(g_med, 4), "ms_per_coil": round(g_best / nc, 4),
          "bytes": nbytes, "bytes_per_pixel": per_pixel, "ms_at_copy_rate": round(floor, 4), "ratio_to_copy_rate": round(g_best / floor, 2)})

    # n_coils x the single-coil spectral gradient (the half plane)
    pf_one = la.L2(Op=la.FourierSampling(shape, mask), b=ksp[0], sigma=1 / SIGMA ** 2)
    s_best, s_med = event_ms(torch, lambda: pf_one.grad(x0), a.repeats)
    emit({"config": "spectral-gradient-one-coil", "size": a.size, "ms_best": round(s_best, 4), "ms_median": round(s_med, 4),
          "times_coils_ms": round(nc * s_best, 4), "sense_over_coils_x_spectral": round(g_best / (nc * s_best), 2)})

    # the same gradient from rocFFT through torch.fft, coil by coil
    S_ = torch.from_numpy(maps).cuda()
    M_ = torch.from_numpy(mask.astype(np.float32)).cuda()
    b_ = torch.from_numpy(ksp.astype(np.complex64)).cuda()
    sig = float(pf.sigma)

    def composed():
        g = None
        for c in range(nc):
            e = M_ * (M_ * torch.fft.fft2(S_[c] * x0, norm="ortho") - b_[c])
            t = (torch.conj(S_[c]) * torch.fft.ifft2(e, norm="ortho")).real
            g = t if g is None else g + t
        return sig * g

    t_best, t_med = event_ms(torch, composed, a.repeats)
    emit({"config": "torch-fft-gradient", "size": a.size, "coils": nc, "ms_best": round(t_best, 4), "ms_median": round(t_med, 4),
          "ratio_to_sense_gradient": round(t_best / g_best, 2)})
    print(json.dumps({"bench": "sense", "size": a.size, "coils": nc, "steps": a.steps, "results": results}))


if __name__ == "__main__":
    main()

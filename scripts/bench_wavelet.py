"""The Daubechies wavelet-l1 prior, in one process: the prox alone (HIP events around `--steps` calls of `lmc_wavelet_l1_prox`, buffers allocated before) and a whole MYULA
iteration (lmc_sampler_last_step_timing: events around each iteration's launches, the prox launches included) on inpainting, mask + wavelet prior, for
(p, levels) in (1, 3), (2, 4), (4, 4).  Beside them, code that exists:

  - the block-Haar prior (`WaveletL1(dims)`: one thread per 8 x 8 block, fused into the register-block step kernel) on the same problem -- the same
    mathematics as (1, 3);
  - the HBM byte floor of the prox: every forward level reads its input once and writes four quarter-size subbands, every inverse level reads them and
    writes the finer approximation, 16 N (1 + 1/4 + ... ) bytes for N pixels and no halo, divided by the copy rate `lmc_hbm_copy_probe` measures in this
    process.
One JSON line per configuration, then one with all of them.

    python scripts/bench_wavelet.py [--size 512x512x1024] [--steps 20] [--warmup 3] [--repeats 3]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIGMA, WEIGHT = 0.75, 2.0
GAMMA, TAU = SIGMA ** 2, 0.2 * SIGMA ** 2
CONFIGS = [("db1", 3), ("db2", 4), ("db4", 4)]


def prox_ms(torch, pg, x, out, calls, repeats):
    """(best, median) event-timed ms per prox, `calls` of them back to back inside every timed window, buffers in place"""
    from lmc_atomi_amd import _dev
    n = x.shape[0]
    H, W = pg.dims

    def call():
        if pg.block_haar:
            _dev.run(x, "lmc_haar_l1_prox", _dev.ptr(x), _dev.ptr(out), n, H, W, pg.sigma * GAMMA)
        else:
            _dev.run(x, "lmc_wavelet_l1_prox", _dev.ptr(x), _dev.ptr(out), n, H, W, pg.p, pg.levels, pg.sigma * GAMMA)

    for _ in range(3):
        call()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            call()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / calls)
    return float(np.min(ms)), float(np.median(ms))


def step_ms(torch, la, pf, pg, shape, C_, x0, steps, warmup, repeats):
    smp = la.MYULASampler(pf, pg, shape, n_chains=C_, tau=TAU, gamma=GAMMA, seed=1, policy={"iterations_per_launch": 1})
    try:
        smp.set_state(x0)
        smp.step(warmup)
        smp.enable_timing(True)
        ms = []
        for _ in range(repeats):
            smp.step(steps)
            t, _ = smp.last_step_timing()
            ms.append(t / steps)
        smp.enable_timing(False)
        torch.cuda.synchronize()
        return float(np.min(ms)), float(np.median(ms)), smp.kernel_name
    finally:
        smp.close()


def floor_bytes(n_pixels, levels):
    return 16.0 * n_pixels * sum(0.25 ** j for j in range(levels))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="512x512x1024")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    import torch
    import lmc_atomi_amd as la
    from lmc_atomi_amd import _dev
    ny, nx, C_ = (int(v) for v in a.size.split("x"))
    shape = (ny, nx)
    rng = np.random.default_rng(0)
    img = np.zeros(shape)
    img[ny // 5:ny // 2, nx // 4:nx // 2] = 190.0
    img += np.linspace(0, 30, nx)[None, :]
    mask = (rng.uniform(size=shape) < 0.5).astype(np.float64)
    y = mask * (img + rng.normal(0, SIGMA, shape))
    pf = la.L2(Op=la.Diagonal(mask, dims=shape), b=y, sigma=1 / SIGMA ** 2, dims=shape)
    x0 = torch.from_numpy(img.astype(np.float32)).cuda()[None].repeat(C_, 1, 1) + 5.0 * torch.randn((C_, ny, nx), device="cuda")
    out = torch.empty_like(x0)
    gbs = C.c_float()
    with torch.cuda.device(x0.device):
        rc = _dev.lib().lmc_hbm_copy_probe(C.c_size_t(min(x0.numel() * 4, 1 << 30)), 3, C.byref(gbs), _dev.stream_ptr())
    assert rc == 0
    copy_gbs = float(gbs.value)
    results = []

    def run(label, pg, levels):
        pb, pm = prox_ms(torch, pg, x0, out, a.steps, a.repeats)
        sb, sm, kernel = step_ms(torch, la, pf, pg, shape, C_, x0, a.steps, a.warmup, a.repeats)
        r = {"config": label, "size": a.size, "levels": levels, "prox_ms_best": round(pb, 4), "prox_ms_median": round(pm, 4),
             "ms_per_iteration_best": round(sb, 4), "ms_per_iteration_median": round(sm, 4), "step_kernel": kernel}
        if not pg.block_haar:
            fl = floor_bytes(x0.numel(), levels) / (copy_gbs * 1e9) * 1e3
            r.update({"prox_floor_ms": round(fl, 4), "prox_over_floor": round(pb / fl, 3), "prox_floor_bytes": floor_bytes(x0.numel(), levels)})
        print(json.dumps(r), flush=True)
        results.append(r)

    run("block-haar", la.WaveletL1(shape, sigma=WEIGHT), 3)
    for name, levels in CONFIGS:
        run(f"{name}-L{levels}", la.WaveletL1(shape, sigma=WEIGHT, levels=levels, wavelet=name), levels)
    print(json.dumps({"bench": "wavelet", "size": a.size, "steps": a.steps, "hbm_copy_gbs": round(copy_gbs, 1), "results": results}))


if __name__ == "__main__":
    main()

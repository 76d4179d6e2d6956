"""The second-order TGV prior, in one process, event-timed: the prox alone (`lmc_tgv_prox`, buffers allocated before) and a whole MYULA iteration with it
(prox launches + the step launch) on a 5 x 5 box deblurring of `--size` HxWxC images, `--niter` primal-dual iterations.  Beside them, from the same process:

  - the copy rate `lmc_hbm_copy_probe` measures, and the HBM byte floor of the prox at that rate: read x and write the prox, 8 B per pixel, plus the
    11-plane state written by every launch but the last and read by the next, 88 B per pixel and chained launch;
  - code that exists, at the same size: the isotropic TV prox at the same iteration count through `lmc_fused_eval` (0, 0, 1) with the tile kernel forced,
    and the MYULA iteration of the same chains with TV(niter=10).
Every window holds `--steps` calls (at least 20) back to back after `--warmup` calls; best and median of `--repeats` windows.  One JSON line.

    python scripts/bench_tgv.py [--size 512x512x1024] [--niter 40] [--steps 20] [--warmup 3] [--repeats 3] [--only-prox]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIGMA, WEIGHT, ALPHA0 = 0.75, 0.3, 2.0
GAMMA, TAU = SIGMA ** 2, 0.2 * SIGMA ** 2


def timed(torch, fn, calls, repeats, warmup=3):
    """(best, median) event-timed ms per call, `calls` of them back to back inside every timed window"""
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / calls)
    return round(float(np.min(ms)), 4), round(float(np.median(ms)), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="512x512x1024")
    ap.add_argument("--niter", type=int, default=40)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only-prox", action="store_true", help="the prox alone and its floor (a library built with another launch length: LMC_ATOMI_LIB)")
    a = ap.parse_args()
    if a.steps < 20:
        ap.error("--steps: at least 20 calls per timed window")
    import torch
    import lmc_atomi_amd as la
    from lmc_atomi_amd import _capi, _dev
    from lmc_atomi_amd.proximal import _Problem
    ny, nx, C_ = (int(v) for v in a.size.split("x"))
    shape, K = (ny, nx), a.niter
    rng = np.random.default_rng(0)
    img = np.zeros(shape)
    img[ny // 5:ny // 2, nx // 4:nx // 2] = 190.0
    img += np.linspace(0, 30, nx)[None, :]
    h = np.ones((5, 5)) / 25.0
    blur = la.Convolve2D(shape, h, offset=(2, 2))
    y = blur.matvec(img.ravel()).reshape(shape) + rng.normal(0, SIGMA, shape)
    x0 = torch.from_numpy(img.astype(np.float32)).cuda()[None].repeat(C_, 1, 1) + 5.0 * torch.randn((C_,) + shape, device="cuda")
    out = torch.empty_like(x0)
    gbs = C.c_float()
    with torch.cuda.device(x0.device):
        assert _dev.lib().lmc_hbm_copy_probe(C.c_size_t(min(x0.numel() * 4, 1 << 30)), 3, C.byref(gbs), _dev.stream_ptr()) == 0
    copy_gbs = float(gbs.value)
    pt = GAMMA * WEIGHT
    L = _capi.tgv_launch_iters()
    launches = -(-K // L)

    r = {"bench": "tgv", "size": a.size, "niter": K, "steps": a.steps, "repeats": a.repeats, "hbm_copy_gbs": round(copy_gbs, 1), "launch_iters": L,
         "launches": launches}
    tgv = lambda: _dev.run(x0, "lmc_tgv_prox", _dev.ptr(x0), _dev.ptr(out), None, C_, ny, nx, pt, ALPHA0, K, 0.0, 0, 0.0, 0.0)
    r["tgv_prox_ms_best"], r["tgv_prox_ms_median"] = timed(torch, tgv, a.steps, a.repeats, a.warmup)
    floor = (8.0 + 88.0 * (launches - 1)) * x0.numel() / (copy_gbs * 1e9) * 1e3
    r["tgv_prox_floor_ms"] = round(floor, 4)
    r["tgv_prox_over_floor"] = round(r["tgv_prox_ms_best"] / floor, 2)
    if a.only_prox:
        print(json.dumps(r))
        return

    grey = _Problem(shape, prior=la.TV(shape, sigma=WEIGHT, niter=K).prior_descriptor(), options={"step_variant": "tile"})
    tile = lambda: _dev.run(x0, "lmc_fused_eval", C.byref(grey.c), _dev.ptr(x0), _dev.ptr(out), C_, 0.0, 0.0, 1.0, GAMMA)
    r["tv_tile_prox_ms_best"], r["tv_tile_prox_ms_median"] = timed(torch, tile, a.steps, a.repeats, a.warmup)
    r["tgv_prox_over_tv_tile_prox"] = round(r["tgv_prox_ms_best"] / r["tv_tile_prox_ms_best"], 2)

    pf = la.L2(Op=blur, b=y, sigma=1 / SIGMA ** 2)
    with la.MYULASampler(pf, la.TGV(shape, sigma=WEIGHT, alpha0=ALPHA0, niter=K), shape, n_chains=C_, tau=TAU, gamma=GAMMA, seed=1) as smp:
        smp.set_state(x0)
        r["tgv_iteration_ms_best"], r["tgv_iteration_ms_median"] = timed(torch, lambda: smp.step(1), a.steps, a.repeats, a.warmup)
        r["tgv_step_kernel"] = smp.kernel_name
    with la.MYULASampler(pf, la.TV(shape, sigma=WEIGHT, niter=10), shape, n_chains=C_, tau=TAU, gamma=GAMMA, seed=1) as smp:
        smp.set_state(x0)
        r["tv10_iteration_ms_best"], r["tv10_iteration_ms_median"] = timed(torch, lambda: smp.step(1), a.steps, a.repeats, a.warmup)
        r["tv10_kernel"] = smp.kernel_name
    r["tgv_iteration_over_tv10_iteration"] = round(r["tgv_iteration_ms_best"] / r["tv10_iteration_ms_best"], 2)
    torch.cuda.synchronize()
    print(json.dumps(r))


if __name__ == "__main__":
    main()

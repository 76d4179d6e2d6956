"""The vectorial TV prior, in one process, event-timed: the coupled prox alone (`lmc_vtv_prox`, buffers allocated before) and a whole iteration of the
multi-channel MYULA sampler (prox launch + one step launch per channel) on a 5 x 5 box deblurring of `--size` HxWxC images of `--channels` channels,
K = `--niter` dual iterations.  Beside them, from the same process:

  - the copy rate `lmc_hbm_copy_probe` measures, and the HBM byte floor of the prox at that rate: read x and write the prox, 8 B per pixel and channel;
  - code that exists, at the same pixel count (channels x C grey images): the isotropic TV prox through `lmc_fused_eval` (0, 0, 1) with the tile kernel
    forced, and the grey MYULA iteration of that many chains with TV(niter).
One JSON line.

    python scripts/bench_vtv.py [--size 512x512x256] [--channels 3] [--niter 10] [--steps 10] [--warmup 3] [--repeats 3]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIGMA, WEIGHT = 0.75, 0.3
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
    ap.add_argument("--size", default="512x512x256")
    ap.add_argument("--channels", type=int, default=3)
    ap.add_argument("--niter", type=int, default=10)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    import torch
    import lmc_atomi_amd as la
    from lmc_atomi_amd import _dev
    from lmc_atomi_amd.proximal import _Problem
    ny, nx, C_ = (int(v) for v in a.size.split("x"))
    shape, nch, K = (ny, nx), a.channels, a.niter
    rng = np.random.default_rng(0)
    img = np.zeros((nch,) + shape)
    for ch in range(nch):
        img[ch, ny // 5:ny // 2, nx // 4:nx // 2] = 190.0 - 40.0 * ch
    img += np.linspace(0, 30, nx)[None, None, :]
    h = np.ones((5, 5)) / 25.0
    blur = lambda: la.Convolve2D(shape, h, offset=(2, 2))
    ys = [blur().matvec(img[ch].ravel()).reshape(shape) + rng.normal(0, SIGMA, shape) for ch in range(nch)]
    x0 = torch.from_numpy(img.astype(np.float32)).cuda()[:, None].repeat(1, C_, 1, 1) + 5.0 * torch.randn((nch, C_) + shape, device="cuda")
    out = torch.empty_like(x0)
    gbs = C.c_float()
    with torch.cuda.device(x0.device):
        assert _dev.lib().lmc_hbm_copy_probe(C.c_size_t(min(x0.numel() * 4, 1 << 30)), 3, C.byref(gbs), _dev.stream_ptr()) == 0
    copy_gbs = float(gbs.value)
    pt = GAMMA * WEIGHT

    pg = la.VectorialTV(shape, nch, sigma=WEIGHT, niter=K)
    betas = _dev.fptr(pg._betas)
    vtv = lambda: _dev.run(x0, "lmc_vtv_prox", _dev.ptr(x0), _dev.ptr(out), C_, nch, C_ * ny * nx, ny, nx, pt, K, 0.125, betas, 0, 0.0, 0.0)
    r = {"bench": "vtv", "size": a.size, "channels": nch, "niter": K, "steps": a.steps, "hbm_copy_gbs": round(copy_gbs, 1)}
    r["vtv_prox_ms_best"], r["vtv_prox_ms_median"] = timed(torch, vtv, a.steps, a.repeats)
    floor = 8.0 * x0.numel() / (copy_gbs * 1e9) * 1e3
    r["vtv_prox_floor_ms"] = round(floor, 4)
    r["vtv_prox_over_floor"] = round(r["vtv_prox_ms_best"] / floor, 2)

    grey = _Problem(shape, prior=la.TV(shape, sigma=WEIGHT, niter=K).prior_descriptor(), options={"step_variant": "tile"})
    tile = lambda: _dev.run(x0, "lmc_fused_eval", C.byref(grey.c), _dev.ptr(x0), _dev.ptr(out), nch * C_, 0.0, 0.0, 1.0, GAMMA)
    r["grey_tile_prox_ms_best"], r["grey_tile_prox_ms_median"] = timed(torch, tile, a.steps, a.repeats)
    r["vtv_prox_over_grey_tile_prox"] = round(r["vtv_prox_ms_best"] / r["grey_tile_prox_ms_best"], 2)

    pf = [la.L2(Op=blur(), b=ys[ch], sigma=1 / SIGMA ** 2) for ch in range(nch)]
    with la.MultichannelMYULASampler(pf, pg, shape, n_chains=C_, tau=TAU, gamma=GAMMA, seed=1) as smp:
        smp.set_state(x0)
        r["mch_iteration_ms_best"], r["mch_iteration_ms_median"] = timed(torch, lambda: smp.step(1), a.steps, a.repeats, a.warmup)
        r["mch_kernels"] = smp.kernel_name
    with la.MYULASampler(pf[0], la.TV(shape, sigma=WEIGHT, niter=K), shape, n_chains=nch * C_, tau=TAU, gamma=GAMMA, seed=1) as smp:
        smp.set_state(x0.reshape((nch * C_,) + shape))
        r["grey_iteration_ms_best"], r["grey_iteration_ms_median"] = timed(torch, lambda: smp.step(1), a.steps, a.repeats, a.warmup)
        r["grey_kernel"] = smp.kernel_name
    r["mch_iteration_over_grey_iteration"] = round(r["mch_iteration_ms_best"] / r["grey_iteration_ms_best"], 2)
    torch.cuda.synchronize()
    print(json.dumps(r))


if __name__ == "__main__":
    main()

"""A SAPG iteration beside a plain MYULA iteration, in one process, alternating: 5 x 5 blur + TV (K = 10), 512 x 512 x 1024 chains by default.

  - wall ms per SAPG iteration (`estimate_prior_weight`: one sampler iteration, the prior statistic, the update kernel and one host wait per
    update) and wall ms per plain iteration (`step`) of the same sampler, in alternating timed regions of --steps iterations, --repeats times;
    the plain iterations run at the weight the estimation left, so both see the same kind of state;
  - the prior statistic alone (`lmc_prior_statistic`) against `lmc_energies(f = NULL)` on the same state, HIP events around --stat-reps calls each,
    alternating, with the bytes per second of the statistic's one read of the state.
Medians with minimum and maximum (the spread), and one JSON line at the end.

    python scripts/bench_sapg.py [--size 512x512x1024] [--steps 40] [--warmup 10] [--repeats 5] [--stat-reps 20]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(a):
    a = np.asarray(a, dtype=np.float64)
    return {"median": float(np.median(a)), "min": float(a.min()), "max": float(a.max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="512x512x1024", help="HxWxchains")
    ap.add_argument("--steps", type=int, default=40, help="iterations per timed region")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--stat-reps", type=int, default=20)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    import lmc_atomi_amd as la
    from lmc_atomi_amd import _capi, _dev

    H, W, Cn = (int(v) for v in args.size.split("x"))
    sigma = 0.75
    gamma = sigma ** 2
    tau = 1.0 / (1 / sigma ** 2 + 1 / gamma)
    rng = np.random.default_rng(0)
    img = np.zeros((H, W), dtype=np.float32)
    img[H // 5:H // 2, W // 6:2 * W // 3] = 160.0
    img += np.linspace(0, 25, W, dtype=np.float32)[None, :]
    Op = la.Convolve2D((H, W), np.ones((5, 5)) / 25.0, offset=(2, 2))
    y = np.asarray(Op.matvec(img.ravel())).reshape(H, W) + rng.normal(0, sigma, (H, W)).astype(np.float32)
    pf, pg = la.L2(Op=Op, b=y, sigma=1 / sigma ** 2), la.TV((H, W), sigma=0.3, niter=10)
    bounds = (1e-3, 1e2)

    smp = la.MYULASampler(pf, pg, (H, W), n_chains=Cn, tau=tau, gamma=gamma, seed=1)
    smp.set_state(y)
    smp.step(args.warmup)
    res0 = smp.estimate_prior_weight(args.warmup, bounds, theta0=0.3)
    sapg, plain = [], []
    for _ in range(args.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = smp.estimate_prior_weight(args.steps, bounds, theta0=smp.prior_weight)
        torch.cuda.synchronize()
        sapg.append((time.perf_counter() - t0) * 1e3 / args.steps)
        t0 = time.perf_counter()
        smp.step(args.steps)
        torch.cuda.synchronize()
        plain.append((time.perf_counter() - t0) * 1e3 / args.steps)
    print(f"{args.size} blur5x5 + TV K=10 ({smp.kernel_name}): SAPG {np.median(sapg):.4f} ms per iteration ({min(sapg):.4f} .. {max(sapg):.4f}), "
          f"plain MYULA {np.median(plain):.4f} ms ({min(plain):.4f} .. {max(plain):.4f}); theta {res0.theta:.4f} -> {r.theta:.4f}", flush=True)

    # the statistic alone against lmc_energies(f = NULL) on the same state
    x = smp.get_state()
    lib = _dev.lib()
    out = torch.empty(Cn, dtype=torch.float64, device=x.device)
    prob = smp._problem.c
    st = _dev.stream_ptr(x.device)
    calls = {"lmc_prior_statistic": lambda: _capi.check(lib.lmc_prior_statistic(C.byref(prob), _dev.ptr(x), Cn, _dev.ptr(out), st)),
             "lmc_energies(f=NULL)": lambda: _capi.check(lib.lmc_energies(C.byref(prob), _dev.ptr(x), Cn, None, _dev.ptr(out), st))}
    times = {k: [] for k in calls}
    for fn in calls.values():
        fn()
    for _ in range(args.repeats):
        for name, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.stat_reps):
                fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) / args.stat_reps)
    smp.close()
    gbs = 4.0 * H * W * Cn / (np.median(times["lmc_prior_statistic"]) * 1e-3) / 1e9
    for name, t in times.items():
        print(f"    {name}: {np.median(t):.4f} ms ({min(t):.4f} .. {max(t):.4f})", flush=True)
    print(f"    the statistic reads the state at {gbs:.0f} GB/s", flush=True)
    print(json.dumps({"config": f"{args.size} blur5x5+tv10", "sapg_ms_per_iteration": spread(sapg), "myula_ms_per_iteration": spread(plain),
                      "prior_statistic_ms": spread(times["lmc_prior_statistic"]), "energies_g_only_ms": spread(times["lmc_energies(f=NULL)"]),
                      "prior_statistic_gbs": float(gbs)}), flush=True)


if __name__ == "__main__":
    main()

"""SK-ROCK beside MYULA in one process: time per iteration and effective samples per second, for 5 x 5 blur + TV (K = 10; VALU-bound pipe kernel)
and 5 x 5 blur + l2 (HBM-bound rows kernel).

Per configuration:
  - MYULA: ms per single-iteration launch (HIP events around each launch, lmc_sampler_last_step_timing; iterations_per_launch = 1) and wall ms per
    step of the default policy;
  - SK-ROCK, s in --stages, Philox noise: wall ms per iteration, the event-timed ms of its s stage launches, and what lies outside the brackets
    (the perturbation launch and launch gaps);
  - the budget of an iteration: s x (MYULA launch) + the perturbation launch (8 B per chain-pixel) + s extra reads of K_{j-2} (4 B per chain-pixel
    each), the last two at the bandwidth lmc_hbm_copy_probe measures in this process, all times 1.05;
  - ESS per second of the ChainTrace probes (8 x 8 block means): MYULA at tau = 1 / L against SK-ROCK at 0.8 l_s / L, L = 1 / sigma^2 + 1 / gamma,
    after the same number of gradient evaluations (--evals; the first fifth discarded), per second of stepping;
  - beside them, min and median over the PIXELS of the effective sample size per second from chain-group moments (chain_groups = 32,
    mcse_from_group_moments) of a second run of the same length: the probes are low frequencies, which the data pins down; the stiff directions
    SK-ROCK is built for live in the pixels.
One JSON line per configuration at the end.

    python scripts/bench_skrock.py [--size 512x512x1024] [--stages 5,10,15] [--steps 60] [--warmup 10] [--repeats 5] [--evals 3000]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def wall_ms_per_iteration(torch, smp, iters, repeats):
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        smp.step(iters)
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3 / iters)
    return np.asarray(out)


def launch_ms(smp, iters, repeats):
    """(event-timed ms per launch, launches per iteration) over `repeats` calls of step(iters)."""
    smp.enable_timing(True)
    ms, per_it = [], 1
    for _ in range(repeats):
        smp.step(iters)
        t, n = smp.last_step_timing()
        ms.append(t / n)
        per_it = n // iters
    smp.enable_timing(False)
    return np.asarray(ms), per_it


def ess_per_second(torch, la, smp, x0, iters, every, burn):
    from lmc_atomi_amd.diagnostics import ChainTrace
    smp.set_state(x0)
    tr = ChainTrace(smp, (8, 8), energies=False)
    spent = 0.0
    for k in range(0, iters, every):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        smp.step(every)
        torch.cuda.synchronize()
        spent += time.perf_counter() - t0
        if k + every > burn:
            tr.record()
    e = tr.summary()["ess"].cpu().numpy()
    e = e[np.isfinite(e)]
    return {"records": len(tr), "step_seconds": spent, "ess_min": float(e.min()), "ess_median": float(np.median(e)),
            "ess_min_per_s": float(e.min() / spent), "ess_median_per_s": float(np.median(e) / spent)}


def pixel_ess_per_second(torch, la, make, x0, iters, burn, groups=32):
    """ESS per second of the pixels: a sampler with chain-group moments runs `iters` iterations in one call, the first `burn` not kept."""
    smp = make(moments=True, burn_in=burn, chain_groups=groups)
    try:
        smp.set_state(x0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        smp.step(iters)
        torch.cuda.synchronize()
        spent = time.perf_counter() - t0
        e = la.mcse_from_group_moments(*smp.group_moments()).ess.cpu().numpy()
    finally:
        smp.close()
    e = e[np.isfinite(e)]
    return {"kept": iters - burn, "step_seconds": spent, "pixel_ess_min": float(e.min()), "pixel_ess_median": float(np.median(e)),
            "pixel_ess_min_per_s": float(e.min() / spent), "pixel_ess_median_per_s": float(np.median(e) / spent)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="512x512x1024", help="HxWxchains")
    ap.add_argument("--stages", default="5,10,15")
    ap.add_argument("--steps", type=int, default=60, help="MYULA steps per timed region (SK-ROCK: steps // s + 1 iterations)")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--evals", type=int, default=3000, help="gradient evaluations of each ESS run (0: skip)")
    ap.add_argument("--priors", default="tv,l2")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    import lmc_atomi_amd as la

    H, W, C = (int(v) for v in args.size.split("x"))
    stages = [int(v) for v in args.stages.split(",")]
    n = H * W * C
    g = ctypes.c_float()
    la._capi.check(la._dev.lib().lmc_hbm_copy_probe(min(4 * n, 1 << 30), 3, ctypes.byref(g), None))
    gbs = float(g.value)
    print(f"lmc_hbm_copy_probe: {gbs:.0f} GB/s (read + write)", flush=True)
    read_ms = 4.0 * n / (gbs * 1e9) * 1e3             # one more 4 B per chain-pixel read
    perturb_ms = 2.0 * read_ms                         # the perturbation launch: 4 B read + 4 B written

    sigma = 0.75
    gamma = sigma ** 2
    L = 1 / sigma ** 2 + 1 / gamma
    rng = np.random.default_rng(0)
    img = np.zeros((H, W), dtype=np.float32)
    img[H // 5:H // 2, W // 6:2 * W // 3] = 160.0
    img += np.linspace(0, 25, W, dtype=np.float32)[None, :]
    h = np.ones((5, 5)) / 25.0
    Op = la.Convolve2D((H, W), h, offset=(2, 2))
    y = np.asarray(Op.matvec(img.ravel())).reshape(H, W) + rng.normal(0, sigma, (H, W)).astype(np.float32)
    pf = la.L2(Op=Op, b=y, sigma=1 / sigma ** 2)
    results = []
    for prior in args.priors.split(","):
        pg = la.TV((H, W), sigma=0.3, niter=10) if prior == "tv" else la.L2(sigma=0.05)
        res = {"config": f"{args.size} blur5x5+{prior}", "hbm_probe_gbs": gbs, "extra_read_ms": read_ms, "perturb_model_ms": perturb_ms, "skrock": {}}
        tau_m = 1.0 / L
        single = la.MYULASampler(pf, pg, (H, W), n_chains=C, tau=tau_m, gamma=gamma, seed=1, policy={"iterations_per_launch": 1})
        single.set_state(y)
        single.step(args.warmup)
        lm, _ = launch_ms(single, args.steps, args.repeats)
        res["myula_kernel"] = single.kernel_name
        single.close()
        plain = la.MYULASampler(pf, pg, (H, W), n_chains=C, tau=tau_m, gamma=gamma, seed=1)
        plain.set_state(y)
        plain.step(args.warmup)
        wm = wall_ms_per_iteration(torch, plain, args.steps, args.repeats)
        res["myula_launch_ms"] = {"median": float(np.median(lm)), "min": float(lm.min()), "max": float(lm.max())}
        res["myula_wall_ms_per_step"] = {"median": float(np.median(wm)), "min": float(wm.min()), "max": float(wm.max())}
        print(f"{res['config']}: MYULA launch {np.median(lm):.4f} ms ({lm.min():.4f} .. {lm.max():.4f}), wall per step {np.median(wm):.4f} ms "
              f"({res['myula_kernel']} / {plain.kernel_name})", flush=True)
        if args.evals:
            res["myula_ess"] = ess_per_second(torch, la, plain, y, args.evals, 10, args.evals // 5)
            print(f"    MYULA tau = 1/L = {tau_m:.4f}: {res['myula_ess']}", flush=True)
        plain.close()
        if args.evals and C >= 32:
            make = lambda **kw: la.MYULASampler(pf, pg, (H, W), n_chains=C, tau=tau_m, gamma=gamma, seed=1, **kw)
            res["myula_pixel_ess"] = pixel_ess_per_second(torch, la, make, y, args.evals, args.evals // 5)
            print(f"        {res['myula_pixel_ess']}", flush=True)
        for s in stages:
            delta = 0.8 * la.skrock_step_bound(L, s)
            smp = la.SKROCKSampler(pf, pg, (H, W), n_stages=s, n_chains=C, tau=delta, gamma=gamma, seed=1)
            smp.set_state(y)
            its = args.steps // s + 1
            smp.step(max(1, args.warmup // s))
            ws = wall_ms_per_iteration(torch, smp, its, args.repeats)
            ls, per_it = launch_ms(smp, its, args.repeats)
            assert per_it == s, (per_it, s)
            budget = 1.05 * (s * float(np.median(lm)) + perturb_ms + s * read_ms)
            r = {"delta": delta, "wall_ms_per_iteration": {"median": float(np.median(ws)), "min": float(ws.min()), "max": float(ws.max())},
                 "stage_launch_ms": float(np.median(ls)), "outside_brackets_ms": float(np.median(ws) - s * np.median(ls)),
                 "budget_ms": budget, "within_budget": bool(np.median(ws) <= budget), "kernel": smp.kernel_name}
            print(f"    SK-ROCK s = {s:2d} delta = {delta:.3f}: wall {np.median(ws):.4f} ms per iteration ({ws.min():.4f} .. {ws.max():.4f}), stage launch "
                  f"{np.median(ls):.4f} ms, outside the brackets {r['outside_brackets_ms']:.4f} ms; budget {budget:.4f} ms -> "
                  f"{'within' if r['within_budget'] else 'OVER'}", flush=True)
            if args.evals:
                every = max(1, 10 // s)
                r["ess"] = ess_per_second(torch, la, smp, y, (args.evals // s // every) * every, every, args.evals // s // 5)
                print(f"        {r['ess']}", flush=True)
                if C >= 32:
                    make = lambda **kw: la.SKROCKSampler(pf, pg, (H, W), n_stages=s, n_chains=C, tau=delta, gamma=gamma, seed=1, **kw)
                    r["pixel_ess"] = pixel_ess_per_second(torch, la, make, y, (args.evals // s // every) * every, args.evals // s // 5)
                    print(f"        {r['pixel_ess']}", flush=True)
            res["skrock"][str(s)] = r
            smp.close()
        results.append(res)
    for res in results:
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Bit-identity of two builds on the pipe kernels' configurations: `bench.py --dump-outputs` with the same arguments in two source trees,
every .npy compared byte for byte -- except the fp64 energies (energy_f.npy / energy_g.npy), which the energy kernels sum with atomic adds in an
order that differs from run to run of one build: those are compared at rtol 1e-12, as tests/test_gpu_pipe_teams.py does.

  compare_dumps.py dump OUT_DIR [--tree TREE]     run the configurations below with TREE/bench.py (default: this tree), one directory each
  compare_dumps.py compare DIR_A DIR_B            compare two such OUT_DIRs; exit status 1 on any difference

Each bench.py run is a process of its own under a time limit; `dump` stops at the first one that fails."""
import argparse, os, subprocess, sys

import numpy as np

COMMON = ["--chains", "4", "--steps", "5", "--warmup", "2", "--no-cpu-baseline", "--no-hbm-probe"]
CONFIGS = {
    "w264": ["--size", "264"],
    "w512": ["--size", "512"],
    "w260_unaligned": ["--size", "64", "--width", "260"],
    "w600_strips": ["--size", "64", "--width", "600"],
    "w264_blur7": ["--size", "264", "--blur-k", "7"],
    "w264_rtol": ["--size", "264", "--tv-rtol", "1e-4"],
    "w264_warm2": ["--size", "264", "--tv-warm", "--tv-iters", "2"],
    "w264_me": ["--size", "264", "--ncvx", "me"],
    "w264_mc": ["--size", "264", "--ncvx", "mc"],
    "w256_pxl4": ["--size", "256"],
    "w264_gauss": ["--size", "264", "--blur", "gaussian"],
    "w512_gauss": ["--size", "512", "--blur", "gaussian"],
    "w264_tv20_chained": ["--size", "264", "--tv-iters", "20"],      # two links through the dual state in HBM
}
ENERGIES = ("energy_f.npy", "energy_g.npy")      # sums of atomic adds: last-bit differences between two runs of one build


def dump(out_dir, tree):
    out_dir = os.path.abspath(out_dir)
    for name, args in CONFIGS.items():
        cmd = ["timeout", "-k", "10", "120", sys.executable, "bench.py"] + args + COMMON + ["--dump-outputs", os.path.join(out_dir, name)]
        r = subprocess.run(cmd, cwd=tree, capture_output=True, text=True)
        print(f"{name}: exit {r.returncode}", flush=True)
        if r.returncode != 0:
            sys.stdout.write(r.stdout[-2000:] + r.stderr[-4000:])
            return r.returncode
    return 0


def compare(a, b):
    bad = 0
    for name in CONFIGS:
        da, db = os.path.join(a, name), os.path.join(b, name)
        fa, fb = sorted(os.listdir(da)), sorted(os.listdir(db))
        if fa != fb or not fa:
            print(f"{name}: file lists differ: {fa} / {fb}")
            bad += 1
            continue
        diff = []
        for f in fa:
            if open(os.path.join(da, f), "rb").read() != open(os.path.join(db, f), "rb").read():
                xa, xb = np.load(os.path.join(da, f)).astype(np.float64), np.load(os.path.join(db, f)).astype(np.float64)
                if f in ENERGIES and xa.shape == xb.shape and np.allclose(xa, xb, rtol=1e-12, atol=0.0):
                    continue
                diff.append(f"{f} (max abs {np.max(np.abs(xa - xb)):.3e})" if xa.shape == xb.shape else f"{f} (shapes)")
        print(f"{name}: {len(fa)} files, " + ("identical" if not diff else "DIFFERENT: " + ", ".join(diff)))
        bad += bool(diff)
    print("all identical (energies to rtol 1e-12, everything else byte for byte)" if not bad else f"{bad} of {len(CONFIGS)} configurations differ")
    return 1 if bad else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    d = sub.add_parser("dump")
    d.add_argument("out_dir")
    d.add_argument("--tree", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    c = sub.add_parser("compare")
    c.add_argument("a")
    c.add_argument("b")
    args = ap.parse_args()
    sys.exit(dump(args.out_dir, args.tree) if args.cmd == "dump" else compare(args.a, args.b))

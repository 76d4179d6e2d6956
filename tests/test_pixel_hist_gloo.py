"""N > 1 path on CPU: world_size-2 gloo.  The host route of allreduce_sampler_histogram is allreduce_counts (the sampler object itself needs a GPU):
two processes sum their int64 counters and their sample counts for real, and the sums are exact -- values above 2^53 included, which a float64
all-reduce would round."""
import os
import socket
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WORKER = r'''
import os, sys, numpy as np, torch, torch.distributed as dist
sys.path.insert(0, sys.argv[1])
from lmc_atomi_amd.sharding import allreduce_counts
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", rank=rank, world_size=world)
rng = np.random.default_rng(100 + rank)
counts = rng.integers(0, 1000, (9, 5, 7))
counts[0, 0, 0] = 2 ** 53 + 1 + rank           # not a float64
g, n = allreduce_counts(torch.from_numpy(counts), 40 + rank)
assert g.dtype == torch.int64 and tuple(g.shape) == (9, 5, 7)
if rank == 0:
    np.savez(sys.argv[2], counts=g.numpy(), count=n)
dist.destroy_process_group()
'''


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_rank_gloo_histogram_counts_sum_exactly(tmp_path):
    out = str(tmp_path / "res.npz")
    port = _free_port()
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, "-c", WORKER, ROOT, out], env=env))
    for p in procs:
        assert p.wait(timeout=300) == 0
    got = np.load(out)
    want = np.zeros((9, 5, 7), dtype=np.int64)
    for r in range(2):
        c = np.random.default_rng(100 + r).integers(0, 1000, (9, 5, 7))
        c[0, 0, 0] = 2 ** 53 + 1 + r
        want += c
    assert int(got["count"]) == 81
    assert got["counts"].dtype == np.int64
    np.testing.assert_array_equal(got["counts"], want)


def test_allreduce_counts_is_the_identity_without_a_process_group():
    import torch
    from lmc_atomi_amd.sharding import allreduce_counts
    a = torch.arange(24, dtype=torch.int64).reshape(4, 2, 3)
    g, n = allreduce_counts(a, 5)
    assert n == 5 and torch.equal(g, a)

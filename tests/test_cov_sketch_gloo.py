"""N > 1 path on CPU: world_size-2 gloo.  allreduce_cov_sketch is the host route of a sharded job (the sampler object itself needs a GPU): two processes
holding 7 and 5 chains of a 12-chain job, with the same probes and centre, sum their Y, s, Q and counts for real, and cov_from_sketch of the result equals
that of the sums formed from all 12 chains at once."""
import os
import socket
import subprocess
import sys

import numpy as np

from tests import _cov_sketch_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, SHAPE, KEPT = 3, (5, 7), 6
SHARDS = ((0, 7), (7, 5))

WORKER = r'''
import os, sys, numpy as np, torch, torch.distributed as dist
sys.path.insert(0, sys.argv[1])
from lmc_atomi_amd.sharding import allreduce_cov_sketch
from tests.test_cov_sketch_gloo import K, SHAPE, SHARDS, shard_sums
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", rank=rank, world_size=world)
Y, s, Q, n = shard_sums(*SHARDS[rank])
gY, gs, gQ, gn = allreduce_cov_sketch(torch.from_numpy(Y), torch.from_numpy(s), torch.from_numpy(Q), n)
assert gY.dtype == torch.float64 and tuple(gY.shape) == (K,) + SHAPE and tuple(gs.shape) == (K,) and tuple(gQ.shape) == (K, K)
assert isinstance(gn, int)
if rank == 0:
    np.savez(sys.argv[2], Y=gY.numpy(), s=gs.numpy(), Q=gQ.numpy(), n=gn)
dist.destroy_process_group()
'''


def job():
    """the kept states of the whole job [KEPT, 12, H, W] (fp32, 100 + N(0, 1)), the probes and the centre every rank uses"""
    rng = np.random.default_rng(77)
    x = (100.0 + rng.standard_normal((KEPT, 12) + SHAPE)).astype(np.float32)
    P = rng.standard_normal((K,) + SHAPE).astype(np.float32)
    m = np.full(SHAPE, 100.0, dtype=np.float32)
    return x, P, m


def shard_sums(off, n):
    """(Y [K, H, W], s, Q, samples) of the chains off .. off + n - 1 over the kept states, float64 by the definition"""
    x, P, m = job()
    Y, s, Q = R.sketch_ref(x[:, off:off + n].reshape((KEPT * n,) + SHAPE), P, m)
    return Y.reshape((K,) + SHAPE), s, Q, KEPT * n


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_rank_gloo_sketch_equals_the_unsharded_sums(tmp_path):
    from lmc_atomi_amd import cov_from_sketch
    out = str(tmp_path / "res.npz")
    port = _free_port()
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, "-c", WORKER, ROOT, out], env=env))
    for p in procs:
        assert p.wait(timeout=300) == 0
    got = np.load(out)
    parts = [shard_sums(off, n) for off, n in SHARDS]
    assert int(got["n"]) == 12 * KEPT == parts[0][3] + parts[1][3] and parts[0][3] != parts[1][3]
    for key, i in (("Y", 0), ("s", 1), ("Q", 2)):
        np.testing.assert_array_equal(got[key], parts[0][i] + parts[1][i])       # the collective is the plain sum of the two ranks
    x, P, m = job()
    whole = shard_sums(0, 12)
    s1 = x.astype(np.float64).sum(axis=(0, 1))
    want = cov_from_sketch(*whole, s1, m)
    have = cov_from_sketch(got["Y"], got["s"], got["Q"], int(got["n"]), s1, m)
    # The two routes add the same 72 terms per entry in different orders: they agree to 72 x 2^-53 sum |term| (the float64 summation bound), and the
    # covariances, sums / 72 minus a product of means, to twice that per sample.
    tol_xt = 2 * 72 * 2.0 ** -53 * np.abs(whole[0]).max()
    tol_tt = 2 * 72 * 2.0 ** -53 * np.abs(whole[2]).max()
    np.testing.assert_allclose(have.cov_xt, want.cov_xt, rtol=0, atol=tol_xt)
    np.testing.assert_allclose(have.cov_tt, want.cov_tt, rtol=0, atol=tol_tt)
    X = x.reshape(72, -1).astype(np.float64)
    S = np.cov(X.T, bias=True)
    P64 = P.reshape(K, -1).astype(np.float64)
    np.testing.assert_allclose(have.cov_tt, P64 @ S @ P64.T, rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(have.cov_xt.reshape(K, -1), P64 @ S, rtol=1e-10, atol=1e-10)


def test_allreduce_cov_sketch_is_the_identity_without_a_process_group():
    import torch
    from lmc_atomi_amd.sharding import allreduce_cov_sketch
    Y = torch.arange(24, dtype=torch.float64).reshape(2, 3, 4)
    s, Q = torch.ones(2, dtype=torch.float64), torch.eye(2, dtype=torch.float64)
    gY, gs, gQ, gn = allreduce_cov_sketch(Y, s, Q, 5)
    assert gY is Y and gs is s and gQ is Q and gn == 5

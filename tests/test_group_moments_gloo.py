"""N > 1 path on CPU: world_size-2 gloo.  The host route of allreduce_sampler_group_moments is allreduce_group_moments (the sampler object itself needs a
GPU): two processes holding 7 and 5 chains of a 12-chain job (chain offsets 0 and 7, 4 groups by global chain id mod 4) sum their S1, S2 and counts for
real, and mcse_from_group_moments of the result equals that of the arrays formed from all 12 chains at once."""
import os
import socket
import subprocess
import sys

import numpy as np

from tests.test_group_moments_api import group_sums

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G, SHAPE, KEPT = 4, (5, 7), 6
SHARDS = ((0, 7), (7, 5))

WORKER = r'''
import os, sys, numpy as np, torch, torch.distributed as dist
sys.path.insert(0, sys.argv[1])
from lmc_atomi_amd.sharding import allreduce_group_moments
from tests.test_group_moments_api import group_sums
from tests.test_group_moments_gloo import G, SHARDS, job_states
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", rank=rank, world_size=world)
off, n = SHARDS[rank]
S1, S2, counts = group_sums(job_states()[:, off:off + n], G, chain_offset=off)
g1, g2, gn = allreduce_group_moments(torch.from_numpy(S1), torch.from_numpy(S2), torch.from_numpy(counts))
assert g1.dtype == torch.float64 and g2.dtype == torch.float64 and tuple(g1.shape) == S1.shape
assert gn.dtype == torch.int64 and not gn.is_cuda and tuple(gn.shape) == (G,)
if rank == 0:
    np.savez(sys.argv[2], S1=g1.numpy(), S2=g2.numpy(), counts=gn.numpy())
dist.destroy_process_group()
'''


def job_states():
    """[KEPT, 12, H, W]: the kept states of the whole job, 100 + N(0, 1)"""
    return 100.0 + np.random.default_rng(77).standard_normal((KEPT, 12) + SHAPE)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_rank_gloo_group_moments_equal_the_unsharded_arrays(tmp_path):
    from lmc_atomi_amd import mcse_from_group_moments
    out = str(tmp_path / "res.npz")
    port = _free_port()
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, "-c", WORKER, ROOT, out], env=env))
    for p in procs:
        assert p.wait(timeout=300) == 0
    got = np.load(out)
    S1, S2, counts = group_sums(job_states(), G)
    np.testing.assert_array_equal(got["counts"], counts)
    np.testing.assert_array_equal(counts, np.full(G, 3 * KEPT))
    parts = [group_sums(job_states()[:, off:off + n], G, chain_offset=off) for off, n in SHARDS]
    assert parts[0][2].tolist() == [2 * KEPT, 2 * KEPT, 2 * KEPT, KEPT] and parts[1][2].tolist() == [KEPT, KEPT, KEPT, 2 * KEPT]      # unequal on every rank
    np.testing.assert_array_equal(got["S1"], parts[0][0] + parts[1][0])          # the collective is the plain sum of the two ranks
    np.testing.assert_array_equal(got["S2"], parts[0][1] + parts[1][1])
    want = mcse_from_group_moments(S1, S2, counts)
    have = mcse_from_group_moments(got["S1"], got["S2"], got["counts"])
    # The two routes add the same 72 terms per entry in different orders, so their sums agree to 72 x 2^-53 relative (the float64 summation bound).
    # mean = S1 / N inherits that.  var = S2 / N - mean^2 is a difference of two numbers near 1e4 (states near 100), each within that bound: an
    # absolute 2 x 2 x 72 x 2^-53 x 1e4 = 3.2e-10 on a variance near 1.  The MCSEs and the ESS are made of differences of group variances and group
    # means (of order 0.3) carrying those absolute errors: 1e-8 relative covers them.
    np.testing.assert_allclose(have.mean, want.mean, rtol=1e-12, atol=0, err_msg="mean")
    np.testing.assert_allclose(have.var, want.var, rtol=0, atol=4 * 72 * 2.0 ** -53 * 1e4, err_msg="var")
    for k in ("mcse_mean", "mcse_var", "ess"):
        np.testing.assert_allclose(getattr(have, k), getattr(want, k), rtol=1e-8, atol=0, err_msg=k)


def test_allreduce_group_moments_is_the_identity_without_a_process_group():
    import torch
    from lmc_atomi_amd.sharding import allreduce_group_moments
    a = torch.arange(24, dtype=torch.float64).reshape(4, 2, 3)
    b = a * a
    n = torch.tensor([3, 3, 2, 2])
    g1, g2, gn = allreduce_group_moments(a, b, n)
    assert g1 is a and g2 is b and gn.dtype == torch.int64 and gn.tolist() == [3, 3, 2, 2]

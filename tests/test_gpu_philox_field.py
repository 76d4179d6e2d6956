"""The device's Philox field (`MYULASampler.noise_field`: `launch_noise`, the quad_normals every step kernel calls) against the oracle's, at every
pixel: |got - ref| <= NOISE_TOL = 2e-5, the error lmc_device.h states for a deviate (hardware log2 / sqrt / sin / cos against exact arithmetic).  The
integer part -- counter words, key halves, the quad index, which lane of a quad a row takes -- has no tolerance: one wrong word gives another deviate, off
by order 1.

Shapes on both sides of a quad boundary and of a wave (H in 1 .. 7, W in 1 .. 257), iterations 0, 1, 2^31, 0xFFFFFFFF, the seed of the Philox cases of
tests/_pixel.py and its half-swapped twin (key0 and key1 exchanged shows), chain offsets 0, 7 and 2^31 - 1 (the chain ids cross the sign bit).

The tails: a field of 8 iterations x 70 000 chains x (4, 4) holds 4.48 million radii; the oracle's integers are scanned for the 64 smallest and the 64
largest u_a among them -- |xi| up to 5.5, where an error of the logarithm is multiplied by the radius, and radii down to 1e-3, where u_a is one float32 step
from 1 -- and those deviates are compared too.  Measured on an MI355X (printed by the test; lmc_device.h and DESIGN section 4.1 hold the figures too):
largest |got - ref| 9.5e-7 overall, 9.5e-7 at |xi| > 4 (554 deviates, up to 5.38), 5.8e-10 at |xi| < 1e-3 (7120 deviates), 4.8e-7 on the 42 small
shapes; the file takes 3 s.  The stated 2e-5 stays the tolerance."""
import numpy as np
import pytest

import _pixel as X
from oracle import lmc_oracle as O

pytestmark = pytest.mark.gpu

SEED_SWAPPED = ((X.SEED_P & 0xFFFFFFFF) << 32) | (X.SEED_P >> 32)
ITERATIONS = (0, 1, 2 ** 31, 0xFFFFFFFF)
N_CHAINS = 3
TAIL_CHAINS, TAIL_ITS, TAIL_SHAPE = 70000, 8, (4, 4)


@pytest.fixture(scope="module")
def la():
    import torch
    assert torch.cuda.is_available()
    import lmc_atomi_amd as la
    return la


def sampler(la, shape, n_chains, seed, chain_offset):
    pf = la.L2(b=np.zeros(shape), sigma=1.0, dims=shape)
    return la.MYULASampler(pf, None, shape, n_chains=n_chains, tau=0.1, gamma=0.5, seed=seed, chain_offset=chain_offset)


@pytest.mark.parametrize("W", (1, 2, 3, 5, 64, 65, 257))
@pytest.mark.parametrize("H", (1, 2, 3, 4, 5, 7))
def test_noise_field_matches_the_oracle_at_every_pixel(la, H, W):
    worst = 0.0
    for seed in (X.SEED_P, SEED_SWAPPED):
        for off in (0, 7, 2 ** 31 - 1):
            with sampler(la, (H, W), N_CHAINS, seed, off) as smp:
                for it in ITERATIONS:
                    got = smp.noise_field(it).cpu().numpy()
                    ref = O.philox_normals(seed, it, off + np.arange(N_CHAINS), H, W)
                    assert got.shape == ref.shape and got.dtype == np.float32
                    d = np.abs(got.astype(np.float64) - ref)
                    k = np.unravel_index(int(np.argmax(d)), d.shape)
                    assert d[k] <= X.NOISE_TOL, (hex(seed), off, hex(it), k, float(d[k]), float(got[k]), float(ref[k]))
                    worst = max(worst, float(d[k]))
    print(f"field {H} x {W}: largest |got - ref| {worst:.3e}")


def test_tails_of_the_field(la):
    """The whole field of 8.96e6 deviates within NOISE_TOL, the 256 deviates behind the 64 smallest and 64 largest u_a among them; prints the largest
    error overall, at |xi| > 4 and at |xi| < 1e-3 (the module's docstring has the figures of an MI355X)."""
    seed, ids = X.SEED_P, np.arange(TAIL_CHAINS)
    nq_w = TAIL_SHAPE[1]       # one quad row-group: the quad index is the column
    refs, uas = [], []
    for it in range(TAIL_ITS):
        c0 = np.broadcast_to(np.arange(nq_w, dtype=np.uint32)[None, :], (TAIL_CHAINS, nq_w))
        o0, o1, o2, o3 = O.philox4x32_10(c0, np.uint32(it), ids.astype(np.uint32)[:, None], np.uint32(O.LMC_PHILOX_STREAM), seed & 0xFFFFFFFF, seed >> 32)
        uas.append(np.stack([o0, o0, o2, o2], axis=1))       # the u_a behind rows 0, 1 (o0) and 2, 3 (o2) of [chain, row, column]
        refs.append(np.stack(O.box_muller(o0, o1) + O.box_muller(o2, o3), axis=1))      # the field, from the integers at hand ...
    assert np.array_equal(refs[-1], O.philox_normals(seed, TAIL_ITS - 1, ids, *TAIL_SHAPE))      # ... as `philox_normals` lays it out
    ua, ref = np.stack(uas), np.stack(refs)
    assert ua.shape == ref.shape and ua[:, :, ::2].size >= 2 ** 22
    order = np.argsort(ua[:, :, ::2], axis=None, kind="stable")
    pick = np.zeros(ua.shape, dtype=bool)
    for idx in np.concatenate([order[:64], order[-64:]]):
        it, ch, pair, col = np.unravel_index(idx, ua[:, :, ::2].shape)
        pick[it, ch, 2 * pair:2 * pair + 2, col] = True       # both deviates of the pair
    assert pick.sum() == 256
    with sampler(la, TAIL_SHAPE, TAIL_CHAINS, seed, 0) as smp:
        got = np.stack([smp.noise_field(it).cpu().numpy() for it in range(TAIL_ITS)])
    d = np.abs(got.astype(np.float64) - ref)
    big, small = np.abs(ref) > 4, np.abs(ref) < 1e-3
    assert big.any() and small.any() and np.abs(ref[pick]).max() > 4
    print(f"tails over {ref.size} deviates: largest |got - ref| {d.max():.3e} overall, {d[big].max():.3e} at |xi| > 4 ({int(big.sum())} deviates, largest |xi| "
          f"{np.abs(ref).max():.3f}), {d[small].max():.3e} at |xi| < 1e-3 ({int(small.sum())}); on the 256 deviates of the 64 smallest and 64 largest u_a "
          f"{d[pick].max():.3e}")
    k = np.unravel_index(int(np.argmax(d)), d.shape)
    assert d[pick].max() <= X.NOISE_TOL, float(d[pick].max())
    assert d[k] <= X.NOISE_TOL, (k, float(d[k]), float(got[k]), float(ref[k]))

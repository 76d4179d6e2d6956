"""Chains across GPUs: one process per GPU, chains sharded by contiguous ranges of GLOBAL chain ids,
no data-path collective; the single collective is one all-reduce (RCCL over xGMI through
``torch.distributed``, backend "nccl"; "gloo" in the CPU tests) of the posterior moment images
{sum x, sum x^2, count} (2*H*W float64 + 1 scalar: 4 MiB at 512x512).

The reference runs exactly one chain in one process (algs.py:564); this module is what lets the
drop-in scale it out.  Because the device noise is keyed by (seed, iteration, global chain id, pixel)
every chain's trajectory is independent of the number of ranks.
"""
from __future__ import annotations

import torch

from .summaries import _check_chain_groups, block_mean_var, mcse_from_group_moments, mean_var_from_moments


def chain_shard(n_total: int, world: int, rank: int):
    """(offset, count) of the contiguous block of global chain ids owned by ``rank``."""
    if not (0 <= rank < world):
        raise ValueError("rank outside world")
    base, rem = divmod(int(n_total), int(world))
    count = base + (1 if rank < rem else 0)
    offset = rank * base + min(rank, rem)
    return offset, count


def allreduce_moments(s1: torch.Tensor, s2: torch.Tensor, count: int, group=None):
    """Sum the per-rank accumulators over all ranks.  Returns (sum, sumsq, count) of the whole job.
    One collective call: the two images and the count travel in one packed float64 buffer."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
        return s1, s2, int(count)
    n = s1.numel()
    # "gloo" (CPU tests, and the two-ranks-on-one-GPU rehearsal of bench.py) reduces host tensors; "nccl" = RCCL reduces in HBM
    dev = torch.device("cpu") if (dist.get_backend(group) == "gloo" and s1.is_cuda) else s1.device
    packed = torch.empty(2 * n + 1, dtype=torch.float64, device=dev)
    packed[:n] = s1.reshape(-1).to(dev)
    packed[n:2 * n] = s2.reshape(-1).to(dev)
    packed[2 * n] = float(count)
    dist.all_reduce(packed, op=dist.ReduceOp.SUM, group=group)
    packed = packed.to(s1.device)
    return packed[:n].reshape(s1.shape), packed[n:2 * n].reshape(s2.shape), int(round(float(packed[2 * n])))


_own_comms = {}      # process group -> ncclComm_t created through the C ABI (lmc_rccl_comm_create)


def rccl_comm(group=None, device=None):
    """An ``ncclComm_t`` (as int) over the ranks of ``group`` with this process's GPU as its rank, for the C-ABI collective
    ``lmc_allreduce_moments``.  Preferred: the communicator ``torch.distributed``'s "nccl" (= RCCL) backend already holds for
    ``device``; if this PyTorch does not expose it, one is created through the C ABI (``lmc_rccl_unique_id`` on rank 0, the 128 bytes
    broadcast with ``torch.distributed``, ``lmc_rccl_comm_create`` on every rank) and cached.  Collective: call on every rank."""
    import ctypes as C
    import torch.distributed as dist
    from . import _capi, _dev
    import os
    pg = group if group is not None else dist.group.WORLD
    dev = _dev.device(device)
    if os.environ.get("LMC_RCCL_COMM", "torch") != "own":
        try:
            with torch.cuda.device(dev):           # the accessor answers for the CURRENT device
                ptr = int(pg._get_backend(dev)._comm_ptr())
            if ptr:
                return ptr
        except Exception:   # older / different PyTorch: no accessor -- fall through to a communicator of our own
            pass
    key = id(pg)
    if key in _own_comms:
        return _own_comms[key]
    lib = _dev.lib()
    world, rank = dist.get_world_size(group), dist.get_rank(group)
    buf = C.create_string_buffer(_capi.RCCL_UNIQUE_ID_BYTES)
    if rank == 0:
        _capi.check(lib.lmc_rccl_unique_id(buf))
    box = [bytes(buf.raw)]
    dist.broadcast_object_list(box, src=dist.get_global_rank(pg, 0) if group is not None else 0, group=group)
    comm = C.c_void_p()
    with torch.cuda.device(dev):
        _capi.check(lib.lmc_rccl_comm_create(C.byref(comm), world, rank, C.create_string_buffer(box[0], _capi.RCCL_UNIQUE_ID_BYTES)))
    _own_comms[key] = int(comm.value)
    return _own_comms[key]


def _route(group, local, nccl, host):
    """The three routes of a sampler's job-wide accumulators: ``local()`` without a process group or with one rank, ``nccl()`` -- the C-ABI
    collective on the RCCL communicator of the group (:func:`rccl_comm`) -- under backend "nccl", else ``host(*local())``, the host all-reduce of what the sampler holds."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
        return local()
    if dist.get_backend(group) == "nccl":
        return nccl()
    return host(*local(), group)


def allreduce_sampler_moments(smp, group=None):
    """Job-wide (sum, sumsq, count) of a sampler's posterior-moment accumulators.  Backend "nccl": ONE ``ncclAllReduce`` issued by
    the library itself (``lmc_allreduce_moments``, C ABI) on the RCCL communicator of the group -- no torch op in between;
    "gloo" (CPU tests, several ranks rehearsed on one GPU): the packed host all-reduce of :func:`allreduce_moments`."""
    return _route(group, smp.moments, lambda: smp.allreduce_moments(rccl_comm(group, smp.device)), allreduce_moments)


def allreduce_sampler_block_moments(smp, scale, group=None):
    """Job-wide (S1, S2, count) of one scale of a sampler's block-moment accumulators (:meth:`MYULASampler.block_moments`), by the same
    routes as :func:`allreduce_sampler_moments`: ``lmc_allreduce_block_moments`` under "nccl", the packed host all-reduce under "gloo"."""
    return _route(group, lambda: smp.block_moments(scale), lambda: smp.allreduce_block_moments(rccl_comm(group, smp.device), scale), allreduce_moments)


def allreduce_counts(counts, count, group=None):
    """Sum integer counters (``torch.int64``, any shape) and a sample count over the ranks of ``group`` on the host: exact, whatever the backend
    (the "gloo" route of :func:`allreduce_sampler_histogram`).  Returns (counts on the device they came from, count)."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
        return counts, int(count)
    packed = torch.cat([counts.detach().reshape(-1).to(device="cpu", dtype=torch.int64), torch.tensor([int(count)], dtype=torch.int64)])
    if dist.get_backend(group) == "nccl":
        packed = packed.to(counts.device)
    dist.all_reduce(packed, op=dist.ReduceOp.SUM, group=group)
    return packed[:-1].reshape(counts.shape).to(counts.device), int(packed[-1])


def allreduce_sampler_histogram(smp, group=None):
    """Job-wide (counts, count) of a sampler's pixel histogram (:meth:`MYULASampler.histogram`), by the same routes as
    :func:`allreduce_sampler_block_moments`: ``lmc_allreduce_histogram`` under "nccl", a host all-reduce of the int64 tensor under "gloo"."""
    return _route(group, smp.histogram, lambda: smp.allreduce_histogram(rccl_comm(group, smp.device)), allreduce_counts)


def allreduce_group_moments(S1, S2, counts, group=None):
    """Sum chain-group moments (:meth:`MYULASampler.group_moments`: ``S1``, ``S2`` float64 ``[G, H, W]``, ``counts`` int64 ``[G]``) over the ranks of
    ``group`` on the host route: the sums in one packed float64 buffer, the counts as integers (exact).  Every rank holds all groups -- the group of a
    chain is its global id mod G -- so the job-wide arrays are plain sums.  The identity without a process group.  Returns (S1, S2) on the device
    they came from and the counts as an int64 CPU tensor."""
    import torch.distributed as dist
    cnt = torch.as_tensor(counts, dtype=torch.int64).detach().reshape(-1).cpu()
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
        return S1, S2, cnt
    n = S1.numel()
    nccl = dist.get_backend(group) == "nccl"
    dev = S1.device if nccl else torch.device("cpu")
    packed = torch.cat([S1.detach().reshape(-1).to(dev, torch.float64), S2.detach().reshape(-1).to(dev, torch.float64)])
    dist.all_reduce(packed, op=dist.ReduceOp.SUM, group=group)
    cnt = cnt.to(dev)
    dist.all_reduce(cnt, op=dist.ReduceOp.SUM, group=group)
    packed = packed.to(S1.device)
    return packed[:n].reshape(S1.shape), packed[n:].reshape(S2.shape), cnt.cpu()


def allreduce_sampler_group_moments(smp, group=None):
    """Job-wide (S1, S2, counts) of a sampler's chain-group moments (:meth:`MYULASampler.group_moments`), by the same routes as
    :func:`allreduce_sampler_block_moments`: ``lmc_allreduce_group_moments`` under "nccl", the host route of :func:`allreduce_group_moments` under "gloo"."""
    return _route(group, smp.group_moments, lambda: smp.allreduce_group_moments(rccl_comm(group, smp.device)), allreduce_group_moments)


def allreduce_cov_sketch(Y, s, Q, n, group=None):
    """Sum the sums of a covariance sketch (:meth:`MYULASampler.cov_sketch`: ``Y`` ``[k, H, W]``, ``s`` ``[k]``, ``Q`` ``[k, k]`` float64, ``n`` the
    samples) over the ranks of ``group``: the three arrays in one packed float64 buffer, the count as an integer (exact).  The sums of chains on
    different ranks add up to the sums of all chains ONLY IF probes and centre are equal on every rank -- same arrays, same
    :func:`lmc_atomi_amd.random_probes` seed; nothing here can check that.  The identity without a process group.  Returns (Y, s, Q) on the device
    they came from and the job-wide count; :func:`lmc_atomi_amd.cov_from_sketch` wants the job-wide ``s1`` (:func:`allreduce_moments`) with them."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
        return Y, s, Q, int(n)
    nccl = dist.get_backend(group) == "nccl"
    dev = Y.device if nccl else torch.device("cpu")
    packed = torch.cat([t.detach().reshape(-1).to(dev, torch.float64) for t in (Y, s, Q)])
    dist.all_reduce(packed, op=dist.ReduceOp.SUM, group=group)
    cnt = torch.tensor([int(n)], dtype=torch.int64, device=dev)
    dist.all_reduce(cnt, op=dist.ReduceOp.SUM, group=group)
    packed = packed.to(Y.device)
    ny, ns = Y.numel(), s.numel()
    return packed[:ny].reshape(Y.shape), packed[ny:ny + ns].reshape(s.shape), packed[ny + ns:].reshape(Q.shape), int(cnt.item())


def allgather_chains(t: torch.Tensor, dim: int = 1, group=None):
    """Concatenate per-rank tensors along their chain dimension in rank order (= global chain order under
    :func:`chain_shard`); ranks may own different numbers of chains.  Used for the diagnostics trace ``[T, C_rank, Q]``
    (a few MB), so that R-hat / ESS run over the chains of the whole job.  Two small collectives (counts, padded payload)."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
        return t
    world = dist.get_world_size(group)
    t = t.movedim(dim, 0).contiguous()
    cnt = torch.tensor([t.shape[0]], dtype=torch.int64, device=t.device)
    counts = [torch.zeros_like(cnt) for _ in range(world)]
    dist.all_gather(counts, cnt, group=group)
    counts = [int(c.item()) for c in counts]
    cmax = max(counts)
    pad = torch.zeros((cmax,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
    pad[:t.shape[0]] = t
    parts = [torch.empty_like(pad) for _ in range(world)]
    dist.all_gather(parts, pad, group=group)
    return torch.cat([p[:c] for p, c in zip(parts, counts)], dim=0).movedim(0, dim)


posterior_mean_var = mean_var_from_moments


class ShardedResult(tuple):
    """What :func:`sharded_myula` returns: the tuple it has always returned -- ``(mean, var, count, state)``, then the scales when ``moment_scales``
    is given, then the histogram when ``hist_bins`` is given, so its length depends on the keywords -- with every part also under a name that does
    not: ``.mean``, ``.var``, ``.count``, ``.state``, ``.scales`` (``{}`` when not asked for) and ``.hist`` (``None`` when not asked for).  ``chain_groups`` adds nothing to the tuple: its job-wide
    results are ``.mcse_mean``, ``.mcse_var``, ``.ess`` and ``.group_counts`` (``None`` when not asked for)."""

    def __new__(cls, items, mean, var, count, state, scales, hist, groups=None):
        self = super().__new__(cls, items)
        self.mean, self.var, self.count, self.state, self.scales, self.hist = mean, var, count, state, scales, hist
        self.mcse_mean, self.mcse_var, self.ess, self.group_counts = groups if groups is not None else (None, None, None, None)
        return self


def sharded_myula(proxf, proxg, dims, n_chains_total, x0, tau, gamma, epsg=1.0, niter=10, seed=0,
                  burn_in=0, thin=1, group=None, device=None, moment_scales=None, hist_bins=None,
                  hist_range=None, chain_groups=None):
    """Run ``n_chains_total`` MYULA chains split over the ranks of the default process group (or run
    them all here when torch.distributed is not initialised) and return the job-wide posterior
    (mean, var, count) plus this rank's final states.  With ``moment_scales`` (block sizes out of 2, 4, 8, 16) a fifth value
    follows: ``{scale: (mean, std)}`` of the image averaged over scale x scale blocks, job-wide as well.  With ``hist_bins`` / ``hist_range`` (as
    :class:`MYULASampler` takes them) the job-wide counters of the pixel histogram ``[hist_bins + 2, H, W]`` follow as the last value.  The tuple is a :class:`ShardedResult`: index it
    as before, or -- since its length depends on the keywords -- read ``.mean``, ``.var``, ``.count``, ``.state``, ``.scales`` and ``.hist``.
    ``chain_groups=G`` (as :class:`MYULASampler` takes it; at most ``n_chains_total``) keeps chain-group moments on every rank and returns the job-wide
    Monte-Carlo error maps under ``.mcse_mean``, ``.mcse_var``, ``.ess`` and ``.group_counts`` (:func:`lmc_atomi_amd.mcse_from_group_moments`)."""
    import torch.distributed as dist
    from .algs import MYULASampler
    _check_chain_groups(chain_groups, True, n_chains_total)
    world = dist.get_world_size(group) if (dist.is_available() and dist.is_initialized()) else 1
    rank = dist.get_rank(group) if world > 1 else 0
    if int(n_chains_total) < world:      # every rank sees the same numbers: all of them raise, none is left waiting in the collective
        raise ValueError(f"{n_chains_total} chains cannot be sharded over {world} ranks (every rank needs at least one)")
    offset, count = chain_shard(n_chains_total, world, rank)
    smp = MYULASampler(proxf, proxg, dims, n_chains=count, tau=tau, gamma=gamma, epsg=epsg, seed=seed,
                       chain_offset=offset, moments=True, burn_in=burn_in, thin=thin, device=device, moment_scales=moment_scales,
                       hist_bins=hist_bins, hist_range=hist_range, chain_groups=chain_groups)
    scales = {}
    hist = None
    groups = None
    try:
        smp.set_state(x0)
        smp.step(niter)
        s1, s2, cnt = allreduce_sampler_moments(smp, group)
        for sc in smp.moment_scales:
            S1, S2, n = allreduce_sampler_block_moments(smp, sc, group)
            m, v = block_mean_var(S1, S2, max(n, 1), sc, smp.dims)
            scales[sc] = (m, v.clamp_min(0).sqrt())
        if smp.hist_bins is not None:
            hist, _ = allreduce_sampler_histogram(smp, group)
        if smp.chain_groups is not None:
            G1, G2, gn = allreduce_sampler_group_moments(smp, group)
            r = mcse_from_group_moments(G1, G2, gn)
            groups = (r.mcse_mean, r.mcse_var, r.ess, gn)
        state = smp.get_state()
    finally:
        smp.close()
    mean, var = posterior_mean_var(s1, s2, cnt)
    out = (mean, var, cnt, state, scales) if moment_scales else (mean, var, cnt, state)
    return ShardedResult(out + (hist,) if hist is not None else out, mean, var, cnt, state, scales, hist, groups)

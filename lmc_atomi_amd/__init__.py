"""lmc_atomi_amd -- MI355X-native Langevin-Monte-Carlo inner loop (drop-in for the hot path of
192459/lmc-atomi): hand-written HIP kernels for gfx950 behind a C ABI (include/lmc_atomi.h),
reached from Python through ctypes.  No CPU fallback: the package raises if liblmc_atomi.so
is missing or no GPU is present."""
from . import _capi
from ._capi import LMCError
from .operators import PSF, Convolve2D, Diagonal, FourierSampling, Gradient, Identity, LinearOperator, MultiCoilFourierSampling, PeriodicConvolve2D, Radon, Wavelet2D, irfft2, rfft2
from .proximal import (L1, L2, L21, TV, L2_ncvx_tv, WaveletL1, ProxOperator, fgp_betas, ElementwiseProx, Laplace, UncenteredLaplace, Gaussian,
                       GenGaussian, Huber, SmoothedLaplace, Box, Poisson, HuberLoss, VectorialTV, TGV)
from .algs import (MYULAResult, MYULASampler, MYMALASampler, MoreauYosidaUnadjustedLangevin, MoreauYosidaMetropolisAdjustedLangevin, ULPDASampler,
                   UnadjustedLangevinPrimalDual, block_mean_var, hist_exceedance, hist_quantiles, mean_var_from_moments, pixel_histogram,
                   set_step_variant, set_cg_tolerance, SKROCKSampler, StabilisedLangevin, skrock_coefficients, skrock_step_bound,
                   SAPGResult, EstimatePriorWeight, prior_statistic, sapg_dimension, sapg_update, GroupMCSE, group_moments, mcse_from_group_moments,
                   CovSketch, cov_sketch, cov_from_sketch, random_probes, MultichannelMYULASampler, SplitGibbs, SplitGibbsResult, SplitGibbsSampler,
                   sgs_step_bound, sgs_xstep)

from . import diagnostics, metrics
from .diagnostics import ChainTrace, chain_probes, ess, split_rhat
from .metrics import MetricsCallback, mean_squared_error, peak_signal_noise_ratio, signal_noise_ratio
from .sharding import (allgather_chains, allreduce_cov_sketch, allreduce_group_moments, allreduce_moments, allreduce_sampler_group_moments, allreduce_sampler_block_moments, allreduce_sampler_histogram, allreduce_sampler_moments, chain_shard, posterior_mean_var, rccl_comm,
                       sharded_myula)

__all__ = [
    "diagnostics", "ChainTrace", "chain_probes", "ess", "split_rhat", "allgather_chains",
    "metrics", "MetricsCallback", "mean_squared_error", "peak_signal_noise_ratio", "signal_noise_ratio",
    "allreduce_moments", "allreduce_sampler_moments", "rccl_comm", "chain_shard", "posterior_mean_var", "sharded_myula",
    "LMCError", "Convolve2D", "PSF", "FourierSampling", "MultiCoilFourierSampling", "PeriodicConvolve2D", "Radon", "rfft2", "irfft2", "Diagonal", "Gradient", "Identity", "LinearOperator", "Wavelet2D",
    "L1", "L2", "L21", "TV", "L2_ncvx_tv", "WaveletL1", "Box", "Poisson", "HuberLoss", "ProxOperator", "fgp_betas",
    "MYULASampler", "MYMALASampler", "MoreauYosidaMetropolisAdjustedLangevin", "MYULAResult", "MoreauYosidaUnadjustedLangevin", "ULPDASampler", "UnadjustedLangevinPrimalDual", "mean_var_from_moments", "set_step_variant", "set_cg_tolerance",
    "block_mean_var", "allreduce_sampler_block_moments",
    "pixel_histogram", "hist_quantiles", "hist_exceedance", "allreduce_sampler_histogram",
    "SKROCKSampler", "StabilisedLangevin", "skrock_coefficients", "skrock_step_bound",
    "group_moments", "mcse_from_group_moments", "GroupMCSE", "allreduce_group_moments", "allreduce_sampler_group_moments",
    "cov_sketch", "cov_from_sketch", "CovSketch", "random_probes", "allreduce_cov_sketch",
    "SAPGResult", "EstimatePriorWeight", "prior_statistic", "sapg_dimension", "sapg_update",
    "VectorialTV", "MultichannelMYULASampler", "TGV",
    "SplitGibbsSampler", "SplitGibbs", "SplitGibbsResult", "sgs_step_bound", "sgs_xstep",
]
__version__ = "0.2.0"

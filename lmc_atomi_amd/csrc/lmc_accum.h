// The accumulators over the kept samples of a sampler handle: the pixel moments and, each optional, the block moments, the pixel histogram, the
// chain-group moments and the covariance sketch.  Every buffer's element count is stated ONCE, in elems() of its struct: set, get, reset, release
// (lmc_accum.hip) and the all-reduces (lmc_rccl.hip) all take it from there.
#pragma once
#include <cstddef>
#include <cstdint>

#include "lmc_launch.h"

namespace lmc::host {

// multi-scale moments (lmc_sampler_set_moment_scales): one packed buffer of the sum b^2 arrays of the enabled scales; scales.s2[i] points into it
struct BlockMoments {
  double* buf = nullptr;
  bool on[4] = {false, false, false, false};   // by scale 2, 4, 8, 16
  lmc::BlockScales scales{};
  static int index(int32_t scale) { return scale == 2 ? 0 : scale == 4 ? 1 : scale == 8 ? 2 : scale == 16 ? 3 : -1; }
  // the blocks of scale 2 << i: [ceil(H / s)][ceil(W / s)]
  static size_t blocks(int H, int W, int i) { const size_t sc = (size_t)2 << i; return ((H + sc - 1) / sc) * ((W + sc - 1) / sc); }
  size_t elems(int H, int W) const { size_t n = 0; for (int i = 0; i < 4; ++i) if (on[i]) n += blocks(H, W, i); return n; }
  void release();
};

// pixel histograms (lmc_sampler_set_histogram): counts [bins + 2][H][W], NULL = off; lo / scale [H][W] are the handle's copies
struct Histogram {
  int bins = 0;
  unsigned long long* counts = nullptr;
  float* lo = nullptr;
  float* scale = nullptr;
  unsigned long long* packed = nullptr;   // [elems + 1]: the send / receive buffer of lmc_allreduce_histogram
  size_t elems(int H, int W) const { return (size_t)(bins + 2) * H * W; }
  void release();
};

// chain-group moments (lmc_sampler_set_chain_groups): sums = {A [n][H][W], B [n][H][W]} in one buffer, NULL = off
struct ChainGroups {
  int n = 0;
  double* sums = nullptr;
  double* packed = nullptr;               // [elems + n]: the send / receive buffer of lmc_allreduce_group_moments
  size_t elems(int H, int W) const { return 2 * (size_t)n * H * W; }
  void release();
};

// covariance sketch (lmc_sampler_set_cov_sketch): buf = {Y [k][H][W], s [k], Q [k][k]} in one buffer, NULL = off; probes [k][H][W] and center [H][W]
// (NULL = 0) are the handle's copies, ws the workspace of lmc_cov_sketch.hip
struct CovSketch {
  int k = 0;
  double* buf = nullptr;
  float* probes = nullptr;
  float* center = nullptr;
  void* ws = nullptr;
  size_t y_elems(int H, int W) const { return (size_t)k * H * W; }                              // Y alone: s follows it, then Q
  size_t elems(int H, int W) const { return y_elems(H, W) + (size_t)k + (size_t)k * k; }
  void release();
};

struct Accumulators {
  int C = 0, H = 0, W = 0;                // the handle's chains and image (alloc)
  int64_t chain_offset = 0;
  uint64_t count = 0;
  double* s1 = nullptr;
  double* s2 = nullptr;
  double* packed = nullptr;               // [packed_elems]: the send / receive buffer of lmc_allreduce_moments and lmc_allreduce_block_moments
  BlockMoments blocks;
  Histogram hist;
  ChainGroups groups;
  CovSketch cov;

  size_t pixels() const { return (size_t)H * W; }
  size_t packed_elems() const { return 2 * pixels() + 1; }   // {sum, sumsq, count}; the blocks of a scale are fewer than the pixels

  // s1, s2 ([H][W] doubles each, zeroed) of a sampler created with moments on
  hipError_t alloc(int C_, int64_t chain_offset_, int H_, int W_);
  hipError_t need_packed() { return packed ? hipSuccess : hipMalloc(&packed, sizeof(double) * packed_elems()); }
  void release();                          // every buffer, the optional ones included
  int reset(hipStream_t st);               // every accumulator to zero, count = 0; LMC_OK or the recorded failure
  // n[g] of the chain-group moments: kept iterations x chains of the handle in group g, into counts[groups.n]
  void group_counts(uint64_t* counts) const {
    const uint64_t G = (uint64_t)groups.n, kept_its = count / (uint64_t)C;
    const uint64_t first = (uint64_t)chain_offset % G;         // the group of local chain 0
    for (uint64_t g = 0; g < G; ++g) {
      const uint64_t c0 = (g + G - first) % G;                 // the first local chain of group g, then every G-th
      counts[g] = kept_its * (c0 < (uint64_t)C ? ((uint64_t)C - c0 + G - 1) / G : 0);
    }
  }

  // the launches that follow the moment reduction of a kept iterate: the histogram, the chain-group moments, then the covariance sketch (none has a
  // paced twin: beside a step kernel they are the in-line forms on the side stream).
  // ONE workspace (T and the slab partials of the sketch) per handle is enough: a handle never has reduce_more in flight on two streams at once.
  // The side stream runs its batches in order, both iterates of a pair launch (x_mid and the result) go to the same stream one after the other,
  // and an in-line reduction on the caller's stream first joins every pending side batch (SideMoments::keep) -- the rule the shared accumulators
  // s1 / s2 already impose.
  hipError_t reduce_more(hipError_t e, const float* x, hipStream_t st);
  // the kept iterate x into the accumulators: the fused multi-scale reduction when scales are enabled, else exactly the launches of before;
  // then what reduce_more adds
  hipError_t reduce(const float* x, hipStream_t st);
  hipError_t reduce_bg(const float* x, int n_wg, hipStream_t st);
};

}  // namespace lmc::host

// Posterior covariance sketch (include/lmc_atomi.h, lmc_sampler_set_cov_sketch): three launches over a kept iterate x[C][H][W] that ADD, for k <= 32
// probe images P[k][H][W] and a centre m[H][W] (NULL = 0), with d_c = x_c - m (fp32) and t_c[j] = <P_j, d_c>,
//   Y[j][p] += sum_c t_c[j] d_c[p]     s[j] += sum_c t_c[j]     Q[j][l] += sum_c t_c[j] t_c[l]          (float64)
// Both passes over x are skinny GEMMs on the fp32-input MFMA (v_mfma_f32_32x32x2_f32: bit for bit an ordered fmaf chain, one rounding per
// product), with the operands going from global memory straight into the MFMA lanes -- no LDS (on the side stream the pass shares a compute unit
// with the pipe kernel, whose LDS is full), no scratch.
//
//  1. cov_sketch_project_kernel: T = D P^T.  A wave owns 32 chains x one slab of <= 2048 pixels and all probes (k padded to 32 by zero rows).  Lane
//     l = 32 h + r holds chain r of the tile as the A operand and probe r as the B operand and loads, per trip, the 4 pixels q + 4 h .. q + 4 h + 3
//     of both rows: 4 MFMAs of k-depth 2 (the halves) take the 8 pixels of a trip.  The fp32 32 x 32 slab partial goes to the workspace.  A
//     float4 form (image size % 4 == 0, 16-byte aligned arrays) and a scalar-load form with the same order of operations, hence the same bits.
//  2. cov_sketch_finish_kernel, launched twice.  Phase 0: one thread per (chain, probe) sums its slab partials in ascending slab order in float64
//     into T[C][32] and leaves the fp32 rounding of it for pass 3.  Phase 1: one wave per probe j adds row j of Q and s[j]: lane 32 h + l walks the
//     chains of parity h in ascending order, the two halves are added, one read-add-write per element.
//  3. cov_sketch_update_kernel: Y += T^T D.  A wave owns all probes x 128 pixels (four column tiles, accumulators in registers: lane 32 h + r holds the
//     pixels 4 r .. 4 r + 3, tile e is the pixels 4 r + e) and walks the chains in pairs (lane half h = chain parity): x is read coalesced, 512
//     consecutive bytes per half wave, T (fp32) from cache.  fp32 runs of at most 1024 chains; every run sum is added to the wave's part of Y with
//     ONE float64 read-add-write (32 bytes per lane and probe).  The same two forms.
//
// No float atomics, one owner per output element and launch: equal runs give equal bits.  Tails (chains past C, probes past k, pixels past the
// image) are zero operands of the same MFMAs, not skipped work.  Launches that share Y, s, Q or the workspace must be ordered (one stream).
//
// Per kept iterate at k = 32: 2 x 4 C HW bytes of x read, 4 k HW (probes) + 8 HW (centre, twice) read, 16 k HW of Y traffic, and the slab partials
// (4 x 32 C HW / 2048 written and read once); 4 x 32 C HW FLOP (the padding to 32 probes is computed whatever k is).
#include "lmc_device.h"
#include "lmc_launch.h"

namespace lmc {

namespace {
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr unsigned kCovSlab = 2048;     // pixels of one fp32 run of the projection
constexpr unsigned kCovRun = 1024;      // chains of one fp32 run of the update

struct CovLayout {
  size_t cpad, nslab, off_tf, off_part, bytes;
};
CovLayout cov_layout(int64_t C, size_t img) {
  CovLayout L;
  L.cpad = ((size_t)C + 31) & ~(size_t)31;
  L.nslab = (img + kCovSlab - 1) / kCovSlab;
  L.off_tf = sizeof(double) * 32 * L.cpad;                         // T (float64) first, then its fp32 rounding, then the slab partials
  L.off_part = L.off_tf + sizeof(float) * 32 * L.cpad;
  L.bytes = L.off_part + sizeof(float) * 32 * L.cpad * L.nslab;
  return L;
}
}  // namespace

// row of the 32 x 32 MFMA result held in register `reg` of lane half h (the column is lane & 31)
__device__ __forceinline__ unsigned cov_row(unsigned reg, unsigned h) { return (reg & 3u) + 8u * (reg >> 2) + 4u * h; }

// part[slab][Cpad][32]: one wave = chain tile `tile`, pixel slab `slab`.  VEC: img % 4 == 0 and x, P, m 16-byte aligned.
template <bool VEC>
__global__ __launch_bounds__(256) void cov_sketch_project_kernel(const float* __restrict__ x, size_t C, size_t img, unsigned k,
                                                                 const float* __restrict__ P, const float* __restrict__ m, size_t cpad,
                                                                 size_t nslab, float* __restrict__ part) {
  const size_t unit = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const size_t ntile = cpad >> 5;
  if (unit >= ntile * nslab) return;                                // wave-uniform
  const size_t tile = unit / nslab, slab = unit - tile * nslab;
  const unsigned lane = threadIdx.x & 63u, r = lane & 31u, h = lane >> 5;
  const size_t chain = tile * 32 + r;
  const bool cv = chain < C, pv = r < k;
  const float* __restrict__ xr = x + (cv ? chain : C - 1) * img;    // a row inside the arrays whatever the tail
  const float* __restrict__ pr = P + (size_t)(pv ? r : k - 1) * img;
  const size_t q0 = slab * kCovSlab, q1 = q0 + kCovSlab < img ? q0 + kCovSlab : img;
  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  // One short trip per turn, the loads predicated.  Measured at 512 x 512 x 1024, k = 32: 0.54 ms; trips of 32 pixels (64 contiguous bytes per lane),
  // with one, two or four of them in flight and unconditional clamped loads, took 0.66 ms each -- the pass is not bound by load latency.
  for (size_t q = q0; q < q1; q += 8) {
    const size_t p = q + 4 * h;
    float d[4], b[4];
    if constexpr (VEC) {
      const bool in = p < q1;
      float4 xv = make_float4(0.f, 0.f, 0.f, 0.f), mv = xv, bv = xv;
      if (in && cv) xv = *reinterpret_cast<const float4*>(xr + p);
      if (in && cv && m) mv = *reinterpret_cast<const float4*>(m + p);
      if (in && pv) bv = *reinterpret_cast<const float4*>(pr + p);
      d[0] = xv.x - mv.x; d[1] = xv.y - mv.y; d[2] = xv.z - mv.z; d[3] = xv.w - mv.w;
      b[0] = bv.x; b[1] = bv.y; b[2] = bv.z; b[3] = bv.w;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const bool in = p + e < q1;
        const float xv = in && cv ? xr[p + e] : 0.f;
        const float mv = in && cv && m ? m[p + e] : 0.f;
        d[e] = xv - mv;
        b[e] = in && pv ? pr[p + e] : 0.f;
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(d[e], b[e], acc, 0, 0, 0);
  }
  float* __restrict__ out = part + (slab * cpad + tile * 32) * 32;
#pragma unroll
  for (unsigned i = 0; i < 16; ++i) out[(size_t)cov_row(i, h) * 32 + r] = acc[i];      // row = chain of the tile, column = probe
}

// phase 0: T[c][j] = sum over slabs (ascending) of part[slab][c][j], Tf = its fp32 rounding; one thread per element of the padded [Cpad][32].
// phase 1: block j (one wave) adds s[j] and Q[j][0 .. k-1] from T.
__global__ __launch_bounds__(256) void cov_sketch_finish_kernel(int phase, size_t C, unsigned k, size_t cpad, size_t nslab,
                                                                const float* __restrict__ part, double* __restrict__ T, float* __restrict__ Tf,
                                                                double* __restrict__ s, double* __restrict__ Q) {
  if (phase == 0) {
    const size_t n = cpad * 32, g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n) return;
    double t = 0.;
#pragma unroll 8
    for (size_t sl = 0; sl < nslab; ++sl) t += (double)part[sl * n + g];
    T[g] = t;
    Tf[g] = (float)t;
    return;
  }
  const unsigned j = blockIdx.x, lane = threadIdx.x & 63u, l = lane & 31u, h = lane >> 5;
  const double* __restrict__ Tc = T;
  double q = 0., a = 0.;
#pragma unroll 4
  for (size_t c = h; c < C; c += 2) {
    const double tj = Tc[c * 32 + j], tl = Tc[c * 32 + l];
    a += tj;
    q += tj * tl;
  }
  q += __shfl_xor(q, 32);                                           // even chains + odd chains: the same bits in both halves
  a += __shfl_xor(a, 32);
  if (h == 0 && l < k) Q[(size_t)j * k + l] += q;
  if (lane == 0) s[j] += a;
}

// Y[j][p] += sum_c Tf[c][j] (x[c][p] - m[p]): one wave = pixels 128 u .. 128 u + 127, all probes.  Lane 32 h + r holds the pixels 4 r .. 4 r + 3 of
// that range (one 16-byte load per chain), column tile e is the pixels 4 r + e.  VEC: img % 4 == 0 and x, m, Y 16-byte aligned.
template <bool VEC>
__global__ __launch_bounds__(256) void cov_sketch_update_kernel(const float* __restrict__ x, size_t C, size_t img, unsigned k,
                                                                const float* __restrict__ m, const float* __restrict__ Tf, double* __restrict__ Y) {
  const size_t unit = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (unit * 128 >= img) return;                                    // wave-uniform
  const unsigned lane = threadIdx.x & 63u, r = lane & 31u, h = lane >> 5;
  const size_t pb = unit * 128 + 4 * r;
  bool in[4];
  float mv[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    in[e] = pb + e < img;                                           // VEC: all four or none
    mv[e] = m && in[e] ? m[pb + e] : 0.f;
  }
  for (size_t cb = 0; cb < C; cb += kCovRun) {
    const size_t ce = cb + kCovRun < C ? cb + kCovRun : C;
    f32x16 acc[4];
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[e][i] = 0.f;
    // four chain pairs per turn, unrolled by hand (a loop with MFMAs takes no remainder loop); a pair past the run is all zero operands
    for (size_t cq = cb; cq < ce; cq += 8)
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const size_t c = cq + 2 * u + h;
      const bool cv = c < ce;
      const size_t cc = cv ? c : ce - 1;                            // unconditional loads inside the arrays; the tail becomes a zero operand
      const float a = cv ? Tf[cc * 32 + r] : 0.f;
      float b[4];
      if constexpr (VEC) {
        const float4 xv = *reinterpret_cast<const float4*>(x + cc * img + (in[0] ? pb : 0));
        b[0] = xv.x; b[1] = xv.y; b[2] = xv.z; b[3] = xv.w;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) b[e] = x[cc * img + (in[e] ? pb + e : 0)];
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, cv && in[e] ? b[e] - mv[e] : 0.f, acc[e], 0, 0, 0);
    }
    // the run sums into Y: row = probe, column tile e = pixel pb + e
#pragma unroll
    for (unsigned i = 0; i < 16; ++i) {
      const unsigned j = cov_row(i, h);
      if (j >= k) continue;
      double* __restrict__ y = Y + (size_t)j * img + pb;
      if constexpr (VEC) {
        if (in[0]) {
          double2* y2 = reinterpret_cast<double2*>(y);
          const double2 u = y2[0], w = y2[1];
          y2[0] = make_double2(u.x + (double)acc[0][i], u.y + (double)acc[1][i]);
          y2[1] = make_double2(w.x + (double)acc[2][i], w.y + (double)acc[3][i]);
        }
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (in[e]) y[e] += (double)acc[e][i];
      }
    }
  }
}

size_t cov_sketch_workspace_bytes(int64_t C, int H, int W, int k) {
  if (C < 1 || H < 1 || W < 1 || k < 1 || k > 32) return 0;
  return cov_layout(C, (size_t)H * W).bytes;
}

// Y[k][H][W], s[k], Q[k][k] += the sketch of x[C][H][W]; ws: cov_sketch_workspace_bytes, 16-byte aligned.  1 <= k <= 32 (the caller checks).
hipError_t launch_cov_sketch(const float* x, int64_t C, int H, int W, int k, const float* P, const float* m, double* Y, double* s, double* Q, void* ws,
                             hipStream_t st) {
  if (C < 1 || H < 1 || W < 1 || k < 1 || k > 32 || (reinterpret_cast<uintptr_t>(ws) & 15)) return hipErrorInvalidValue;
  const size_t img = (size_t)H * W;
  const CovLayout L = cov_layout(C, img);
  double* T = static_cast<double*>(ws);
  float* Tf = reinterpret_cast<float*>(static_cast<char*>(ws) + L.off_tf);
  float* part = reinterpret_cast<float*>(static_cast<char*>(ws) + L.off_part);
  const size_t pblocks = ((L.cpad >> 5) * L.nslab + 3) / 4, fblocks = (L.cpad * 32 + 255) / 256, ublocks = ((img + 127) / 128 + 3) / 4;
  if (pblocks > 0x7fffffffu || fblocks > 0x7fffffffu || ublocks > 0x7fffffffu) return hipErrorInvalidValue;
  const uintptr_t bits = reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(P) | reinterpret_cast<uintptr_t>(m);
  if ((img & 3) == 0 && (bits & 15) == 0)
    hipLaunchKernelGGL(cov_sketch_project_kernel<true>, dim3((unsigned)pblocks), dim3(256), 0, st, x, (size_t)C, img, (unsigned)k, P, m, L.cpad, L.nslab, part);
  else
    hipLaunchKernelGGL(cov_sketch_project_kernel<false>, dim3((unsigned)pblocks), dim3(256), 0, st, x, (size_t)C, img, (unsigned)k, P, m, L.cpad, L.nslab, part);
  hipLaunchKernelGGL(cov_sketch_finish_kernel, dim3((unsigned)fblocks), dim3(256), 0, st, 0, (size_t)C, (unsigned)k, L.cpad, L.nslab, part, T, Tf, s, Q);
  hipLaunchKernelGGL(cov_sketch_finish_kernel, dim3((unsigned)k), dim3(64), 0, st, 1, (size_t)C, (unsigned)k, L.cpad, L.nslab, part, T, Tf, s, Q);
  if ((img & 3) == 0 && ((bits | reinterpret_cast<uintptr_t>(Y)) & 15) == 0)
    hipLaunchKernelGGL(cov_sketch_update_kernel<true>, dim3((unsigned)ublocks), dim3(256), 0, st, x, (size_t)C, img, (unsigned)k, m, Tf, Y);
  else
    hipLaunchKernelGGL(cov_sketch_update_kernel<false>, dim3((unsigned)ublocks), dim3(256), 0, st, x, (size_t)C, img, (unsigned)k, m, Tf, Y);
  return hipGetLastError();
}

}  // namespace lmc

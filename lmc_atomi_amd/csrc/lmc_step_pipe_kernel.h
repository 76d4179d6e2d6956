// Fused MYULA update with the isotropic-TV prox (K FGP dual iterations), "pipe" variant:
//     out = a*x - t*sigma_f H^T(Hx - y) + b*prox_{gamma TV}(x) + s*xi                      (algs.py:569)
//
// Same row pipeline as lmc_step_split.hip (stage k runs on row t-E-2k, one barrier per tick) but laid out the other way
// round: a wavefront owns the FULL WIDTH of the image (lane = PXL consecutive pixels, W <= 64*PXL) and the pipeline STAGES
// are spread over the wavefronts of the workgroup:
//   wave 0      "L": HBM load of row t -> x ring (LDS); blur-gradient pipeline on the ring, one row ahead of the output
//   wave 1..NT  "T": two TV stages each (2j-1, 2j); stage outputs handed to the next wave through LDS (parity double
//                    buffer, read one tick later -- the latency a stage boundary has anyway)
//   wave NT+1   "C": final primal step x - gamma div(rr^K, ss^K), combine, HBM store
//   wave NT+2   "N": Philox normals of the next quad row-group into an LDS slab (read by C four ticks later)
// Because a wave spans the image width, horizontal neighbours are in the same lane (7 of 8) or one wave-shift DPP move
// away (2 per stage per PXL pixels): no row-edge ghost exchange, no per-pixel DPP.  One workgroup = one chain.
#pragma once
#include "lmc_device.h"
#include "lmc_launch.h"

namespace lmc {

// Timing experiments of round 2 that were measured and removed again (git history): stage k1's hand-off reads before stage
// k2's arithmetic (1.876 ms), the same with stage k2's stores interleaved with its arithmetic behind scheduling barriers (1.799 ms), and the
// two-team layout -- 16 waves of 4 pixels per lane, the teams' roles on complementary SIMDs, the column seam through LDS; exact -- at commit
// 4183175 (1.811 ms).  Base: 1.749 ms.

// The kernels that run the stages with the momentum folded into the projection scale (pipe_stage, FOLD): one fixed-count launch from the zero dual state
// with the isotropic projection
__host__ __device__ constexpr bool pipe_fold(bool chain, bool warm, bool rt, bool aniso) { return !chain && !warm && !rt && !aniso; }
// The kernels that fold the wave shifts of a stage into the differences that use them (sub_left_pair, right_pair_sub) and select the row-edge
// coefficient in scalar registers (pipe_cdown): the folded-momentum kernels, but for the two-iteration launches without a blur (K = 2, KT = 0, aligned
// rows, 4 and 8 pixels per lane), which would take 6 / 12 more VGPRs -- a block of 8 more -- and for the 7-tap kernels, which ran 1.5 % slower with the
// folded shifts (512 x 512, 1024 chains: 1.748 against 1.723 ms per step; their L wave is the long one).  That one measurement is of the one-team kernel at
// 8 pixels per lane; the 7-tap kernels at 4 pixels per lane are kept out with it UNMEASURED (the 5-tap layout at 4 pixels per lane gained the most,
// 3.7 %, so they may well gain too: a lead, not a finding).  Those keep the built pairs and the parent's instruction streams
// (tests/golden/pipe_shift_gated_code_hashes.txt).
__host__ __device__ constexpr bool pipe_shift(bool fold, int k, int kt) { return fold && !(k == 2 && kt == 0) && kt != 7; }

template <int K>
struct PipeGeom {
  static constexpr int D = (2 * K + 2 > 10) ? 2 * K + 2 : 10;   // output row lag: o = t - D
  static constexpr int E = D - (2 * K + 2);                     // extra lag of the TV pipeline
  static constexpr int RB = D + 1;                              // x ring rows: t-D .. t
  static constexpr int NT = (K + 1) / 2;                        // TV waves (two stages each; odd K: the last one runs stage K alone)
};

template <int K, int PXL, bool CHAIN = false, int TEAMS = 1>
struct PipeLds {
  static constexpr int BW = 64 * PXL;
  // two-team layout (TEAMS = 2): the teams' copies of a row sit side by side (row pitch RP = 2 BW), so that a wave reaches the other
  // team's copy of the row it works on at a fixed distance of BW floats -- a constant offset of the same address
  static constexpr int RP = TEAMS * BW;
  static constexpr int o_x = 0;                                        // [RB][RP]
  static constexpr int o_hand = o_x + PipeGeom<K>::RB * RP;            // [NT][2][4][RP]: rr, ss, p, q of the wave's last stage (pipe_fold kernels: rr, ss, u, v; DualRow)
  // chained launches (more than K dual iterations): the last boundary (T_NT -> C) carries rr, ss only, [2][2][BW], and the 8*BW
  // saved hold the dual state of the previous launch for stage 1, [2][4][BW] (LDS budget: 160 KB)
  static constexpr int o_hand_last = o_hand + (PipeGeom<K>::NT - 1) * 8 * RP;
  static constexpr int o_hand0 = o_hand_last + 4 * RP;
  static constexpr int o_g = CHAIN ? o_hand0 + 8 * RP : o_hand + PipeGeom<K>::NT * 2 * 4 * RP;    // [2][RP] gradient of the output row
  static constexpr int SLAB = 2 * 4 * PXL * 64;
  static constexpr int o_slab = o_g + 2 * RP;                          // [TEAMS][2][4][PXL][64] normals of this and the next quad row-group
  // seam records of the two-team layout (PipeSeam below), zero-filled with the rows
  static constexpr int o_seam = o_slab + TEAMS * SLAB;
  static constexpr int total = o_seam + (TEAMS == 2 ? 64 : 0);
};

// LDS rows: a lane's PXL pixels are held as NP = PXL / 2 pixel pairs (i, i + NP) -- see "Packed fp32" below -- and a row stores them pair by pair:
// slot s of a lane holds its pixel (s >> 1) + NP * (s & 1) (PXL = 4: pixels 0, 2, 1, 3; PXL = 8: 0, 4, 1, 5 | 2, 6, 3, 7), slot s of lane l at
// (s >> 2) * 256 + 4 * l + (s & 3), so that every 16-byte access of a wave is contiguous and returns two whole pairs.  This holds for every row of
// every pipe kernel (ring, hand-offs, gradient row, state hand-over); everything in HBM is in natural order.  prow_load / prow_store address a row by
// PIXEL (the permutation is a renaming of registers), pairs_load / pairs_store by pair.
template <int PXL>
__host__ __device__ constexpr int pipe_slot(int k) { return k < PXL / 2 ? 2 * k : 2 * (k - PXL / 2) + 1; }      // pixel of a lane -> slot
template <int PXL>
__host__ __device__ constexpr int pipe_pixel(int s) { return (s >> 1) + (PXL / 2) * (s & 1); }                // slot -> pixel of a lane
template <int PXL>
__host__ __device__ constexpr int pipe_slot_offset(int k) { return (pipe_slot<PXL>(k) >> 2) * 256 + (pipe_slot<PXL>(k) & 3); }   // of lane 0, in floats
template <int PXL>
__device__ __forceinline__ void prow_load(float (&v)[PXL], const float* row, int lane) {
#pragma unroll
  for (int g = 0; g < PXL / 4; ++g) {
    const float4 q = *reinterpret_cast<const float4*>(row + g * 256 + lane * 4);
    v[pipe_pixel<PXL>(4 * g)] = q.x; v[pipe_pixel<PXL>(4 * g + 1)] = q.y; v[pipe_pixel<PXL>(4 * g + 2)] = q.z; v[pipe_pixel<PXL>(4 * g + 3)] = q.w;
  }
}
template <int PXL>
__device__ __forceinline__ void prow_store(float* row, int lane, const float (&v)[PXL]) {
#pragma unroll
  for (int g = 0; g < PXL / 4; ++g)
    *reinterpret_cast<float4*>(row + g * 256 + lane * 4) =
        make_float4(v[pipe_pixel<PXL>(4 * g)], v[pipe_pixel<PXL>(4 * g + 1)], v[pipe_pixel<PXL>(4 * g + 2)], v[pipe_pixel<PXL>(4 * g + 3)]);
}

// Packed fp32: gfx950 issues one wave64 VALU instruction per 4 cycles per SIMD, and v_pk_fma/mul/add_f32 process two floats
// per lane in that slot.  The waves therefore work on pixel PAIRS held in even-aligned register pairs, and pair i of a lane is its pixels
// (i, i + NP): the left neighbours of pair i are then pair i - 1 as it stands, the right neighbours pair i + 1, and only the two pairs at the
// ends of a lane are built -- {from_left(pair[NP-1].y), pair[NP-1].x} and {pair[0].y, from_right(pair[0].x)}, the wave shift a stage makes
// anyway plus one move each, whatever PXL is.  (Pairs of ADJACENT pixels (2i, 2i + 1), the layout before, make every neighbour operand straddle
// two register pairs: one VALU instruction in six of a TV wave was a move that re-paired them.)  max / rsq stay scalar.
typedef float v2f __attribute__((ext_vector_type(2)));
typedef float v4f __attribute__((ext_vector_type(4)));      // what the non-temporal builtins take (float4 is a class)
__device__ __forceinline__ v2f pk_fma(v2f a, v2f b, v2f c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ v2f pk_set(float a) { return v2f{a, a}; }
// projection onto [-1, 1] per component (the dual ball of the anisotropic TV prior)
__device__ __forceinline__ v2f pipe_clamp1(v2f a) { return v2f{__builtin_amdgcn_fmed3f(a.x, -1.f, 1.f), __builtin_amdgcn_fmed3f(a.y, -1.f, 1.f)}; }
// Poisson data term, two pixels: rho(u) = 1 - y t (1 - t min(u, 0)), t = 1 / (max(u, 0) + beta) (pois_rho, lmc_device.h; lmc_atomi.h).  The reciprocal
// is v_rcp_f32 with one Newton step (two packed fmas; half an ulp of t) instead of the IEEE division sequence: the L wave is the short wave every
// other one waits for at the barrier.
__device__ __forceinline__ v2f pois_rho2(v2f u, v2f y, v2f beta) {
  const v2f den = v2f{fmaxf(u.x, 0.f), fmaxf(u.y, 0.f)} + beta, un = v2f{fminf(u.x, 0.f), fminf(u.y, 0.f)};
  const v2f t0 = v2f{__builtin_amdgcn_rcpf(den.x), __builtin_amdgcn_rcpf(den.y)};
  const v2f t = pk_fma(t0, pk_fma(-den, t0, pk_set(1.f)), t0);
  return pk_fma(-(y * t), pk_fma(-t, un, pk_set(1.f)), pk_set(1.f));
}
// projection of the primal iterate onto [lo, hi] (the box-constrained prior: one v_med3_f32 per pixel; infinite ends pass through)
__device__ __forceinline__ v2f pipe_clamp_box(v2f a, float lo, float hi) { return v2f{__builtin_amdgcn_fmed3f(a.x, lo, hi), __builtin_amdgcn_fmed3f(a.y, lo, hi)}; }

template <int NP>   // NP = PXL / 2 pairs
__device__ __forceinline__ void pairs_load(v2f (&v)[NP], const float* row, int lane) {
#pragma unroll
  for (int g = 0; g < NP / 2; ++g) {
    const float4 q = *reinterpret_cast<const float4*>(row + g * 256 + lane * 4);
    v[2 * g] = v2f{q.x, q.y};
    v[2 * g + 1] = v2f{q.z, q.w};
  }
}
template <int NP>
__device__ __forceinline__ void pairs_store(float* row, int lane, const v2f (&v)[NP]) {
#pragma unroll
  for (int g = 0; g < NP / 2; ++g)
    *reinterpret_cast<float4*>(row + g * 256 + lane * 4) = make_float4(v[2 * g].x, v[2 * g].y, v[2 * g + 1].x, v[2 * g + 1].y);
}

// pixel k of a lane (natural order) in its pair array
template <int NP>
__device__ __forceinline__ float pair_px(const v2f (&v)[NP], int k) { return k < NP ? v[k].x : v[k - NP].y; }
// The neighbour rows of pair i: the pair beside it, and at the ends of a lane the one pair that is built.  `from_left` = pixel NP-1's
// value of the lane to the left (v[NP-1].y shifted), `from_right` = pixel 0's value of the lane to the right (v[0].x shifted).
template <int NP>
__device__ __forceinline__ v2f left_pair(const v2f (&v)[NP], float from_left, int i) {
  if (i == 0) return v2f{from_left, v[NP - 1].x};
  return v[i - 1];
}
template <int NP>
__device__ __forceinline__ v2f right_pair(const v2f (&v)[NP], float from_right, int i) {
  if (i == NP - 1) return v2f{v[0].y, from_right};
  return v[i + 1];
}

// (rr, ss): the extrapolated dual; (p, q): the projected dual -- in the kernels with the folded momentum (pipe_stage, FOLD) scaled by the stage's
// 1 + beta_k: u, v.  Nothing but the next stage's momentum reads p, q there.
template <int NP>
struct DualRow { v2f rr[NP], ss[NP], p[NP], q[NP]; };

// Horizontal pass of the uniform 5-tap box (pipe_body, UNI): the plain sum of the window, per pixel c
//     a_c = x_c + x_{c+1},   S_c = (a_{c-2} + a_c) + x_{c+2}
// -- a fixed tree that does not depend on how pixels are laid out over lanes, so every layout gives the same bits.  e = the lane's 2 NP pixels in natural
// order with two halo pixels on either side (e[2 + k] = pixel k); the halo a's are formed from the shifted x values, never by shifting a.  On pairs:
// E(m) = pixels (m, m + NP), m = -2 .. NP + 1; A(m) = E(m) + E(m + 1), m = -2 .. NP - 1; S(j) = (A(j - 2) + A(j)) + E(j + 2): 3 NP + 2 packed additions
// for 2 NP pixels against 5 NP packed multiply-adds.
template <int NP>
__device__ __forceinline__ void uni_hsum(const float (&e)[2 * NP + 4], v2f (&out)[NP]) {
  v2f E[NP + 4], A[NP + 2];
#pragma unroll
  for (int m = 0; m < NP + 4; ++m) E[m] = v2f{e[m], e[m + NP]};
#pragma unroll
  for (int m = 0; m < NP + 2; ++m) A[m] = E[m] + E[m + 1];
#pragma unroll
  for (int j = 0; j < NP; ++j) out[j] = (A[j] + A[j + 2]) + E[j + 4];
}

// Wave shifts whose vacant lane takes `edge` instead of 0 (DPP without bound_ctrl: the lane with no source keeps the old value).  The
// two-team layout puts a team's seam column in lane 63 (left team) or lane 0 (right team), so the neighbour across the seam enters with
// the same one instruction as the neighbour inside the wave.
__device__ __forceinline__ float wave_from_left(float v, float edge) {    // lane i <- v[i-1]; lane 0 <- edge
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, edge), __builtin_bit_cast(int, v), 0x138, 0xf, 0xf, false));
}
__device__ __forceinline__ float wave_from_right(float v, float edge) {   // lane i <- v[i+1]; lane 63 <- edge
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, edge), __builtin_bit_cast(int, v), 0x130, 0xf, 0xf, false));
}

// The difference with the one BUILT neighbour pair of a lane (left_pair(v, ., 0) / right_pair(v, ., NP - 1)), the wave shift folded into the
// subtraction that uses it (pipe_shift kernels).  Building the pair costs a DPP move for the shift and a plain move to put the other pixel beside it (a
// second one at the team seam, where the shift lands in the register the seam record was read into) before the one packed subtraction; formed half by
// half the shift is the DPP operand of its own subtraction (v_subrev_f32_dpp / v_sub_f32_dpp; the compiler places the wait states a DPP read needs) and the
// other half is one plain subtraction: two instructions and no move.  At the seam (SEAM: the vacant lane keeps `edge`) the DPP move into the record's
// register stays, then two plain subtractions.  Each half is kept from being re-packed by an empty asm: without it the SLP vectoriser rebuilds the
// pair.  The same IEEE subtraction on the same operands per pixel: the bits do not change.
__device__ __forceinline__ v2f pk_halves(float hx, float hy) {
  asm("" : "+v"(hx));
  asm("" : "+v"(hy));
  return v2f{hx, hy};
}
template <int NP, bool SEAM>      // a - left_pair(v, from_left(v[NP-1].y), 0)
__device__ __forceinline__ v2f sub_left_pair(v2f a, const v2f (&v)[NP], float edge) {
  const float vy = v[NP - 1].y, ax = a.x, ay = a.y, vx = v[NP - 1].x;
  const float sh = SEAM ? wave_from_left(vy, edge) : dpp_left0(vy);
  return pk_halves(ax - sh, ay - vx);
}
template <int NP, bool SEAM>      // right_pair(v, from_right(v[0].x), NP - 1) - b
__device__ __forceinline__ v2f right_pair_sub(const v2f (&v)[NP], float edge, v2f b) {
  const float vx = v[0].x, vy = v[0].y, bx = b.x, by = b.y;
  const float sh = SEAM ? wave_from_right(vx, edge) : dpp_right0(vx);
  return pk_halves(vy - bx, sh - by);
}
// The row-edge coefficient of a stage, cstep or 0 by row: wave-uniform, so in the pipe_shift kernels it is selected on the bit pattern in scalar registers (a float
// select goes through v_cndmask_b32 and a move per stage) and the packed multiply-add reads the scalar.
__device__ __forceinline__ float pipe_cdown(int a, int H, float cstep) {
  int b = ((unsigned)(a - 1) >= (unsigned)(H - 1)) ? (int)0x80000000 : __builtin_bit_cast(int, -cstep);     // the stages read -cdown
  asm("" : "+s"(b));
  return -__builtin_bit_cast(float, b);
}

// One FGP dual iteration on NP pixel pairs per lane.  r1, s1 = (rr, ss)^{k-1} on row a; in0 = (rr, ss, p, q)^{k-1} on row
// b = a-1; solb = sol^k on row b (in) -> sol^k on row a (out); out = (rr, ss, p, q)^k on row b.
// The horizontal step coefficient per pixel: -c, and 0 for the pixel in the last image column (no difference across it).  LASTLANE: the image
// width is a multiple of the pixels per lane, so that pixel is the last one of a lane (cr_last, a per-lane scalar: the .y of the last pair); otherwise it can be any
// pixel of a lane and the coefficients are a per-lane register array (ncrv; pair i = pixels (i, i + NP)).
template <int NP>
struct PipeCr { float cstep, cr_last; v2f ncrv[NP]; };
template <int NP, bool LASTLANE>
__device__ __forceinline__ v2f pipe_ncr(const PipeCr<NP>& c, int i) {
  if constexpr (LASTLANE) return i == NP - 1 ? v2f{-c.cstep, -c.cr_last} : pk_set(-c.cstep);
  else return c.ncrv[i];
}

// Objective by-products of a stage (RT instantiations: the per-chain early exit of the TV prox).  The stage forms the iterate sol = x - gam div(rr, ss)
// on row a and has the one on row b = a - 1 from the previous tick: the pieces of its primal objective 0.5 ||x - sol||^2 + gam TV(sol) are sums of
// what the stage computes anyway -- x - sol = gam T with T = div(rr, ss) on row a, and the forward differences of sol on row b (masked like the dual
// step: none across the last row / column).  sq += sum T^2 (row a), tv += sum |grad sol| (row b), fp32 per row; the caller folds rows into fp64.
struct StageObj { v2f sq, tv; };
// PERPIX (rows whose last column can be any pixel of a lane, and column strips): per-pixel 1 / 0 weights instead of mlast -- mx: the column belongs to
// the sums of this workgroup (its strip's interior, inside the image); my: the same, and a column to its right exists in the IMAGE (a strip's edge is
// no image edge: the neighbour in the halo is a value of the same iterate).  Set once per wave, before the tick loop: they do not depend on the row.
template <int NP, bool PERPIX = false>
struct ObjMask {
  float md; v2f mlast;                        // 1 / 0: the row below exists; the column to the right of the lane's last pair exists
  v2f mx[PERPIX ? NP : 1], my[PERPIX ? NP : 1];
};
// the objective terms of one pixel pair: T^2 -> sq, |grad sol| -> tv
template <int NP, bool LASTLANE>
__device__ __forceinline__ v2f obj_sq(const ObjMask<NP, !LASTLANE>* om, int i, v2f T) {
  if constexpr (LASTLANE) return T;
  else return T * om->mx[i];
}
template <int NP, bool LASTLANE>
__device__ __forceinline__ v2f obj_tv(const ObjMask<NP, !LASTLANE>* om, int i, v2f dxv, v2f dyv) {
  v2f dxm, dym;
  if constexpr (LASTLANE) { dxm = dxv * pk_set(om->md); dym = i == NP - 1 ? dyv * om->mlast : dyv; }
  else { dxm = dxv * pk_set(om->md) * om->mx[i]; dym = dyv * om->my[i]; }
  const v2f n = pk_fma(dxm, dxm, dym * dym);
  return v2f{__builtin_amdgcn_sqrtf(n.x), __builtin_amdgcn_sqrtf(n.y)};
}

// SEAML / SEAMR (two-team layout): lane 0's left neighbour of s1 / lane 63's right neighbour of solb is the other team's, `ssl_edge` / `solr_edge`.
// ANISO: the anisotropic prior sigma (|d_r x|_1 + |d_c x|_1): the dual is projected onto the l-infinity unit ball, one clamp per component
// (v_med3_f32), instead of the pixel-norm ball; everything else in the stage is shared.
// BOX: g = sigma TV + the indicator of [blo, bhi] (Beck and Teboulle's constrained FGP): the primal iterate the stage forms is projected onto the box
// before it is differenced and before it is kept as solb.  Pixels outside the image (lanes past W, rows outside, vacant lanes of a wave shift) then
// hold blo / bhi / 0 instead of 0; no difference that reaches an image pixel depends on them: vertical ones across the image's first / last row are cut
// by cdown, the horizontal one across the last column by pipe_ncr, and the dual of column W - 1 (s = 0 there) shields the image from the columns to its right.
// FOLD (pipe_fold: one fixed-count launch from the zero dual state, isotropic projection): the momentum is folded into the projection scale.  The fields
// p, q of a DualRow then hold u = (1 + beta_k) p_k, v = (1 + beta_k) q_k, the factor goes into the one `inv` both components share, and the
// extrapolation p_k + beta_k (p_k - p_{k-1}) = u_k - c_k u_{k-1} (c_k = beta_k / (1 + beta_{k-1}); lmc_tv_fold.h) never forms p_{k-1}: per pixel pair
//     invs = inv (1 + beta_k);  u = r invs;  v = s invs;  rr = fma(-c_k, u_old, u);  ss = fma(-c_k, v_old, v)
// -- five packed instructions where pn = r inv, qn = s inv, rr = fma(beta, pn - p_old, pn), ss = fma(beta, qn - q_old, qn) are six, 15 per pair and
// stage in all instead of 16.  The same number in exact arithmetic, another association of the same products in fp32.  `mom`, `cfold`: beta_k and
// nothing, or 1 + beta_k and c_k.
// SHIFT (pipe_shift kernels): the two differences with a built pair take their wave shift as an operand (sub_left_pair, right_pair_sub).  How it is
// written: `SHIFT && i == 0 ? sub_left_pair(...) : s1[i] - ssl` with SHIFT and i compile-time constants after unrolling, so exactly one arm exists per
// pair.  With SHIFT on, ssl0 / solr_last are a dummy 0 and the built pair of left_pair(., 0) / right_pair(., NP - 1) is formed but never read: dead code
// that the compiler removes (no DPP move and no v_mov in the ISA).  With SHIFT off every statement is the one the kernels had before, in the same
// order: the unfolded kernels' instruction streams are pinned by hash (tests/test_pipe_fold_resources.py) and depend on that order, which an
// `if constexpr` block around the built-pair path changed when it was tried.  The same form in pipe_stage_first and in the combine wave.
template <int NP, bool LASTLANE = true, bool OBJ = false, bool SEAML = false, bool SEAMR = false, bool ANISO = false, bool BOX = false, bool FOLD = false,
          bool SHIFT = false>
__device__ __forceinline__ void pipe_stage(const v2f (&xa)[NP], const v2f (&r1)[NP], const v2f (&s1)[NP], const DualRow<NP>& in0,
                                           v2f (&solb)[NP], float gam, float cdown, const PipeCr<NP>& cr, float mom,
                                           DualRow<NP>& out, StageObj* ob = nullptr, const ObjMask<NP, !LASTLANE>* om = nullptr,
                                           float ssl_edge = 0.f, float solr_edge = 0.f, float blo = 0.f, float bhi = 0.f, float cfold = 0.f) {
  static_assert(!FOLD || (!ANISO && !OBJ), "the folded momentum needs the shared scale of the isotropic projection; the early exit keeps p, q");
  static_assert(!SHIFT || FOLD, "the folded shifts go where the folded momentum goes");
  v2f sol[NP];
  const float ssl0 = SHIFT ? 0.f : SEAML ? wave_from_left(s1[NP - 1].y, ssl_edge) : dpp_left0(s1[NP - 1].y);
  const v2f ngam = pk_set(-gam), ncd = pk_set(-cdown), vb = pk_set(mom), nvc = pk_set(-cfold);
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    const v2f ssl = left_pair(s1, ssl0, i);
    const v2f T = (r1[i] - in0.rr[i]) + (SHIFT && i == 0 ? sub_left_pair<NP, SEAML>(s1[i], s1, ssl_edge) : s1[i] - ssl);
    sol[i] = pk_fma(ngam, T, xa[i]);
    if constexpr (BOX) sol[i] = pipe_clamp_box(sol[i], blo, bhi);
    if constexpr (OBJ) { const v2f Tm = obj_sq<NP, LASTLANE>(om, i, T); ob->sq = i == 0 ? Tm * Tm : pk_fma(Tm, Tm, ob->sq); }
  }
  const float solr_last = SHIFT ? 0.f : SEAMR ? wave_from_right(solb[0].x, solr_edge) : dpp_right0(solb[0].x);
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    const v2f solr = right_pair(solb, solr_last, i);
    const v2f ncr = pipe_ncr<NP, LASTLANE>(cr, i);
    const v2f dxv = sol[i] - solb[i], dyv = SHIFT && i == NP - 1 ? right_pair_sub<NP, SEAMR>(solb, solr_edge, solb[i]) : solr - solb[i];
    if constexpr (OBJ) {
      const v2f nr = obj_tv<NP, LASTLANE>(om, i, dxv, dyv);
      ob->tv = i == 0 ? nr : ob->tv + nr;
    }
    const v2f r = pk_fma(ncd, dxv, in0.rr[i]);
    const v2f s = pk_fma(ncr, dyv, in0.ss[i]);
    v2f pn, qn;
    if constexpr (ANISO) {
      pn = pipe_clamp1(r);
      qn = pipe_clamp1(s);
    } else {
      const v2f n2 = pk_fma(r, r, s * s);
      // min(1, rsq(n2)) == rsq(max(n2, 1)) bit for bit (rsq is monotone, rsq(1) = 1); written as a [0,1] clamp it folds into the
      // output modifier of v_rsq_f32 and the v_max disappears
      const v2f inv = v2f{__builtin_amdgcn_fmed3f(__builtin_amdgcn_rsqf(n2.x), 0.f, 1.f), __builtin_amdgcn_fmed3f(__builtin_amdgcn_rsqf(n2.y), 0.f, 1.f)};
      if constexpr (FOLD) {
        const v2f invs = inv * vb;           // ONE packed multiply for both components (vb = 1 + beta_k)
        pn = r * invs; qn = s * invs;        // u, v
      } else {
        pn = r * inv; qn = s * inv;
      }
    }
    if constexpr (FOLD) {
      out.rr[i] = pk_fma(nvc, in0.p[i], pn);
      out.ss[i] = pk_fma(nvc, in0.q[i], qn);
    } else {
      out.rr[i] = pk_fma(vb, pn - in0.p[i], pn);
      out.ss[i] = pk_fma(vb, qn - in0.q[i], qn);
    }
    out.p[i] = pn;
    out.q[i] = qn;
  }
#pragma unroll
  for (int i = 0; i < NP; ++i) solb[i] = sol[i];
}

// Stage 1 of a launch that starts from the zero dual state: (rr, ss, p, q)^0 = 0, so sol^1 = x and the differences with the previous
// iterate vanish.  Bit-identical to pipe_stage() fed with zeros (x - 0 = x, fma(c, d, 0) = c*d), at ~60 % of its instructions.
// BOX: sol^0 = clip(x).  FOLD (`mom` = 1 + beta_1): u_0 = 0, so rr = u and ss = v -- the two fma(beta, pn, pn) go, the one scaled `inv` comes.
template <int NP, bool LASTLANE = true, bool OBJ = false, bool SEAMR = false, bool ANISO = false, bool BOX = false, bool FOLD = false, bool SHIFT = false>
__device__ __forceinline__ void pipe_stage_first(const v2f (&xa)[NP], v2f (&solb)[NP], float cdown, const PipeCr<NP>& cr, float mom,
                                                 DualRow<NP>& out, StageObj* ob = nullptr, const ObjMask<NP, !LASTLANE>* om = nullptr,
                                                 float solr_edge = 0.f, float blo = 0.f, float bhi = 0.f) {
  const float solr_last = SHIFT ? 0.f : SEAMR ? wave_from_right(solb[0].x, solr_edge) : dpp_right0(solb[0].x);
  static_assert(!FOLD || (!ANISO && !OBJ), "as pipe_stage");
  static_assert(!SHIFT || FOLD, "as pipe_stage");
  const v2f ncd = pk_set(-cdown), vb = pk_set(mom);
  if constexpr (OBJ) ob->sq = pk_set(0.f);       // sol^0 = x
  v2f xc[BOX ? NP : 1];
  if constexpr (BOX) {
#pragma unroll
    for (int i = 0; i < NP; ++i) xc[i] = pipe_clamp_box(xa[i], blo, bhi);
  }
  auto x0 = [&](int i) __attribute__((always_inline)) -> v2f { if constexpr (BOX) return xc[i]; else return xa[i]; };
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    const v2f solr = right_pair(solb, solr_last, i);
    const v2f ncr = pipe_ncr<NP, LASTLANE>(cr, i);
    const v2f dxv = x0(i) - solb[i], dyv = SHIFT && i == NP - 1 ? right_pair_sub<NP, SEAMR>(solb, solr_edge, solb[i]) : solr - solb[i];
    if constexpr (OBJ) {
      const v2f nr = obj_tv<NP, LASTLANE>(om, i, dxv, dyv);
      ob->tv = i == 0 ? nr : ob->tv + nr;
    }
    const v2f r = ncd * dxv;
    const v2f s = ncr * dyv;
    v2f pn, qn;
    if constexpr (ANISO) {
      pn = pipe_clamp1(r);
      qn = pipe_clamp1(s);
    } else {
      const v2f n2 = pk_fma(r, r, s * s);
      const v2f inv = v2f{__builtin_amdgcn_fmed3f(__builtin_amdgcn_rsqf(n2.x), 0.f, 1.f), __builtin_amdgcn_fmed3f(__builtin_amdgcn_rsqf(n2.y), 0.f, 1.f)};
      if constexpr (FOLD) {
        // rr = u and ss = v are plain products here, and stage 2 of the same wave subtracts them in registers: left contractable, the compiler fuses
        // product and difference in some instantiations and not in others, and the layouts no longer give the same bits
#pragma clang fp contract(off)
        const v2f invs = inv * vb;
        pn = r * invs; qn = s * invs;
      } else {
        pn = r * inv; qn = s * inv;
      }
    }
    if constexpr (FOLD) {
      out.rr[i] = pn;
      out.ss[i] = qn;
    } else {
      out.rr[i] = pk_fma(vb, pn, pn);
      out.ss[i] = pk_fma(vb, qn, qn);
    }
    out.p[i] = pn;
    out.q[i] = qn;
  }
#pragma unroll
  for (int i = 0; i < NP; ++i) solb[i] = x0(i);
}

// Row load with zero fill.  The load itself is unconditional (masked-off lanes read the start of the row, always a valid address:
// callers pass a clamped row) and the mask is applied to the value: a predicated load costs an exec-mask branch per access and
// splits the tick into basic blocks the scheduler cannot move loads across.  `al`: rows start on 16-byte boundaries (W % 4 == 0): one
// float4 per group of four pixels; otherwise (any W, e.g. the reference's 667 x 877 image) dword-aligned 16-byte accesses (lmc_device.h) and per-pixel masks.
template <int PXL>
__device__ __forceinline__ void gload_row(float (&dst)[PXL], const float* __restrict__ row, int c0, int W, bool ok, bool al = true) {
  if (al) {
#pragma unroll
    for (int g = 0; g < PXL / 4; ++g) {
      const bool okg = ok && c0 + 4 * g < W;
      const float4 v = *reinterpret_cast<const float4*>(row + (okg ? c0 + 4 * g : 0));
      dst[4 * g] = okg ? v.x : 0.f; dst[4 * g + 1] = okg ? v.y : 0.f; dst[4 * g + 2] = okg ? v.z : 0.f; dst[4 * g + 3] = okg ? v.w : 0.f;
    }
  } else {
#pragma unroll
    for (int g = 0; g < PXL / 4; ++g) {
      float v[4];
      load4_dword_aligned(v[0], v[1], v[2], v[3], row, c0 + 4 * g, W);
#pragma unroll
      for (int q = 0; q < 4; ++q) dst[4 * g + q] = (ok && c0 + 4 * g + q < W) ? v[q] : 0.f;
    }
  }
}

// The same without the select: for values that are masked where they are USED (a select at load time makes the wave wait for
// the prefetch at once).  Lanes / pixels past the row read its start.
// STREAM (aligned rows only): a row that is read once -- the load carries the non-temporal policy (`nt` in the ISA).
template <int PXL, bool STREAM = false>
__device__ __forceinline__ void gload_raw(float (&dst)[PXL], const float* __restrict__ row, int c0, int W, bool al = true) {
  if (al) {
#pragma unroll
    for (int g = 0; g < PXL / 4; ++g) {
      if constexpr (STREAM) {
        const v4f v = __builtin_nontemporal_load(reinterpret_cast<const v4f*>(row + (c0 + 4 * g < W ? c0 + 4 * g : 0)));
        dst[4 * g] = v.x; dst[4 * g + 1] = v.y; dst[4 * g + 2] = v.z; dst[4 * g + 3] = v.w;
      } else {
        const float4 v = *reinterpret_cast<const float4*>(row + (c0 + 4 * g < W ? c0 + 4 * g : 0));
        dst[4 * g] = v.x; dst[4 * g + 1] = v.y; dst[4 * g + 2] = v.z; dst[4 * g + 3] = v.w;
      }
    }
  } else {
#pragma unroll
    for (int g = 0; g < PXL / 4; ++g) load4_dword_aligned_raw(dst[4 * g], dst[4 * g + 1], dst[4 * g + 2], dst[4 * g + 3], row, c0 + 4 * g, W);
  }
}
// ... whose consumer moves the group that holds the row end into place first (AL = false only; nothing to do for aligned rows)
template <int PXL, bool AL>
__device__ __forceinline__ void gfix_raw(float (&r)[PXL], int c0, int W) {
  if constexpr (!AL) unshift_row_dword_aligned<PXL>(r, c0, W);
}

// Four pixels of a row to global memory: columns c .. c + 3, of which those in [lo, hi) are written (the interior of a column strip, and < W).
// STREAM (aligned rows only): a non-temporal store, for rows nobody reads back before the next launch.  Written as four scalar stores that the SLP
// vectoriser joins into one global_store_dwordx4 nt: a vector built by hand re-pairs the combine wave's arithmetic and costs it 7 v_mov_b32 per tick.
template <bool STREAM = false>
__device__ __forceinline__ void gstore4(float* __restrict__ row, int c, int lo, int hi, bool al, float v0, float v1, float v2, float v3) {
  if (al) {        // W, lo, hi multiples of 4: the group is inside or outside as a whole
    if (c >= lo && c < hi) {
      if constexpr (STREAM) {
        float* const p = static_cast<float*>(__builtin_assume_aligned(row + c, 16));
        __builtin_nontemporal_store(v0, p); __builtin_nontemporal_store(v1, p + 1); __builtin_nontemporal_store(v2, p + 2); __builtin_nontemporal_store(v3, p + 3);
      } else *reinterpret_cast<float4*>(row + c) = make_float4(v0, v1, v2, v3);
    }
  } else store4_dword_aligned(row, c, lo, hi, v0, v1, v2, v3);
}

// Column strips (images wider than one wave: W > 64 PXL): a workgroup handles the columns [col_start, col_start + 64 PXL) of its chain, of which
// the interior [strip U, (strip + 1) U) is written; the HALO columns on either side are recomputed, not exchanged: the update of a pixel
// depends on x within K + 1 columns (one per dual iteration, one for the final divergence) and within 2 HW columns for the blur gradient.
// Rounded up to the pixels per lane, so that every strip starts on a lane-sized column multiple: 16-byte aligned accesses stay aligned and the
// last image column of an image whose width is a multiple of PXL stays the last pixel of a lane (LASTLANE) in every strip.
__host__ __device__ constexpr int pipe_halo(int K, int KT, int PXL) {
  const int need = (K + 1 > KT - 1 ? K + 1 : KT - 1);
  return (need + PXL - 1) / PXL * PXL;
}

// Which role a hardware wave plays.  Roles: 0 = L, 1 .. NT = T, NT + 1 = C, NT + 2 = N (file header).  Hardware waves w and w + 4 share a SIMD (two teams:
// w, w + 4, w + 8, w + 12), so the map decides which roles compete for one SIMD's issue slots.  Role of hardware wave w = nibble w of the case's code.
// All 105 pairings of the eight roles were timed in round 3 (512 x 512 x 1024, 16 launches each, the role map taken from an environment variable; the search
// script and its build switch were removed, they are at commit b3bb1ec: scripts/round3/perm_search.py).  Results are exact under any pairing.
//   case                                      code          pairing (one SIMD each)                measured
//   K != 10                                   plain         L + T4 | T1 + T5 | T2 + C | T3 + N     not searched
//   K = 10, one launch, 5 taps / no blur      0x76325410u   L + T2 | T1 + T3 | T4 + C | T5 + N     1.736 ms against 1.775 plain, 2.07 worst (L + C or L + N, two TV waves together)
//   K = 10, one launch, 7 taps                0x75264310u   L + C  | T1 + T2 | T3 + T5 | T4 + N    1.838 against 1.875
//   K = 10, one launch, MC-TV term (in C)     0x76354210u   L + T5 | T1 + T3 | T2 + C  | T4 + N    1.962 against 1.983
//   K = 10, link of a fixed-count chain       0x67325410u   L + T2 | T1 + T3 | T4 + N | T5 + C     ME-TV, 50 passes: 13.27 against 13.95 ms per iteration
//   RT, kc = 5: one live stage per wave       0x76543210u   plain                                  \  live TV waves beside L, N, C or a pass-through wave, never beside
//   RT, kc = 4: one live stage per wave       0x67514320u   L + T1 | T2 + T5 | T3 + N | T4 + C      > each other.  bench.py's data (chains settle at 4 passes, 3 with the 7-tap
//   RT, kc <= 3: one live stage per wave      0x64753210u   L + T5 | T1 + N  | T2 + T4 | T3 + C    /  models): 1.504 / 1.511 ms per iteration against 1.591 / 1.566 plain
//   RT, kc > 5, link of a chained prox        0x67254310u   L + T5 | T1 + T2 | T3 + N | T4 + C     ME-TV as configured: 15.95 against 16.73 ms
//   RT, kc > 5, one launch                    0x74563210u   L + C  | T1 + T5 | T2 + T4 | T3 + N    DESIGN 3.0r (no figure of its own)
//   two teams (16 waves; kPipe2Roles, nibble = team << 3 | role, decoded in pipe_body; a = left team, b = right team; hardware waves w, w + 4, w + 8, w + 12
//   share a SIMD, in that order):                           L.a T4.a C.a T5.b | T1.a T5.a T1.b C.b | T2.a N.a T3.b T4.b | T3.a L.b T2.b N.b
//                                                           1.711 ms per step against 1.742 for round 4's map 0x5D3BC4A291E6F780 (L.a C.a T2.a T3.b | L.b C.b T2.b T3.a |
//                                                           N.a T1.a T4.a T5.b | N.b T1.b T4.b T5.a), five alternating pairs.  Searched in round 5 with a build that read the
//                                                           map at run time (4400 placements from 34 structured seeds by swaps between SIMDs, then 940 orders of the waves:
//                                                           1.60 - 1.92 ms per launch); that build only ranks -- its kernel is another instruction stream -- so nine of its
//                                                           best were rebuilt as constants and timed with bench.py: 1.707 - 1.739 ms per step.  The ORDER of the waves on a SIMD
//                                                           counts as much as the placement (the same four sets in another order: 1.739), and the per-SIMD VALU sums still
//                                                           predict nothing (this map: 298 / 281 / 367 / 354 slots per tick, round 4's: 301 / 352).  DESIGN section 7.
// RT (per-chain exit): the kc live stages are a prefix; up to NT of them run one per wave (t_role: spread), the other T waves only pass the dual on, and the best
// pairing for one live count is among the worst for another -- so the map follows kc.
// The compiler's output follows the form of these expressions, not only their values: the last one-team row is a swap of hardware waves 4 and 6 because its
// nibble code changes the instruction streams of the twelve one-launch RT kernels, and the two-team nibble is split where it is used because returning it
// from here changes the two two-team kernels (scripts/kernel_resources.py --code-hash shows which kernels an edit moves).
constexpr unsigned long long kPipe2Roles = 0xFCEDAB9687543210ull;
template <int K, int KT, bool CHAIN, bool RT>
__device__ __forceinline__ int pipe_role(int hw_wave, int kc, int ncvx_kind) {
  constexpr int NT = PipeGeom<K>::NT;
  if constexpr (K != 10) {
    return hw_wave;
  } else if constexpr (!RT) {
    const unsigned code = CHAIN ? 0x67325410u : ncvx_kind == LMC_NCVX_MC_TV ? 0x76354210u : (KT == 7 ? 0x75264310u : 0x76325410u);
    return (code >> (4 * hw_wave)) & 15;
  } else {
    if (kc <= NT) {
      const unsigned code = kc >= 5 ? 0x76543210u : kc == 4 ? 0x67514320u : 0x64753210u;
      return (code >> (4 * hw_wave)) & 15;
    }
    if (CHAIN) return (0x67254310u >> (4 * hw_wave)) & 15;
    return hw_wave == 4 ? 6 : hw_wave == 6 ? 4 : hw_wave;
  }
}

// KT = 0: no data term (pure prox, or t = 0).  CHAIN: the launch is one link of a chain of launches that together run more than K
// dual iterations: stage 1 starts from the dual state A.tv_in of the previous link ([C][4][H][W]: rr, ss, p, q; NULL = zeros), the last
// stage's state goes to A.tv_out (NULL = not stored), and with A.tv_state_only the combine / store of x_out is skipped.
// WARM (with CHAIN): the state is the two-field projected dual carried between MYULA iterations (A.tv_warm) instead of the four-field
// link state -- a template parameter because the L wave's prefetch registers for the state rows set the kernel's VGPR count.
// AL: image rows start on 16-byte boundaries (W % 4 == 0): float4 global accesses; AL = false (any W): pixel-by-pixel accesses with per-pixel bounds
// (instantiated for K = 10 only: the reference's 667 x 877 image with niter_tv = 10 and the 10-iteration links of its ME-TV term).
// RT: per-chain early exit of the prox (StepArgs::rt_*; pyproximal.TV's rtol): the chain of this workgroup runs kc <= K live stages, the stages after
// them pass (rr, ss) through unchanged -- a delay line with the live stages' timing, so the combine wave forms x - gamma div(rr^kc, ss^kc) -- and every
// iterate formed leaves its primal objective behind.  In a chained launch the link a chain leaves in does its combine; the links before it only
// advance the dual state, the ones after it return at once.
// RT with AL = false: any width the fixed-count kernel covers.  A chain is then gridDim.y workgroups (column strips) that read the same live count, so they
// run, return and combine together; each adds to the chain's objective slots only what lies in the columns it writes (ObjMask: per-pixel weights).
// (Round 3, measured and removed again -- git history, commit 49bc3f1 and the three builds after it: the posterior moments of the INPUT state reduced inside this
// kernel, workgroup b summing the 256-pixel slices b, b + C, ... over all chains, two 1 KB reads per tick.  As a ninth wave: three waves on one SIMD cap the kernel
// at 168 VGPRs, 128-184 spilled.  In the combine wave: its conditional stores make the compiler wait for every load in flight each tick, 4.05 ms per iteration.  In the
// Philox wave, sums in registers, loads 4 / 8 ticks ahead: 2.41 / 2.32 ms against 1.92 with the reduction on a side stream -- and with the loads alone, no arithmetic,
// still 2.61 against 2.05 with the arithmetic alone: the CU's outstanding-miss capacity is what the scattered reads take from the L wave's row prefetches.)
// TEAMS = 2 (myula_step_pipe2_kernel below): the image width is split between two teams of waves, each a complete set of roles on its half
// -- 4 pixels per lane, so sixteen waves, four per SIMD, are resident in the LDS and register budget of one 8-pixel team.  The left team's
// lanes are right-aligned (its last column is lane 63's last pixel; lanes left of column 0 compute on zeros and store nothing), the right
// team's start at lane 0, so every neighbour across the seam enters through the wave shift the stage makes anyway, with the other team's
// value in the vacant lane (wave_from_left / wave_from_right).  Those values are in LDS already (ring rows, hand-off rows: the other team's
// copy sits BW floats away) or are published once per wave per tick into a small record (o_seam):
//   SA [2][2 (NT + 1)]  left team, lane 63: stage k1's ss edge (slot 2j - 1) and stage k2's = the hand-off's (slot 2j) of wave j
//   SB [2][2 NT]        right team, lane 0: sol1, sol2 of wave j's first column (slots 2j - 2, 2j - 1)
//   SR [2][4]           residual edge columns of the blur wave: left team lane 63's last HW (0, 1), right team lane 0's first HW (2, 3)
// A T wave reads one 8-byte record per tick; the blur wave forms the residual row one tick before its adjoint (the row's seam columns
// travel through SR).  Every pixel runs the arithmetic of the one-team kernel on the same operands: the results are bit-identical.
// ANISO (myula_step_pipe_aniso_kernel, lmc_step_pipe_aniso.hip): the stages project the dual onto the box (pipe_stage); fixed count, cold start.
// BOX (myula_step_pipe_box_kernel, lmc_step_pipe_box.hip): the prior is sigma TV + the indicator of [A.box_lo, A.box_hi]: every stage and the combine
// wave project the primal iterate they form onto the box (pipe_stage); fixed count, cold start.  Links with tv_state_only do not combine and clamp nothing there.
// TERM (DataTerm, lmc_common.h; the instantiations are in lmc_step_pipe_term.hip; below, POIS, WL2 and HUB stand for TERM == kTermPois, kTermWl2, kTermHub):
// POIS (myula_step_pipe_pois_kernel, myula_step_pipe_pois_box_kernel): the Poisson data term -- A.y is [2][H][W], counts then
// background; where the L wave forms the residual d = H x - y (blur) or the pointwise gradient (identity, mask) it forms rho(H x) instead.  The
// background row travels through a second prefetch ring (bpre) with the slots and the lead of ypre.  The residual stays masked by a 0 / 1 FACTOR: every
// raw row load returns values of the row it reads (lanes and pixels past the row end read inside it, rows outside the image are clamped), so with the
// documented precondition beta > 0 over the whole plane t = 1 / (max(u, 0) + beta) is finite in every lane and rho * 0 is 0, never NaN (a zero-FILLED
// background would make it inf * 0).  One team, one launch, no energy by-products (pipe_links).
// WL2 (myula_step_pipe_wl2_kernel, myula_step_pipe_wl2_box_kernel): the weighted Gaussian data term -- A.y is [2][H][W], observation
// then weights; the L wave forms d = (H x - y) w (blur: one packed multiply per pixel pair, BEFORE the adjoint) or the pointwise gradient
// sigma_f w (x - y) (identity).  The weight row travels through bpre exactly as the background does.  The residual stays masked by the 0 / 1 factor:
// gload_raw never zero-fills but returns values of the row it reads, and with the documented precondition (w finite over the whole plane) d is finite in
// every lane, so d * 0 is 0, never NaN.  One team, one launch, no energy by-products (pipe_links).
// HUB (myula_step_pipe_hub_kernel, myula_step_pipe_hub_box_kernel): the Huber data term -- A.y is [2][H][W], observation then
// thresholds delta in [0, +inf]; the L wave forms d = clamp(H x - y, -delta, delta) (blur: one v_med3_f32 per pixel where WL2 multiplies, BEFORE the
// adjoint) or the pointwise gradient sigma_f clamp(x - y, -delta, delta) (identity).  The delta row travels through bpre exactly as the weights do.
// The 0 / 1 factor argument of WL2 carries over: the clamp returns one of H x - y, -delta and delta, and it returns +-delta only where that lies
// inside [-|r|, |r|], so with y finite d is finite in every lane whatever delta is (+inf included), and d * 0 is 0.  One team, one launch, no energy
// by-products (pipe_links).
// UNI (myula_step_pipe_uni_kernel, myula_step_pipe_uni2_kernel, lmc_step_pipe_uni.hip): the blur is a uniform 5 x 5 box (centred taps one constant on the whole
// window in both directions; uniform_window, lmc_host.h), so the four 5-tap passes of the L wave are plain sums with shared partial sums -- horizontally
// uni_hsum, vertically V_i = (h_i + p_{i-1}) + p_{i-3} with p_i = h_i + h_{i-1}, the p rows in a ring of four slots indexed by (tick & 3), the previous h row
// kept by parity: no row is copied and nothing is subtracted, so nothing drifts down the image -- and the scale c_u c_v enters once, H x = c V and
// gradient = (sigma_f c) V'.  Every sum is defined per pixel, so 4 and 8 pixels per lane, one and two teams give the same bits; against the general form the
// states move at rounding level (another order of additions, one rounded constant for five taps).  One fixed-count launch of 10 dual iterations from the
// zero dual state on aligned rows, one strip, update alone.  EVERYTHING ELSE KEEPS THE GENERAL FORM: RT, chained links, the warm dual, the anisotropic
// prior, the box constraint, the Poisson and weighted data terms, 7 taps, non-uniform taps, unaligned widths, column strips, the energy by-products.
template <int K, int PXL, int KT, bool CHAIN, bool WARM, bool AL, bool RT, int TEAMS, bool ANISO = false, bool BOX = false, int TERM = kTermL2, bool UNI = false>
__device__ __forceinline__ void pipe_body(const StepArgs& A) {
  static_assert(TERM >= kTermL2 && TERM <= kTermHub, "TERM is a DataTerm");
  constexpr bool kPlane2 = TERM != kTermL2;     // the term reads a second plane of A.y (background, weights, thresholds): the bpre ring beside ypre
  static_assert(!UNI || (K == 10 && KT == 5 && AL && !CHAIN && !WARM && !RT && !ANISO && !BOX && !kPlane2),
                "uniform-box form: one fixed-count launch of 10 dual iterations, 5 taps, aligned rows, plain Gaussian data term, isotropic prior");
  static_assert(!kPlane2 || (TEAMS == 1 && !CHAIN && !WARM && !RT && !ANISO && K == 10),
                "Poisson, weighted and Huber data terms: one team, one launch of 10 dual iterations, isotropic prior, general blur form");
  static_assert(!WARM || CHAIN, "the warm dual uses the state hand-over of the chained launches");
  static_assert(!ANISO || (!WARM && !RT), "anisotropic prior: the early exit's objective and the warm dual are not built");
  static_assert(!BOX || (!WARM && !RT), "box constraint: the early exit's objective and the warm dual are not built");
  // Anisotropic prior or box constraint, the link of a chain that carries the blur (the last one) at 8 pixels per lane: the N wave, not L, hands the dual state of the
  // previous link to stage 1.  With the state rows' prefetch registers beside the blur windows the L wave needs more than 256 VGPRs (the isotropic
  // twins of these four kernels spill 20 to 90 of them); the N wave has them to spare and issues no other global access.
  constexpr bool kStateInN = (ANISO || BOX) && CHAIN && KT > 0 && PXL == 8;
  static_assert(!RT || (!WARM && (K & 1) == 0), "per-chain exit: cold start, even K");
  // RT with AL = false: any width, column strips included.  The objective of an iterate reads it one column beyond the strip's interior, which needs
  // the dual one column further out than the update itself does (K + 1)
  static_assert(!RT || AL || pipe_halo(K, KT, PXL) >= K + 2, "per-chain exit on column strips: the halo holds the objective's extra column");
  static_assert(TEAMS == 1 || (TEAMS == 2 && K == 10 && PXL == 4 && KT == 5 && AL && !CHAIN && !WARM && !RT),
                "two teams: one fixed-count launch, 5 taps, aligned rows, 4 pixels per lane");
  // Momentum folded into the projection scale (pipe_stage): wherever nothing but the next stage's momentum reads p, q -- not where they travel through HBM
  // (links, the warm dual), not with the early exit (pass-through slots copy them, and a rounding-level move can flip an exit pass), not with the
  // anisotropic clamp (no shared scale).  Those keep the code and the bits they had.
  constexpr bool FOLD = pipe_fold(CHAIN, WARM, RT, ANISO);
  static_assert(!FOLD || K <= kTvFoldMax, "the folded table holds one launch's stages");
  // Wave shifts folded into the differences that use them, the row-edge coefficient in scalar registers (sub_left_pair, right_pair_sub, pipe_cdown)
  constexpr bool SHIFT = pipe_shift(FOLD, K, KT);
  using G = PipeGeom<K>;
  using L = PipeLds<K, PXL, CHAIN, TEAMS>;
  constexpr int D = G::D, E = G::E, RB = G::RB, NT = G::NT, BW = L::BW, RP = L::RP, HW = KT > 0 ? (KT - 1) / 2 : 0;
  constexpr int LAGT = TEAMS == 2 ? 1 : 0;     // two teams: the residual row is formed one tick before its horizontal adjoint (seam columns via SR)
  static_assert(K >= 1, "at least one dual iteration");
  static_assert(D >= KT + 1 + LAGT, "the blur pipeline reads ring rows at least one tick old");
  extern __shared__ float lds_all[];
  const int lane = threadIdx.x & 63;
  const int hw_wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int chain = blockIdx.x;
  const int H = A.H, W = A.W;
  // per-chain exit: live stages of this launch, and whether this link only advances the dual state of this chain (it leaves in a later link)
  int kc = K;
  bool state_only = CHAIN && A.tv_state_only;
  if constexpr (RT) {
    const int kc_g = __builtin_amdgcn_readfirstlane(A.rt_kc[chain]);
    if (kc_g <= A.rt_base) return;                   // whole workgroup, before any barrier: left in an earlier link, or no run needed
    if (CHAIN && A.rt_start && A.rt_base < K * (__builtin_amdgcn_readfirstlane(A.rt_start[chain]) & 0xFFFF)) return;   // this link's work of an earlier round stands
    kc = min(kc_g - A.rt_base, K);
    state_only = CHAIN && kc_g > A.rt_base + K;
  }
  // `wave` = the ROLE index used below, not the hardware wave (table above pipe_role); two teams: and the team
  int team = 0, wave;
  if constexpr (TEAMS == 2) {
    const unsigned nib = (unsigned)(kPipe2Roles >> (4 * hw_wave)) & 15u;
    team = nib >> 3;
    wave = nib & 7;
  } else {
    wave = pipe_role<K, KT, CHAIN, RT>(hw_wave, kc, A.ncvx_kind);
  }
  // column strip of this workgroup (blockIdx.y; one strip = the whole row when W <= 64 PXL): c0 is a GLOBAL column, LDS rows are indexed by lane
  constexpr int HALO = pipe_halo(K, KT, PXL);
  const int strip = blockIdx.y;
  const int strip_u = gridDim.y > 1 ? BW - 2 * HALO : W;
  int c0 = (strip ? strip * strip_u - HALO : 0) + lane * PXL;
  int st_lo = strip * strip_u, st_hi = min(W, st_lo + strip_u);       // columns this workgroup writes
  if constexpr (TEAMS == 2) {          // left team [0, W/2), lanes right-aligned; right team [W/2, W) from lane 0 (one strip)
    const int Wt = W >> 1;
    c0 = team ? Wt + lane * PXL : Wt - BW + lane * PXL;
    st_lo = team ? Wt : 0;
    st_hi = team ? W : Wt;
  }
  // the lane's columns are image columns of its team (two teams; one group of 4 pixels per lane), and the column its global loads start at
  const bool cok = c0 >= st_lo && c0 < st_hi;
  const int cl = TEAMS == 2 ? (cok ? c0 : 0) : c0;
  auto col_in = [&](int k) __attribute__((always_inline)) -> bool { return TEAMS == 2 ? cok : c0 + k < W; };
  constexpr bool al = AL;                                                    // rows are 16-byte aligned (strip_u and HALO are multiples of 4)
  const size_t img = (size_t)H * W;
  const float* __restrict__ xin = A.x_in + (size_t)chain * img;
  float* __restrict__ xout = A.x_out + (size_t)chain * img;
  // Two teams: the state is a use-once stream through L2 -- every row of x_in is read once and every row of x_out written once per launch, while
  // the observation rows are re-read by every chain of the XCD.  The L wave's x prefetch and the C wave's stores carry the non-temporal policy, the
  // y loads keep the default one (round 10: -2 % per step, and as much with the kernel alone).  The anisotropic two-team
  // kernel and the one-team kernels keep their instruction streams (tests/test_stream_policy_resources.py).
  constexpr bool kStream = TEAMS == 2 && !ANISO;

  // ring rows < 0, hand-offs of tick -1, g, the normals' slab (read by C whatever the noise mode) and, two teams, the seam records
  for (int e = threadIdx.x; e < L::total; e += blockDim.x) lds_all[e] = 0.f;
  __syncthreads();
  float* const lds = lds_all + team * BW;                   // this team's copy of every row (row pitch RP)
  float* const slab_base = lds_all + L::o_slab + team * L::SLAB;
  float* const seam = lds_all + L::o_seam;
  constexpr int SA = 0, SB = 4 * (NT + 1), SR = SB + 4 * NT;  // seam records (see above), [2 parities] each
  static_assert(TEAMS == 1 || SR + 8 <= L::total - L::o_seam, "seam records");

  const int T_end = (H + D + 3) & ~3;          // ticks, rounded up to the unroll factor (extra ticks write nothing)
  float* const xring = lds + L::o_x;
  auto ring_row = [&](int row) -> float* { return xring + ((unsigned)(row + RB) % (unsigned)RB) * RP; };   // row >= -RB

  // Issue arbitration on the shared SIMDs: the short, latency-bound waves everybody waits for at the barrier (L publishes the
  // ring row, C frees the hand-off slot) go first, the TV waves next, the Philox wave -- pure arithmetic, a quad row-group ahead
  // of its consumer -- last.  Measured: 2.04 -> 1.98 ms; the other way round (TV waves first) 2.37 ms.
  // (Two teams with every role above the side-stream moment reduction's waves, 3 / 3 / 2 / 1: measured in round 10, no gain, not kept)
  constexpr int kPrioL = 3, kPrioC = 3, kPrioT = 1, kPrioN = 0;
  if (wave == 0) __builtin_amdgcn_s_setprio(kPrioL);
  else if (wave == NT + 1) __builtin_amdgcn_s_setprio(kPrioC);
  else if (wave <= NT) __builtin_amdgcn_s_setprio(kPrioT);
  else __builtin_amdgcn_s_setprio(kPrioN);
  // the roles, once per team (two teams: the seam code of each team is static)
  auto roles = [&](auto team_tag) __attribute__((always_inline)) {
  constexpr int TM = decltype(team_tag)::value;
  if (wave == 0) {
    // ---------------- L: loader + blur gradient -------------------------------------------------------------
    const float* __restrict__ uv = A.blur.h;   // centred taps: u[0..KT) then v[0..KT) at h[kMaxBlur..]
    // the windows of the last KT-1 horizontally filtered rows: with KT = 5 they are rings indexed by (tick & 3), static under the
    // x4 unroll (row i-a in slot (U-a)&3, the new row replaces the oldest); otherwise they are rotated by moves
    constexpr bool kRing4 = (KT == 5);
    constexpr int NWIN = KT > 1 ? KT - 1 : 1;
    // x rows: fetched kXPF ticks ahead, slot (tick & 3) (8 ahead was measured: no gain, +50 VGPRs)
    constexpr int kXPF = 4;
    constexpr int NP = PXL / 2;
    float xpre[kXPF][PXL], ypre[4][PXL];
    float bpre[kPlane2 ? 4 : 1][kPlane2 ? PXL : 1];      // POIS: the background rows, WL2: the weight rows, slot for slot beside ypre
    v2f hxw[NWIN][NP], hrw[NWIN][NP];   // y rows: fetched kYPF ticks ahead, slot (tick & 3)
    // UNI: hxw / hrw hold the pair sums p_i = h_i + h_{i-1} of the horizontally summed rows (ring, slot (tick & 3)), hxp / hrp the previous h row by parity
    v2f hxp[UNI ? 2 : 1][NP], hrp[UNI ? 2 : 1][NP];
    const float cbox = UNI ? uv[0] * uv[kMaxBlur] : 0.f;       // c_u c_v
#pragma unroll
    for (int a = 0; a < (UNI ? 2 : 1); ++a)
#pragma unroll
      for (int k = 0; k < NP; ++k) { hxp[a][k] = pk_set(0.f); hrp[a][k] = pk_set(0.f); }
    // 7 taps: the windows already take 96 registers; two teams: 112 VGPRs per wave, so that a wave of the side-stream moment reduction (64)
    // still fits beside the four of a workgroup on each SIMD (at 120 it waited for whole CUs: 2.08 against 1.80 ms per step)
    constexpr int kYPF = (KT == 7 || TEAMS == 2) ? 2 : 3;
#pragma unroll
    for (int a = 0; a < NWIN; ++a)
#pragma unroll
      for (int k = 0; k < NP; ++k) { hxw[a][k] = pk_set(0.f); hrw[a][k] = pk_set(0.f); }
#pragma unroll
    for (int u = 0; u < kXPF; ++u) gload_raw<PXL, kStream>(xpre[u], xin + (size_t)min(u, H - 1) * W, cl, W, al);
    // Vector-memory loads return in order: waiting for a load also waits for every load issued before it.  So the loads a tick
    // consumes must be the OLDEST in flight: y rows are requested three ticks ahead and, inside a tick, before the x row that is only
    // needed four ticks later (with y one tick ahead and issued after x, every tick waited for a fresh HBM access: ~2000 cycles).
    if constexpr (KT > 0) {   // observation rows of the first kYPF residual rows
#pragma unroll
      for (int u = 0; u < kYPF; ++u) {
        const int r = u + 1 - D + (KT - 1) - HW + LAGT;
        gload_raw<PXL>(ypre[u], A.y + (size_t)min(max(r, 0), H - 1) * W, cl, W, al);
        if constexpr (kPlane2) gload_raw<PXL>(bpre[u], A.y + img + (size_t)min(max(r, 0), H - 1) * W, cl, W, al);
      }
    }
    // Without a blur: pointwise data terms (identity, diagonal mask).  Their gradient sigma_f m (m x - y) of row t + 1 - D -- the row the
    // combine wave emits next tick -- is formed HERE (this wave issues no stores, so its loads never queue behind stores in vmcnt) from
    // the ring copy of x and the observation / mask rows requested kYPF ticks ahead, and handed over through the same o_g slots as the
    // blur gradient.
    const bool pw_id = KT == 0 && A.data_kind == LMC_DATA_IDENTITY, pw_mask = KT == 0 && A.data_kind == LMC_DATA_MASK;
    float mpre[KT == 0 ? 4 : 1][KT == 0 ? PXL : 1];
    if constexpr (KT == 0) {
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int k = 0; k < PXL; ++k) { ypre[u][k] = 0.f; mpre[u][k] = 0.f; }
      if constexpr (kPlane2) {
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int k = 0; k < PXL; ++k) bpre[u][k] = 1.f;
      }
      if (pw_id || pw_mask) {
#pragma unroll
        for (int u = 0; u < kYPF; ++u) {
          const size_t ro = (size_t)min(max(u + 1 - D, 0), H - 1) * W;
          gload_raw<PXL>(ypre[u], A.y + ro, c0, W, al);
          if constexpr (kPlane2) gload_raw<PXL>(bpre[u], A.y + img + ro, c0, W, al);
          if (pw_mask) gload_raw<PXL>(mpre[u], A.mask + ro, c0, W, al);
        }
      }
    }
    // chained launch: the dual state rows for stage 1, fetched two ticks ahead (row t - E - 1 is published at tick t)
    // (warm dual, A.tv_warm: the state is the projected dual (p, q) of the previous MYULA iteration, two fields; it enters stage 1 as
    // both the extrapolated and the projected iterate -- the momentum restarts, beta_1 = 0)
    constexpr int nsf = CHAIN ? (WARM ? 2 : 4) : 0;           // fields per pixel of the incoming state
    // state rows are fetched kSPF = 2 ticks ahead (4 for the two-field warm dual was measured: K = 1 / 2 / 3: 1.43 / 1.55 / 2.18 ms against
    // 1.44 / 1.41 / 2.13 -- the 32 extra VGPRs cost more than the deeper prefetch gains)
    constexpr int kSPF = 2;
    float spre[CHAIN ? kSPF : 1][CHAIN ? nsf : 1][CHAIN ? PXL : 1];
    const float* const sin = CHAIN && A.tv_in ? A.tv_in + (size_t)chain * nsf * img : nullptr;
    if constexpr (CHAIN && !kStateInN) {
#pragma unroll
      for (int u = 0; u < kSPF; ++u) {
        const int rs = u - E - 1;
#pragma unroll
        for (int f = 0; f < nsf; ++f)      // raw: masked where the row is handed over (a select here would wait for the load at once)
          gload_raw<PXL>(spre[u][f], sin ? sin + (size_t)f * img + (size_t)min(max(rs, 0), H - 1) * W : xin, c0, W, al);
      }
    }
    double facc = 0.0;        // sum of squared residuals (A.f_out)
    v2f Rprev[TEAMS == 2 ? NP : 1];      // two teams: last tick's residual row (LAGT)
#pragma unroll
    for (int k = 0; k < (TEAMS == 2 ? NP : 1); ++k) Rprev[k] = pk_set(0.f);
    auto tick = [&](auto uu, const int t) __attribute__((always_inline)) {
      constexpr int U = decltype(uu)::value, P = U & 1;
      if constexpr (KT > 0) {   // observation row of the residual row kYPF ticks from now
        const int r3 = t + kYPF + 1 - D + (KT - 1) - HW + LAGT;
        gload_raw<PXL>(ypre[(U + kYPF) & 3], A.y + (size_t)min(max(r3, 0), H - 1) * W, cl, W, al);
        if constexpr (kPlane2) gload_raw<PXL>(bpre[(U + kYPF) & 3], A.y + img + (size_t)min(max(r3, 0), H - 1) * W, cl, W, al);
      } else if (pw_id || pw_mask) {
        const size_t ro = (size_t)min(max(t + kYPF + 1 - D, 0), H - 1) * W;
        gload_raw<PXL>(ypre[(U + kYPF) & 3], A.y + ro, c0, W, al);
        if constexpr (kPlane2) gload_raw<PXL>(bpre[(U + kYPF) & 3], A.y + img + ro, c0, W, al);
        if (pw_mask) gload_raw<PXL>(mpre[(U + kYPF) & 3], A.mask + ro, c0, W, al);
      }
      {   // row t arrives: publish it in the ring (zeros below the image); fetch row t + 4
        float xv[PXL];
        gfix_raw<PXL, AL>(xpre[U], c0, W);
#pragma unroll
        for (int k = 0; k < PXL; ++k) xv[k] = (t < H && col_in(k)) ? xpre[U][k] : 0.f;
        prow_store<PXL>(ring_row(t), lane, xv);
        gload_raw<PXL, kStream>(xpre[U], xin + (size_t)min(t + kXPF, H - 1) * W, cl, W, al);
      }
      if constexpr (CHAIN && !kStateInN) {   // dual state row t - E - 1 of the previous link -> stage 1's hand-off slot P (read next tick)
        float* hb = lds + L::o_hand0 + P * 4 * RP;
        constexpr int SP = U & (kSPF - 1);
        const int rh = t - E - 1;                                  // the row fetched kSPF ticks ago
        const bool rowok_h = sin && rh >= 0 && rh < H;
#pragma unroll
        for (int f = 0; f < nsf; ++f) {
          gfix_raw<PXL, AL>(spre[SP][f], c0, W);
          float sv[PXL];
#pragma unroll
          for (int k = 0; k < PXL; ++k) sv[k] = (rowok_h && c0 + (AL ? (k & ~3) : k) < W) ? spre[SP][f][k] : 0.f;
          prow_store<PXL>(hb + f * RP, lane, sv);
        }
        const int rs = t + kSPF - E - 1;
#pragma unroll
        for (int f = 0; f < nsf; ++f)
          gload_raw<PXL>(spre[SP][f], sin ? sin + (size_t)f * img + (size_t)min(max(rs, 0), H - 1) * W : xin, c0, W, al);
      }
      if constexpr (KT > 0) {
      // The blur pipeline works on the lane's pixel pairs (j, j + NP) like the TV stages: a horizontal pass reads its in-lane operands as the pairs
      // they are, and each of its 2 HW halo pairs is one wave shift plus one move; the vertical passes are elementwise on pairs.
      const int i = t + 1 - D + (KT - 1) + LAGT;       // blur input row (<= t-1: published in an earlier tick)
      v2f hxn[NP];
      {
        v2f xi[NP];
        float e[PXL + 2 * HW];
        const float* const xr = ring_row(i);
        pairs_load<NP>(xi, xr, lane);
        // two teams: across the seam, the other team's copy of the same ring row (the left team's last HW columns are lane 63's of its copy)
#pragma unroll
        for (int m = 0; m < HW; ++m)
          e[m] = (TEAMS == 2 && TM == 1) ? wave_from_left(pair_px<NP>(xi, PXL - HW + m), xr[63 * 4 + pipe_slot_offset<PXL>(PXL - HW + m) - BW])
                                         : dpp_left0(pair_px<NP>(xi, PXL - HW + m));
#pragma unroll
        for (int k = 0; k < PXL; ++k) e[HW + k] = pair_px<NP>(xi, k);
#pragma unroll
        for (int m = 0; m < HW; ++m)
          e[HW + PXL + m] = (TEAMS == 2 && TM == 0) ? wave_from_right(pair_px<NP>(xi, m), xr[BW + pipe_slot_offset<PXL>(m)]) : dpp_right0(pair_px<NP>(xi, m));
        if constexpr (UNI) {
          uni_hsum<NP>(e, hxn);
        } else {
#pragma unroll
        for (int j = 0; j < NP; ++j) {
          v2f acc = pk_set(uv[kMaxBlur]) * v2f{e[j + 2 * HW], e[j + 2 * HW + NP]};
#pragma unroll
          for (int b = 1; b < KT; ++b) acc = pk_fma(pk_set(uv[kMaxBlur + b]), v2f{e[j + 2 * HW - b], e[j + 2 * HW - b + NP]}, acc);
          hxn[j] = acc;
        }
        }
      }
      const int r = i - HW;                     // residual row: Hx[r] = sum_a u[a] hx[i - a]
      v2f R[NP];
      {
        const bool rowok = r >= 0 && r < H;
        const float rmask = rowok ? 1.f : 0.f;
        gfix_raw<PXL, AL>(ypre[U & 3], c0, W);
        if constexpr (kPlane2) gfix_raw<PXL, AL>(bpre[U & 3], c0, W);
#pragma unroll
        for (int j = 0; j < NP; ++j) {
          v2f acc;
          if constexpr (UNI) {   // V_i = (h_i + p_{i-1}) + p_{i-3}: rows i - 4 .. i
            acc = (hxn[j] + hxw[(U - 1) & 3][j]) + hxw[(U - 3) & 3][j];
          } else {
          acc = pk_set(uv[0]) * hxn[j];
#pragma unroll
          for (int a = 1; a < KT; ++a) acc = pk_fma(pk_set(uv[a]), hxw[kRing4 ? ((U - a) & 3) : a - 1][j], acc);
          }
          // masked by a factor, not a select: a select on (row, column) turns into one exec-masked block per pixel (8 per tick: the wave's longest
          // stretch of unpacked arithmetic and half of its scalar instructions); every operand is finite (clamped rows, zeroed ring rows).
          // The observation row arrives in natural order: its subtraction is unpacked (as many instructions as a re-pairing move and a packed one)
          v2f d;
          if constexpr (TERM == kTermPois) d = pois_rho2(acc, v2f{ypre[U & 3][j], ypre[U & 3][j + NP]}, v2f{bpre[U & 3][j], bpre[U & 3][j + NP]});     // (finite in every lane: see POIS above)
          else if constexpr (UNI) d = v2f{__builtin_fmaf(cbox, acc.x, -ypre[U & 3][j]), __builtin_fmaf(cbox, acc.y, -ypre[U & 3][j + NP])};   // c V - y, one rounding
          else d = v2f{acc.x - ypre[U & 3][j], acc.y - ypre[U & 3][j + NP]};
          if constexpr (TERM == kTermWl2) d = d * v2f{bpre[U & 3][j], bpre[U & 3][j + NP]};     // w (H x - y): the weight enters before the adjoint (finite in every lane: see WL2 above)
          if constexpr (TERM == kTermHub) d = v2f{hub_psi(d.x, bpre[U & 3][j]), hub_psi(d.y, bpre[U & 3][j + NP])};     // clamp(H x - y, -delta, delta), before the adjoint (finite in every lane: see HUB above)
          R[j] = d * v2f{(TEAMS == 2 ? cok : AL ? c0 < W : c0 + j < W) ? rmask : 0.f, (TEAMS == 2 ? cok : AL ? c0 < W : c0 + j + NP < W) ? rmask : 0.f};
        }
        if (TEAMS == 1 && A.f_out) {     // (the energy by-products are not built for two teams: pipe_teams_covered); pixels in natural order
#pragma unroll
          for (int k = 0; k < PXL; ++k) facc = fma((double)pair_px<NP>(R, k), (double)pair_px<NP>(R, k), facc);
        }
        if constexpr (!kRing4) {
#pragma unroll
          for (int a = KT - 2; a >= 1; --a)
#pragma unroll
            for (int j = 0; j < NP; ++j) hxw[a][j] = hxw[a - 1][j];
        }
#pragma unroll
        for (int j = 0; j < NP; ++j) {
          if constexpr (UNI) { hxw[U & 3][j] = hxn[j] + hxp[P ^ 1][j]; hxp[P][j] = hxn[j]; }
          else hxw[kRing4 ? (U & 3) : 0][j] = hxn[j];
        }
      }
      if constexpr (TEAMS == 2) {   // publish this row's seam columns for the other team; the adjoint below runs on LAST tick's row
        if (TM == 0 ? lane == 63 : lane == 0) {
#pragma unroll
          for (int m = 0; m < HW; ++m) seam[SR + P * 4 + 2 * TM + m] = pair_px<NP>(R, TM == 0 ? PXL - HW + m : m);
        }
#pragma unroll
        for (int j = 0; j < NP; ++j) { const v2f tmp = R[j]; R[j] = Rprev[j]; Rprev[j] = tmp; }
      }
      {   // horizontal adjoint, then G[r - HW] = sum_a u[a] hR[r - 2HW + a]
        float e[PXL + 2 * HW];
        v2f gout[NP];
        const float* const sr = seam + SR + (P ^ 1) * 4;          // two teams: the other team's seam columns of the row
#pragma unroll
        for (int m = 0; m < HW; ++m)
          e[m] = (TEAMS == 2 && TM == 1) ? wave_from_left(pair_px<NP>(R, PXL - HW + m), sr[m]) : dpp_left0(pair_px<NP>(R, PXL - HW + m));
#pragma unroll
        for (int k = 0; k < PXL; ++k) e[HW + k] = pair_px<NP>(R, k);
#pragma unroll
        for (int m = 0; m < HW; ++m) e[HW + PXL + m] = (TEAMS == 2 && TM == 0) ? wave_from_right(pair_px<NP>(R, m), sr[2 + m]) : dpp_right0(pair_px<NP>(R, m));
        if constexpr (UNI) {
          v2f hrn[NP];
          uni_hsum<NP>(e, hrn);
#pragma unroll
          for (int j = 0; j < NP; ++j) {
            const v2f acc = (hrn[j] + hrw[(U - 1) & 3][j]) + hrw[(U - 3) & 3][j];     // rows r - 4 .. r
            hrw[U & 3][j] = hrn[j] + hrp[P ^ 1][j];
            hrp[P][j] = hrn[j];
            gout[j] = pk_set(A.sigma_f * cbox) * acc;
          }
        } else {
#pragma unroll
        for (int j = 0; j < NP; ++j) {
          v2f hrn = pk_set(uv[kMaxBlur]) * v2f{e[j], e[j + NP]};
#pragma unroll
          for (int b = 1; b < KT; ++b) hrn = pk_fma(pk_set(uv[kMaxBlur + b]), v2f{e[j + b], e[j + b + NP]}, hrn);
          v2f acc = pk_set(uv[KT - 1]) * hrn;
#pragma unroll
          for (int a = 0; a < KT - 1; ++a) acc = pk_fma(pk_set(uv[a]), hrw[kRing4 ? ((U - (KT - 1 - a)) & 3) : KT - 2 - a][j], acc);
          if constexpr (!kRing4) {
#pragma unroll
            for (int a = KT - 2; a >= 1; --a) hrw[a][j] = hrw[a - 1][j];
          }
          hrw[kRing4 ? (U & 3) : 0][j] = hrn;
          gout[j] = pk_set(A.sigma_f) * acc;
        }
        }
        pairs_store<NP>(lds + L::o_g + P * RP, lane, gout);      // row t + 1 - D, read by C next tick
      }
      }   // KT > 0
      if constexpr (KT == 0) {
        if (pw_id || pw_mask) {
          const int i = t + 1 - D;                // <= t - 1: published in an earlier tick
          float xi[PXL], gout[PXL];
          prow_load<PXL>(xi, ring_row(i), lane);
          const bool rowok = i >= 0 && i < H;
          gfix_raw<PXL, AL>(ypre[U & 3], c0, W);
          if (pw_mask) gfix_raw<PXL, AL>(mpre[U & 3], c0, W);
          if constexpr (kPlane2) gfix_raw<PXL, AL>(bpre[U & 3], c0, W);
#pragma unroll
          for (int k = 0; k < PXL; ++k) {
            float g = 0.f;
            if (rowok && c0 + k < W) {
              if constexpr (TERM == kTermPois) {
                if (pw_id) g = A.sigma_f * pois_rho(xi[k], ypre[U & 3][k], bpre[U & 3][k]);
                else g = A.sigma_f * mpre[U & 3][k] * pois_rho(mpre[U & 3][k] * xi[k], ypre[U & 3][k], bpre[U & 3][k]);
              } else if constexpr (TERM == kTermWl2) {
                g = A.sigma_f * (bpre[U & 3][k] * (xi[k] - ypre[U & 3][k]));     // (identity: pipe_links keeps the mask kind away)
              } else if constexpr (TERM == kTermHub) {
                g = A.sigma_f * hub_psi(xi[k] - ypre[U & 3][k], bpre[U & 3][k]);     // (identity, likewise)
              } else {
              if (pw_id) g = A.sigma_f * (xi[k] - ypre[U & 3][k]);
              else g = A.sigma_f * mpre[U & 3][k] * fmaf(mpre[U & 3][k], xi[k], -ypre[U & 3][k]);
              }
            }
            gout[k] = g;
          }
          prow_store<PXL>(lds + L::o_g + P * RP, lane, gout);      // row t + 1 - D, read by C next tick
        }
      }
      __syncthreads();
    };
    for (int t = 0; t < T_end; t += 4) static_for<0, 4>([&](auto uu) { tick(uu, t + decltype(uu)::value); });
    if (TEAMS == 1 && A.f_out) {
      const double tot = wave_sum(facc);
      if (lane == 0) unsafeAtomicAdd(&A.f_out[chain], 0.5 * (double)A.sigma_f * tot);
    }
  } else if (wave <= NT) {
    // ---------------- T: TV stages k1 = 2*wave - 1 and k2 = 2*wave -----------------------------------------
    // Wave 1 of a launch that starts from the zero dual state runs a specialised stage 1 (its own copy of the loop, no branch inside):
    // it shares a SIMD with wave 5, and two full T waves on one SIMD are what bounds the tick.
    auto t_role = [&](auto first_tag, auto single_tag) __attribute__((always_inline)) {
    constexpr bool FIRST = decltype(first_tag)::value;      // stage k1 starts from the zero dual state
    constexpr bool SINGLE = decltype(single_tag)::value;    // odd K, last wave: stage k1 = K only, its output goes straight to the hand-off
    const int k1 = 2 * wave - 1, k2 = 2 * wave;        // the wave's two SLOTS of the row schedule (rows a1, a2 below)
    // RT, at most NT live stages (the chain the reference configures settles at 4): ONE live stage per wave -- slot k1 of wave j runs stage j, slot k2 only
    // hands its state on -- instead of two stages each in the first waves and none in the rest: a wave's tick is then half as long, and what the others wait for at
    // the barrier is no longer the two-stage waves' chain of hand-off reads, two stages and stores.  Same arithmetic on the same data: bit-identical.
    const bool spread = RT && kc <= NT;
    const int g1 = spread ? wave : k1, g2 = k2;          // the STAGES the slots run (momentum coefficient, objective slot)
    const float gam = A.tv.gamma, cstep = A.tv.c;
    const float blo = BOX ? A.box_lo : 0.f, bhi = BOX ? A.box_hi : 0.f;
    // FOLD: 1 + beta_g and c_g of the launcher's table (lmc_common.h: kTvFoldAt) in place of beta_g
    const float beta1 = A.tv.betas[FOLD ? kTvFoldAt + 2 * (g1 - 1) : g1 - 1], beta2 = SINGLE ? 0.f : A.tv.betas[FOLD ? kTvFoldAt + 2 * (g2 - 1) : g2 - 1];
    const float cf1 = FOLD ? A.tv.betas[kTvFoldAt + 2 * (g1 - 1) + 1] : 0.f, cf2 = FOLD && !SINGLE ? A.tv.betas[kTvFoldAt + 2 * (g2 - 1) + 1] : 0.f;
    PipeCr<PXL / 2> crc;                                              // see PipeCr: AL kernels need W % PXL == 0 (host check), the others take any W
    crc.cstep = cstep;
    crc.cr_last = (c0 + PXL - 1 == W - 1 || (TEAMS == 2 && !cok)) ? 0.f : cstep;   // (two teams: ss stays 0 left of column 0)
#pragma unroll
    for (int i = 0; i < PXL / 2; ++i) crc.ncrv[i] = v2f{c0 + i == W - 1 ? 0.f : -cstep, c0 + i + PXL / 2 == W - 1 ? 0.f : -cstep};
    float* const hout = lds + L::o_hand + (wave - 1) * 8 * RP;       // this wave's hand-off [2][4][BW] ([2][2][BW] for the last one if CHAIN)
    const bool from_state = CHAIN && wave == 1 && A.tv_in != nullptr;
    constexpr bool warm = WARM;
    const float* const hin = from_state ? lds + L::o_hand0 : hout - 8 * RP;   // the previous wave's / the previous link's state
    constexpr int nof = warm ? 2 : 4;                                // fields per pixel of the outgoing state
    float* const sout = CHAIN && wave == NT && A.tv_out && (!RT || state_only) ? A.tv_out + (size_t)chain * nof * img : nullptr;
    constexpr int NP = PXL / 2;
    const bool live1 = !RT || g1 <= kc, live2 = !RT || (!spread && g2 <= kc);      // wave-uniform; live stages are a prefix
    const bool fullpass2 = spread && wave < kc;          // a later wave still runs a live stage: slot k2 hands all four fields on, not (rr, ss) only
    ObjMask<NP, !AL> om;
    om.md = 0.f;
    om.mlast = v2f{1.f, (c0 + PXL - 1 == W - 1) ? 0.f : 1.f};
    if constexpr (RT && !AL) {
#pragma unroll
      for (int i = 0; i < NP; ++i) {
        const int ca = c0 + i, cb = ca + NP;            // pair i = pixels (i, i + NP)
        const bool ina = ca >= st_lo && ca < st_hi, inb_ = cb >= st_lo && cb < st_hi;      // st_hi <= W
        om.mx[i] = v2f{ina ? 1.f : 0.f, inb_ ? 1.f : 0.f};
        om.my[i] = v2f{ina && ca < W - 1 ? 1.f : 0.f, inb_ && cb < W - 1 ? 1.f : 0.f};
      }
    }
    double osq1 = 0.0, otv1 = 0.0, osq2 = 0.0, otv2 = 0.0;            // RT: objective sums of the iterates stages k1 / k2 form (fp64 over rows)
    DualRow<NP> inb[2], o1[2];
    v2f sol1[NP], sol2[NP];
    v2f xk[2][NP];        // x rows read for stage k1 (row a1 = a2 + 2), reused by stage k2 two ticks later: one ring read per tick
#pragma unroll
    for (int k = 0; k < NP; ++k) {
      sol1[k] = sol2[k] = pk_set(0.f);
      xk[0][k] = xk[1][k] = pk_set(0.f);
#pragma unroll
      for (int pp = 0; pp < 2; ++pp) {
        inb[pp].rr[k] = inb[pp].ss[k] = inb[pp].p[k] = inb[pp].q[k] = pk_set(0.f);
        o1[pp].rr[k] = o1[pp].ss[k] = o1[pp].p[k] = o1[pp].q[k] = pk_set(0.f);
      }
    }
    // the wave's last stage hands its output (dual state of row `brow`) to the next wave / the combine wave, and, in the last wave of a
    // chained launch, to HBM for the next link (all four fields) or the next MYULA iteration (warm dual: p, q)
    auto emit = [&](const DualRow<NP>& out, const int P, const int brow, const bool live) __attribute__((always_inline)) {
      if (RT && !live) {             // pass-through: only (rr, ss) travel on (the combine wave's operands); same slots in both hand-off layouts
        float* hb = hout + P * ((!CHAIN || wave < NT) ? 4 : 2) * RP;
        pairs_store<NP>(hb, lane, out.rr);
        pairs_store<NP>(hb + RP, lane, out.ss);
      } else if (!CHAIN || wave < NT) {
        float* hb = hout + P * 4 * RP;
        pairs_store<NP>(hb, lane, out.rr);
        pairs_store<NP>(hb + RP, lane, out.ss);
        if (wave < NT) {     // the combine wave reads rr, ss only: the last TV wave (which shares its SIMD with T1) skips half of its hand-off stores
          pairs_store<NP>(hb + 2 * RP, lane, out.p);
          pairs_store<NP>(hb + 3 * RP, lane, out.q);
        }
      } else {
        float* hb = hout + P * 2 * RP;                   // last boundary of a chained launch: rr, ss for the final primal step ...
        pairs_store<NP>(hb, lane, out.rr);
        pairs_store<NP>(hb + RP, lane, out.ss);
        if (sout && brow >= 0 && brow < H) {             // ... and the dual state of row brow for the next link / iteration
#pragma unroll
          for (int g = 0; g < NP / 2; ++g) {
            float* d = sout + (size_t)brow * W;
            const int cg = c0 + 4 * g;
            if (warm) {
              gstore4(d, cg, st_lo, st_hi, al, pair_px<NP>(out.p, 4 * g), pair_px<NP>(out.p, 4 * g + 1), pair_px<NP>(out.p, 4 * g + 2), pair_px<NP>(out.p, 4 * g + 3));
              gstore4(d + img, cg, st_lo, st_hi, al, pair_px<NP>(out.q, 4 * g), pair_px<NP>(out.q, 4 * g + 1), pair_px<NP>(out.q, 4 * g + 2), pair_px<NP>(out.q, 4 * g + 3));
            } else {
              gstore4(d, cg, st_lo, st_hi, al, pair_px<NP>(out.rr, 4 * g), pair_px<NP>(out.rr, 4 * g + 1), pair_px<NP>(out.rr, 4 * g + 2), pair_px<NP>(out.rr, 4 * g + 3));
              gstore4(d + img, cg, st_lo, st_hi, al, pair_px<NP>(out.ss, 4 * g), pair_px<NP>(out.ss, 4 * g + 1), pair_px<NP>(out.ss, 4 * g + 2), pair_px<NP>(out.ss, 4 * g + 3));
              gstore4(d + 2 * img, cg, st_lo, st_hi, al, pair_px<NP>(out.p, 4 * g), pair_px<NP>(out.p, 4 * g + 1), pair_px<NP>(out.p, 4 * g + 2), pair_px<NP>(out.p, 4 * g + 3));
              gstore4(d + 3 * img, cg, st_lo, st_hi, al, pair_px<NP>(out.q, 4 * g), pair_px<NP>(out.q, 4 * g + 1), pair_px<NP>(out.q, 4 * g + 2), pair_px<NP>(out.q, 4 * g + 3));
            }
          }
        }
      }
    };
    // two teams: the neighbours across the seam, published by the other team one tick ago (left team: sol1, sol2 of the right team's
    // first column, for solr; right team: the left team's ss edges of stage k1 of the previous wave's hand-off and of this wave's stage k1, for ssl)
    constexpr bool SL = TEAMS == 2 && TM == 1, SRt = TEAMS == 2 && TM == 0;
    const float* const seam_in = seam + (TM == 1 ? SA + 2 * wave - 2 : SB + 2 * (wave - 1));
    float* const seam_out = seam + (TM == 0 ? SA + 2 * wave - 1 : SB + 2 * (wave - 1));
    auto tick = [&](auto uu, const int t) __attribute__((always_inline)) {
      constexpr int P = decltype(uu)::value & 1;
      const int a2 = t - E - 2 * k2, a1 = t - E - 2 * k1;
      float2 edge = make_float2(0.f, 0.f);     // (k1, k2): ssl edges (right team) or solr edges (left team)
      if constexpr (TEAMS == 2) edge = *reinterpret_cast<const float2*>(seam_in + (P ^ 1) * (TM == 1 ? 2 * (NT + 1) : 2 * NT));
      float ss2_edge = 0.f;
      if constexpr (!SINGLE) {   // stage k2 on row a2: inputs are this wave's stage k1, one tick (row a2) and two ticks (row a2-1) old
        const float cdown = SHIFT ? pipe_cdown(a2, H, cstep) : ((unsigned)(a2 - 1) >= (unsigned)(H - 1)) ? 0.f : cstep;
        DualRow<NP> out;
        if (live2) {
          StageObj ob;
          om.md = cdown != 0.f ? 1.f : 0.f;
          pipe_stage<NP, AL, RT, SL, SRt, ANISO, BOX, FOLD, SHIFT>(xk[P], o1[P ^ 1].rr, o1[P ^ 1].ss, o1[P], sol2, gam, cdown, crc, beta2, out, &ob, &om, edge.y, edge.y, blo, bhi, cf2);
          if constexpr (RT) { osq2 += (double)(ob.sq.x + ob.sq.y); otv2 += (double)(ob.tv.x + ob.tv.y); }
        } else {                 // pass-through: the state of row a2 - 1 as stage k1 left it
#pragma unroll
          for (int k = 0; k < NP; ++k) { out.rr[k] = o1[P].rr[k]; out.ss[k] = o1[P].ss[k]; }
          if (fullpass2) {
#pragma unroll
            for (int k = 0; k < NP; ++k) { out.p[k] = o1[P].p[k]; out.q[k] = o1[P].q[k]; }
          }
        }
        emit(out, P, a2 - 1, live2 || fullpass2);
        ss2_edge = out.ss[NP - 1].y;
      }
      {   // stage k1 on row a1: inputs from the previous wave's hand-off (row a1) and the one read a tick earlier (row a1-1)
        if constexpr (!FIRST) {
          if (k1 > 1 || from_state) {
            const float* hb = hin + (P ^ 1) * 4 * RP;
            pairs_load<NP>(inb[P].rr, hb, lane);
            pairs_load<NP>(inb[P].ss, hb + RP, lane);
            if (from_state && warm) {     // warm dual: the state IS the projected iterate (beta_1 = 0 makes its role as p_old void)
#pragma unroll
              for (int k = 0; k < NP; ++k) { inb[P].p[k] = inb[P].rr[k]; inb[P].q[k] = inb[P].ss[k]; }
            } else if (live1) {           // (a pass-through stage moves rr, ss only)
              pairs_load<NP>(inb[P].p, hb + 2 * RP, lane);
              pairs_load<NP>(inb[P].q, hb + 3 * RP, lane);
            }
          }
        }
        if (live1) {
          pairs_load<NP>(xk[P], ring_row(a1), lane);      // read two ticks ago as row a1 = this tick's a2: consumed above
          const float cdown = SHIFT ? pipe_cdown(a1, H, cstep) : ((unsigned)(a1 - 1) >= (unsigned)(H - 1)) ? 0.f : cstep;
          StageObj ob;
          om.md = cdown != 0.f ? 1.f : 0.f;
          if constexpr (FIRST) pipe_stage_first<NP, AL, RT, SRt, ANISO, BOX, FOLD, SHIFT>(xk[P], sol1, cdown, crc, beta1, o1[P], &ob, &om, edge.x, blo, bhi);
          else pipe_stage<NP, AL, RT, SL, SRt, ANISO, BOX, FOLD, SHIFT>(xk[P], inb[P].rr, inb[P].ss, inb[P ^ 1], sol1, gam, cdown, crc, beta1, o1[P], &ob, &om, edge.x, edge.x, blo, bhi, cf1);
          if constexpr (RT) { osq1 += (double)(ob.sq.x + ob.sq.y); otv1 += (double)(ob.tv.x + ob.tv.y); }
        } else {                 // pass-through: the state of row a1 - 1, read one tick ago
#pragma unroll
          for (int k = 0; k < NP; ++k) { o1[P].rr[k] = inb[P ^ 1].rr[k]; o1[P].ss[k] = inb[P ^ 1].ss[k]; }
        }
        if constexpr (SINGLE) emit(o1[P], P, a1 - 1, live1);
      }
      if constexpr (TEAMS == 2) {   // this tick's seam values for the other team's next tick: one record per wave, from the seam lane
        float* const so = seam_out + P * (TM == 0 ? 2 * (NT + 1) : 2 * NT);
        if (TM == 0 ? lane == 63 : lane == 0) {
          so[0] = TM == 0 ? o1[P].ss[NP - 1].y : sol1[0].x;
          so[1] = TM == 0 ? ss2_edge : sol2[0].x;
        }
      }
      __syncthreads();
    };
    for (int t = 0; t < T_end; t += 4) static_for<0, 4>([&](auto uu) { tick(uu, t + decltype(uu)::value); });
    if constexpr (RT) {          // objectives of the iterates this wave's live stages formed: sol^{g-1} in stage g = rt_base + k
      const double dg = (double)gam;
      double* const ob = A.rt_obj + (size_t)chain * A.rt_stride + A.rt_base;
      if (live1) {
        const double tot = wave_sum(0.5 * dg * dg * osq1 + dg * otv1);
        if (lane == 0) unsafeAtomicAdd(ob + (g1 - 1), tot);
      }
      if (!SINGLE && live2) {
        const double tot = wave_sum(0.5 * dg * dg * osq2 + dg * otv2);
        if (lane == 0) unsafeAtomicAdd(ob + (g2 - 1), tot);
      }
    }
    };   // t_role
    constexpr bool kOdd = (K & 1) != 0;
    bool ran = false;
    if constexpr (!CHAIN) {
      if (wave == 1) {
        if constexpr (K == 1) t_role(std::true_type{}, std::true_type{});
        else t_role(std::true_type{}, std::false_type{});
        ran = true;
      }
    }
    if constexpr (kOdd) {
      if (!ran && wave == NT) { t_role(std::false_type{}, std::true_type{}); ran = true; }
    }
    if constexpr (K > 1) {
      if (!ran) t_role(std::false_type{}, std::false_type{});
    }
  } else if (wave == NT + 2) {
    // ---------------- N: Philox normals, one quad row-group ahead of C -------------------------------------
    // In the tick of row 4q + NI the normals of pixels NI*PXL/4 .. of quad q + 1 are drawn into the other half of the slab
    // (spread evenly over the ticks: a burst every 4th tick would stall every wave at the barrier).
    float* const slab = slab_base + lane;              // normal (row q of the quad, pixel k) at slab[(q*PXL + pipe_slot(k))*64]
    const uint32_t iter = A.iteration;
    // kStateInN: the state hand-over of the L wave, here (four fields per pixel, rows fetched kSPF = 2 ticks ahead; row t - E - 1 is published at tick t)
    constexpr int nsf = 4, kSPF = 2;
    float spre[kStateInN ? kSPF : 1][kStateInN ? nsf : 1][kStateInN ? PXL : 1];
    const float* const sin = kStateInN && A.tv_in ? A.tv_in + (size_t)chain * nsf * img : nullptr;
    if constexpr (kStateInN) {
#pragma unroll
      for (int u = 0; u < kSPF; ++u) {
        const int rs = u - E - 1;
#pragma unroll
        for (int f = 0; f < nsf; ++f)      // raw: masked where the row is handed over
          gload_raw<PXL>(spre[u][f], sin ? sin + (size_t)f * img + (size_t)min(max(rs, 0), H - 1) * W : xin, c0, W, al);
      }
    }
    auto tick = [&](auto uu, const int t) __attribute__((always_inline)) {
      constexpr int U = decltype(uu)::value;
      constexpr int NI = ((U - D) % 4 + 4) % 4;        // == o & 3  (t = 4m + U)
      const int o = t - D;
      if constexpr (kStateInN) {   // dual state row t - E - 1 of the previous link -> stage 1's hand-off slot P (read next tick)
        constexpr int P = U & 1, SP = U & (kSPF - 1);
        float* hb = lds + L::o_hand0 + P * 4 * RP;
        const int rh = t - E - 1;                                  // the row fetched kSPF ticks ago
        const bool rowok_h = sin && rh >= 0 && rh < H;
#pragma unroll
        for (int f = 0; f < nsf; ++f) {
          gfix_raw<PXL, AL>(spre[SP][f], c0, W);
          float sv[PXL];
#pragma unroll
          for (int k = 0; k < PXL; ++k) sv[k] = (rowok_h && c0 + (AL ? (k & ~3) : k) < W) ? spre[SP][f][k] : 0.f;
          prow_store<PXL>(hb + f * RP, lane, sv);
        }
        const int rs = t + kSPF - E - 1;
#pragma unroll
        for (int f = 0; f < nsf; ++f)
          gload_raw<PXL>(spre[SP][f], sin ? sin + (size_t)f * img + (size_t)min(max(rs, 0), H - 1) * W : xin, c0, W, al);
      }
      if (A.noise_mode == LMC_NOISE_PHILOX && !state_only) {
        const int qn = ((o - NI) >> 2) + 1;             // quad row-group being prepared (o - NI is a multiple of 4)
        if (qn >= 0 && 4 * qn < H) {
          float* const sl = slab + (qn & 1) * (4 * PXL * 64);
#pragma unroll
          for (int kk = 0; kk < PXL / 4; ++kk) {
            const int k = NI * (PXL / 4) + kk;
            float n4[4];
            quad_normals(A.key0, A.key1, iter, A.chain_offset + (uint32_t)chain, (uint32_t)qn * (uint32_t)W + (uint32_t)(c0 + k), n4);
#pragma unroll
            for (int q = 0; q < 4; ++q) sl[(q * PXL + pipe_slot<PXL>(k)) * 64] = n4[q];
          }
        }
      }
      __syncthreads();
    };
    for (int t = 0; t < T_end; t += 4) static_for<0, 4>([&](auto uu) { tick(uu, t + decltype(uu)::value); });
  } else {
    // ---------------- C: final primal step, combine, store --------------------------------------------------
    // Two copies of the role (like the T role's): VM = this wave issues global LOADS (rows of the ME-TV prox image, injected noise).  Memory operations
    // retire in order through one counter, so wherever a conditional load merges back the compiler waits for vmcnt(0) -- in a wave that also stores, that
    // is a wait for its own stores of the previous tick, every tick (counters of the combine wave running alone: 55 % of its cycles in s_waitcnt, 529 ns
    // per tick for 126 ns of arithmetic).  The copy without loads has no such wait.
    auto c_role = [&](auto vm_tag) __attribute__((always_inline)) {
    constexpr bool VM = decltype(vm_tag)::value;
    const float gam = A.tv.gamma;
    const float* const hin = lds + L::o_hand + (NT - 1) * 8 * RP;      // [2][4][BW], or [2][2][BW] in a chained launch
    constexpr int HSTR = CHAIN ? 2 * RP : 4 * RP;
    float* const slab = slab_base + lane;              // normal (row q of the quad, pixel k) at slab[(q*PXL + pipe_slot(k))*64]
    double gacc = 0.0;        // sum |grad x_in| (A.g_out)
    constexpr int NP = PXL / 2;        // the lane's pixel pairs (j, j + NP), as in the TV stages
    v2f crr[2][NP];
    float xprev[PXL];
#pragma unroll
    for (int k = 0; k < NP; ++k) crr[0][k] = crr[1][k] = pk_set(0.f);
#pragma unroll
    for (int k = 0; k < PXL; ++k) xprev[k] = 0.f;
    // RT: primal objective of the iterate this wave returns, sol^kc (the one the exit test of pass kc looks at; not needed when kc is the
    // last pass, whose iterate is returned untested): sum of squared divergences row by row, |grad sol| of row o - 1 once row o is known
    const bool want_obj = RT && !state_only && A.rt_base + kc < A.rt_total;
    double osq = 0.0, otv = 0.0;
    float pprev[RT ? PXL : 1];
#pragma unroll
    for (int k = 0; k < (RT ? PXL : 1); ++k) pprev[k] = 0.f;
    // AL = false: per-pixel weights of the sums, as in the stages (ObjMask): the strip's interior; no horizontal difference across the last image column
    constexpr bool PM = RT && !AL;
    float cmx[PM ? PXL : 1], cmy[PM ? PXL : 1];
    if constexpr (PM) {
#pragma unroll
      for (int j = 0; j < PXL; ++j) {
        const bool in = c0 + j >= st_lo && c0 + j < st_hi;
        cmx[j] = in ? 1.f : 0.f;
        cmy[j] = in && c0 + j + 1 < W ? 1.f : 0.f;
      }
    }
    // rows of the ME-TV term's prox image (A.extra), requested three ticks ahead of their use (slot tick & 3): a load issued at
    // its point of use would expose an HBM access per tick
    float exq[4][PXL];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int k = 0; k < PXL; ++k) exq[u][k] = 0.f;
    constexpr bool XT = TEAMS == 1;      // the ME-TV / MC-TV terms and the energy by-products (one team only: pipe_teams_covered)
    if (XT && VM && A.extra) {
#pragma unroll
      for (int u = 0; u < 3; ++u) {
        const int r = u - D;
        gload_raw<PXL>(exq[u], A.extra + (size_t)chain * img + (size_t)min(max(r, 0), H - 1) * W, cl, W, al);
      }
    }
    auto tick = [&](auto uu, const int t) __attribute__((always_inline)) {
      constexpr int U = decltype(uu)::value, P = U & 1;
      constexpr int NI = ((U - D) % 4 + 4) % 4;        // == o & 3  (t = 4m + U)
      const int o = t - D;
      if (state_only) { __syncthreads(); return; }     // this link only advances the dual state (of this chain)
      if (XT && VM && A.extra) {
        const int r3 = o + 3;
        gload_raw<PXL>(exq[(U + 3) & 3], A.extra + (size_t)chain * img + (size_t)min(max(r3, 0), H - 1) * W, cl, W, al);
      }
      v2f css[NP], xop[NP], gvp[NP], proxp[NP];
      pairs_load<NP>(crr[P], hin + (P ^ 1) * HSTR, lane);            // rr^K on row o (written last tick)
      pairs_load<NP>(css, hin + (P ^ 1) * HSTR + RP, lane);
      pairs_load<NP>(xop, ring_row(o), lane);
      if (KT > 0 || A.data_kind == LMC_DATA_IDENTITY || A.data_kind == LMC_DATA_MASK) {
        pairs_load<NP>(gvp, lds + L::o_g + (P ^ 1) * RP, lane);
      } else {                                  // no data term: o_g is never written (stale LDS could hold NaN bit patterns)
#pragma unroll
        for (int j = 0; j < NP; ++j) gvp[j] = pk_set(0.f);
      }
      // two teams, right team: the left team's ss^K edge, published with its hand-off row (SA slot 2 NT)
      const float ssl0 = SHIFT ? 0.f : (TEAMS == 2 && TM == 1) ? wave_from_left(css[NP - 1].y, seam[SA + (P ^ 1) * 2 * (NT + 1) + 2 * NT]) : dpp_left0(css[NP - 1].y);
      const v2f ngam = pk_set(-gam);
      v2f dvp[NP];
#pragma unroll
      for (int j = 0; j < NP; ++j) {
        const v2f ssl = left_pair(css, ssl0, j);
        dvp[j] = (crr[P][j] - crr[P ^ 1][j]) + (SHIFT && j == 0 ? sub_left_pair<NP, TEAMS == 2 && TM == 1>(css[j], css, (TEAMS == 2 && TM == 1) ? seam[SA + (P ^ 1) * 2 * (NT + 1) + 2 * NT] : 0.f) : css[j] - ssl);
        proxp[j] = pk_fma(ngam, dvp[j], xop[j]);
        if constexpr (BOX) proxp[j] = pipe_clamp_box(proxp[j], A.box_lo, A.box_hi);
      }
      // the by-products below (early exit's objective, MC-TV term, TV energy) name pixels in natural order: their sums keep their order
      float xo[PXL], gv[PXL], prox[PXL];
#pragma unroll
      for (int j = 0; j < PXL; ++j) { xo[j] = pair_px<NP>(xop, j); gv[j] = pair_px<NP>(gvp, j); prox[j] = pair_px<NP>(proxp, j); }
      float dvs = 0.f;
      if constexpr (RT) {
#pragma unroll
        for (int j = 0; j < PXL; ++j) {
          const float dv = pair_px<NP>(dvp, j);
          if constexpr (PM) { const float dm = dv * cmx[j]; dvs = fmaf(dm, dm, dvs); }
          else dvs = fmaf(dv, dv, dvs);
        }
      }
      if constexpr (RT) {
        if (want_obj && o >= 0 && o < H) {
          osq += (double)dvs;
          if (o >= 1) {               // row o - 1: the row below it is this one
            const float pr_last = dpp_right0(pprev[0]);
            float tvs = 0.f;
#pragma unroll
            for (int j = 0; j < PXL; ++j) {
              if constexpr (PM) {
                const float dx = (prox[j] - pprev[j]) * cmx[j];
                const float dy = ((j == PXL - 1 ? pr_last : pprev[j + 1]) - pprev[j]) * cmy[j];
                tvs += __builtin_amdgcn_sqrtf(fmaf(dx, dx, dy * dy));
              } else {
                const float dx = prox[j] - pprev[j];
                const float dy = (c0 + j + 1 < W) ? (j == PXL - 1 ? pr_last : pprev[j + 1]) - pprev[j] : 0.f;
                tvs += __builtin_amdgcn_sqrtf(fmaf(dx, dx, dy * dy));
              }
            }
            otv += (double)tvs;
          }
#pragma unroll
          for (int j = 0; j < PXL; ++j) pprev[j] = prox[j];
        }
      }
      if (XT && A.ncvx_kind == LMC_NCVX_MC_TV) {   // - lambda * A^T(A x / max(|A x|, gamma))  (algs.py:273-277, 291), added to the gradient
        // v = A x / max(|A x|, gamma) is formed ONCE per pixel, row by row: (vx, vy) of row o from ring rows o, o + 1; A^T v at (o, j) = -((vx[o][j] -
        // vx[o-1][j]) + (vy[o][j] - vy[o][j-1])) with vx of the previous row kept in registers.  The same values, operation for operation, as
        // mc_tv_grad (lmc_device.h) recomputes per pixel for its three weights -- a third of the square roots and reciprocals (round 3: the
        // per-pixel form made this wave the slowest of the workgroup, 3.0 ms per launch against 1.75 without the term).
        float xp[PXL], vx[PXL], vy[PXL];
        prow_load<PXL>(xp, ring_row(o + 1), lane);
        const float x0_r = dpp_right0(xo[0]);
        const bool an = A.ncvx_gamma < 0.f, rowin = o >= 0 && o < H, down = o + 1 < H;
        const float gth = fabsf(A.ncvx_gamma);
#pragma unroll
        for (int j = 0; j < PXL; ++j) {
          const float dx = (rowin && down) ? xp[j] - xo[j] : 0.f;
          const float dy = (rowin && c0 + j + 1 < W) ? (j == PXL - 1 ? x0_r : xo[j + 1]) - xo[j] : 0.f;
          if (an) {
            vx[j] = __builtin_amdgcn_rcpf(fmaxf(fabsf(dx), gth)) * dx;
            vy[j] = __builtin_amdgcn_rcpf(fmaxf(fabsf(dy), gth)) * dy;
          } else {
            const float w = __builtin_amdgcn_rcpf(fmaxf(__builtin_amdgcn_sqrtf(fmaf(dx, dx, dy * dy)), gth));
            vx[j] = w * dx;
            vy[j] = w * dy;
          }
        }
        const float vy_l = dpp_left0(vy[PXL - 1]);
#pragma unroll
        for (int j = 0; j < PXL; ++j) {
          gv[j] -= A.ncvx_lambda * -((vx[j] - xprev[j]) + (vy[j] - (j == 0 ? vy_l : vy[j - 1])));
          xprev[j] = vx[j];          // (xprev: vx of the previous row)
        }
      }
      if (XT && A.g_out && o >= 0 && o < H) {   // isotropic TV of the input image, row o: forward differences, zero across the last row / column
        float xq[PXL];
        prow_load<PXL>(xq, ring_row(o + 1), lane);
        const float xr_last = dpp_right0(xo[0]);
        const bool down = o + 1 < H;
#pragma unroll
        for (int j = 0; j < PXL; ++j) {
          const float dx = down ? xq[j] - xo[j] : 0.f;
          const float dy = (c0 + j + 1 < W) ? (j == PXL - 1 ? xr_last : xo[j + 1]) - xo[j] : 0.f;
          gacc += (double)__builtin_amdgcn_sqrtf(fmaf(dx, dx, dy * dy));
        }
      }
      if (o >= 0 && o < H) {
        const float* const slr = slab + ((o >> 2) & 1) * (4 * PXL * 64);
        const size_t go = (size_t)o * W;
        // noise and prox-image rows arrive per pixel in natural order, the stores leave in natural order; in between the combine runs on the pairs.
        // A group of four columns outside this workgroup's interior loads nothing and stores nothing; its lanes' arithmetic is discarded.
        // The slab is read whatever the noise mode (zero-filled before the first tick, written by the N wave for Philox noise only), pair by pair:
        // the slab holds a row's normals in slot order like every other LDS row, so a pair is two adjacent entries
        float xi[PXL], ex[PXL];
#pragma unroll
        for (int j = 0; j < NP; ++j) { xi[j] = slr[(NI * PXL + 2 * j) * 64]; xi[j + NP] = slr[(NI * PXL + 2 * j + 1) * 64]; }
#pragma unroll
        for (int k = 0; k < PXL; ++k) ex[k] = 0.f;
        if constexpr (VM) {
#pragma unroll
          for (int g = 0; g < PXL / 4; ++g) {
            if (c0 + 4 * g < st_hi && c0 + 4 * g + 3 >= st_lo) {      // the group touches this workgroup's interior
              if (A.noise_mode == LMC_NOISE_INJECTED) {
                const float* nrow = A.noise + (size_t)chain * img + go;
                if (al) {
                  const float4 v = *reinterpret_cast<const float4*>(nrow + c0 + 4 * g);
                  xi[4 * g] = v.x; xi[4 * g + 1] = v.y; xi[4 * g + 2] = v.z; xi[4 * g + 3] = v.w;
                } else load4_dword_aligned(xi[4 * g], xi[4 * g + 1], xi[4 * g + 2], xi[4 * g + 3], nrow, c0 + 4 * g, W);
              }
              if (XT && A.extra) {
                ex[4 * g] = exq[U][4 * g]; ex[4 * g + 1] = exq[U][4 * g + 1]; ex[4 * g + 2] = exq[U][4 * g + 2]; ex[4 * g + 3] = exq[U][4 * g + 3];
                if constexpr (!AL) unshift4_dword_aligned(ex[4 * g], ex[4 * g + 1], ex[4 * g + 2], ex[4 * g + 3], c0 + 4 * g, W);
              }
            }
          }
        }
        v2f ovp[NP];
#pragma unroll
        for (int j = 0; j < NP; ++j) {
          const v2f x = xop[j];
          v2f gr = v2f{gv[j], gv[j + NP]};      // (gv: with the MC-TV term, if any)
          if (XT && VM && A.extra) gr = pk_fma(pk_set(A.extra_coef), x - v2f{ex[j], ex[j + NP]}, gr);
          const v2f in = pk_fma(pk_set(-A.t), gr, pk_fma(pk_set(A.b), proxp[j], pk_set(A.s) * v2f{xi[j], xi[j + NP]}));
          ovp[j] = pk_fma(pk_set(A.a), x, in);
        }
#pragma unroll
        for (int g = 0; g < PXL / 4; ++g) {
          if (c0 + 4 * g < st_hi && c0 + 4 * g + 3 >= st_lo)
            gstore4<kStream>(xout + go, c0 + 4 * g, st_lo, st_hi, al, pair_px<NP>(ovp, 4 * g), pair_px<NP>(ovp, 4 * g + 1), pair_px<NP>(ovp, 4 * g + 2), pair_px<NP>(ovp, 4 * g + 3));
        }
      }
      __syncthreads();
    };
    for (int t = 0; t < T_end; t += 4) static_for<0, 4>([&](auto uu) { tick(uu, t + decltype(uu)::value); });
    if (XT && A.g_out) {
      const double tot = wave_sum(gacc);
      if (lane == 0) unsafeAtomicAdd(&A.g_out[chain], (double)A.g_scale * tot);
    }
    if constexpr (RT) {
      if (want_obj) {               // the last image row: no row below it, horizontal differences only
        const float pr_last = dpp_right0(pprev[0]);
        float tvs = 0.f;
#pragma unroll
        for (int j = 0; j < PXL; ++j) {
          if constexpr (PM) tvs += fabsf((j == PXL - 1 ? pr_last : pprev[j + 1]) - pprev[j]) * cmy[j];
          else tvs += (c0 + j + 1 < W) ? fabsf((j == PXL - 1 ? pr_last : pprev[j + 1]) - pprev[j]) : 0.f;
        }
        otv += (double)tvs;
        const double dg = (double)gam;
        const double tot = wave_sum(0.5 * dg * dg * osq + dg * otv);
        if (lane == 0) unsafeAtomicAdd(A.rt_obj + (size_t)chain * A.rt_stride + A.rt_base + kc, tot);
      }
    }
    };   // c_role
    if (A.extra != nullptr || A.noise_mode == LMC_NOISE_INJECTED) c_role(std::true_type{});
    else c_role(std::false_type{});
  }
  };   // roles
  if constexpr (TEAMS == 2) {
    if (team) roles(std::integral_constant<int, 1>{});
    else roles(std::integral_constant<int, 0>{});
  } else {
    roles(std::integral_constant<int, 0>{});
  }
}

template <int K, int PXL, int KT, bool CHAIN = false, bool WARM = false, bool AL = true, bool RT = false>
__global__ __launch_bounds__(64 * ((K + 1) / 2 + 3), (PXL == 8 || CHAIN) ? 1 : 2) void myula_step_pipe_kernel(const StepArgs A) {
  pipe_body<K, PXL, KT, CHAIN, WARM, AL, RT, 1>(A);
}

// the two-team layout (pipe_body, TEAMS = 2): 16 waves of 4 pixels per lane, four per SIMD (at most 128 VGPRs)
template <int K, int KT>
__global__ __launch_bounds__(128 * ((K + 1) / 2 + 3), 4) void myula_step_pipe2_kernel(const StepArgs A) {
  pipe_body<K, 4, KT, false, false, true, false, 2>(A);
}


template <int K, int PXL, int KT, bool CHAIN = false>
static constexpr size_t pipe_lds_bytes() { return sizeof(float) * (size_t)PipeLds<K, PXL, CHAIN>::total; }
template <int K>
static constexpr size_t pipe_teams_lds_bytes() { return sizeof(float) * (size_t)PipeLds<K, 4, false, 2>::total; }
static_assert(pipe_teams_lds_bytes<10>() <= 160 * 1024, "LDS of one workgroup");

// The one launcher of every pipe kernel, one and two teams, either prior.  The dynamic-LDS limit belongs to the function's code object on
// each device and is set once per device; Kern is a template argument so that every kernel has a memo of its own.
// The folded momentum table (lmc_common.h: kTvFoldAt) goes into this launch's copy of the argument, for every kernel: the ones without the fold never read it.
template <auto Kern>
static hipError_t pipe_launch(size_t lds_bytes, dim3 grid, dim3 block, const StepArgs& a0, hipStream_t st) {
  StepArgs a = a0;
  const bool fold_ok = tv_fold_table(a0.tv.betas, a0.tv.niter < kTvFoldMax ? a0.tv.niter : kTvFoldMax, a.tv.betas + kTvFoldAt);
  if (!fold_ok && pipe_fold(a.tv_in || a.tv_out || a.tv_state_only, a.tv_warm != 0, a.rt_kc != nullptr, a.tv_aniso != 0)) return hipErrorInvalidConfiguration;
  static bool attr_set[64] = {};
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  if (dev < 0 || dev >= 64 || !attr_set[dev]) {
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(Kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    if (e != hipSuccess) return e;
    if (dev >= 0 && dev < 64) attr_set[dev] = true;
  }
  hipLaunchKernelGGL(Kern, grid, block, lds_bytes, st, a);
  return hipGetLastError();
}

// column strips of a one-team launch (wider than one wave: strips with recomputed halos, pipe_halo)
template <int K, int PXL, int KT>
static int pipe_nstrips(int W) {
  constexpr int BWk = 64 * PXL, U = BWk - 2 * pipe_halo(K, KT, PXL);
  return W <= BWk ? 1 : (W + U - 1) / U;
}
constexpr int pipe_block(int K, int teams) { return 64 * teams * ((K + 1) / 2 + 3); }

// the last image column is the last pixel of a lane, rows are 16-byte aligned (the AL = true kernels)
static bool pipe_lastlane(int W) { return (W & (W > 256 ? 7 : 3)) == 0; }

// Pixels per lane and blur taps of a launch as compile-time values: 8 pixels per lane above 256 columns, else 4; taps 5 / 7 / none.
// f(std::integral_constant<int, PXL>, std::integral_constant<int, KT>) launches the kernel of its family.
template <class F>
static hipError_t pipe_select(int W, int KT, F&& f) {
  auto taps = [&](auto pxl) {
    if (KT == 5) return f(pxl, std::integral_constant<int, 5>{});
    if (KT == 7) return f(pxl, std::integral_constant<int, 7>{});
    return f(pxl, std::integral_constant<int, 0>{});
  };
  return W > 256 ? taps(std::integral_constant<int, 8>{}) : taps(std::integral_constant<int, 4>{});
}

template <int PXL, int KT, bool CHAIN, int K = 10, bool WARM = false, bool AL = true, bool RT = false>
static hipError_t pipe_launch_one(const StepArgs& a, hipStream_t st) {
  return pipe_launch<myula_step_pipe_kernel<K, PXL, KT, CHAIN, WARM, AL, RT>>(pipe_lds_bytes<K, PXL, KT, CHAIN>(), dim3(a.C, pipe_nstrips<K, PXL, KT>(a.W)),
                                                                              dim3(pipe_block(K, 1)), a, st);
}

// the two-team kernel (one launch, K = 10, 5 taps, 264 <= W <= 512, W % 8 == 0: pipe_teams_covered)
template <int K, int KT>
static hipError_t pipe_launch_teams(const StepArgs& a, hipStream_t st) {
  return pipe_launch<myula_step_pipe2_kernel<K, KT>>(pipe_teams_lds_bytes<K>(), dim3(a.C), dim3(pipe_block(K, 2)), a, st);
}

// one launch with K dual iterations.  Widths that are not a multiple of the pixels per lane (rows not 16-byte aligned: W % 4 != 0): the
// pixel-by-pixel instantiations, K = 10 without the warm dual only (see pipe_links)
template <int K, bool CHAIN, bool WARM = false>
static hipError_t pipe_dispatch_k(const StepArgs& a, int KT, hipStream_t st) {
  return pipe_select(a.W, KT, [&](auto pxl, auto kt) {
    constexpr int PXL = decltype(pxl)::value, KTc = decltype(kt)::value;
    if (pipe_lastlane(a.W)) return pipe_launch_one<PXL, KTc, CHAIN, K, WARM>(a, st);
    if constexpr (K == 10 && !WARM) return pipe_launch_one<PXL, KTc, CHAIN, K, false, false>(a, st);
    else return hipErrorInvalidConfiguration;
  });
}

// lmc_step_pipe.hip: geometry / data term the pipe kernels cover, and the centred taps (returns KT)
bool pipe_geometry_ok(const StepArgs& a);
int pipe_taps(StepArgs& a);

// lmc_step_pipe_chain.hip: the CHAIN instantiations (dual state in / out through HBM): links of a chained launch (K = 9, 10) and the
// warm-started prox (a.tv_warm: K = 1, 2, 3)
hipError_t pipe_dispatch_chain(const StepArgs& a, int K, int KT, hipStream_t st);

// lmc_step_pipe_box.hip: the box-constrained instantiations (myula_step_pipe_box_kernel / myula_step_pipe_box2_kernel: isotropic prior, K = 10, one launch or a link
// of a chain; teams = 2 covers what pipe_teams_covered names)
hipError_t pipe_dispatch_box(const StepArgs& a, int KT, bool chain, int teams, hipStream_t st);

// lmc_step_pipe_aniso.hip: the anisotropic-prior instantiations (myula_step_pipe_aniso_kernel: K = 10, one launch or a link of a chain; the
// two-team layout, teams = 2, covers what pipe_teams_covered names)
hipError_t pipe_dispatch_aniso(const StepArgs& a, int KT, bool chain, int teams, hipStream_t st);

// lmc_step_pipe_uni.hip: the uniform-box instantiations (myula_step_pipe_uni_kernel / myula_step_pipe_uni2_kernel: K = 10, one launch, 5 taps, aligned rows, one strip;
// teams = 2 covers what pipe_teams_covered names)
hipError_t pipe_dispatch_uni(const StepArgs& a, int KT, int teams, hipStream_t st);

// lmc_step_pipe_term.hip: the Poisson, weighted and Huber data terms, by a.term (myula_step_pipe_{pois,wl2,hub}_kernel and their _box_kernel: isotropic prior,
// K = 10, one launch, one team)
hipError_t pipe_dispatch_term(const StepArgs& a, int KT, hipStream_t st);

}  // namespace lmc

// The element counts of the accumulators (lmc_atomi_amd/csrc/lmc_accum.h) against the layouts include/lmc_atomi.h states, on the host and without a
// device: no HIP call is made.  Build and run it under the host sanitizers:
//   hipcc -std=c++17 --offload-arch=gfx950 -Iinclude -Ilmc_atomi_amd/csrc -Xarch_host -fsanitize=address,undefined scripts/check_accum_sizes.hip -o check_accum_sizes
//   ./check_accum_sizes
#include <cstdio>

#include "lmc_accum.h"

static int bad = 0;
static void expect(const char* what, size_t got, size_t want) {
  std::printf("%-34s %8zu %s %zu\n", what, got, got == want ? "==" : "!=", want);
  if (got != want) ++bad;
}

int main() {
  const int H = 20, W = 27, C = 5, bins = 8, G = 2, k = 3;
  lmc::host::Accumulators a;
  a.C = C; a.H = H; a.W = W; a.chain_offset = 3;
  a.blocks.on[lmc::host::BlockMoments::index(2)] = true;
  a.blocks.on[lmc::host::BlockMoments::index(16)] = true;
  a.hist.bins = bins;
  a.groups.n = G;
  a.cov.k = k;
  expect("pixels [H][W]", a.pixels(), 540);
  expect("packed {sum, sumsq, count}", a.packed_elems(), 2 * 540 + 1);
  // [ceil(H/scale)][ceil(W/scale)] per enabled scale: 10 x 14 at 2, 2 x 2 at 16
  expect("blocks of scale 2", lmc::host::BlockMoments::blocks(H, W, 0), 10 * 14);
  expect("blocks of scale 16", lmc::host::BlockMoments::blocks(H, W, 3), 2 * 2);
  expect("block moments, scales 2 and 16", a.blocks.elems(H, W), 140 + 4);
  expect("histogram [(n_bins+2)*H*W]", a.hist.elems(H, W), (8 + 2) * 540);
  expect("chain groups 2 x [n_groups*H*W]", a.groups.elems(H, W), 2 * 2 * 540);
  expect("sketch Y [k][H][W]", a.cov.y_elems(H, W), 3 * 540);
  expect("sketch Y, s [k], Q [k][k]", a.cov.elems(H, W), 3 * 540 + 3 + 9);
  // the group counts of 3 kept iterations: global chain ids 3 .. 7 mod 2 put 2 chains in group 0 and 3 in group 1
  a.count = 3 * C;
  uint64_t n[2] = {0, 0};
  a.group_counts(n);
  expect("samples of group 0", n[0], 6);
  expect("samples of group 1", n[1], 9);
  return bad ? 1 : 0;
}

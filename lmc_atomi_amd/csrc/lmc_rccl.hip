// Multi-GPU: the RCCL entry points and the all-reduces of the posterior moments (pixels, the blocks of one scale, the chain groups) and of the histogram.
#include <dlfcn.h>
#include <rccl/rccl.h>   // types and enums only: the library itself is dlopen'd (liblmc_atomi loads without RCCL)

#include <cstdlib>
#include <cstring>
#include <string>

#include "lmc_host.h"

using namespace lmc::host;

// ---- multi-GPU: the one collective of the path -----------------------------------------------------------------
// RCCL is reached through dlopen so that the library (and every single-GPU use) does not depend on it.  When the host process has
// RCCL loaded already (PyTorch-ROCm ships its own librccl.so.1) that instance is the one bound, so a communicator created by the host
// framework is valid here.
namespace {
struct RcclApi {
  void* lib = nullptr;
  ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*CommCount)(const ncclComm_t, int*) = nullptr;
  ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
  const char* (*GetErrorString)(ncclResult_t) = nullptr;
  std::string why;
};
RcclApi* rccl_api() {
  static RcclApi api = [] {
    RcclApi a;
    const char* env = getenv("LMC_RCCL_LIB");
    const char* names[] = {env, "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    for (const char* n : names) {
      if (!n || !*n) continue;
      a.lib = dlopen(n, RTLD_NOW | RTLD_NOLOAD);          // the instance the process already has, if any
      if (!a.lib) a.lib = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
      if (a.lib) break;
    }
    if (!a.lib) { const char* e = dlerror(); a.why = std::string("librccl not found (set LMC_RCCL_LIB): ") + (e ? e : ""); return a; }
    auto sym = [&](const char* n) { void* p = dlsym(a.lib, n); if (!p && a.why.empty()) a.why = std::string("librccl lacks ") + n; return p; };
    a.GetUniqueId = reinterpret_cast<decltype(a.GetUniqueId)>(sym("ncclGetUniqueId"));
    a.CommInitRank = reinterpret_cast<decltype(a.CommInitRank)>(sym("ncclCommInitRank"));
    a.CommDestroy = reinterpret_cast<decltype(a.CommDestroy)>(sym("ncclCommDestroy"));
    a.CommCount = reinterpret_cast<decltype(a.CommCount)>(sym("ncclCommCount"));
    a.AllReduce = reinterpret_cast<decltype(a.AllReduce)>(sym("ncclAllReduce"));
    a.GetErrorString = reinterpret_cast<decltype(a.GetErrorString)>(sym("ncclGetErrorString"));
    if (!a.why.empty()) { dlclose(a.lib); a.lib = nullptr; }
    return a;
  }();
  return &api;
}
#define RCCL_TRY(api, expr)                                                                                       \
  do {                                                                                                            \
    ncclResult_t r_ = (expr);                                                                                     \
    if (r_ != ncclSuccess) return fail(LMC_E_HIP, "%s failed: %s", #expr, (api)->GetErrorString(r_));            \
  } while (0)
}  // namespace

extern "C" {

int lmc_rccl_available(void) { return rccl_api()->lib ? 1 : 0; }

int lmc_rccl_unique_id(void* id128_host) {
  RcclApi* R = rccl_api();
  if (!R->lib) return fail(LMC_E_UNSUPPORTED, "%s", R->why.c_str());
  if (!id128_host) return fail(LMC_E_INVALID, "NULL argument");
  static_assert(sizeof(ncclUniqueId) == LMC_RCCL_UNIQUE_ID_BYTES, "ncclUniqueId size");
  ncclUniqueId id;
  RCCL_TRY(R, R->GetUniqueId(&id));
  std::memcpy(id128_host, &id, sizeof id);
  return LMC_OK;
}

int lmc_rccl_comm_create(void** comm_out, int32_t world, int32_t rank, const void* id128_host) {
  RcclApi* R = rccl_api();
  if (!R->lib) return fail(LMC_E_UNSUPPORTED, "%s", R->why.c_str());
  if (!comm_out || !id128_host) return fail(LMC_E_INVALID, "NULL argument");
  if (world < 1 || rank < 0 || rank >= world) return fail(LMC_E_INVALID, "bad rank %d of %d", rank, world);
  ncclUniqueId id;
  std::memcpy(&id, id128_host, sizeof id);
  ncclComm_t comm = nullptr;
  RCCL_TRY(R, R->CommInitRank(&comm, world, id, rank));      // on the current device: one process per GPU
  *comm_out = comm;
  return LMC_OK;
}

int lmc_rccl_comm_destroy(void* comm) {
  RcclApi* R = rccl_api();
  if (!R->lib) return fail(LMC_E_UNSUPPORTED, "%s", R->why.c_str());
  if (!comm) return LMC_OK;
  RCCL_TRY(R, R->CommDestroy(static_cast<ncclComm_t>(comm)));
  return LMC_OK;
}

// The collective of the moments: s->acc.packed holds {sum [n], sumsq [n]} of this rank; the count joins them, ONE ncclAllReduce(sum) over xGMI
// (4 MiB at 512 x 512) in place, and the three come back out.
static int allreduce_packed(Accumulators& a, RcclApi* R, void* rccl_comm, size_t n, double* sum_dev, double* sumsq_dev, uint64_t* count, hipStream_t st) {
  const double cnt = (double)a.count;                      // exact below 2^53 samples
  HIP_TRY(hipMemcpyAsync(a.packed + 2 * n, &cnt, sizeof(double), hipMemcpyHostToDevice, st));
  RCCL_TRY(R, R->AllReduce(a.packed, a.packed, 2 * n + 1, ncclFloat64, ncclSum, static_cast<ncclComm_t>(rccl_comm), st));
  if (sum_dev) HIP_TRY(hipMemcpyAsync(sum_dev, a.packed, sizeof(double) * n, hipMemcpyDeviceToDevice, st));
  if (sumsq_dev) HIP_TRY(hipMemcpyAsync(sumsq_dev, a.packed + n, sizeof(double) * n, hipMemcpyDeviceToDevice, st));
  double total = 0.0;
  HIP_TRY(hipMemcpyAsync(&total, a.packed + 2 * n, sizeof(double), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (count) *count = (uint64_t)(total + 0.5);
  return LMC_OK;
}

int lmc_allreduce_moments(lmc_sampler* s, void* rccl_comm, double* sum_dev, double* sumsq_dev, uint64_t* count, void* stream) {
  if (!s) return fail(LMC_E_INVALID, "NULL sampler");
  DeviceGuard dg(s->device);
  if (!s->moments) return fail(LMC_E_STATE, "sampler was created with moments = 0");
  hipStream_t st = S(stream);
  Accumulators& a = s->acc;
  const size_t n = a.pixels();
  if (!rccl_comm) return lmc_sampler_get_moments(s, sum_dev, sumsq_dev, count, stream);   // a job of one rank
  RcclApi* R = rccl_api();
  if (!R->lib) return fail(LMC_E_UNSUPPORTED, "%s", R->why.c_str());
  HIP_TRY(a.need_packed());
  HIP_TRY(hipMemcpyAsync(a.packed, a.s1, sizeof(double) * n, hipMemcpyDeviceToDevice, st));
  HIP_TRY(hipMemcpyAsync(a.packed + n, a.s2, sizeof(double) * n, hipMemcpyDeviceToDevice, st));
  return allreduce_packed(a, R, rccl_comm, n, sum_dev, sumsq_dev, count, st);
}

int lmc_allreduce_block_moments(lmc_sampler* s, void* rccl_comm, int32_t scale, double* sum_dev, double* sumsq_dev, uint64_t* count, void* stream) {
  if (!s) return fail(LMC_E_INVALID, "NULL sampler");
  DeviceGuard dg(s->device);
  if (!rccl_comm) return lmc_sampler_get_block_moments(s, scale, sum_dev, sumsq_dev, count, stream);   // a job of one rank
  hipStream_t st = S(stream);
  RcclApi* R = rccl_api();
  if (!R->lib) return fail(LMC_E_UNSUPPORTED, "%s", R->why.c_str());
  Accumulators& a = s->acc;
  HIP_TRY(a.need_packed());                                                                 // the blocks of a scale are fewer than the pixels
  const int k = BlockMoments::index(scale);
  const size_t n = k < 0 ? 0 : BlockMoments::blocks(a.H, a.W, k);
  int rc = lmc_sampler_get_block_moments(s, scale, a.packed, a.packed + n, nullptr, stream);   // refuses a scale that is not enabled
  if (rc) return rc;
  return allreduce_packed(a, R, rccl_comm, n, sum_dev, sumsq_dev, count, st);
}

// The collective of the histogram: the counts of this rank and its count in one uint64 buffer, ONE ncclAllReduce(ncclUint64, sum).
int lmc_allreduce_histogram(lmc_sampler* s, void* rccl_comm, uint64_t* counts_dev, uint64_t* count, void* stream) {
  if (!s) return fail(LMC_E_INVALID, "NULL sampler");
  DeviceGuard dg(s->device);
  Histogram& h = s->acc.hist;
  if (!h.counts) return fail(LMC_E_INVALID, "the sampler has no histogram (lmc_sampler_set_histogram)");
  if (!rccl_comm) return lmc_sampler_get_histogram(s, counts_dev, count, stream);   // a job of one rank
  hipStream_t st = S(stream);
  RcclApi* R = rccl_api();
  if (!R->lib) return fail(LMC_E_UNSUPPORTED, "%s", R->why.c_str());
  const size_t n = h.elems(s->acc.H, s->acc.W);
  if (!h.packed) HIP_TRY(hipMalloc(&h.packed, sizeof(unsigned long long) * (n + 1)));
  const unsigned long long cnt = s->acc.count;
  HIP_TRY(hipMemcpyAsync(h.packed, h.counts, sizeof(unsigned long long) * n, hipMemcpyDeviceToDevice, st));
  HIP_TRY(hipMemcpyAsync(h.packed + n, &cnt, sizeof cnt, hipMemcpyHostToDevice, st));
  RCCL_TRY(R, R->AllReduce(h.packed, h.packed, n + 1, ncclUint64, ncclSum, static_cast<ncclComm_t>(rccl_comm), st));
  if (counts_dev) HIP_TRY(hipMemcpyAsync(counts_dev, h.packed, sizeof(unsigned long long) * n, hipMemcpyDeviceToDevice, st));
  unsigned long long total = 0;
  HIP_TRY(hipMemcpyAsync(&total, h.packed + n, sizeof total, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (count) *count = total;
  return LMC_OK;
}

// The collective of the chain-group moments: {A [n], B [n], counts [G] as doubles (exact far below 2^53)} of this rank in one float64 buffer,
// ONE ncclAllReduce(sum) in place, and the three come back out.
int lmc_allreduce_group_moments(lmc_sampler* s, void* rccl_comm, double* sum_dev, double* sumsq_dev, uint64_t* counts_host, void* stream) {
  if (!s) return fail(LMC_E_INVALID, "NULL sampler");
  DeviceGuard dg(s->device);
  ChainGroups& g = s->acc.groups;
  if (!g.sums) return fail(LMC_E_INVALID, "the sampler has no chain groups (lmc_sampler_set_chain_groups)");
  if (!rccl_comm) return lmc_sampler_get_group_moments(s, sum_dev, sumsq_dev, counts_host, stream);   // a job of one rank
  hipStream_t st = S(stream);
  RcclApi* R = rccl_api();
  if (!R->lib) return fail(LMC_E_UNSUPPORTED, "%s", R->why.c_str());
  const size_t G = (size_t)g.n, n = g.elems(s->acc.H, s->acc.W) / 2;
  if (!g.packed) HIP_TRY(hipMalloc(&g.packed, sizeof(double) * (2 * n + G)));
  uint64_t cnt[LMC_MAX_CHAIN_GROUPS];
  double cntd[LMC_MAX_CHAIN_GROUPS];
  s->acc.group_counts(cnt);
  for (size_t g = 0; g < G; ++g) cntd[g] = (double)cnt[g];
  HIP_TRY(hipMemcpyAsync(g.packed, g.sums, sizeof(double) * 2 * n, hipMemcpyDeviceToDevice, st));
  HIP_TRY(hipMemcpyAsync(g.packed + 2 * n, cntd, sizeof(double) * G, hipMemcpyHostToDevice, st));
  HIP_TRY(hipStreamSynchronize(st));                          // cntd is pageable host memory of this frame
  RCCL_TRY(R, R->AllReduce(g.packed, g.packed, 2 * n + G, ncclFloat64, ncclSum, static_cast<ncclComm_t>(rccl_comm), st));
  if (sum_dev) HIP_TRY(hipMemcpyAsync(sum_dev, g.packed, sizeof(double) * n, hipMemcpyDeviceToDevice, st));
  if (sumsq_dev) HIP_TRY(hipMemcpyAsync(sumsq_dev, g.packed + n, sizeof(double) * n, hipMemcpyDeviceToDevice, st));
  HIP_TRY(hipMemcpyAsync(cntd, g.packed + 2 * n, sizeof(double) * G, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (counts_host)
    for (size_t g = 0; g < G; ++g) counts_host[g] = (uint64_t)(cntd[g] + 0.5);
  return LMC_OK;
}

}  // extern "C"

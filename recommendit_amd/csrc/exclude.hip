// Per-user exclusion of already-seen items from a retrieval result -- not in the reference, whose
// RecommendationPipeline.get_recommendations (src/serving/recommender.py:269-387) and run_evaluate
// (src/pipelines/run_pipeline.py:153-230) hand every retrieved candidate on, rated before or not (SURVEY.md §3.4,
// hazard ii).  Replaces the host-side `[i for i in ids if i not in seen][:k]` a caller would write after
// FAISSIndex.batch_search, which would put a host round trip into the serving chain.
//
// exclude_topk_kernel: one wave per query row.  The row is an over-fetched search result (kc >= k + |seen| entries in
// the search's stable order); the wave walks it 256 candidates at a time, every lane binary-searches its four
// candidates side by side in the user's ascending id list (staged in LDS when it has <= EXCL_LDS_ITEMS entries, read
// through the caches otherwise), a 64-bit ballot of "keep" gives each kept candidate its output position (popcount of
// the lower lanes), and the walk stops as soon as k entries are written or the -1 tail begins: a user with e seen
// items costs about k + e candidate reads, not kc.  The rest of the output row is -1 / -inf.  Order-preserving, no
// atomics on the outputs: deterministic.  No host synchronisation, no allocation; capturable in a hipGraph.
#include <math.h>

#include "common.h"
#include "recommendit_hip.h"

namespace {

constexpr int EXCL_LDS_ITEMS = 4096;   // 16 KiB of LDS per one-wave block: 10 blocks per CU (160 KiB)

constexpr int EXCL_ILP = 4;            // candidates per lane and iteration: independent searches hide the LDS latency

// hit[j] = v[j] is in the ascending, unique list[0..n), n >= 1, pow2 = the largest power of two <= n.  A bit descent
// with the same number of steps for every candidate (lo = how many entries are < v), so that the EXCL_ILP dependent
// read chains of a lane advance side by side; a read past the end is clamped, its result unused.
template <typename P>
__device__ __forceinline__ void in_list(P list, int n, int pow2, const int32_t (&v)[EXCL_ILP], bool (&hit)[EXCL_ILP]) {
  int lo[EXCL_ILP];
#pragma unroll
  for (int j = 0; j < EXCL_ILP; ++j) lo[j] = 0;
  for (int step = pow2; step > 0; step >>= 1) {
#pragma unroll
    for (int j = 0; j < EXCL_ILP; ++j) {
      const int idx = lo[j] + step;
      const int32_t x = list[min(idx, n) - 1];            // unconditional: the four reads of a step go out together
      lo[j] = ((idx <= n) & (x < v[j])) ? idx : lo[j];
    }
  }
#pragma unroll
  for (int j = 0; j < EXCL_ILP; ++j) hit[j] = (lo[j] < n) & (list[min(lo[j], n - 1)] == v[j]);
}

__global__ __launch_bounds__(64) void exclude_topk_kernel(
    const float* __restrict__ scores, const int64_t* __restrict__ ids, int kc, const int64_t* __restrict__ user_ids,
    const int64_t* __restrict__ seen_offsets, int64_t n_seen_rows, const int32_t* __restrict__ seen_items, int k,
    float* __restrict__ out_scores, int64_t* __restrict__ out_ids, const int* __restrict__ out_slot,
    int* __restrict__ deficit) {
  __shared__ int32_t sh[EXCL_LDS_ITEMS];
  const int64_t q = blockIdx.x;
  const int lane = threadIdx.x;
  const int64_t u = user_ids ? user_ids[q] : q;
  int64_t off = 0, len = 0;
  if (u >= 0 && u < n_seen_rows) {
    off = seen_offsets[u];
    len = seen_offsets[u + 1] - off;
  }
  const int n = len > 0 ? (int)(len < 0x7fffffff ? len : 0x7fffffff) : 0;   // item ids are int32: a list cannot be longer
  const int32_t* __restrict__ list = seen_items + off;
  const bool staged = n > 0 && n <= EXCL_LDS_ITEMS;   // wave-uniform
  if (staged) {
    for (int i = lane; i < n; i += 64) sh[i] = list[i];
    __syncthreads();
  }
  const float* __restrict__ srow = scores + q * (int64_t)kc;
  const int64_t* __restrict__ irow = ids + q * (int64_t)kc;
  const int64_t orow = out_slot ? (int64_t)out_slot[q] : q;
  float* __restrict__ os = out_scores + orow * (int64_t)k;
  int64_t* __restrict__ oi = out_ids + orow * (int64_t)k;

  int base = 0;        // entries written so far (wave-uniform)
  bool tail = false;   // the input row holds a -1 entry: nothing but padding follows it
  const int pow2 = n > 0 ? 1 << (31 - __clz(n)) : 0;
  constexpr int STEP = 64 * EXCL_ILP;
  // the next STEP candidates are loaded before the current ones are searched: the walk is a chain of dependent
  // iterations (base), so the load latency sits under the searches, not in front of them
  int64_t v_next[EXCL_ILP];
  float s_next[EXCL_ILP];
  auto fetch = [&](int c0) {
#pragma unroll
    for (int j = 0; j < EXCL_ILP; ++j) {
      const int c = c0 + 64 * j + lane;
      v_next[j] = c < kc ? irow[c] : -1;
      s_next[j] = c < kc ? srow[c] : -INFINITY;
    }
  };
  fetch(0);
  for (int c0 = 0; c0 < kc && base < k && !tail; c0 += STEP) {
    int64_t v[EXCL_ILP];
    float s[EXCL_ILP];
    int32_t v32[EXCL_ILP];
    bool keep[EXCL_ILP], hit[EXCL_ILP];
#pragma unroll
    for (int j = 0; j < EXCL_ILP; ++j) {
      v[j] = v_next[j];
      s[j] = s_next[j];
      keep[j] = v[j] >= 0;
      hit[j] = false;
      v32[j] = v[j] >= 0 && v[j] <= 0x7fffffffll ? (int32_t)v[j] : -1;   // -1 is in no list (ids are >= 0)
    }
    if (c0 + STEP < kc) fetch(c0 + STEP);
    if (n > 0) {      // wave-uniform
      if (staged) in_list(sh, n, pow2, v32, hit); else in_list(list, n, pow2, v32, hit);
    }
#pragma unroll
    for (int j = 0; j < EXCL_ILP; ++j) {      // in candidate order
      const bool kj = keep[j] && !hit[j];
      const unsigned long long m = __ballot(kj);
      tail = tail || __ballot(c0 + 64 * j + lane < kc && v[j] < 0) != 0ull;
      const int pos = base + __popcll(m & ((1ull << lane) - 1ull));
      if (kj && pos < k) {
        os[pos] = s[j];
        oi[pos] = v[j];
      }
      base += __popcll(m);
    }
  }
  for (int p = base + lane; p < k; p += 64) {
    os[p] = -INFINITY;
    oi[p] = -1;
  }
  // fewer than k although the row had no padding: the caller fetched too few candidates for this user
  if (deficit && lane == 0 && base < k && !tail) atomicAdd(deficit, 1);
}

}  // namespace

extern "C" int rihip_exclude_topk(const float* scores, const int64_t* ids, int64_t nq, int kc, const int64_t* user_ids,
                                  const int64_t* seen_offsets, int64_t n_seen_rows, const int32_t* seen_items, int k,
                                  float* out_scores, int64_t* out_ids, const int* out_slot, int* deficit, void* stream) {
  RIHIP_REQUIRE(nq >= 0 && kc >= 1 && k >= 1, RIHIP_ERR_ARG, "exclude_topk: nq=%lld, kc=%d, k=%d", (long long)nq, kc, k);
  RIHIP_REQUIRE(nq <= 0x7fffffffll, RIHIP_ERR_ARG, "exclude_topk: nq=%lld > 2^31-1", (long long)nq);
  if (nq == 0) return RIHIP_OK;
  RIHIP_REQUIRE(scores && ids && out_scores && out_ids, RIHIP_ERR_ARG, "exclude_topk: null pointer");
  RIHIP_REQUIRE(n_seen_rows >= 0 && (n_seen_rows == 0 || (seen_offsets && seen_items)), RIHIP_ERR_ARG,
                "exclude_topk: n_seen_rows=%lld without a list table", (long long)n_seen_rows);
  RIHIP_REQUIRE(user_ids || n_seen_rows == 0 || n_seen_rows >= nq, RIHIP_ERR_ARG,
                "exclude_topk: %lld lists for %lld queries (user_ids NULL: one list per query)", (long long)n_seen_rows,
                (long long)nq);
  hipLaunchKernelGGL(exclude_topk_kernel, dim3((unsigned)nq), dim3(64), 0, (hipStream_t)stream, scores, ids, kc, user_ids,
                     seen_offsets, n_seen_rows, seen_items, k, out_scores, out_ids, out_slot, deficit);
  RIHIP_CHECK_LAUNCH();
  return RIHIP_OK;
}

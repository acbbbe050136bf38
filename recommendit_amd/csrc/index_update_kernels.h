// The id side of an index update, shared by index_update.hip (f32 index) and sq8_update.hip (8-bit index): sorted drop / add
// ids, keep flags of the stored rows in insertion and in physical order, the id checks, the kept rows per list and the
// ids of the result.  What is moved (f32 rows or int8 codes) is each file's own repack kernel.  Everything here has
// internal linkage: each file that includes it compiles its own copy.
#pragma once
#include "common.h"

#include <stdint.h>

namespace {

constexpr unsigned long long NO_ID = ~0ull;
__device__ __forceinline__ unsigned long long id_key(int64_t id) { return (unsigned long long)id ^ (1ull << 63); }

__device__ __forceinline__ bool sorted_has(const int64_t* __restrict__ s, int64_t n, int64_t v) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (s[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo < n && s[lo] == v;
}

// host block (int64): [0] lowest id repeated among the drop ids, [1] among the add ids, [2] lowest add id that stays
// stored (all as id_key, NO_ID = none), [3] rows dropped, [4] spare (the 8-bit index: code values clamped), [5 ..] kept
// rows per list, then the bounds of the grouped new rows
constexpr int HB_REP_DROP = 0, HB_REP_ADD = 1, HB_STORED = 2, HB_NDROP = 3, HB_SPARE = 4, HB_LISTS = 5;

__global__ void index_update_init_kernel(unsigned long long* hb) {
  if (threadIdx.x < 3) hb[threadIdx.x] = NO_ID;
  else if (threadIdx.x < HB_LISTS) hb[threadIdx.x] = 0;
}

// neighbours of a sorted id array that are equal: a repeated id
__global__ void index_update_repeat_kernel(const int64_t* __restrict__ s, int64_t n, unsigned long long* slot) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i + 1 < n && s[i] == s[i + 1]) atomicMin(slot, id_key(s[i]));
}

// keep[r] = 0 when the id of stored row r is among the sorted drop ids (keep[N] = 0 closes the scan); a row that stays
// and whose id is among the sorted add ids is a duplicate
__global__ __launch_bounds__(256) void index_update_mask_kernel(const int64_t* __restrict__ item_ids, int64_t N,
                                                                const int64_t* __restrict__ sdrop, int64_t n_drop,
                                                                const int64_t* __restrict__ sadd, int64_t n_add, int* keep,
                                                                unsigned long long* hb) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool drop = false;
  if (r < N) {
    const int64_t id = item_ids[r];
    drop = sorted_has(sdrop, n_drop, id);
    keep[r] = drop ? 0 : 1;
    if (!drop && sorted_has(sadd, n_add, id)) atomicMin(hb + HB_STORED, id_key(id));
  } else if (r == N) {
    keep[r] = 0;
  }
  const unsigned long long b = __ballot(drop);
  if ((threadIdx.x & 63) == 0 && b) atomicAdd(hb + HB_NDROP, (unsigned long long)__popcll(b));
}

// keep flag of every physical row (padding: 0; pkeep[Np] = 0 closes the scan)
__global__ void index_update_pmask_kernel(const int64_t* __restrict__ row_ids, int64_t Np, const int* __restrict__ keep,
                                          int* pkeep) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p > Np) return;
  int k = 0;
  if (p < Np) {
    const int64_t rid = row_ids[p];
    if (rid >= 0) k = keep[rid];
  }
  pkeep[p] = k;
}

__global__ void index_update_list_count_kernel(const int* __restrict__ pscan, const int64_t* __restrict__ poff,
                                               const int* __restrict__ goff, int nlist, unsigned long long* hb) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < nlist) hb[HB_LISTS + c] = (unsigned long long)(pscan[poff[c + 1]] - pscan[poff[c]]);
  if (c <= nlist) hb[HB_LISTS + nlist + c] = (unsigned long long)goff[c];
}

__global__ void index_update_ids_kernel(const int64_t* __restrict__ item_ids, int64_t N, const int* __restrict__ keep,
                                        const int* __restrict__ rscan, const int64_t* __restrict__ add_ids, int64_t n_add,
                                        int64_t n_keep, int64_t* out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < N) {
    if (keep[i]) out[rscan[i]] = item_ids[i];
  } else if (i < N + n_add) {
    out[n_keep + (i - N)] = add_ids[i - N];
  }
}

// f32 rows in insertion order (the flat f32 index; the 8-bit index's attached vectors): kept rows close up, the new
// rows follow
__global__ __launch_bounds__(256) void index_update_compact_kernel(const float* __restrict__ X_old, int64_t N,
                                                                   const int* __restrict__ keep, const int* __restrict__ rscan,
                                                                   const float* __restrict__ X_add, int64_t n_add,
                                                                   int64_t n_keep, int d4, float* X_new) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t it = idx / d4;
  const int c4 = (int)(idx % d4);
  if (it < N) {
    if (!keep[it]) return;
    reinterpret_cast<f32x4*>(X_new + (size_t)rscan[it] * d4 * 4)[c4] = reinterpret_cast<const f32x4*>(X_old + (size_t)it * d4 * 4)[c4];
  } else if (it < N + n_add) {
    reinterpret_cast<f32x4*>(X_new + (size_t)(n_keep + it - N) * d4 * 4)[c4] =
        reinterpret_cast<const f32x4*>(X_add + (size_t)(it - N) * d4 * 4)[c4];
  }
}

inline int64_t id_of(unsigned long long key) { return (int64_t)(key ^ (1ull << 63)); }
inline size_t up256(size_t b) { return (b + 255) / 256 * 256; }

struct UpdateScratch {   // one allocation, carved
  char* base = nullptr;
  size_t used = 0;
  template <typename T> size_t plan(int64_t n) { const size_t o = used; used += up256(sizeof(T) * (size_t)(n > 0 ? n : 1)); return o; }
  template <typename T> T* at(size_t off) const { return reinterpret_cast<T*>(base + off); }
};

}  // namespace

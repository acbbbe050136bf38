// Device helpers shared by the index-search kernels: the orderable 64-bit candidate key and the tag predicate of the
// filtered search.
#pragma once
#include "common.h"

namespace rihip_index {

__device__ __forceinline__ uint32_t f2ord(float f) {
  uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ord2f(uint32_t o) {
  uint32_t u = (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o;
  return __uint_as_float(u);
}
__device__ __forceinline__ uint64_t make_key(float s, uint32_t row) {
  return ((uint64_t)f2ord(s) << 32) | (uint64_t)(0xFFFFFFFFu - row);
}

// Filtered search: row r passes query q's predicate iff (any_of == 0 or tag[r] & any_of) and (tag[r] & all_of) == all_of
// and (tag[r] & none_of) == 0.  (0,0,0) passes every row.
struct Pred {
  uint32_t any_of, all_of, none_of;
  __device__ __forceinline__ bool pass(uint32_t t) const {
    return (any_of == 0u || (t & any_of) != 0u) && (t & all_of) == all_of && (t & none_of) == 0u;
  }
};
__device__ __forceinline__ Pred load_pred(const uint32_t* pred, int64_t q, int stride) {
  const uint32_t* p = pred + q * stride;
  return Pred{p[0], p[1], p[2]};
}
// What a scan's emit tests besides the threshold (template parameter of the scan kernels): the tag predicate, the seen-item
// mask (search_exclude.hip), both, or nothing
enum FilterMode { FM_NONE = 0, FM_TAGS = 1, FM_TAGS_MASK = 2, FM_MASK = 3 };

// the tag words of a lane's 16 accumulator rows: four runs of four rows (acc_row)
__device__ __forceinline__ uint32_t tag_of(const uint4* tw, int r) {
  const uint4 t = tw[r >> 2];
  return (r & 3) == 0 ? t.x : (r & 3) == 1 ? t.y : (r & 3) == 2 ? t.z : t.w;
}

}  // namespace rihip_index

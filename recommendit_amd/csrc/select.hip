// Select and re-score: what turns candidate keys into the sorted top-k.  finalize_kernel radix-selects and sorts the k best
// keys of a candidate list (or writes the rank-th best score as a threshold); refine_kernel is the fused refinement of
// the two-precision search; compact_segments_kernel + rerank_kernel are its unfused form for k > 2048.
#include "search_kernels.h"
#include "search_keys.h"

using namespace rihip_index;

namespace {

// segments -> the contiguous candidate list of query blockIdx.x (split order, then slot order: deterministic); a
// segment that overflowed marks the query as overflowed (count > cap => exact re-do)
__global__ __launch_bounds__(256) void compact_segments_kernel(const uint64_t* __restrict__ seg, const int* __restrict__ seg_cnt,
                                                               int nsplit, int seg_cap, uint64_t* cand, int64_t cap,
                                                               int* count, int cs) {
  __shared__ int off[1025];
  __shared__ int over;
  const int64_t q = blockIdx.x;
  const int tid = threadIdx.x;
  if (tid == 0) {
    int run = 0, ov = 0;
    for (int s = 0; s < nsplit; ++s) {
      int c = seg_cnt[q * nsplit + s];
      if (c > seg_cap) { ov = 1; c = seg_cap; }
      off[s] = run; run += c;
    }
    off[nsplit] = run;
    over = ov || run > cap;
    count[q * cs] = over ? (int)(cap + 1) : run;
  }
  __syncthreads();
  if (over) return;
  for (int s = tid >> 6; s < nsplit; s += 4) {          // one wave per segment
    const int n = off[s + 1] - off[s];
    const uint64_t* src = seg + ((size_t)q * nsplit + s) * seg_cap;
    uint64_t* dst = cand + (size_t)q * cap + off[s];
    for (int i = tid & 63; i < n; i += 64) dst[i] = src[i];
  }
}

// exact f32 re-score of the survivors: 16 lanes per candidate, fixed summation order
template <int D>
__global__ __launch_bounds__(256) void rerank_kernel(const float* __restrict__ X, const float* __restrict__ Q,
                                                     uint64_t* cand, int64_t cap, const int* __restrict__ count,
                                                     float* qnorm, int64_t N, const float* __restrict__ kth_approx,
                                                     float eps_scale, int cs) {
  constexpr int PER = D / 16;  // floats per lane
  const int64_t q = blockIdx.x;
  const int tid = threadIdx.x, l16 = tid & 15, grp = tid >> 4;
  float qv[PER];
  float cut;
#pragma unroll
  for (int j = 0; j < PER; ++j) qv[j] = Q[q * D + l16 * PER + j];
  {
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < PER; ++j) s += qv[j] * qv[j];
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (tid == 0) qnorm[q] = sqrtf(s);
    // At least k candidates have an approximate score >= kth_approx[q], hence exact scores >= kth_approx - eps, so the
    // exact k-th score T* >= kth_approx - eps; a candidate whose approximate score is below kth_approx - 2 eps has an
    // exact score < kth_approx - eps <= T*: it cannot be in the top-k and its row is not fetched (key zeroed).
    cut = kth_approx ? kth_approx[q] - 2.f * eps_scale * sqrtf(s) - 1e-6f : -INFINITY;
  }
  const int cnt = count[q * cs];
  const int64_t n = cnt <= cap ? cnt : 0;  // overflowed list: the query is re-done exactly anyway
  uint64_t* keys = cand + (size_t)q * cap;
  for (int64_t i = grp; i < n; i += 16) {
    const uint64_t key = keys[i];
    const uint32_t row = 0xFFFFFFFFu - (uint32_t)(key & 0xFFFFFFFFull);
    if ((int64_t)row >= N) continue;
    if (ord2f((uint32_t)(key >> 32)) < cut) {
      if (l16 == 0) keys[i] = 0ull;
      continue;
    }
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < PER; ++j) s = fmaf(qv[j], X[(size_t)row * D + l16 * PER + j], s);
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (l16 == 0) keys[i] = make_key(s, row);
  }
}

// ---- finalize: radix-select the k_sel best keys of query q, sort them, emit (FinArgs: search_kernels.h) ------
#ifdef RIHIP_FIN_PROBE
__device__ unsigned long long g_fin_probe[16];
#define FIN_STAMP(k) do { if (blockIdx.x == 0 && threadIdx.x == 0) g_fin_probe[k] = wall_clock64(); } while (0)
extern "C" int rihip_debug_fin_probe(unsigned long long* out) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_fin_probe), sizeof(unsigned long long) * 16) == hipSuccess ? 0 : 1;
}
#else
#define FIN_STAMP(k)
#endif
// radix passes + compaction of finalize_kernel over the key list `kp` (the query's slice of the global candidate list, or
// its copy in LDS: the address space is inferred after inlining, so the LDS call compiles to ds_* instructions)
__device__ __forceinline__ uint64_t finalize_select(const FinArgs& a, const uint64_t* kp, const int64_t n, const int k_sel,
                                                    unsigned* hist, unsigned& s_bin, unsigned& s_above, unsigned& s_cnt,
                                                    uint64_t* sbuf, int P) {
  const int tid = threadIdx.x, lane = tid & 63;
  uint64_t T = 0;  // k_sel-th largest key
  if (k_sel > 0) {
    uint64_t prefix = 0, mask = 0;
    unsigned need = (unsigned)k_sel;
    for (int pass = 0; pass < 8; ++pass) {
      const int shift = 56 - 8 * pass;
      hist[tid] = 0;
      __syncthreads();
      {  // scores share their leading bytes: in the first passes almost every key lands in the same one or two bins, and
         // 12k atomics on one LDS word serialise (that, not the memory passes, was most of this kernel's time for a single
         // request).  Each thread counts runs of equal bins in a register and issues one atomic per run.
        unsigned run_bin = 0xFFFFFFFFu, run_cnt = 0;
        for (int64_t i = tid; i < n; i += 256) {
          const uint64_t key = kp[i];
          if ((key & mask) == prefix) {
            const unsigned b = (unsigned)(key >> shift) & 255u;
            if (b == run_bin) ++run_cnt;
            else { if (run_cnt) atomicAdd(&hist[run_bin], run_cnt); run_bin = b; run_cnt = 1; }
          }
        }
        if (run_cnt) atomicAdd(&hist[run_bin], run_cnt);
      }
      __syncthreads();
      if (tid < 64) {  // wave 0: suffix scan over bins 255..0, 4 bins per lane
        const int b0 = 255 - 4 * lane;
        const unsigned h0 = hist[b0], h1 = hist[b0 - 1], h2 = hist[b0 - 2], h3 = hist[b0 - 3];
        const unsigned mine = h0 + h1 + h2 + h3;
        unsigned incl = mine;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
          const unsigned t = __shfl_up(incl, o, 64);
          if (lane >= o) incl += t;
        }
        const unsigned before = incl - mine;
        if (before < need && need <= incl) {
          unsigned c = before;
          int b = b0;
          if (c + h0 >= need) { b = b0; }
          else { c += h0; if (c + h1 >= need) { b = b0 - 1; }
          else { c += h1; if (c + h2 >= need) { b = b0 - 2; }
          else { c += h2; b = b0 - 3; } } }
          s_bin = (unsigned)b;
          s_above = c;
        }
      }
      __syncthreads();
      need -= s_above;
      prefix |= (uint64_t)s_bin << shift;
      mask |= 0xFFull << shift;
      // every key left in the chosen bucket is needed => the remaining low bytes cannot change the selection:
      // stop (typically after 3-4 of the 8 passes); T = prefix with zero low bytes still satisfies
      // #{key >= T} == k_sel
      const bool done = (hist[s_bin] == need);
      __syncthreads();
      FIN_STAMP(4 + pass);
      if (done) break;
    }
    T = prefix;
  }
  if (a.mode == 1) return T;
  // compact keys >= T (exactly k_sel of them: keys are unique), pad to pow2
  if (tid == 0) s_cnt = 0;
  for (int i = tid; i < P; i += 256) sbuf[i] = 0ull;
  __syncthreads();
  if (k_sel > 0) {
    for (int64_t i = tid; i < n; i += 256) {
      const uint64_t key = kp[i];
      if (key > T) {
        const unsigned pos = atomicAdd(&s_cnt, 1u);
        if (pos < (unsigned)P) sbuf[pos] = key;
      }
    }
  }
  __syncthreads();
  return T;
}

template <bool FILT = false>
__global__ __launch_bounds__(256) void finalize_kernel(FinArgs a) {
  __shared__ unsigned hist[256];
  extern __shared__ __attribute__((aligned(16))) uint64_t sbuf[];  // [pow2 >= k] (mode 0 only), then [lds_keys] key copy
  __shared__ unsigned s_bin, s_above, s_cnt;
  const int tid = threadIdx.x;
  const int64_t qi = blockIdx.x;
  if (a.zero_me && qi == 0 && tid == 0) *a.zero_me = 0;
  const int64_t q = a.qmap ? a.qmap[qi] : qi;
  const int cnt_raw = a.count ? a.count[q * (a.count_stride > 1 ? a.count_stride : 1)] : (int)a.cap;   // null: full lists
  const int64_t n = cnt_raw < a.cap ? cnt_raw : a.cap;
  const uint64_t* keys = a.cand + (size_t)q * a.cap;
  const int64_t oslot = a.out_slot ? a.out_slot[qi] : qi;

  bool fail = (cnt_raw > a.cap) || (a.need_min > 0 && cnt_raw < a.need_min);
  if constexpr (FILT) {
    const int np = a.n_pass[q * a.n_pass_stride];
    fail = (cnt_raw > a.cap) || cnt_raw < (np < a.k ? np : a.k);
  } else {
    if (a.ivf_thr && cnt_raw < a.k && a.ivf_thr[q] > -INFINITY) fail = true;
  }
  int k_sel = (a.mode == 0) ? a.k : a.rank;
  if (k_sel > n) k_sel = (int)n;
  int P = 64;
  while (P < k_sel) P <<= 1;

  // Small launches (single requests: a handful of workgroups, each a chain of up to 8 dependent passes over its list)
  // copy the list into LDS once and select there: 48 -> 2x us for the 12k-slot lists of one request's probes.
  uint64_t T;
  FIN_STAMP(0);
  if (a.lds_keys > 0 && n <= a.lds_keys) {
    uint64_t* kS = sbuf + a.sort_slots;
    for (int64_t i0 = tid; i0 < n; i0 += 256 * 8) {     // 8 independent loads in flight per thread
      uint64_t v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) { const int64_t i = i0 + u * 256; v[u] = keys[i < n ? i : n - 1]; }
#pragma unroll
      for (int u = 0; u < 8; ++u) { const int64_t i = i0 + u * 256; if (i < n) kS[i] = v[u]; }
    }
    __syncthreads();
    FIN_STAMP(1);
    T = finalize_select(a, kS, n, k_sel, hist, s_bin, s_above, s_cnt, sbuf, P);
  } else {
    T = finalize_select(a, keys, n, k_sel, hist, s_bin, s_above, s_cnt, sbuf, P);
  }

  if (a.mode == 1) {
    // A list with fewer than `rank` real keys has the empty key 0 as its rank-th best: that is no threshold (-inf, every
    // row a candidate), not ord2f(0) -- a NaN that `score >= thr` rejects for every row and that `ivf_thr > -inf`
    // below does not count as a threshold either, so an IVF query with few sampled rows came back empty.
    if (tid == 0)
      a.thr_out[q] = (k_sel > 0 && k_sel == a.rank && (uint32_t)(T >> 32) != 0u) ? ord2f((uint32_t)(T >> 32)) : -INFINITY;
    return;
  }
  FIN_STAMP(2);
  {  // keys are unique except the all-zero padding key: the remaining slots all equal T
    const int cgt = (int)s_cnt;
    for (int i = cgt + tid; i < k_sel; i += 256) sbuf[i] = T;
  }
  __syncthreads();
  // (the hierarchical select's first level hands its k keys to a second finalize, which sorts: no sort here -- 45
  // barrier-separated stages, 12 us, for nothing)
  const bool need_sort = a.out_keys == nullptr || a.thr_chk != nullptr;
  for (int size = 2; need_sort && size <= P; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int i = tid; i < P / 2; i += 256) {
        const int lo = (i / stride) * (stride << 1) + (i % stride);
        const int hi = lo + stride;
        const bool desc = ((lo & size) == 0);
        const uint64_t x = sbuf[lo], y = sbuf[hi];
        if (desc ? (x < y) : (x > y)) { sbuf[lo] = y; sbuf[hi] = x; }
      }
      __syncthreads();
    }
  }
  FIN_STAMP(3);
  if (a.thr_chk && k_sel == a.k && k_sel > 0) {  // completeness proof of the approximate filter
    const float sk = ord2f((uint32_t)(sbuf[k_sel - 1] >> 32));
    if (sk < a.thr_chk[q] + a.eps_scale * a.qnorm[q] + 2e-6f) fail = true;
  }
  if (a.fail_flags && tid == 0) a.fail_flags[q] = fail ? 1 : 0;
  if (fail && a.fail_list && tid == 0) a.fail_list[atomicAdd(a.n_fail, 1)] = (int)q;   // (order immaterial: each is re-done on its own)
  if (a.out_keys) {
    for (int i = tid; i < a.k; i += 256) a.out_keys[oslot * a.k + i] = i < k_sel ? sbuf[i] : 0ull;
    return;
  }
  for (int i = tid; i < a.k; i += 256) {
    float sc = -INFINITY;
    int64_t row = -1;
    if (i < k_sel && sbuf[i] != 0ull) {
      const uint64_t key = sbuf[i];
      sc = ord2f((uint32_t)(key >> 32));
      row = (int64_t)(0xFFFFFFFFu - (uint32_t)(key & 0xFFFFFFFFull));
      if (a.id_map) row = a.id_map[row];
    }
    a.out_scores[oslot * a.k + i] = sc;
    a.out_rows[oslot * a.k + i] = row;
  }
}

// ---- fused refinement of the two-precision search (one workgroup per query, candidates in LDS) ------------------
// segments -> LDS | k-th largest APPROXIMATE score (radix select) | exact f32 re-score of the candidates that can still
// reach the top-k | top-k select + sort of the exact keys | completeness proof -> outputs.  Same selections and the same
// arithmetic as compact_segments_kernel + finalize_kernel(mode 1) + rerank_kernel + finalize_kernel(mode 0), without
// the three candidate-list round trips through HBM and three kernel boundaries.

// k_sel-th largest of n unique keys (LDS or global); returns the prefix T with zero low bytes once every key left in
// the chosen bucket is needed (#{key >= T} == k_sel).  All 256 threads call it; hist/s_bin/s_above are workgroup LDS.
__device__ __forceinline__ uint64_t radix_select_256(const uint64_t* keys, int64_t n, int k_sel, unsigned* hist,
                                                     unsigned* s_bin, unsigned* s_above) {
  const int tid = threadIdx.x, lane = tid & 63;
  uint64_t prefix = 0, mask = 0;
  unsigned need = (unsigned)k_sel;
  for (int pass = 0; pass < 8; ++pass) {
    const int shift = 56 - 8 * pass;
    hist[tid] = 0;
    __syncthreads();
    {  // one atomic per run of equal bins (see finalize_select)
      unsigned run_bin = 0xFFFFFFFFu, run_cnt = 0;
      for (int64_t i = tid; i < n; i += 256) {
        const uint64_t key = keys[i];
        if ((key & mask) == prefix) {
          const unsigned b = (unsigned)(key >> shift) & 255u;
          if (b == run_bin) ++run_cnt;
          else { if (run_cnt) atomicAdd(&hist[run_bin], run_cnt); run_bin = b; run_cnt = 1; }
        }
      }
      if (run_cnt) atomicAdd(&hist[run_bin], run_cnt);
    }
    __syncthreads();
    if (tid < 64) {  // wave 0: suffix scan over bins 255..0, 4 bins per lane
      const int b0 = 255 - 4 * lane;
      const unsigned h0 = hist[b0], h1 = hist[b0 - 1], h2 = hist[b0 - 2], h3 = hist[b0 - 3];
      const unsigned mine = h0 + h1 + h2 + h3;
      unsigned incl = mine;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const unsigned t = __shfl_up(incl, o, 64);
        if (lane >= o) incl += t;
      }
      const unsigned before = incl - mine;
      if (before < need && need <= incl) {
        unsigned c = before;
        int b = b0;
        if (c + h0 >= need) { b = b0; }
        else { c += h0; if (c + h1 >= need) { b = b0 - 1; }
        else { c += h1; if (c + h2 >= need) { b = b0 - 2; }
        else { c += h2; b = b0 - 3; } } }
        *s_bin = (unsigned)b;
        *s_above = c;
      }
    }
    __syncthreads();
    need -= *s_above;
    prefix |= (uint64_t)(*s_bin) << shift;
    mask |= 0xFFull << shift;
    const bool done = (hist[*s_bin] == need);
    __syncthreads();
    if (done) break;
  }
  return prefix;
}

// the part of refine_kernel after the candidate count is known; `ck` is the LDS list (address space inferred after
// inlining: ds_* instructions) or the query's slice of the global scratch list
template <int D>
__device__ __forceinline__ void refine_body(const RefineArgs& a, uint64_t* ck, uint64_t* sbuf, const int n, const int* off,
                                            unsigned* hist, unsigned& s_bin, unsigned& s_above, unsigned& s_cnt,
                                            const float qn, const float (&qv)[D / 16], const int64_t q) {
  constexpr int PER = D / 16;
  const int tid = threadIdx.x, l16 = tid & 15, grp = tid >> 4;
  for (int s = tid >> 6; s < a.nsplit; s += 4) {          // one wave per segment
    const int cnt = off[s + 1] - off[s];
    const uint64_t* src = a.seg + ((size_t)q * a.nsplit + s) * a.seg_cap;
    for (int i = tid & 63; i < cnt; i += 64) ck[off[s] + i] = src[i];
  }
  __syncthreads();
  // ---- k-th largest approximate score (a lower bound of it: the select stops early)
  float kth = -INFINITY;
  if (n >= a.k) kth = ord2f((uint32_t)(radix_select_256(ck, n, a.k, hist, &s_bin, &s_above) >> 32));
  // At least k candidates have an approximate score >= kth, hence exact scores >= kth - eps, so the exact k-th score
  // T* >= kth - eps; a candidate whose approximate score is below kth - 2 eps has an exact score < kth - eps <= T*: it
  // cannot be in the top-k and its row is not fetched (key zeroed).
  const float cut = kth - 2.f * a.eps_scale * qn - 1e-6f;
  // four candidates per lane group and iteration: their row loads are in flight together
  typedef float rowvec __attribute__((ext_vector_type(PER)));
  for (int i0 = grp * 4; i0 < n; i0 += 64) {
    uint32_t row[4];
    bool go[4];
    rowvec xv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = i0 + u;
      const uint64_t key = i < n ? ck[i] : 0ull;
      row[u] = 0xFFFFFFFFu - (uint32_t)(key & 0xFFFFFFFFull);
      go[u] = i < n && (int64_t)row[u] < a.N && !(ord2f((uint32_t)(key >> 32)) < cut);
      if (go[u]) xv[u] = *reinterpret_cast<const rowvec*>(a.X + (size_t)row[u] * D + l16 * PER);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      uint64_t nk = 0ull;
      if (go[u]) {
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < PER; ++j) s = fmaf(qv[j], xv[u][j], s);
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        nk = make_key(s, row[u]);
      }
      if (l16 == 0 && i0 + u < n) ck[i0 + u] = nk;
    }
  }
  __syncthreads();
  // ---- top-k of the exact keys, sorted
  const int64_t need_min = a.k < a.N ? a.k : a.N;
  bool fail = n < need_min;
  int k_sel = a.k < n ? a.k : n;
  uint64_t T = 0;
  if (k_sel > 0) T = radix_select_256(ck, n, k_sel, hist, &s_bin, &s_above);
  int P = 64;
  while (P < k_sel) P <<= 1;
  if (tid == 0) s_cnt = 0;
  for (int i = tid; i < P; i += 256) sbuf[i] = 0ull;
  __syncthreads();
  if (k_sel > 0) {
    for (int i = tid; i < n; i += 256) {
      const uint64_t key = ck[i];
      if (key > T) {
        const unsigned pos = atomicAdd(&s_cnt, 1u);
        if (pos < (unsigned)P) sbuf[pos] = key;
      }
    }
  }
  __syncthreads();
  {  // keys are unique except the all-zero padding key: the remaining slots all equal T
    const int cgt = (int)s_cnt;
    for (int i = cgt + tid; i < k_sel; i += 256) sbuf[i] = T;
  }
  __syncthreads();
  {  // exchanges at distance <= 64 stay inside the 128-key segment one wave owns: barrier only around the others
    int prev = 128;
    for (int size = 2; size <= P; size <<= 1) {
      for (int stride = size >> 1; stride > 0; stride >>= 1) {
        if (stride >= 128 || prev >= 128) __syncthreads();
        else __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        prev = stride;
        for (int i = tid; i < P / 2; i += 256) {
          const int lo = (i / stride) * (stride << 1) + (i % stride);
          const int hi = lo + stride;
          const bool desc = ((lo & size) == 0);
          const uint64_t x = sbuf[lo], y = sbuf[hi];
          if (desc ? (x < y) : (x > y)) { sbuf[lo] = y; sbuf[hi] = x; }
        }
      }
    }
    __syncthreads();
  }
  if (k_sel == a.k && k_sel > 0) {  // completeness proof of the approximate filter
    const float sk = ord2f((uint32_t)(sbuf[k_sel - 1] >> 32));
    if (sk < a.thr[q] + a.eps_scale * qn + 2e-6f) fail = true;
  }
  if (tid == 0) {
    a.fail_flags[q] = fail ? 1 : 0;
    if (fail) a.fail_list[atomicAdd(a.n_fail, 1)] = (int)q;   // (order immaterial: every failed query is re-done on its own)
  }
  for (int i = tid; i < a.k; i += 256) {
    float sc = -INFINITY;
    int64_t row = -1;
    if (i < k_sel && sbuf[i] != 0ull) {
      const uint64_t key = sbuf[i];
      sc = ord2f((uint32_t)(key >> 32));
      row = (int64_t)(0xFFFFFFFFu - (uint32_t)(key & 0xFFFFFFFFull));
      if (a.id_map) row = a.id_map[row];
    }
    a.out_scores[q * a.k + i] = sc;
    a.out_rows[q * a.k + i] = row;
  }
}

template <int D>
__global__ __launch_bounds__(256) void refine_kernel(RefineArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint64_t rbuf[];   // [cap] candidates | [P] sort buffer
  __shared__ unsigned hist[256];
  __shared__ int off[1025];
  __shared__ unsigned s_bin, s_above, s_cnt;
  __shared__ int s_over;
  __shared__ float s_qn;
  constexpr int PER = D / 16;
  const int tid = threadIdx.x, l16 = tid & 15, grp = tid >> 4;
  const int64_t q = blockIdx.x;
  uint64_t* sbuf = rbuf + a.lds_slots;
  {  // exclusive prefix of the (clamped) segment counts: 4 segments per thread, wave scan, 4 wave totals
    int c[4], ov = 0, mine = 0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int sg = tid * 4 + u;
      int v = sg < a.nsplit ? a.seg_cnt[q * a.nsplit + sg] : 0;
      if (v > a.seg_cap) { ov = 1; v = a.seg_cap; }
      c[u] = v; mine += v;
    }
    int incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int t = __shfl_up(incl, o, 64);
      if ((tid & 63) >= o) incl += t;
    }
    if ((tid & 63) == 63) hist[tid >> 6] = (unsigned)incl;
    if (tid == 0) s_over = 0;
    __syncthreads();
    int base = incl - mine;
    for (int w2 = 0; w2 < (tid >> 6); ++w2) base += (int)hist[w2];
    if (ov) s_over = 1;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int sg = tid * 4 + u;
      if (sg <= a.nsplit) off[sg] = base;
      base += c[u];
    }
    if (tid == 255) {   // base = the total here
      off[a.nsplit] = base;
      if (base > a.cap) s_over = 1;
    }
    __syncthreads();
  }
  float qv[PER];
#pragma unroll
  for (int j = 0; j < PER; ++j) qv[j] = a.Q[q * D + l16 * PER + j];
  {
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < PER; ++j) s += qv[j] * qv[j];
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (tid == 0) s_qn = sqrtf(s);
  }
  __syncthreads();
  if (s_over) {   // a segment or the list overflowed: exact re-do of this query (outputs are overwritten by it)
    if (tid == 0) {
      a.fail_flags[q] = 1;
      a.fail_list[atomicAdd(a.n_fail, 1)] = (int)q;
    }
    return;
  }
  const int n = off[a.nsplit];
  if (n <= a.lds_slots) refine_body<D>(a, rbuf, sbuf, n, off, hist, s_bin, s_above, s_cnt, s_qn, qv, q);
  else refine_body<D>(a, a.cand + (size_t)q * a.cap, sbuf, n, off, hist, s_bin, s_above, s_cnt, s_qn, qv, q);
}

__global__ void collect_fail_kernel(const int* __restrict__ flags, int64_t nq, int* list, int* n_fail) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nq && flags[i]) list[atomicAdd(n_fail, 1)] = (int)i;
}

}  // namespace

namespace rihip_index {

int launch_finalize(const FinArgs& f0, unsigned n, hipStream_t st) {
  FinArgs f = f0;
  size_t lds = 0;
  static bool granted = false;
  if (!granted) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(finalize_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)(sizeof(uint64_t) * K_MAX));
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(finalize_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)(sizeof(uint64_t) * K_MAX));
    granted = true;
  }
  int P = 0;
  if (f.mode == 0) {
    P = 64;
    while (P < f.k) P <<= 1;
    lds = sizeof(uint64_t) * (size_t)P;
  }
  // few workgroups (single requests / small batches) whose lists fit: select in LDS instead of 4-8 dependent passes over
  // global memory; large launches keep their occupancy (the LDS copy would cut it to one workgroup per CU)
  f.lds_keys = 0; f.sort_slots = P;
  if (n <= 2u * RIHIP_NCU && f.cap > 0 && (size_t)(P + f.cap) <= (size_t)K_MAX) {
    f.lds_keys = (int)f.cap;
    lds = sizeof(uint64_t) * (size_t)(P + f.cap);
  }
  if (f.n_pass) hipLaunchKernelGGL(finalize_kernel<true>, dim3(n), dim3(256), lds, st, f);
  else hipLaunchKernelGGL(finalize_kernel<false>, dim3(n), dim3(256), lds, st, f);
  return check_launch("finalize");
}

int launch_refine(int d, const RefineArgs& r, int64_t nq, hipStream_t st) {
  static bool granted = false;
  if (!granted) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(refine_kernel<32>), hipFuncAttributeMaxDynamicSharedMemorySize, 8 * (2048 + 2048));
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(refine_kernel<64>), hipFuncAttributeMaxDynamicSharedMemorySize, 8 * (2048 + 2048));
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(refine_kernel<128>), hipFuncAttributeMaxDynamicSharedMemorySize, 8 * (2048 + 2048));
    granted = true;
  }
  int P = 64;   // candidates in LDS, then the sort buffer: the power of two >= k
  while (P < r.k) P <<= 1;
  const size_t lds = sizeof(uint64_t) * (size_t)(r.lds_slots + P);
  RCCHK(dispatch_d(d, [&](auto D) { hipLaunchKernelGGL((refine_kernel<decltype(D)::value>), dim3((unsigned)nq), dim3(256), lds, st, r); }));
  return check_launch("refine");
}

void launch_compact_segments(const uint64_t* seg, const int* seg_cnt, int nsplit, int seg_cap, uint64_t* cand, int64_t cap,
                             int* count, int cs, int64_t nq, hipStream_t st) {
  hipLaunchKernelGGL(compact_segments_kernel, dim3((unsigned)nq), dim3(256), 0, st, seg, seg_cnt, nsplit, seg_cap, cand, cap,
                     count, cs);
}

int launch_rerank(int d, const float* X, const float* Q, uint64_t* cand, int64_t cap, const int* count, float* qnorm,
                  int64_t N, const float* kth_approx, float eps_scale, int cs, int64_t nq, hipStream_t st) {
  return dispatch_d(d, [&](auto D) {
    hipLaunchKernelGGL((rerank_kernel<decltype(D)::value>), dim3((unsigned)nq), dim3(256), 0, st, X, Q, cand, cap, count, qnorm, N, kth_approx,
                       eps_scale, cs);
  });
}

void launch_collect_fail(const int* flags, int64_t nq, int* list, int* n_fail, hipStream_t st) {
  hipLaunchKernelGGL(collect_fail_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, st, flags, nq, list, n_fail);
}

}  // namespace rihip_index

// Handle of the 8-bit scalar-quantised index, the one function that makes a code, and what its units call of each other:
// sq8_build.hip (quantiser, build, handle lifetime, accessors), sq8_scan.hip (the int8 scan), sq8.hip (search driver; plain,
// filtered and excluding search), sq8_refine.hip (attached f32 rows, refined search, certificate), sq8_state.hip (state
// files), sq8_update.hip (add / remove / replace), pq.hip (the product-quantised storage of the same handle: training,
// encoding, decoding) and pq_update.hip (add / remove / replace on that storage).  All eight compile with `#pragma clang fp
// contract(off)` at their top: the quantisers, the query transform, the decode, the refine and the certificate are
// specified operation by operation.
#pragma once
#include "common.h"
#include "ip_index.h"
#include "search_kernels.h"

#include <vector>

namespace rihip_index {

struct Sq8Index {
  int du = 0;        // caller's width (1 .. 128)
  int dk = 0;        // width of the f32 side (centroids, coarse queries): 32 / 64 / 128, as the source index
  int dpad = 0;      // bytes per code row: 64 / 128
  int64_t N = 0, Np = 0;
  int nlist = 0, nprobe = 1;
  int8_t* codes = nullptr;        // [Np, dpad] physical order, padding rows and columns 0 (null on a PQ handle)
  // product-quantised storage (pq.hip) in place of `codes`: the row's SQ8 code is book[m][pq_codes[p][m]][:] per sub-space
  uint8_t* pq_codes = nullptr;    // [Np, M] physical order, M = dpad / pq_dsub; padding rows 0
  int8_t* pq_book = nullptr;      // [M, 256, pq_dsub], entries in [-127, 127]
  int pq_dsub = 0;                // 8 / 16 (0: an SQ8 handle)
  std::vector<int64_t> pq_trace;  // distortion of every assignment pass of the build (empty: injected codebooks, loaded)
  int64_t pq_peak_bytes = 0;      // device bytes at the build's peak (the transient SQ8 codes included)
  double pq_ms[3] = {0, 0, 0};    // host time of the build: range pass + SQ8 encode, codebook training, final assignment
  // residual PQ (by_residual): the codebooks quantise c - K_l, K_l the list's centroid on the SQ8 grid; the decoded code
  // K_l + entry is an int16 in [-254, 254] and the scan adds T[q, l] = sum_j n_j K_l[j] to the gathered dot product
  int8_t* pq_list_codes = nullptr;   // [nlist, dpad], padding columns 0 (null: not a residual handle)
  bool pq_residual = false;
  int64_t pq_clamped = 0;            // residual values of the build that left [-127, 127] (0 after load)
  float* centre = nullptr;       // [dpad] (columns >= du: 0)
  float* scale = nullptr;         // [dpad] (columns >= du: 1)
  float* C = nullptr;             // [nlist, dk]
  int64_t* list_poff = nullptr;   // [nlist+1]
  int* list_len_dev = nullptr;    // [nlist]
  int64_t* row_ids = nullptr;     // [Np] original row, -1 = padding
  std::vector<int64_t> list_len;
  const int64_t* id_map = nullptr;   // not owned
  int64_t stats[2] = {0, 0};         // queries searched thresholded, of those re-done dense
  // filtered search (rihip_sq8_filter_set_tags): one 32-bit tag word per physical row, padding rows 0, or null
  uint32_t* tags = nullptr;          // [Np]
  int64_t filt_stats[2] = {0, 0};    // queries searched filtered, of those re-done dense
  // seen-item exclusion inside the scan (rihip_sq8_exclude_search): as IpIndex's -- the inverse of row_ids (built on first
  // use, dropped with the row order), the mask scratch (all zero between calls) and its budget
  int* inv_pos = nullptr;            // [N] original row -> physical position
  DevBuf<uint32_t> xmask;
  bool xmask_dirty = false;
  int64_t xmask_budget = XMASK_BUDGET;
  int64_t excl_stats[3] = {0, 0, 0};   // queries searched this way, of those re-done dense, mask chunks
  // refined search (rihip_sq8_refine_attach_vectors): the f32 rows next to the codes, or null
  float* vec = nullptr;              // [N, dk] insertion-row order (stage 1 returns rows: no inverse map)
  double* ref_e = nullptr;           // [dk] e_j = max_i |x_ij - (m_j + s_j c_ij)| over the stored rows
  double* ref_a = nullptr;           // [dk] a_j = max_i |x_ij|
  // updates (rihip_sq8_update_apply): calls that changed the index, rows dropped, rows added, code values clamped
  int64_t upd_stats[4] = {0, 0, 0, 0};
  // a PQ handle's updates (rihip_pq_update_apply) next to those: residual values of added rows clamped, the summed
  // smallest D of added rows (both cumulative), and the two of the last update that changed the index
  int64_t pq_upd_stats[4] = {0, 0, 0, 0};
  // scratch
  DevBuf<int8_t> qhi, qlo, fhi, flo;
  DevBuf<float> qt, qpad, fQ, coarse, thr;
  DevBuf<double> qb;
  DevBuf<uint64_t> cand, scand, fcand;
  DevBuf<uint32_t> fpred;            // the predicates of one re-do chunk
  // refined search: stage 1's output at k_scan, the f32 keys, valid candidates and smallest integer score per query
  DevBuf<float> rs;
  DevBuf<int64_t> rr;
  DevBuf<int> ri, rnv, rcut;
  DevBuf<uint64_t> rkeys;
  DevBuf<int> pair_t;                // residual PQ: T of every (query, probed list) pair of one pass, [nq * nprobe]
  DevBuf<int> count, probe_list, list_q, list_cnt, list_qoff, list_cur, work_off, plan, fail_flags, fail_list, n_fail;
  int* h_nfail = nullptr;   // pinned
};

inline bool sq8_has_storage(const Sq8Index* h) { return h && (h->codes || h->pq_codes); }

// ---- sq8_build.hip: the SQ8 build of a fresh handle (layout, row ids, quantiser, codes), the list offsets / lengths on the
// device from the host copy list_len, the bytes a handle holds, its destructor and those of its two optional parts
int sq8_build(Sq8Index* h, const IpIndex* src, const float* centre, const float* scale, hipStream_t st);
int sq8_upload_layout(Sq8Index* h, hipStream_t st);
int64_t sq8_held_bytes(const Sq8Index* h);
void sq8_free(Sq8Index* h);
// the decoded rows (out_x f32 [N, du]) and / or the stored or decoded codes (out_c int8 [N, du]; int16 on a residual PQ
// handle) in original row order on the host; either may be null
int sq8_rows_out(Sq8Index* h, float* out_x, void* out_c);
void sq8_drop_vectors(Sq8Index* h);
void sq8_drop_tags(Sq8Index* h);

// ---- sq8.hip: the search driver
// what a search adds to the plain one: tag predicates (query q's at pred[q * pred_stride]), seen lists (the queries are
// query q_base .. of the batch the lists describe), and whether the result holds mapped ids (h->id_map) or rows
struct Sq8SearchOpts {
  const uint32_t* pred = nullptr;
  int pred_stride = 0;
  const SeenArgs* seen = nullptr;
  int64_t q_base = 0;
  bool map_ids = true;
};
int sq8_search(Sq8Index* h, const float* Q, int64_t nq, int k, int mode, float* out_s, int64_t* out_r, int* out_i, hipStream_t st,
               const Sq8SearchOpts& o);
// what a search entry point was given and what it needs: the argument check of all six (`who` leads every message)
struct Sq8SearchCall {
  const char* who;
  const float* Q; int64_t nq;
  int k, k_scan, mode;          // k_scan > 0: a refined search (vectors attached, 1 <= k <= k_scan <= K_MAX)
  bool outputs;                 // every mandatory output is there
  bool filtered;                // predicates are mandatory (given ones always need a tagged index)
  const uint32_t* pred; int64_t pred_stride;
  const SeenArgs* seen;         // an excluding search: its lists, or null
};
int sq8_check_search(const Sq8Index* h, const Sq8SearchCall& c);
// limb rows, t and b of the queries into the handle's scratch (t_out / b_out null) or the caller's arrays
int sq8_transform_queries(Sq8Index* h, const float* Q, int64_t nq, int16_t* n16, float* t_out, double* b_out, hipStream_t st);
int sq8_ensure_inv_pos(Sq8Index* h, hipStream_t st);   // the handle's inverse of row_ids, made on first use
// X [n, du] device rows -> the same rows at the f32 side's width dk (through the handle's qpad when du != dk); a result
// that is not 16-byte aligned is refused with `misaligned`
int sq8_rows_at_dk(Sq8Index* h, const float*& X, int64_t n, const char* misaligned, hipStream_t st);

// ---- sq8_refine.hip: e_j = max |x_ij - (m_j + s_j c_ij)| and a_j = max |x_ij| over the n_rows physical rows that hold a
// row, in f64.  by_row: the f32 row of physical row r is X[row_ids[r]] (insertion order), else X[r].  part: nb * 2 * dk
// doubles of scratch.  Maxima: the same bits for every nb.
void sq8_launch_ranges(bool by_row, const float* X, const int8_t* codes, const int64_t* row_ids, int64_t n_rows, int dk, int dpad,
                       const float* centre, const float* scale, double* part, int nb, double* e_out, double* a_out, hipStream_t st);
// (the int16 decoded codes of a residual PQ handle)
void sq8_launch_ranges(bool by_row, const float* X, const int16_t* codes, const int64_t* row_ids, int64_t n_rows, int dk, int dpad,
                       const float* centre, const float* scale, double* part, int nb, double* e_out, double* a_out, hipStream_t st);

// ---- sq8_update.hip: everything of an update that does not depend on how the handle stores its codes -- argument and id
// checks, masks, renumbering, the list of every new row, grouping, the one host read in the middle of the call, the new
// offsets, row ids, tag words, attached vectors and the swap -- with the storage's own stages called where they belong.
struct Sq8UpdateCtx {   // what the driver hands a stage; device pointers unless said otherwise
  Sq8Index* h; hipStream_t st;
  const float* X_add; const uint32_t* add_tags; int64_t n_add;    // new rows at width dk; tag words (null: 0, or untagged)
  const int* keep; const int* rscan; const int* pscan;            // keep flag and new number of an old row; kept physical rows before p
  const int* tile_list_old;                                       // list of every old granule
  const int* g_rows; const int* g_keys; const int* g_off;         // new rows grouped by list: row, list, list bounds [nlist+1]
  unsigned long long* words;                                      // the storage's own n_words counters, zero before `encode`
  // from `repack` on: the new layout (row_ids_new / tags_new are written by the storage's repack kernel)
  const unsigned long long* cnt_keep; const int64_t* poff_new; int64_t n_keep, Np_new;
  int64_t* row_ids_new; uint32_t* tags_new;                       // tags_new: null on an untagged handle
  const float* vec_new; double* part; int nb; double* e_new; double* a_new;   // `ranges`: the compacted f32 rows and where e_j / a_j go
};
struct Sq8UpdateStorage {   // one per call, on the caller's stack; its destructor frees what `swap` did not hand over
  const char* who = "";     // leads every message
  int n_words = 0;          // counters of its own that travel to the host with the checks
  virtual int encode(const Sq8UpdateCtx&) { return RIHIP_OK; }   // before the host read (n_add > 0): work on the new rows that counts
  virtual int repack(const Sq8UpdateCtx&) = 0;                   // allocate the new code storage, write every row of [0, Np_new) once
  virtual int ranges(const Sq8UpdateCtx&) = 0;                   // e_j / a_j of the new state (a handle with vectors)
  virtual void swap(Sq8Index* h, const unsigned long long* words_host) = 0;   // install the new codes, book the counters: cannot fail
  virtual ~Sq8UpdateStorage() {}
};
int sq8_update_run(Sq8Index* h, Sq8UpdateStorage& s, const int64_t* item_ids, const int64_t* drop_ids, int64_t n_drop,
                   const float* X_add, const int64_t* add_ids, const uint32_t* add_tags, int64_t n_add, int64_t* item_ids_out,
                   int64_t* n_total, int64_t* n_dropped, int64_t* n_clamped, int64_t* bad_id, int* bad_kind, hipStream_t st);

// ---- sq8_state.hip: one writer and one reader for the SQ8, the PQ and the residual PQ state file.  All are magic[8], n_hdr int64 header
// words {version 1, du, dk, dpad, N, Np, nlist, nprobe, format's own ...}, centre f32[dpad], scale f32[dpad], centroids
// f32[nlist, dk], list lengths int64[nlist], row ids int64[Np], and the format's payload
struct Sq8StateFormat {
  const char* magic;     // 8 characters
  const char* name;      // leads every message: "sq8_index" / "pq_index"
  const char* kind;      // "an SQ8" / "a PQ" / "a residual PQ"
  int n_extra;           // header words of its own behind the common eight (x: those words)
  bool (*extra_ok)(const int64_t* x, int64_t dpad);
  int64_t (*payload_bytes)(const int64_t* x, int64_t Np, int64_t dpad);
  // checks the payload and uploads it into the fresh handle (its sizes are set, nothing else is)
  int (*fill)(Sq8Index* h, const int64_t* x, const int8_t* payload, const char* path);
};
struct Sq8StateBlock { const void* dev; size_t bytes; };   // a piece of the payload on the device
int sq8_state_save(const Sq8Index* h, const char* path, const Sq8StateFormat& f, const int64_t* x, const Sq8StateBlock* blocks,
                   int n_blocks);
int sq8_state_load(const char* path, const Sq8StateFormat& f, void** handle);

// ---- pq.hip: the decoded code matrix [Np, dpad] of a PQ handle in a fresh device allocation the caller frees (a
// transient Np * dpad bytes)
int pq_decode_all(const Sq8Index* h, int8_t** out_dev, hipStream_t st);
// a residual PQ handle: its decoded codes K_l + entry as int16 [Np, dpad] (a transient 2 * Np * dpad bytes)
int pq_decode_all16(const Sq8Index* h, int16_t** out_dev, hipStream_t st);

__device__ __forceinline__ int sq8_code(float x, float m, float s) {
  float v = rintf((x - m) / s);            // one f32 subtraction, one correctly rounded f32 division, round to nearest even
  v = fminf(fmaxf(v, -127.f), 127.f);
  return (int)v;
}

}  // namespace rihip_index

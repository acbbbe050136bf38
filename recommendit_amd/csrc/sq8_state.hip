// State files of the 8-bit index: one writer and one reader over a description of the format (Sq8StateFormat in
// sq8_index.h), and the SQ8 format with its C ABI.  The PQ format is described in pq.hip.
//
// SQ8 file: "RIHIPSQ8", int64 header {version 1, du, dk, dpad, N, Np, nlist, nprobe}, centre f32[dpad], scale f32[dpad],
// centroids f32[nlist, dk], list lengths int64[nlist], row ids int64[Np], codes int8[Np, dpad]
#pragma clang fp contract(off)   // as every unit of the 8-bit index (sq8_index.h)
#include "common.h"
#include "recommendit_hip.h"

#include <math.h>
#include <stdio.h>
#include <string.h>
#include <vector>

#include "sq8_index.h"

using namespace rihip_index;

namespace rihip_index {

int sq8_state_save(const Sq8Index* h, const char* path, const Sq8StateFormat& f, const int64_t* x, const Sq8StateBlock* blocks,
                   int n_blocks) {
  std::vector<float> m(h->dpad), s(h->dpad), C((size_t)h->nlist * h->dk);
  std::vector<int64_t> rid((size_t)h->Np);
  std::vector<std::vector<int8_t>> payload(n_blocks);
  for (int b = 0; b < n_blocks; ++b) payload[b].resize(blocks[b].bytes);
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(m.data(), h->centre, sizeof(float) * m.size(), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(s.data(), h->scale, sizeof(float) * s.size(), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(C.data(), h->C, sizeof(float) * C.size(), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(rid.data(), h->row_ids, sizeof(int64_t) * rid.size(), hipMemcpyDeviceToHost));
  for (int b = 0; b < n_blocks; ++b) HIPCHK(hipMemcpy(payload[b].data(), blocks[b].dev, blocks[b].bytes, hipMemcpyDeviceToHost));
  FILE* fp = fopen(path, "wb");
  RIHIP_REQUIRE(fp, RIHIP_ERR_IO, "%s_save: cannot open %s", f.name, path);
  int64_t hdr[16] = {1, h->du, h->dk, h->dpad, h->N, h->Np, h->nlist, h->nprobe};
  const size_t n_hdr = 8 + (size_t)f.n_extra;
  for (int i = 0; i < f.n_extra; ++i) hdr[8 + i] = x[i];
  bool ok = fwrite(f.magic, 1, 8, fp) == 8 && fwrite(hdr, sizeof(int64_t), n_hdr, fp) == n_hdr &&
            fwrite(m.data(), sizeof(float), m.size(), fp) == m.size() && fwrite(s.data(), sizeof(float), s.size(), fp) == s.size() &&
            fwrite(C.data(), sizeof(float), C.size(), fp) == C.size() &&
            fwrite(h->list_len.data(), sizeof(int64_t), h->nlist, fp) == (size_t)h->nlist &&
            fwrite(rid.data(), sizeof(int64_t), rid.size(), fp) == rid.size();
  for (int b = 0; b < n_blocks; ++b) ok = ok && fwrite(payload[b].data(), 1, payload[b].size(), fp) == payload[b].size();
  ok = (fclose(fp) == 0) && ok;
  RIHIP_REQUIRE(ok, RIHIP_ERR_IO, "%s_save: short write to %s", f.name, path);
  return RIHIP_OK;
}

int sq8_state_load(const char* path, const Sq8StateFormat& f, void** handle) {
  RIHIP_REQUIRE(path && handle, RIHIP_ERR_ARG, "%s_load: bad arguments", f.name);
  FILE* fp = fopen(path, "rb");
  RIHIP_REQUIRE(fp, RIHIP_ERR_IO, "%s_load: cannot open %s", f.name, path);
  char magic[8]; int64_t hdr[16];
  const size_t n_hdr = 8 + (size_t)f.n_extra;
  if (fread(magic, 1, 8, fp) != 8 || memcmp(magic, f.magic, 8) != 0 || fread(hdr, sizeof(int64_t), n_hdr, fp) != n_hdr || hdr[0] != 1) {
    fclose(fp); rihip_set_error("%s_load: %s is not %s index file (magic / version)", f.name, path, f.kind); return RIHIP_ERR_IO;
  }
  const int64_t du = hdr[1], dk = hdr[2], dpad = hdr[3], N = hdr[4], Np = hdr[5], nlist = hdr[6], nprobe = hdr[7];
  const int64_t* x = hdr + 8;
  const bool hdr_ok = du >= 1 && du <= 128 && dk == (du <= 32 ? 32 : (du <= 64 ? 64 : 128)) && dpad == (dk <= 64 ? 64 : 128) &&
                      N >= 1 && N < (1ll << 31) && nlist >= 1 && nlist <= NLIST_MAX && nprobe >= 1 && nprobe < (1ll << 31) &&
                      Np >= N && Np % TR == 0 && Np <= N + (int64_t)TR * nlist && f.extra_ok(x, dpad);
  int64_t expect = 0, have = -1, n_payload = 0;
  if (hdr_ok) {
    n_payload = f.payload_bytes(x, Np, dpad);
    expect = 8 + 8 * (int64_t)n_hdr + 8 * dpad + 4 * nlist * dk + 8 * nlist + 8 * Np + n_payload;
    if (fseek(fp, 0, SEEK_END) == 0) have = (int64_t)ftell(fp);
    if (fseek(fp, 8 + 8 * (long)n_hdr, SEEK_SET) != 0) have = -1;
  }
  if (!hdr_ok || have != expect) {
    fclose(fp);
    rihip_set_error("%s_load: %s: %s", f.name, path, hdr_ok ? "file size does not match its header (truncated?)" : "header field out of range");
    return RIHIP_ERR_IO;
  }
  std::vector<float> m(dpad), s(dpad), C((size_t)nlist * dk);
  std::vector<int64_t> ll(nlist), rid((size_t)Np);
  std::vector<int8_t> payload((size_t)n_payload);
  bool ok = fread(m.data(), sizeof(float), m.size(), fp) == m.size() && fread(s.data(), sizeof(float), s.size(), fp) == s.size() &&
            fread(C.data(), sizeof(float), C.size(), fp) == C.size() && fread(ll.data(), sizeof(int64_t), nlist, fp) == (size_t)nlist &&
            fread(rid.data(), sizeof(int64_t), rid.size(), fp) == rid.size() && fread(payload.data(), 1, payload.size(), fp) == payload.size();
  fclose(fp);
  RIHIP_REQUIRE(ok, RIHIP_ERR_IO, "%s_load: short read from %s", f.name, path);
  int64_t tot = 0, ptot = 0;
  for (int64_t c = 0; c < nlist; ++c) {
    RIHIP_REQUIRE(ll[c] >= 0 && ll[c] <= N, RIHIP_ERR_IO, "%s_load: %s: list %lld has length %lld", f.name, path, (long long)c, (long long)ll[c]);
    tot += ll[c]; ptot += (ll[c] + TR - 1) / TR * TR;
  }
  RIHIP_REQUIRE(tot == N && ptot == Np, RIHIP_ERR_IO, "%s_load: %s: list lengths do not add up to the header's row counts", f.name, path);
  for (int64_t p = 0; p < Np; ++p)
    RIHIP_REQUIRE(rid[p] >= -1 && rid[p] < N, RIHIP_ERR_IO, "%s_load: %s: row id %lld out of range", f.name, path, (long long)rid[p]);
  for (int64_t j = 0; j < dpad; ++j)
    RIHIP_REQUIRE(isfinite(m[j]) && isfinite(s[j]) && s[j] > 0.f, RIHIP_ERR_IO, "%s_load: %s: quantiser column %lld is not finite", f.name, path, (long long)j);
  Sq8Index* h = new Sq8Index();
  h->du = (int)du; h->dk = (int)dk; h->dpad = (int)dpad; h->N = N; h->Np = Np; h->nlist = (int)nlist; h->nprobe = (int)nprobe;
  h->list_len = ll;
  auto fill = [&]() -> int {
    RCCHK(f.fill(h, x, payload.data(), path));
    RCCHK(sq8_upload_layout(h, 0));
    HIPCHK(hipMalloc((void**)&h->row_ids, sizeof(int64_t) * rid.size()));
    HIPCHK(hipMalloc((void**)&h->C, sizeof(float) * C.size()));
    HIPCHK(hipMalloc((void**)&h->centre, sizeof(float) * dpad));
    HIPCHK(hipMalloc((void**)&h->scale, sizeof(float) * dpad));
    HIPCHK(hipMemcpy(h->row_ids, rid.data(), sizeof(int64_t) * rid.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->C, C.data(), sizeof(float) * C.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->centre, m.data(), sizeof(float) * dpad, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->scale, s.data(), sizeof(float) * dpad, hipMemcpyHostToDevice));
    return RIHIP_OK;
  };
  const int rc = fill();
  if (rc) { sq8_free(h); return rc; }
  *handle = h;
  return RIHIP_OK;
}

}  // namespace rihip_index

namespace {

int sq8_fill(Sq8Index* h, const int64_t*, const int8_t* payload, const char*) {
  const size_t n = (size_t)h->Np * h->dpad;
  HIPCHK(hipMalloc((void**)&h->codes, n));
  HIPCHK(hipMemcpy(h->codes, payload, n, hipMemcpyHostToDevice));
  return RIHIP_OK;
}

const Sq8StateFormat SQ8_FORMAT = {
    "RIHIPSQ8", "sq8_index", "an SQ8", 0,
    [](const int64_t*, int64_t) { return true; },
    [](const int64_t*, int64_t Np, int64_t dpad) { return Np * dpad; },
    sq8_fill,
};

}  // namespace

extern "C" int rihip_sq8_index_save(void* handle, const char* path) {
  Sq8Index* h = (Sq8Index*)handle;
  RIHIP_REQUIRE(h && path, RIHIP_ERR_ARG, "sq8_index_save: bad arguments");
  RIHIP_REQUIRE(!h->pq_codes, RIHIP_ERR_STATE, "sq8_index_save: a PQ index has a file format of its own (rihip_pq_index_save)");
  RIHIP_REQUIRE(h->codes, RIHIP_ERR_STATE, "sq8_index_save: index is empty");
  const Sq8StateBlock codes{h->codes, (size_t)h->Np * h->dpad};
  return sq8_state_save(h, path, SQ8_FORMAT, nullptr, &codes, 1);
}

extern "C" int rihip_sq8_index_load(const char* path, void** handle) { return sq8_state_load(path, SQ8_FORMAT, handle); }

/*
 * rgb_wal_host.cpp -- the host-only half of include/ra_gpu_wal.h: record layout and the WAL file walk
 * of recover_records/5.  No HIP here, so the file also builds on its own under the sanitizers
 * (tests/test_wal_framing.py::test_scan_under_sanitizers).
 */
#include <stdint.h>
#include <vector>
#include "../../include/ra_gpu_wal.h"

extern "C" uint64_t rgb_wal_layout(rgb_wal_record *records, uint32_t n, uint64_t base) {
  for (uint32_t i = 0; i < n; ++i) {
    records[i].out_offset = base;
    base += (uint64_t)records[i].hdr_len + 24u + records[i].data_len;   /* DataSize, src/ra_log_wal.erl:526 */
  }
  return base;
}

/* ---- recovery: the record walk of recover_records/5 (src/ra_log_wal.erl:877-984), host code ---- */
namespace {
inline uint64_t be(const unsigned char *p, int nbytes) {
  uint64_t v = 0;
  for (int k = 0; k < nbytes; ++k) v = (v << 8) | p[k];
  return v;
}
}  // namespace

extern "C" int rgb_wal_scan(const void *bytes, uint64_t n_bytes, rgb_wal_scanned *out, uint32_t cap,
                            uint32_t *n_out, uint64_t *consumed, uint32_t *end) {
  if (!bytes || !n_out || !consumed || !end) return RGB_E_INVAL;
  const bool count_only = out == nullptr;              /* out = NULL: count the records, store nothing */
  const unsigned char *b = (const unsigned char *)bytes;
  /* <<"RAWA", 1:8/unsigned>> (:34-36, :826-835) */
  if (n_bytes < 5 || b[0] != 'R' || b[1] != 'A' || b[2] != 'W' || b[3] != 'A' || b[4] != 1) return RGB_E_INVAL;
  std::vector<bool> named(1u << 22, false);             /* IdRefs introduced by a long header so far */
  uint64_t pos = 5;
  uint32_t n = 0;
  *end = RGB_WAL_END_DATA;
  for (;;) {
    const uint64_t left = n_bytes - pos;
    if (left < 3) break;
    const uint32_t h = (uint32_t)be(b + pos, 3);
    const uint32_t trunc = h >> 23, form = (h >> 22) & 1u, id_ref = h & 0x3FFFFFu;
    uint64_t fixed = pos + 3;                           /* -> Checksum */
    uint32_t uid_len = 0;
    uint64_t uid_off = 0;
    if (form == 0) {
      if (left < 5) break;
      uid_len = (uint32_t)be(b + pos + 3, 2);
      uid_off = pos + 5;
      fixed = uid_off + uid_len;
    }
    if (fixed + 8 > n_bytes) break;
    const uint32_t checksum = (uint32_t)be(b + fixed, 4), data_len = (uint32_t)be(b + fixed + 4, 4);
    /* first clause: an all-zero record ends a pre-allocated file (:877-883) */
    if (h == 0 && checksum == 0 && data_len == 0) { *end = RGB_WAL_END_ZEROS; break; }
    if (fixed + 24 > n_bytes || fixed + 24 + (uint64_t)data_len > n_bytes) break;
    if (count_only) {
      if (form == 0) named[id_ref] = true;
      n += 1;
      pos = fixed + 24 + data_len;
      continue;
    }
    if (n == cap) { *end = RGB_WAL_END_CAP; break; }
    rgb_wal_scanned &r = out[n++];
    r.index = be(b + fixed + 8, 8);
    r.term = be(b + fixed + 16, 8);
    r.data_offset = fixed + 24;
    r.data_len = data_len;
    r.checksum = checksum;
    r.uid_offset = uid_off;
    r.id_ref = id_ref;
    r.uid_len = (uint16_t)uid_len;
    r.trunc = (uint8_t)trunc;
    r.next_offset = fixed + 24 + data_len;
    if (form == 0) {
      named[id_ref] = true;
      r.flags = RGB_WAL_REC_FIRST | RGB_WAL_REC_VALIDATE;
    } else {
      r.flags = named[id_ref] ? RGB_WAL_REC_VALIDATE : RGB_WAL_REC_UNKNOWN;
    }
    pos = r.next_offset;
  }
  *n_out = n;
  *consumed = pos;
  return RGB_OK;
}


/* ---- WAL batch: validation, the stable per-writer order of the commands, the bound ---------------------- */

/* The validation of every rgb_wal_batch call, and in the same pass what the device kernels take as staged input:
 * wstart[w] (n_writers + 1 values) = the commands of the writers in front of w, order[wstart[w] ..) = the positions of
 * w's commands, ascending.  order / wstart may be NULL (both): validation and sums only.  *payload_bytes = the sum of
 * data_len, *header_bytes = the sum of 2 + uid_len over the writers, *longest = the most commands of one writer. */
extern "C" int rgb_wal_batch_check(const rgb_wal_cmd *cmds, uint32_t n, const rgb_wal_writer *writers, uint32_t n_writers,
                                   const rgb_wal_file *file, uint64_t data_bytes, uint32_t flags, uint32_t *order,
                                   uint32_t *wstart, uint64_t *payload_bytes, uint64_t *header_bytes, uint32_t *longest) {
  if (!file || (n && !cmds) || (n_writers && !writers) || (flags & ~RGB_WAL_NO_CHECKSUMS)) return RGB_E_INVAL;
  if ((order == nullptr) != (wstart == nullptr)) return RGB_E_INVAL;
  auto slice_ok = [&](uint64_t off, uint64_t len) { return off <= data_bytes && len <= data_bytes - off; };
  uint64_t unnamed = 0, hdr = 0, pay = 0;
  for (uint32_t w = 0; w < n_writers; ++w) {
    const rgb_wal_writer &wr = writers[w];
    if (wr.state > RGB_WAL_W_OUT_OF_SEQ || wr.uid_len > 65535u || !slice_ok(wr.uid_offset, wr.uid_len)) return RGB_E_INVAL;
    if (wr.id_ref == RGB_WAL_NO_ID_REF) unnamed += 1;
    else if (wr.id_ref >= RGB_WAL_MAX_ID_REFS) return RGB_E_INVAL;
    hdr += 2u + wr.uid_len;
  }
  if (file->next_id_ref > RGB_WAL_MAX_ID_REFS || unnamed > RGB_WAL_MAX_ID_REFS - file->next_id_ref) return RGB_E_INVAL;
  for (uint32_t i = 0; i < n; ++i) {
    if (cmds[i].writer >= n_writers || !slice_ok(cmds[i].data_offset, cmds[i].data_len)) return RGB_E_INVAL;
    pay += cmds[i].data_len;
  }
  uint32_t most = 0;
  if (wstart) {                                         /* counting sort by writer: stable, so mailbox order within one */
    for (uint32_t w = 0; w <= n_writers; ++w) wstart[w] = 0;
    for (uint32_t i = 0; i < n; ++i) wstart[cmds[i].writer + 1u] += 1u;
    for (uint32_t w = 0; w < n_writers; ++w) {
      most = wstart[w + 1u] > most ? wstart[w + 1u] : most;
      wstart[w + 1u] += wstart[w];
    }
    for (uint32_t i = 0; i < n; ++i) order[wstart[cmds[i].writer]++] = i;   /* wstart[w] is now the END of w ... */
    for (uint32_t w = n_writers; w > 0; --w) wstart[w] = wstart[w - 1u];       /* ... which is the start of w + 1 */
    wstart[0] = 0;
  }
  if (payload_bytes) *payload_bytes = pay;
  if (header_bytes) *header_bytes = hdr;
  if (longest) *longest = most;
  return RGB_OK;
}

extern "C" int rgb_wal_batch_bound(const rgb_wal_cmd *cmds, uint32_t n, const rgb_wal_writer *writers, uint32_t n_writers,
                                   const rgb_wal_file *file, uint64_t data_bytes, uint64_t *out_bound,
                                   uint32_t *events_bound, uint32_t *ranges_bound) {
  if (!out_bound || !events_bound || !ranges_bound) return RGB_E_INVAL;
  uint64_t pay = 0, hdr = 0;
  const int rc = rgb_wal_batch_check(cmds, n, writers, n_writers, file, data_bytes, 0u, nullptr, nullptr, &pay, &hdr, nullptr);
  if (rc) return rc;
  *out_bound = pay + 27ull * n + hdr;                   /* 3 + 24 per record, and 2 + uid_len more for each long header */
  *events_bound = n;
  *ranges_bound = n;
  return RGB_OK;
}

/* the emulated library (tests/native) builds the WAL sources as one unit: the segment part rides along */
#ifdef RGB_HOST_EMULATION
#include "rgb_segment.hip"
#include "rgb_segment_host.cpp"
#endif

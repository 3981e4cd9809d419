/*
 * ra_gpu_wal.h -- batched WAL entry checksums, record framing and recovery validation for
 * libra_gpu_batch.
 *
 * The reference checksums every WAL record with Adler-32 over the entry as it is framed on disk,
 *
 *     Entry    = [<<Idx:64/unsigned, Term:64/unsigned>> | EntryData],
 *     Checksum = erlang:adler32(Entry)                       (src/ra_log_wal.erl:528-534)
 *     Record   = [HeaderData, <<Checksum:32/integer, EntryDataLen:32/unsigned>> | Entry]
 *
 * when writing (compute_checksums = true) and again for every record it reads back
 * (validate_checksum, src/ra_log_wal.erl:861, 873, 1028).  erlang:adler32/1 is zlib's Adler-32
 * (RFC 1950 section 8.2).  This entry point computes the checksums of a whole batch of entries
 * whose payload bytes are resident in device memory; framing, file I/O, fsync and the
 * durability decision stay on the host, exactly as in ra_log_wal.
 *
 * Plain C ABI: device pointers and sizes only.
 */
#ifndef RA_GPU_WAL_H
#define RA_GPU_WAL_H
#include "ra_gpu_batch.h"
#ifdef __cplusplus
extern "C" {
#endif

/* One WAL entry of the batch, 32 bytes.  The payload is data[data_offset .. data_offset+data_len)
 * of the batch's data buffer (any alignment, any length including 0). */
typedef struct rgb_wal_entry {
  uint64_t index;        /* Idx  -- framed big endian, as <<Idx:64/unsigned>>  */
  uint64_t term;         /* Term -- framed big endian, as <<Term:64/unsigned>> */
  uint64_t data_offset;
  uint32_t data_len;     /* EntryDataLen */
  uint32_t _pad;
} rgb_wal_entry;

/* d_checksums[i] = adler32(<<index:64, term:64, payload/binary>>) for the n entries of d_entries.
 * d_data must be readable for 16-byte aligned accesses around every payload (allocate the buffer
 * 16 bytes longer than its content; hipMalloc aligns its start).  Enqueued on `stream` (NULL = the
 * context's stream); no synchronisation.  Replaces erlang:adler32/1 at src/ra_log_wal.erl:532
 * (write path) and :861/:873/:1028 (recovery: compare with the stored Checksum on the host). */
int rgb_wal_adler32_device(rgb_ctx *ctx, const void *d_entries, uint32_t n, const void *d_data,
                           uint64_t data_bytes, void *d_checksums, void *stream);

/* Host-buffer form (what the NIF binds): entries and the packed payload bytes come from host
 * memory, the n checksums go back to host memory.  Stages through device buffers the context
 * keeps (grown on demand), synchronises before returning: PCIe-inclusive. */
int rgb_wal_adler32(rgb_ctx *ctx, const rgb_wal_entry *entries, uint32_t n, const void *data,
                    uint64_t data_bytes, uint32_t *checksums);

/* ---- record framing (write path) ---------------------------------------------------------
 *
 * The reference writes, per entry (src/ra_log_wal.erl:513-537),
 *
 *     Record = [HeaderData, <<Checksum:32/integer, EntryDataLen:32/unsigned>>,
 *               <<Idx:64/unsigned, Term:64/unsigned>> | EntryData]
 *
 * where HeaderData is what serialize_header/3 (:482-499) returns: 3 bytes <<Trunc:1, 1:1, IdRef:22>>
 * for a writer already named in this file, or <<Trunc:1, 0:1, IdRef:22, IdDataLen:16, UId/binary>>
 * on its first appearance.  The writer-name cache is a map of binaries and stays on the host; the
 * host hands the HeaderData bytes over verbatim (inside the batch's data buffer) and the device
 * produces the batch's contiguous on-disk bytes -- checksum, lengths, big-endian cursors and the
 * payload copy -- in one pass over the payload.  Writing the bytes to the file, fsync and the
 * `written` notifications stay in ra_log_wal. */
typedef struct rgb_wal_record {
  uint64_t index;        /* Idx  */
  uint64_t term;         /* Term */
  uint64_t data_offset;  /* EntryData = data[data_offset .. +data_len) */
  uint32_t data_len;     /* EntryDataLen */
  uint32_t hdr_len;      /* byte_size(HeaderData): 3, or 5 + IdDataLen */
  uint64_t hdr_offset;   /* HeaderData = data[hdr_offset .. +hdr_len) */
  uint64_t out_offset;   /* where the record starts in the output (rgb_wal_layout fills it) */
} rgb_wal_record;

#define RGB_WAL_NO_CHECKSUMS 1u   /* compute_checksums = false: Checksum = 0 (src/ra_log_wal.erl:531-534) */

/* Host helper: out_offset of every record when they are written back to back from `base`
 * (DataSize = HeaderLen + 24 + EntryDataLen each); returns the offset behind the last one. */
uint64_t rgb_wal_layout(rgb_wal_record *records, uint32_t n, uint64_t base);

/* d_out[out_offset ..) = the framed record, for the n records of d_records.  d_checksums (may be
 * NULL) receives the n checksums as well.  d_data and d_out may have any alignment (payloads are read and written
 * in 16-byte pieces at their own byte alignment), d_out must hold the highest out_offset + record size; records may
 * not overlap.  Only the payload's own bytes are read, only the record's own bytes are written.  `flags`:
 * RGB_WAL_NO_CHECKSUMS.  Enqueued on `stream`, no synchronisation. */
int rgb_wal_frame_device(rgb_ctx *ctx, const void *d_records, uint32_t n, const void *d_data,
                         uint64_t data_bytes, void *d_out, uint64_t out_bytes, void *d_checksums,
                         uint32_t flags, void *stream);

/* Host-buffer form: records (out_offset filled, e.g. by rgb_wal_layout from 0) and data in host
 * memory, the framed bytes [0, out_bytes) back into `out`.  Synchronises; PCIe-inclusive. */
int rgb_wal_frame(rgb_ctx *ctx, const rgb_wal_record *records, uint32_t n, const void *data,
                  uint64_t data_bytes, void *out, uint64_t out_bytes, uint32_t flags);

/* ---- recovery (read path) ---------------------------------------------------------------
 *
 * recover_records/5 (src/ra_log_wal.erl:884-984) walks a WAL file record by record; every record of
 * a known writer is validated with validate_checksum/4 (:1022-1033) before it is recovered.  The
 * walk is a dependent chain over a few header bytes per record and is host code here
 * (rgb_wal_scan); the checksums of all records it finds are one device batch (rgb_wal_validate). */
typedef struct rgb_wal_scanned {
  uint64_t index;
  uint64_t term;
  uint64_t data_offset;  /* EntryData inside the file bytes */
  uint32_t data_len;
  uint32_t checksum;     /* the stored Checksum */
  uint64_t uid_offset;   /* UId bytes inside the file (first appearance only) */
  uint32_t id_ref;       /* IdRef:22 */
  uint16_t uid_len;      /* IdDataLen (first appearance only) */
  uint8_t  trunc;        /* Trunc:1 */
  uint8_t  flags;        /* RGB_WAL_REC_* */
  uint64_t next_offset;  /* file offset behind this record (`Rest`) */
} rgb_wal_scanned;

#define RGB_WAL_REC_FIRST    1u  /* long header: first appearance of the writer in this file */
#define RGB_WAL_REC_VALIDATE 2u  /* to be checksum-validated; the caller clears it for writers that are
                                    not registered (ra_directory:is_registered_uid, :902).  The scan
                                    cannot ask the directory, so it treats every long header as
                                    introducing its IdRef: for a writer the caller finds unregistered
                                    the reference leaves the IdRef out of its cache (:902-904, :929-931) and
                                    skips that writer's later short-header records (:968-971) — the
                                    caller must therefore clear VALIDATE on EVERY later record of that
                                    id_ref in this file, not only on the RGB_WAL_REC_FIRST one */
#define RGB_WAL_REC_UNKNOWN  4u  /* short header whose IdRef was never introduced: skipped (:968-971) */

#define RGB_WAL_END_ZEROS 0u     /* all-zero record: end of a pre-allocated file (:877-883) */
#define RGB_WAL_END_DATA  1u     /* not enough bytes left for a whole record: end of file (:973-984) */
#define RGB_WAL_END_CAP   2u     /* `cap` records written, more may follow from *consumed */

/* Parse `bytes` (a whole WAL file including its 5-byte "RAWA", version 1 header, :826-835; an
 * unknown header gives RGB_E_INVAL) into at most `cap` records.  out = NULL counts the records of the
 * file into *n_out without storing them (size the array, then scan again).  Pure host code. */
int rgb_wal_scan(const void *bytes, uint64_t n_bytes, rgb_wal_scanned *out, uint32_t cap,
                 uint32_t *n_out, uint64_t *consumed, uint32_t *end);

#define RGB_WAL_CLEAN        0u  /* every validated record matched */
#define RGB_WAL_DROPPED_LAST 1u  /* record *n_ok failed its checksum and is the last one: dropped,
                                    recovery resumes (is_last_record/3, :994-1004) */
#define RGB_WAL_CORRUPT      2u  /* record *n_ok failed and data follows: the reference throws
                                    wal_checksum_validation_failure (:1006-1008) */

/* Validate the scanned records of a file in order (stored Checksum 0 = "checksum not used", always
 * ok, :1022-1024).  *n_ok = number of leading records that are good, *status = RGB_WAL_*. */
int rgb_wal_validate(rgb_ctx *ctx, const void *bytes, uint64_t n_bytes, const rgb_wal_scanned *recs,
                     uint32_t n, uint32_t *n_ok, uint32_t *status);

/* ==== WAL batch: one mailbox-ordered batch of append commands in one call ========================
 *
 * ra_log_wal:handle_batch/2 for a batch of {append, ...} messages of any number of writers: the gap detection and
 * smallest-live-index drop of handle_msg/2 (src/ra_log_wal.erl:551-586), serialize_header/3 with its writer-name
 * cache (:482-499), the roll test (should_roll_wal/1, :1050-1066), the framed bytes of write_data/8 (:501-548) and the
 * `written` events of incr_batch/8 and complete_batch_writer/3 (:596-635, :800-812).
 *
 * Per command, in mailbox order, with Trunc = (index == smallest_index) and the writer's state
 * undefined | {in_seq, P} | {out_of_seq, P}; the clauses are tried in this order:
 *   1. index < smallest_index                 DROP; the state becomes {in_seq, smallest_index - 1}
 *   2. state {_, P}, prev_index =< P or Trunc  WRITE with Trunc
 *   3. state undefined                         WRITE with Trunc = false
 *   4. state {out_of_seq, _}                   IGNORE; the state stays
 *   5. state {in_seq, P}                       RESEND, value = P + 1; the state becomes {out_of_seq, P}
 * A WRITE first runs the roll test on the file as the commands before it left it: file_size > max_size, or
 * max_entries != 0 and entry_count + 1 > max_entries.  The first WRITE command that finds it true is NOT consumed:
 * status ROLL, n_consumed = its position, and verdicts, writer rows, bytes and events cover the commands before it.
 * The caller writes the bytes, sends the events, rolls the file and calls again from that command with a fresh
 * rgb_wal_file (and id_ref = RGB_WAL_NO_ID_REF in every writer row).  Otherwise the record is framed: 3 header bytes
 * <<Trunc:1, 1:1, IdRef:22>> for a writer that has an id_ref, else <<Trunc:1, 0:1, Next:22, IdDataLen:16, UId/binary>>
 * with id_ref = next_id_ref, which rises by one (mailbox order of first appearance); then
 * <<Checksum:32, EntryDataLen:32, Idx:64, Term:64>> and the payload.  The state becomes {in_seq, index}, entry_count
 * rises by one, and file_size by the reference's DataSize -- which counts a HeaderLen of 2 for the 3 bytes of a known
 * writer with Trunc set (:484-485): the roll test and the returned file_size use that accounted size, offsets into
 * `out` the real one.
 *
 * Events: per writer the consumed WRITE commands fall into runs of consecutive commands with equal (term, tid); each
 * run is one event, oldest first.  Its indexes are those of its commands that are smaller than every later index of
 * the run (ra_seq:append(Idx, ra_seq:limit(Idx - 1, Seq))), not below the smallest_index of the run's LAST command
 * (ra_seq:floor/2): never empty.  Event rows are sorted by (writer, run order); an event owns range_n ascending, not
 * adjacent (first, last) pairs of uint64_t from pair range_first of the pair list -- the form rgb_submit_seq takes.
 *
 * `cmds` and `writers` are HOST arrays in both forms: validated on the host and staged by the library, which also
 * orders the commands by writer (one counting pass).  RGB_E_INVAL, nothing enqueued and nothing written: a writer slot
 * >= n_writers, a payload or uid outside the data buffer, uid_len > 65535, an unknown state, id_ref >= 2^22 (other than
 * RGB_WAL_NO_ID_REF), next_id_ref + the writers without an id_ref > 2^22, unknown flags, NULLs.  n == 0 is legal.
 * rollover, forget_writer and query messages, a UId whose Pid changes (a slot is one {UId, Pid}), update_ranges/5,
 * roll_over/1, counters, file I/O and sync stay with the caller, which splits its batch there.
 *
 * SPACE: out_bytes, events_cap or ranges_cap is too small; the total says what is needed.  `out` is not touched; the
 * command rows (checksums included), the writer rows and the total are written as they would be; the event rows and
 * the pair list are written whenever both fit their caps.
 *
 * Seven launches whatever n and n_writers are.  The scratch lives in the context (released by rgb_close): one batch
 * call per context at a time.  Only a payload's and a uid's own bytes are read, only the records' own bytes written. */
typedef struct rgb_wal_cmd {         /* 64 bytes */
  uint32_t writer;                   /* slot in `writers` */
  uint32_t data_len;
  uint64_t index, term;
  uint64_t prev_index;               /* ExpectedPrevIdx; -1 (index 0) is passed as 0: the same against every P >= 0 */
  uint64_t smallest_index;           /* smallest_live_index/2 as read for THIS message (:554) */
  uint64_t tid;                      /* MtTid, an opaque value compared for equality */
  uint64_t data_offset;              /* payload = data[data_offset .. + data_len) */
  uint64_t _pad;
} rgb_wal_cmd;

#define RGB_WAL_W_UNDEFINED  0u
#define RGB_WAL_W_IN_SEQ     1u
#define RGB_WAL_W_OUT_OF_SEQ 2u
#define RGB_WAL_NO_ID_REF    0xFFFFFFFFu   /* the writer is not in this file's writer-name cache */
#define RGB_WAL_MAX_ID_REFS  (1u << 22)

typedef struct rgb_wal_writer {      /* 32 bytes, in and out */
  uint32_t state;                    /* RGB_WAL_W_* */
  uint32_t id_ref;                   /* or RGB_WAL_NO_ID_REF */
  uint64_t prev_index;               /* P; ignored with RGB_WAL_W_UNDEFINED */
  uint64_t uid_offset;               /* UId = data[uid_offset .. + uid_len) */
  uint32_t uid_len, _pad;
} rgb_wal_writer;

typedef struct rgb_wal_file {        /* 40 bytes; the total returns the fields that change */
  uint64_t file_size, entry_count;
  uint64_t max_size, max_entries;    /* max_entries 0 = undefined */
  uint32_t next_id_ref, _pad;
} rgb_wal_file;

#define RGB_WAL_V_NOT_CONSUMED 0u
#define RGB_WAL_V_WRITE        1u
#define RGB_WAL_V_DROP         2u
#define RGB_WAL_V_IGNORE       3u
#define RGB_WAL_V_RESEND       4u
#define RGB_WAL_V_MASK         0xFFu
#define RGB_WAL_V_TRUNC        0x100u  /* WRITE: the record's Trunc bit */
#define RGB_WAL_V_FIRST        0x200u  /* WRITE: the long header (first appearance in this file) */

typedef struct rgb_wal_cmd_result {  /* 16 bytes, one per command */
  uint32_t verdict;                  /* RGB_WAL_V_* | flags */
  uint32_t checksum;                 /* WRITE: the record's Checksum (0 with RGB_WAL_NO_CHECKSUMS) */
  uint64_t value;                    /* WRITE: the record's offset in `out`; RESEND: P + 1; otherwise 0 */
} rgb_wal_cmd_result;

typedef struct rgb_wal_event {       /* 32 bytes: {written, Term, Seq} to one writer, with the run's MtTid */
  uint32_t writer, range_first;
  uint64_t term, tid;
  uint32_t range_n, _pad;
} rgb_wal_event;

#define RGB_WAL_BATCH_OK    0u
#define RGB_WAL_BATCH_ROLL  1u       /* command n_consumed found the roll test true */
#define RGB_WAL_BATCH_SPACE 2u       /* wins over ROLL; n_consumed still says where the call would have ended */

typedef struct rgb_wal_batch_total { /* 64 bytes */
  uint32_t status, n_consumed;
  uint32_t n_written, n_events;
  uint32_t n_ranges, next_id_ref;
  uint64_t out_bytes;                /* OK, ROLL: bytes of `out` written; SPACE: bytes needed */
  uint64_t file_size, entry_count;   /* of the file behind the consumed commands (accounted size) */
  uint64_t _pad[2];
} rgb_wal_batch_total;

/* Host helper, pure: the validation of the calls below, and sizes that always suffice: *out_bound = the payload bytes
 * + 27 * n + the sum of 2 + uid_len over the writers, *events_bound = *ranges_bound = n. */
int rgb_wal_batch_bound(const rgb_wal_cmd *cmds, uint32_t n, const rgb_wal_writer *writers, uint32_t n_writers,
                        const rgb_wal_file *file, uint64_t data_bytes, uint64_t *out_bound, uint32_t *events_bound,
                        uint32_t *ranges_bound);

/* d_results: n rgb_wal_cmd_result rows, d_writers_out: n_writers rgb_wal_writer rows, d_events: events_cap
 * rgb_wal_event rows, d_ranges: 2 * ranges_cap uint64_t, *d_total: one rgb_wal_batch_total -- all in device memory,
 * 8-byte aligned; d_data and d_out may have any alignment.  flags: RGB_WAL_NO_CHECKSUMS.  Enqueued on `stream`
 * (NULL = the context's stream), no synchronisation. */
int rgb_wal_batch_device(rgb_ctx *ctx, const rgb_wal_cmd *cmds, uint32_t n, const rgb_wal_writer *writers,
                         uint32_t n_writers, const rgb_wal_file *file, const void *d_data, uint64_t data_bytes,
                         uint32_t flags, void *d_results, void *d_writers_out, void *d_out, uint64_t out_bytes,
                         void *d_events, uint32_t events_cap, void *d_ranges, uint32_t ranges_cap, void *d_total,
                         void *stream);
/* Host-buffer form: synchronises.  `out` (its first out_bytes bytes) is written with the status OK or ROLL only;
 * events and ranges (their first n_events rows / n_ranges pairs) whenever both fit. */
int rgb_wal_batch(rgb_ctx *ctx, const rgb_wal_cmd *cmds, uint32_t n, const rgb_wal_writer *writers, uint32_t n_writers,
                  const rgb_wal_file *file, const void *data, uint64_t data_bytes, uint32_t flags,
                  rgb_wal_cmd_result *results, rgb_wal_writer *writers_out, void *out, uint64_t out_bytes,
                  rgb_wal_event *events, uint32_t events_cap, uint64_t *ranges, uint32_t ranges_cap,
                  rgb_wal_batch_total *total);

/* ==== segments and snapshots: batched CRC-32 ===============================================
 *
 * Everything Ra writes behind the WAL is checksummed with erlang:crc32 -- zlib's CRC-32 (reflected
 * polynomial 0xEDB88320, initial value and final xor 0xFFFFFFFF; the CRC of "123456789" is 0xCBF43926,
 * of nothing 0):
 *
 *   - every entry a mem-table flush appends to a segment file (src/ra_log_segment.erl:277, compute_checksum
 *     :1240-1243), validated again on every read (:670, validate_checksum :1245-1248);
 *   - the segment file itself: <<"RASG", Version:16, MaxCount:16>> (:41-43, :1118-1122), MaxCount index
 *     records <<Idx:64, Term:64, DataOffset:64, Length:32, Crc:32>> (version 2, 32 bytes; version 1 has a
 *     32-bit DataOffset and 28 bytes, :44-45, :1197-1219), then the payloads back to back from
 *     8 + MaxCount * 32 (data_start, :247);
 *   - one CRC over a whole snapshot file, also chunk by chunk as erlang:crc32(Old, Chunk) while a
 *     snapshot is received (src/ra_log_snapshot.erl:57, 81, 94, 107, 256; src/ra_snapshot.erl:1020, 1038).
 *
 * Device forms enqueue on `stream` (NULL = the context's stream) and do not synchronise; host-buffer forms
 * stage through device buffers the context keeps and synchronise (PCIe-inclusive).  Only a payload's own
 * bytes are read (16-byte pieces at the payload's own alignment), only the file's own bytes are written:
 * no padding is needed around d_data or d_out, which may have any alignment.  The stream form keeps its
 * partial values in a buffer of the context: one stream-form call per context at a time. */
typedef struct rgb_seg_entry {
  uint64_t index;        /* Idx  */
  uint64_t term;         /* Term */
  uint64_t data_offset;  /* payload = data[data_offset .. +data_len); from a scan: the absolute file offset */
  uint32_t data_len;     /* Length */
  uint32_t crc;          /* from a scan: the stored Crc; ignored on input */
} rgb_seg_entry;

#define RGB_SEG_NO_CHECKSUMS   1u   /* compute_checksums = false: Crc = 0 (src/ra_log_segment.erl:1240-1241) */
#define RGB_SEG_VERSION        2u
#define RGB_SEG_HEADER_BYTES   8u
#define RGB_SEG_RECORD_BYTES   32u  /* version 2 */
#define RGB_SEG_RECORD_BYTES_V1 28u

/* d_crcs[i] = crc32(payload i) for the n entries of d_entries.  An entry whose payload does not lie inside
 * [0, data_bytes) is skipped (its d_crcs slot is not written). */
int rgb_crc32_device(rgb_ctx *ctx, const void *d_entries, uint32_t n, const void *d_data,
                     uint64_t data_bytes, void *d_crcs, void *stream);
/* Host-buffer form; a payload outside data_bytes is RGB_E_INVAL. */
int rgb_crc32(rgb_ctx *ctx, const rgb_seg_entry *entries, uint32_t n, const void *data,
              uint64_t data_bytes, uint32_t *crcs);

/* *d_crc (one uint32_t in device memory) = erlang:crc32(init, Data) for one long buffer; init = 0 starts a
 * new checksum, chaining calls over consecutive chunks gives the checksum of the whole. */
int rgb_crc32_stream_device(rgb_ctx *ctx, const void *d_data, uint64_t n_bytes, uint32_t init,
                            void *d_crc, void *stream);
int rgb_crc32_stream(rgb_ctx *ctx, const void *data, uint64_t n_bytes, uint32_t init, uint32_t *crc_out);

/* Host helper: out_offsets[i] = the absolute file offset of payload i (DataOffset) when the n payloads are
 * written back to back, in the caller's order, behind MaxCount index records; returns the file size.
 * out_offsets may be NULL. */
uint64_t rgb_segment_layout(const rgb_seg_entry *entries, uint32_t n, uint32_t max_count,
                            uint64_t *out_offsets);

/* d_out[0 .. file size) = the segment file: header, n index records in the caller's order (the reference
 * does not sort), zeros for the MaxCount - n unused records, the payload copies.  CRC and copy share the one
 * read of each payload.  d_out_offsets = the n offsets rgb_segment_layout returned, in device memory.
 * n > max_count, max_count > 65535, out_bytes below the index region or unknown flags: RGB_E_INVAL, nothing
 * is enqueued.  Whether the segment is full (count or max_size) is the caller's decision.  An entry whose
 * payload lies outside d_data, or whose copy would lie outside out_bytes, is skipped by the kernel. */
int rgb_segment_build_device(rgb_ctx *ctx, const void *d_entries, uint32_t n, uint32_t max_count,
                             const void *d_out_offsets, const void *d_data, uint64_t data_bytes,
                             void *d_out, uint64_t out_bytes, uint32_t flags, void *stream);
/* Host-buffer form: lays the file out itself; out_bytes below the file size or a payload outside data_bytes
 * is RGB_E_INVAL and `out` is not written.  Bytes of `out` behind the file size are never written. */
int rgb_segment_build(rgb_ctx *ctx, const rgb_seg_entry *entries, uint32_t n, uint32_t max_count,
                      const void *data, uint64_t data_bytes, void *out, uint64_t out_bytes, uint32_t flags);

#define RGB_SEG_END_ZEROS     0u   /* an all-zero index record: the end of the index (:1199-1201) */
#define RGB_SEG_END_FULL      1u   /* MaxCount records read */
#define RGB_SEG_END_TRUNCATED 2u   /* the file ends inside the index region, or record *n_out points behind
                                      the end of the file: it is counted out, never read */
#define RGB_SEG_END_CAP       3u   /* `cap` records stored, more follow */

/* read_header/1 + the index walk (src/ra_log_segment.erl:1124-1138, 1197-1219) over the bytes of a whole
 * segment file: unknown magic, fewer than 8 bytes, Version 0 or Version > 2 is RGB_E_INVAL.  out = NULL
 * counts the records into *n_out.  Pure host code. */
int rgb_segment_scan(const void *bytes, uint64_t n_bytes, rgb_seg_entry *out, uint32_t cap, uint32_t *n_out,
                     uint32_t *version_out, uint32_t *max_count_out, uint32_t *end);

/* validate_checksum/2 (:1245-1248) for the scanned records in order: a stored Crc of 0 means "not
 * checked" and is always good.  *n_ok = the number of leading good records. */
int rgb_segment_validate(rgb_ctx *ctx, const void *bytes, uint64_t n_bytes, const rgb_seg_entry *recs,
                         uint32_t n, uint32_t *n_ok);

/* ==== major compaction: what is in a segment file, and the copy of its live entries ======================
 *
 * ra_log_segments:major_compaction/3 (src/ra_log_segments.erl:741-835) asks every file of a compaction group what
 * is in it (ra_log_segment:info/2, src/ra_log_segment.erl:736-790, parse_index_info :1080-1116), opens one new
 * segment whose MaxCount is the number of live indexes and copies the live entries of every source into it with
 * ra_log_segment:copy/3 (:819-869), which keeps each entry's stored Crc (append_raw/6, :873-908).
 *
 * The index walk of a source (parse_index_data_loop, :1057-1075) reads records from byte 8 until the first all-zero
 * record, MaxCount records, or the end of the file inside the index region.  The records form a map Idx => entry; a
 * record whose Idx is smaller than its predecessor's first removes every key greater than its own Idx.  Read in
 * parallel: record j is in the final map ("effective") iff Idx_j is smaller than every later record's Idx -- the
 * effective records are strictly ascending in file order, which is the order copy/3 wants (lists:sort of the live
 * indexes), so nothing is ever sorted.
 *
 * Choosing which live indexes belong to which source (ra_seq:in_range/2 and the progressive ra_seq:limit/2 of
 * src/ra_log_segments.erl:745-761) and grouping (take_group, :911-950) are the host helpers of "major compaction
 * for many members in one call" below.  File I/O, renames, symlinks and compaction markers stay with the caller.
 *
 * All sources of a group lie in ONE files buffer; the live indexes of all sources in ONE list of (first, last) pairs
 * of uint64_t (2 * n_live values), each source owning a slice of it.  Within a slice the pairs are ascending and
 * not adjacent (first <= last, last + 1 < next first): the form rgb_submit_seq takes a ra_seq in.  `sources` and
 * `live` are HOST arrays in every form: they are validated on the host (a malformed slice, a source outside the
 * files buffer, too many sources: RGB_E_INVAL, nothing enqueued) and staged by the library.
 *
 * The scratch plan of a call lives in the context (released by rgb_close): one info / compact call per context at a
 * time.  Only a file's own bytes are read, only the new image's own bytes are written, whatever the alignment of
 * d_files and d_out; payloads move in 16-byte pieces at the payload's own alignment. */
typedef struct rgb_seg_source {
  uint64_t offset;       /* the file = files[offset .. offset + n_bytes) */
  uint64_t n_bytes;
  uint32_t live_first;   /* this source's live indexes: pairs live_first .. live_first + live_n of the live list */
  uint32_t live_n;       /* 0: nothing is copied from this source */
  uint64_t _pad;
} rgb_seg_source;

/* info/2 of one source (src/ra_log_segment.erl:763-772) */
typedef struct rgb_seg_info {
  uint64_t size;          /* Offset + Length of the last record walked; index_size when there is none */
  uint64_t index_size;    /* data_start = 8 + MaxCount * record size */
  uint64_t live_size;     /* sum of Length over EVERY walked record whose Idx is live (all records without a live list) */
  uint64_t range_first;   /* update_range/2 (:919-922): the smallest Idx walked ...            } undefined when        */
  uint64_t range_last;    /* ... and the Idx of the last record walked                         } num_entries == 0      */
  uint32_t num_entries;   /* records walked, trimmed and overwritten ones included */
  uint32_t num_indexes;   /* effective records: ra_seq:length(indexes) */
  uint32_t max_count;
  uint32_t version;       /* 1 or 2; 0 with RGB_SEG_COMPACT_BAD_SOURCE */
  uint32_t status;        /* RGB_SEG_COMPACT_OK or RGB_SEG_COMPACT_BAD_SOURCE */
  uint32_t _pad;
} rgb_seg_info;

typedef struct rgb_seg_compact_result {
  uint32_t status;        /* RGB_SEG_COMPACT_* */
  uint32_t n_entries;     /* index records written (MaxCount when OK) */
  uint64_t file_bytes;    /* size of the new image (OK and SPACE) */
  uint64_t index;         /* MISSING, FULL, TRUNCATED, CRC: the index the status is about */
  uint32_t source;        /* ... and its source (BAD_SOURCE: the first bad one) */
  uint32_t _pad;
} rgb_seg_compact_result;

/* A non-zero status means the reference would have crashed: the contents of the output buffer are then unspecified
 * (the host-buffer form leaves `out` unwritten).  BAD_SOURCE comes first; then the first entry in copy order (sources
 * in the caller's order, indexes ascending) that is MISSING, TRUNCATED or FULL, tested in that order; SPACE; and CRC
 * only when everything else is in order. */
#define RGB_SEG_COMPACT_OK         0u
#define RGB_SEG_COMPACT_MISSING    1u  /* exit({copy_missing_key, Idx}) (:864-869): a live index that is not in its source */
#define RGB_SEG_COMPACT_FULL       2u  /* {error, full} from append_raw: payload bytes already appended > max_size (:1250-1255) */
#define RGB_SEG_COMPACT_TRUNCATED  3u  /* the payload of a SELECTED record lies outside its file */
#define RGB_SEG_COMPACT_SPACE      4u  /* out_bytes < file_bytes */
#define RGB_SEG_COMPACT_CRC        5u  /* RGB_SEG_COMPACT_VERIFY: the first copied payload that does not match its stored Crc */
#define RGB_SEG_COMPACT_BAD_SOURCE 6u  /* bad magic, fewer than 8 bytes, Version 0 or > 2 (device forms; the host-buffer
                                          forms see the bytes and answer RGB_E_INVAL) */

#define RGB_SEG_COMPACT_VERIFY      1u    /* flag: CRC-32 of every copied payload in the read that copies it, compared
                                             with the stored Crc (0 = not checked, validate_checksum/2 :1245-1248).
                                             Without the flag the copy does no table lookups at all. */
#define RGB_SEG_COMPACT_MAX_SOURCES 256u
#define RGB_SEG_MAX_SIZE_DEFAULT    64000000ull   /* ?SEGMENT_MAX_SIZE_B, src/ra.hrl:227 */

/* Host helper, pure: validates the descriptors (as every call below does) and returns through *bound_out
 * 8 + 32 * MaxCount + the sum of the sources' n_bytes -- always enough for the new image, no device work -- and
 * through *max_count_out MaxCount = the number of live indexes.  MaxCount > 65535 is RGB_E_INVAL (the header field
 * has 16 bits); 0 is legal (a header-only 8-byte image).  A caller that has the info rows may size tighter:
 * 8 + 32 * MaxCount + the sum of live_size. */
int rgb_segment_compact_bound(const rgb_seg_source *sources, uint32_t n_sources, const uint64_t *live, uint32_t n_live,
                              uint64_t files_bytes, uint64_t *bound_out, uint32_t *max_count_out);

/* d_infos[s] = info/2 of source s.  live = NULL (n_live = 0): every record counts into live_size and the sources'
 * slices are ignored.  Enqueued on `stream` (NULL = the context's stream), no synchronisation. */
int rgb_segment_info_device(rgb_ctx *ctx, const rgb_seg_source *sources, uint32_t n_sources, const void *d_files,
                            uint64_t files_bytes, const uint64_t *live, uint32_t n_live, void *d_infos, void *stream);
/* Host-buffer form; a source with a bad header is RGB_E_INVAL. */
int rgb_segment_info(rgb_ctx *ctx, const rgb_seg_source *sources, uint32_t n_sources, const void *files,
                     uint64_t files_bytes, const uint64_t *live, uint32_t n_live, rgb_seg_info *infos);

/* d_out[0 .. file_bytes) = the new segment: <<"RASG", 2:16, MaxCount:16>>, the index records of the live entries in
 * copy order with the SOURCE's stored Crc (0 included) and DataOffsets counted from 8 + 32 * MaxCount, the payloads
 * back to back.  An index that is live in two sources is copied twice, as the reference does.  *d_result = one
 * rgb_seg_compact_result in device memory.  max_size: the reference's default is RGB_SEG_MAX_SIZE_DEFAULT.  Unknown
 * flags: RGB_E_INVAL.  Three launches (four with VERIFY) on `stream`, no synchronisation. */
int rgb_segment_compact_device(rgb_ctx *ctx, const rgb_seg_source *sources, uint32_t n_sources, const void *d_files,
                               uint64_t files_bytes, const uint64_t *live, uint32_t n_live, uint64_t max_size,
                               uint32_t flags, void *d_out, uint64_t out_bytes, void *d_result, void *stream);
/* Host-buffer form: synchronises; `out` is written (its first file_bytes bytes only) when the status is OK. */
int rgb_segment_compact(rgb_ctx *ctx, const rgb_seg_source *sources, uint32_t n_sources, const void *files,
                        uint64_t files_bytes, const uint64_t *live, uint32_t n_live, uint64_t max_size, uint32_t flags,
                        void *out, uint64_t out_bytes, rgb_seg_compact_result *result);

/* ==== major compaction for many members in one call: the plan, and the batched copy ====================
 *
 * A snapshot or a released cursor makes many members of a node compact at once, each with a few small groups.  The
 * calls below serve all of them together: three pure host helpers restate the plan of major_compaction/3 -- which
 * live indexes belong to which file, which files form a group -- and one device call copies ANY number of groups of
 * ANY number of sources, each group failing on its own.  Between the plan and the copy the caller writes its
 * .compaction_group markers (src/ra_log_segments.erl:783-786); renames, symlinks, deletes and sync_dir stay with the
 * caller too.
 *
 * rgb_segment_compact_select: the fold of major_compaction/3 (src/ra_log_segments.erl:745-761) and of
 * minor_compaction/2 (:843-854) for M members.  A member owns a slice of `segrefs` -- (range_first, range_last) pairs
 * of uint64_t in the order compactable_segrefs/2 gives them, newest first -- and a slice of `live`, pairs in the form
 * described above (live_n = 0: an empty or undefined sequence).  Per segref, in slice order: its selection is the
 * member's live indexes inside {Start, min(End, ceiling)} (ra_seq:in_range/2 over the progressively limited Live);
 * `ceiling` starts unbounded and drops to min(ceiling, End) only behind a segref whose selection was not empty
 * (ra_seq:limit/2); an empty selection leaves Live as it was.  Nothing is assumed about the order of the ranges: what
 * the reference's fold gives for overlapping or ascending ranges is what comes out.  A segref with
 * range_first > range_last selects nothing (the reference's `undefined` range).
 *
 * picks[k] (one row per segref): the selection as pairs live_first .. live_first + live_n of `live_out`, clipped to
 * the effective range; num_live = ra_seq:length of it (saturating at 2^64 - 1); flags = RGB_SEG_PICK_UNREFERENCED when
 * it is empty -- exactly the Delete list of both compaction kinds.  The rows of the segrefs that members name are
 * written (a row of a segref that no member's slice names is NOT written at all: it keeps what the caller put there),
 * the pairs of `live_out` back to back in segref order, so picks[k].live_first / live_n are a source's live_first /
 * live_n as they are.  *n_live_out = the pairs written.  Segrefs whose ranges do not overlap never need more than
 * n_live + n_segrefs pairs; picks = NULL and live_out = NULL is the sizing form: nothing but the exact *n_live_out.
 * RGB_E_INVAL, nothing written: a slice outside its list, segref slices not ascending by segref_first or not
 * disjoint, live pairs not ascending / adjacent / first > last, more than live_out_cap (or 2^32 - 1) pairs. */
typedef struct rgb_seg_member {
  uint32_t segref_first, segref_n;   /* pairs segref_first .. segref_first + segref_n of `segrefs`, newest first */
  uint32_t live_first, live_n;       /* pairs live_first .. live_first + live_n of `live` */
} rgb_seg_member;

typedef struct rgb_seg_pick {
  uint64_t num_live;
  uint32_t live_first, live_n;       /* in live_out */
  uint32_t flags;                    /* RGB_SEG_PICK_UNREFERENCED or 0 */
  uint32_t _pad;
} rgb_seg_pick;
#define RGB_SEG_PICK_UNREFERENCED 1u

int rgb_segment_compact_select(const rgb_seg_member *members, uint32_t n_members, const uint64_t *segrefs,
                               uint32_t n_segrefs, const uint64_t *live, uint32_t n_live, rgb_seg_pick *picks,
                               uint64_t *live_out, uint32_t live_out_cap, uint32_t *n_live_out);

/* rgb_segment_compact_take_groups: compaction_groups/3 with take_group/3 (src/ra_log_segments.erl:901-950) per
 * member.  A member owns the slice src_first .. src_first + src_n of `infos` and `num_live`: its compactable sources
 * OLDEST first (the order the fold's reversal produces), each with its info row (rgb_segment_info with the source's
 * selection as the live list) and NumLive = ra_seq:length of that selection -- the length of the slice, not the number
 * of live records found.  group_of[s] = the ordinal of the source's group within its member, counted from 0 in the
 * order the groups are taken, or RGB_SEG_GROUP_NONE for a source that is skipped (or that no member names);
 * members[m].n_groups = the groups.
 *
 * A source is compactable iff NumLive / NumEnts < 0.5 orelse LiveSz / (Sz - IdxSz) < 0.5; the ratios are compared as
 * integers (2 * NumLive < NumEnts), which is the float comparison exactly while both operands are below 2^53.
 * Over the remaining budgets (MaxCnt - NumLive < 0 orelse MaxSz - LiveSz < 0) with nothing accumulated: the source is
 * skipped; with a group accumulated: the group is closed and the source STAYS for the next one; not compactable with
 * a group accumulated: the group is closed and the source is dropped.  The budgets start again with every group.
 * NumEnts == 0, and Sz - IdxSz == 0 when the first test was false (orelse), are badarith in the reference: the member
 * gets status RGB_SEG_TAKE_BADARITH, no groups and RGB_SEG_GROUP_NONE throughout; other members are unaffected.
 * RGB_E_INVAL, nothing written: a slice outside n_sources, slices not ascending by src_first or not disjoint. */
typedef struct rgb_seg_take_member {
  uint32_t src_first, src_n;         /* in */
  uint32_t n_groups, status;         /* out: RGB_SEG_TAKE_OK / RGB_SEG_TAKE_BADARITH */
} rgb_seg_take_member;
#define RGB_SEG_TAKE_OK       0u
#define RGB_SEG_TAKE_BADARITH 1u
#define RGB_SEG_GROUP_NONE    0xFFFFFFFFu

int rgb_segment_compact_take_groups(rgb_seg_take_member *members, uint32_t n_members, const rgb_seg_info *infos,
                                    const uint64_t *num_live, uint32_t n_sources, uint64_t max_count, uint64_t max_size,
                                    uint32_t *group_of);

/* One compaction group of a batched call: the sources src_first .. src_first + src_n of the call's `sources`, oldest
 * first, and the bytes of `out` its image may use.  Groups own disjoint, ascending slices of `sources` (a file that
 * belongs to two groups is named by two sources); a source no group names is not copied from.  The live slices of
 * the sources that groups name are either the same from their first pair on (the same live_first) or disjoint: a pair
 * of the live list that two such sources reach from different live_first is RGB_E_INVAL for the call (its rank within
 * its source is kept per pair). */
typedef struct rgb_seg_group {
  uint32_t src_first, src_n;
  uint64_t out_offset;               /* the image = out[out_offset .. out_offset + file_bytes), any byte offset */
  uint64_t out_bytes;                /* SPACE is tested against this */
} rgb_seg_group;

/* Host helper, pure: validates groups, sources and live slices as the calls below do and lays the images out back to
 * back without padding: groups[g].out_offset and out_bytes = 8 + 32 * MaxCount_g + the sum of the group's sources'
 * n_bytes are FILLED IN, *total_out = their sum, max_counts[g] (NULL: not wanted) = MaxCount_g.  A group with
 * MaxCount > 65535 is RGB_E_INVAL for the call, as rgb_segment_compact_bound treats it; a group of no sources or no
 * live indexes is legal: its image is the 8-byte header.  No cap on sources or groups beyond uint32_t (and
 * 2^32 - 257 live indexes in all). */
int rgb_segment_compact_groups_bound(rgb_seg_group *groups, uint32_t n_groups, const rgb_seg_source *sources,
                                     uint32_t n_sources, const uint64_t *live, uint32_t n_live, uint64_t files_bytes,
                                     uint64_t *total_out, uint32_t *max_counts);

/* The batched copy.  Per group g: d_out[out_offset_g ..) and d_results[g] (rgb_seg_compact_result rows in device
 * memory) are EXACTLY what rgb_segment_compact_device gives for that group alone with out_bytes_g -- every status,
 * the precedence documented above, `source` counted within the group, the source's stored Crc, an index live in two
 * sources copied twice.  A group that fails leaves its neighbours' images and rows as they are; its own output bytes
 * are unspecified.  `groups`, `sources` and `live` are HOST arrays, validated before anything is enqueued
 * (RGB_E_INVAL: what rgb_segment_compact_groups_bound refuses, a group's out range outside out_bytes, out ranges that
 * overlap, unknown flags, NULLs).  RGB_SEG_COMPACT_VERIFY is the only flag.
 *
 * Launches: resolve (one workgroup per source), place (one lane per group: the walk of the single-group call, the
 * row, and the 8 header bytes of a good image), copy (GROUP lanes per plan entry across all groups; the width is
 * chosen once per call from the mean of the sources' bytes per live index), finish (VERIFY: the first mismatch in
 * copy order PER GROUP).  The scratch plan is sized from the call and kept in the context: one such call per context
 * at a time.  Only an image's own bytes are written, whatever the alignment of d_out and of the offsets. */
int rgb_segment_compact_groups_device(rgb_ctx *ctx, const rgb_seg_group *groups, uint32_t n_groups,
                                      const rgb_seg_source *sources, uint32_t n_sources, const void *d_files,
                                      uint64_t files_bytes, const uint64_t *live, uint32_t n_live, uint64_t max_size,
                                      uint32_t flags, void *d_out, uint64_t out_bytes, void *d_results, void *stream);
/* Host-buffer form: synchronises; results[g] as above (a source with a bad header is BAD_SOURCE of its group here
 * too: a batch across members survives one bad file); of `out` only the good images' own bytes are written. */
int rgb_segment_compact_groups(rgb_ctx *ctx, const rgb_seg_group *groups, uint32_t n_groups,
                               const rgb_seg_source *sources, uint32_t n_sources, const void *files, uint64_t files_bytes,
                               const uint64_t *live, uint32_t n_live, uint64_t max_size, uint32_t flags, void *out,
                               uint64_t out_bytes, rgb_seg_compact_result *results);

/* ==== mem-table flush: the entries of many writers appended to their segment files in one call ==========
 *
 * When a WAL file rolls over, ra_log_segment_writer flushes the mem tables of every writer that had entries in it
 * (flush_mem_table_ranges/2, src/ra_log_segment_writer.erl:268-329): per writer the entries are appended to the
 * writer's open segment, and a successor is opened whenever append/4 answers {error, full} (append_to_segment/6,
 * :425-500; ra_log_segment:append/4 and is_full/1, src/ra_log_segment.erl:252-292, 1250-1255; flush/1, :316-338).
 * One call here does that for W writers: it splits each writer's entries over its open segment and successors by the
 * reference's rule, computes the CRCs while it copies the payloads and returns the exact bytes the host has to
 * pwrite, with a table that says where each run of bytes goes.
 *
 * The rule.  Per writer, in entry order, the state is (count c, data bytes b, file k), at first (open_count,
 * open_data_bytes, 0).  Before each entry the file is full iff c >= MaxCount of this file or b > max_size (strictly
 * greater, and tested BEFORE the append: a file may exceed max_size by one entry, and a fresh file always takes at
 * least one entry).  A full file is left: k += 1, c = 0, b = 0, MaxCount = the call's max_count.  The entry then gets
 * DataOffset = 8 + 32 * MaxCount + b and its record <<Idx:64, Term:64, DataOffset:64, Length:32, Crc:32>> at
 * 8 + 32 * c; then c += 1, b += Length.  The range of a file becomes {min(First, Idx), Idx} (update_range/2,
 * :919-922): the LAST index wins even when it is lower.  An open segment that is already full yields no piece of
 * ordinal 0: the writer's first piece then has ordinal 1.
 *
 * A piece is one run of appended entries in ONE file: two pwrites (index records, payloads).  Pieces are stored sorted
 * by (writer, ordinal); `out` is packed in that order without padding: the 8 header bytes (ordinal > 0 only), the index
 * records, the payloads.
 *
 * File I/O, fsync, file naming (zpad_filename_incr), maybe_open_new_segment, the ra_seq:floor / in_range / limit
 * selection of which indexes to flush, term_to_iovec and the `segments` notification stay with the caller.  Only
 * version-2 open segments are served: a writer whose open file is version 1 finishes that file through the reference
 * path.  The sums open_data_bytes + payload bytes are the caller's to keep below 2^64.
 *
 * `writers` is a HOST array in every form: validated on the host, staged by the library.  RGB_E_INVAL, nothing
 * enqueued: a slice outside n_entries, slices not ascending by entry_first or not disjoint, open_max_count or
 * max_count outside 1 .. 65535, open_count > open_max_count, a range that is not (undefined iff open_count == 0,
 * otherwise range_first <= range_last), unknown flags.  Entries that no slice names are ignored. */
typedef struct rgb_seg_writer {      /* 48 bytes */
  uint32_t entry_first, entry_n;     /* this writer's entries = entries[entry_first .. +entry_n), in append order */
  uint32_t open_count;               /* index records already in its open segment: (index_offset - 8) / 32 */
  uint32_t open_max_count;           /* MaxCount of the OPEN segment's header (successors take the call's max_count) */
  uint64_t open_data_bytes;          /* data_offset - data_start of the open segment */
  uint64_t range_first, range_last;  /* ra_log_segment:range/1 of the open segment; both RGB_UNDEF iff open_count == 0 */
  uint64_t _pad;
} rgb_seg_writer;

typedef struct rgb_seg_piece {       /* 80 bytes: one run of appended entries in ONE file */
  uint32_t writer, ordinal;          /* ordinal 0 = the open segment, k = its k-th successor */
  uint32_t entry_first, entry_n;     /* global entry numbers; entry_n >= 1 always */
  uint64_t index_file_off;           /* pwrite target of the index bytes: 8 + 32 * records already in the file */
  uint64_t data_file_off;            /* pwrite target of the payload bytes */
  uint64_t out_index_off;            /* out[out_index_off .. + 32 * entry_n) = the index records; when ordinal > 0 the 8
                                        bytes in front of it are the header <<"RASG", 2:16, MaxCount:16>> */
  uint64_t out_data_off, data_bytes; /* out[out_data_off .. + data_bytes) = the payloads back to back */
  uint64_t range_first, range_last;  /* the file's range after the piece */
  uint32_t max_count, _pad;          /* of this file */
} rgb_seg_piece;

typedef struct rgb_seg_flush_result {
  uint32_t status;        /* RGB_SEG_FLUSH_* */
  uint32_t n_pieces;      /* OK: rows written; SPACE: rows needed */
  uint64_t out_bytes;     /* OK: bytes of `out` written; SPACE: bytes needed */
  uint32_t writer, entry; /* ENTRY: the entry the status is about and its writer */
  uint64_t _pad;
} rgb_seg_flush_result;

#define RGB_SEG_FLUSH_OK    0u
#define RGB_SEG_FLUSH_SPACE 1u   /* out_bytes or pieces_cap too small; n_pieces and out_bytes say what is needed */
#define RGB_SEG_FLUSH_ENTRY 2u   /* device form: the first entry, in entry order, whose payload lies outside d_data
                                    (looked at before SPACE) */

/* Host helper, pure: the descriptor validation of the calls below, and sizes that always suffice:
 * *pieces_bound = n_entries (a piece holds at least one entry), *out_bound = data_bytes + 32 * n_entries +
 * 8 * n_entries. */
int rgb_segment_flush_bound(const rgb_seg_writer *writers, uint32_t n_writers, uint32_t n_entries, uint64_t data_bytes,
                            uint64_t *out_bound, uint32_t *pieces_bound);

/* d_entries: n_entries rgb_seg_entry rows in device memory (crc ignored), d_pieces: room for pieces_cap rgb_seg_piece
 * rows (8-byte aligned), *d_result: one rgb_seg_flush_result; d_data and d_out may have any alignment.  d_pieces and
 * d_out are written only when the status is OK, and then only their first n_pieces rows / out_bytes bytes.  flags:
 * RGB_SEG_NO_CHECKSUMS.  Three launches on `stream` (NULL = the context's stream), no synchronisation.  The plan
 * scratch lives in the context (released by rgb_close): one flush call per context at a time. */
int rgb_segment_flush_device(rgb_ctx *ctx, const rgb_seg_writer *writers, uint32_t n_writers, const void *d_entries,
                             uint32_t n_entries, const void *d_data, uint64_t data_bytes, uint32_t max_count,
                             uint64_t max_size, uint32_t flags, void *d_pieces, uint32_t pieces_cap, void *d_out,
                             uint64_t out_bytes, void *d_result, void *stream);
/* Host-buffer form: synchronises; a payload outside `data` is RGB_E_INVAL; `pieces` and `out` are written only when
 * the status is OK. */
int rgb_segment_flush(rgb_ctx *ctx, const rgb_seg_writer *writers, uint32_t n_writers, const rgb_seg_entry *entries,
                      uint32_t n_entries, const void *data, uint64_t data_bytes, uint32_t max_count, uint64_t max_size,
                      uint32_t flags, rgb_seg_piece *pieces, uint32_t pieces_cap, void *out, uint64_t out_bytes,
                      rgb_seg_flush_result *result);

/* ==== reading entries back: read plans, folds and term queries over many segment files in one call =======
 *
 * The read half of ra_log_segment: read_sparse/4 and read_sparse_no_checks/4 (src/ra_log_segment.erl:375-598), fold/6,7
 * and fold0 (:340-359, :661-689), term_query/2 (:652-659), driven over many files by ra_log_segments:exec_read_plan/6,
 * segment_sparse_read, segment_fold and segment_term_query (src/ra_log_segments.erl:398-622).  One call reads any number
 * of segment files ("sources", of any number of groups): for every requested index one rgb_seg_entry row
 * (Idx, Term, where the payload is, Length, the stored Crc), the payloads packed back to back in request order.
 *
 * All sources lie in ONE files buffer, all requests in ONE flat list `req` of indexes, each source owning a slice of
 * it, in the caller's order: ascending, descending, repeated -- whatever a read_sparse index list may be; a fold of
 * From..To is the caller's expansion of that range.  `sources` and `req` are HOST arrays in both forms: validated on
 * the host and staged by the library.  Slices ascend by req_first and are disjoint; requests that no slice names are
 * ignored and their rows are not written.  RGB_E_INVAL, nothing enqueued: a slice outside n_req, slices not ascending
 * or not disjoint, a source outside files_bytes, unknown flags, VERIFY together with NO_DATA, more than
 * RGB_SEG_READ_MAX_SOURCES sources.  n_sources == 0 and n_req == 0 are legal.
 *
 * Lookup is in the map of parse_index_data_loop (:1057-1075), as in "major compaction" above: the walk ends at the
 * first all-zero record, at MaxCount records or where the file ends inside the index region; a backwards step trims
 * every greater key; an equal Idx overwrites -- the effective records.  The reference's binary index mode (:411-572)
 * is defined only for files whose records ascend and gives the same answers there.  Version 1 and 2 are served.
 *
 * Rows are independent; row r answers request r.
 *   good       index and term the record's, data_len its Length, crc the stored Crc, data_offset where the payload
 *              starts in `out` (with RGB_SEG_READ_NO_DATA: in the files buffer, source.offset + DataOffset); never
 *              RGB_UNDEF
 *   MISSING    the index is not in the map (exit({missing_key, Idx}); not_found in fold0 and term_query)
 *   TRUNCATED  the record's payload lies outside its file: DataOffset > n_bytes or Length > n_bytes - DataOffset
 *              (read_error, unexpected_eof, the short pread)
 *              -- with NO_DATA too, where the reference's term_query/2, which reads the index only, answers the Term
 * MISSING and TRUNCATED rows are {index = the requested one, term = 0, data_offset = RGB_UNDEF, data_len = 0, crc = 0}
 * and take no bytes of `out`; the later rows of the source are still looked up and delivered.
 *
 * The per-source result reports the first bad row of the slice in request order: its kind, its index and n_read, its
 * position in the slice (a fold with the `return` strategy takes the first n_read rows; with `error` the caller
 * crashes that server).  data_bytes counts the payloads of all good rows of the slice (0 with NO_DATA).
 *
 * RGB_SEG_READ_VERIFY: the CRC-32 of every copied payload is computed in the read that copies it and compared with
 * the stored Crc; a stored Crc of 0 is always good (validate_checksum/2, :1245-1248).  A mismatching row is still
 * delivered.  A source without a MISSING or TRUNCATED row and with a mismatch gets the status CRC, index and n_read
 * from the first mismatch in request order: MISSING and TRUNCATED win over CRC.  Without the flag no table is loaded
 * and no CRC computed (read_sparse does not validate).
 *
 * BAD_SOURCE: bad magic, fewer than 8 bytes, Version 0 or > 2.  n_read = 0, index = 0, every row of the slice is a
 * MISSING row.  Per source in BOTH forms (unlike compact's host-buffer form): a batch across groups survives one bad
 * file.
 *
 * SPACE: out_bytes < the bytes needed: total.status = SPACE, total.out_bytes = needed, `out` is not touched, rows and
 * results are written exactly as they would be, except that CRC is never reported (nothing was copied).  out = NULL,
 * out_bytes = 0 is therefore the sizing call.  With NO_DATA nothing is needed and SPACE never occurs.
 *
 * Only a file's own bytes are read, only the rows in [0, n_req) that slices name and the first total.out_bytes bytes of
 * `out` are written; d_files and d_out may have any alignment, d_rows, d_results and d_total are 8-byte aligned.  The
 * scratch lives in the context (released by rgb_close): one read call per context at a time.  Its size: 44 bytes per
 * source, 32 bytes per request (none with NO_DATA) and, for the tables of effective records, 4 bytes for every record a
 * source could hold -- min(65535, (n_bytes - 8) / 28) per source, about a seventh of the sources' bytes -- reserved
 * whether or not a source turns out to need its table.
 *
 * ra_lol search of the segrefs, is_modified/1, the fd LRU, binary_to_term, the mem-table overlay and file I/O stay with
 * the caller. */
typedef struct rgb_seg_read_source {   /* 32 bytes, the layout of rgb_seg_source */
  uint64_t offset, n_bytes;            /* the file = files[offset .. offset + n_bytes) */
  uint32_t req_first, req_n;           /* its requests = req[req_first .. + req_n), in the caller's order */
  uint64_t _pad;
} rgb_seg_read_source;

typedef struct rgb_seg_read_result {   /* 32 bytes, one per source */
  uint32_t status;                     /* RGB_SEG_READ_* of the first bad row in request order */
  uint32_t n_read;                     /* leading good rows of the slice (== req_n when OK) */
  uint64_t index;                      /* the index the status is about */
  uint64_t data_bytes;                 /* payload bytes this source contributes to out */
  uint64_t _pad;
} rgb_seg_read_result;

typedef struct rgb_seg_read_total {    /* 16 bytes, one per call */
  uint32_t status;                     /* RGB_SEG_READ_OK or RGB_SEG_READ_SPACE */
  uint32_t n_bad;                      /* sources whose status is not OK */
  uint64_t out_bytes;                  /* OK: bytes of out written; SPACE: bytes needed */
} rgb_seg_read_total;

#define RGB_SEG_READ_OK         0u
#define RGB_SEG_READ_MISSING    1u
#define RGB_SEG_READ_TRUNCATED  2u
#define RGB_SEG_READ_CRC        3u
#define RGB_SEG_READ_BAD_SOURCE 4u
#define RGB_SEG_READ_SPACE      5u   /* rgb_seg_read_total only */

#define RGB_SEG_READ_VERIFY      1u  /* flag: fold0's validate_checksum */
#define RGB_SEG_READ_NO_DATA     2u  /* flag: rows only (term_query); out may be NULL */
#define RGB_SEG_READ_MAX_SOURCES 65536u

/* d_rows: n_req rgb_seg_entry rows, d_results: n_sources rgb_seg_read_result rows, *d_total: one rgb_seg_read_total,
 * all in device memory.  The rows and d_out of a read can be handed unchanged to rgb_crc32_device,
 * rgb_segment_build_device or rgb_segment_flush_device.  Three launches (two with NO_DATA, four with VERIFY) on
 * `stream` (NULL = the context's stream), no synchronisation. */
int rgb_segment_read_device(rgb_ctx *ctx, const rgb_seg_read_source *sources, uint32_t n_sources, const void *d_files,
                            uint64_t files_bytes, const uint64_t *req, uint32_t n_req, uint32_t flags, void *d_rows,
                            void *d_out, uint64_t out_bytes, void *d_results, void *d_total, void *stream);
/* Host-buffer form: synchronises.  `results` and `total` are always written, the named rows too; `out` (its first
 * total.out_bytes bytes) only when total.status is OK. */
int rgb_segment_read(rgb_ctx *ctx, const rgb_seg_read_source *sources, uint32_t n_sources, const void *files,
                     uint64_t files_bytes, const uint64_t *req, uint32_t n_req, uint32_t flags, rgb_seg_entry *rows,
                     void *out, uint64_t out_bytes, rgb_seg_read_result *results, rgb_seg_read_total *total);

/* ==== snapshots and checkpoints: ragged CRC batches, file images and their validation ====================
 *
 * The snapshot family -- snapshot.dat of snapshots, checkpoints and recovery checkpoints (src/ra_log_snapshot.erl) and
 * the `indexes` file beside it (src/ra_snapshot.erl:1008-1059) -- for many members in one call:
 *   - recovery: pick_first_valid/4, find_checkpoints/4, find_recovery_checkpoint/1 (src/ra_snapshot.erl:343-479) call
 *     Mod:validate/1 and Mod:read_meta/1 on every member's files            -> rgb_snapshot_validate
 *   - writing: ra_log_snapshot:write/4 (:49-68), write_indexes/2             -> rgb_snapshot_build
 *   - receiving: begin_accept/2 (:80-81), accept_chunk/2's erlang:crc32(PartialCrc0, Chunk) (:104-108) for every
 *     transfer in flight                                                     -> rgb_crc32_spans
 * A batch is RAGGED: items of a few hundred bytes beside items of gigabytes.  The work is split by bytes, not by item:
 * short items get a group of lanes each, long ones are cut into 64 KiB blocks that all share one capped grid, and a
 * per-item step joins the blocks.  The number of launches does not depend on the number of items (at most five).
 *
 * Descriptor arrays are HOST arrays in every form: validated on the host (RGB_E_INVAL, nothing enqueued: a span, piece,
 * file or image outside its buffer, an unknown kind, unknown flags, meta_len != 0 on an indexes item, more than
 * 2^31 - 1 items) and staged by the library.  n == 0 is legal.  Device forms enqueue on `stream` (NULL = the context's
 * stream) and do not synchronise; host-buffer forms stage and synchronise.  The scratch lives in the context (released
 * by rgb_close): one snapshot call per context at a time.  Only a span's own bytes are read and only an image's own
 * bytes are written, whatever the alignment of the buffers.
 *
 * File I/O and fsync, the pwrite of the Crc at byte 5 in complete_accept/2, term_to_binary / term_to_iovec /
 * binary_to_term, directory listing and sorting, and the decision which file to try next and what to delete stay with
 * the caller. */
typedef struct rgb_crc_span {          /* 32 bytes */
  uint64_t offset, n_bytes;            /* the bytes = data[offset .. offset + n_bytes); any length, above 2^32 included */
  uint32_t init, _pad;                 /* PartialCrc0; 0 starts a checksum */
  uint64_t _pad2;
} rgb_crc_span;

/* d_crcs[i] = erlang:crc32(init_i, data[offset_i .. + n_bytes_i)) for the n spans.  Spans may overlap or name the same
 * bytes. */
int rgb_crc32_spans_device(rgb_ctx *ctx, const rgb_crc_span *spans, uint32_t n, const void *d_data, uint64_t data_bytes,
                           void *d_crcs, void *stream);
int rgb_crc32_spans(rgb_ctx *ctx, const rgb_crc_span *spans, uint32_t n, const void *data, uint64_t data_bytes,
                    uint32_t *crcs);

#define RGB_SNAP_KIND_SNAPSHOT 0u      /* <<"RASN", 1:8, Crc:32, MetaSize:32, Meta/binary, Data/binary>>,
                                          Crc = crc32(<<MetaSize:32>>, Meta, Data) (src/ra_log_snapshot.erl:54-63) */
#define RGB_SNAP_KIND_INDEXES  1u      /* <<"RASI", 1:8, Crc:32, Data/binary>>, Crc = crc32(Data)
                                          (src/ra_snapshot.erl:1017-1026) */
#define RGB_SNAP_HEADER_BYTES      9u  /* magic, Version, Crc */
#define RGB_SNAP_META_HEADER_BYTES 13u /* ... and MetaSize */

typedef struct rgb_snap_item {         /* 40 bytes: one image to write */
  uint32_t kind;                       /* RGB_SNAP_KIND_* */
  uint32_t meta_len;                   /* MetaSize; 0 for the indexes kind */
  uint64_t meta_offset;                /* Meta = data[meta_offset .. + meta_len) */
  uint64_t data_offset, data_bytes;    /* Data = data[data_offset .. + data_bytes) */
  uint64_t out_offset;                 /* where the image starts in the output (rgb_snapshot_layout fills it) */
} rgb_snap_item;

/* Host helper, pure: out_offset of every item when the images (13 + meta_len + data_bytes bytes, the indexes kind
 * 9 + data_bytes) are written back to back from `base`; returns the offset behind the last one. */
uint64_t rgb_snapshot_layout(rgb_snap_item *items, uint32_t n, uint64_t base);

/* d_out[out_offset ..) = the image of every item; every payload byte is read once, CRC and copy share the load.
 * d_crcs (may be NULL) receives the Crc written into each image.  Images may not overlap. */
int rgb_snapshot_build_device(rgb_ctx *ctx, const rgb_snap_item *items, uint32_t n, const void *d_data,
                              uint64_t data_bytes, void *d_out, uint64_t out_bytes, void *d_crcs, void *stream);
/* Host-buffer form: only the images' own bytes of `out` are written; crcs may be NULL. */
int rgb_snapshot_build(rgb_ctx *ctx, const rgb_snap_item *items, uint32_t n, const void *data, uint64_t data_bytes,
                       void *out, uint64_t out_bytes, uint32_t *crcs);

typedef struct rgb_snap_file {         /* 32 bytes: one file to check */
  uint64_t offset, n_bytes;            /* the file = files[offset .. offset + n_bytes) */
  uint32_t kind;                       /* RGB_SNAP_KIND_* */
  uint32_t flags;                      /* RGB_SNAP_META_ONLY */
  uint64_t _pad;
} rgb_snap_file;

#define RGB_SNAP_META_ONLY 1u          /* read_meta_internal/1 (src/ra_log_snapshot.erl:234-253): the header alone, no CRC */

/* recover/1 and validate/2 (src/ra_log_snapshot.erl:176-187, 255-261), indexes/1 (src/ra_snapshot.erl:1028-1059), in
 * this order: */
#define RGB_SNAP_OK              0u
#define RGB_SNAP_INVALID_FORMAT  1u    /* fewer than 9 bytes, or other magic.  The indexes kind: the legacy file without
                                          a header (:1046-1054) -- the caller tries binary_to_term */
#define RGB_SNAP_INVALID_VERSION 2u    /* magic good, at least 9 bytes, Version /= 1: `version` holds it.  META_ONLY, the
                                          snapshot kind: also 9 .. 12 bytes with good magic, even with Version 1 -- the
                                          reference's second clause of read_meta_internal/1 */
#define RGB_SNAP_CHECKSUM        3u    /* crc32 of everything behind byte 9 /= the stored Crc.  A stored 0 is NOT
                                          "unchecked" here, unlike segments: it must equal the computed value */
#define RGB_SNAP_BAD_META        4u    /* the snapshot kind: parse_snapshot/1 (:263-266) has no clause -- fewer than 4
                                          bytes behind byte 9, or MetaSize > n_bytes - 13 (META_ONLY: the short read) */
#define RGB_SNAP_EOF             5u    /* META_ONLY: 0 bytes (unexpected_eof_when_parsing_header) */

typedef struct rgb_snap_info {         /* 48 bytes, one per file */
  uint32_t status;                     /* RGB_SNAP_* */
  uint32_t version;                    /* INVALID_VERSION and behind; 0 before */
  uint32_t stored_crc;                 /* the header's Crc: INVALID_VERSION and behind */
  uint32_t computed_crc;               /* CHECKSUM, BAD_META, OK; 0 with META_ONLY */
  uint64_t meta_offset;                /* OK only, offsets into the files buffer: Meta ...                          */
  uint32_t meta_len, _pad;
  uint64_t data_offset, data_bytes;    /* ... and what follows it: what parse_snapshot/1 hands to binary_to_term    */
} rgb_snap_info;

/* d_infos[i] = the row of file i (8-byte aligned, device memory).  Files fail independently: one bad file leaves every
 * other row as it would have been.  The CRC of a file is computed whenever it has 9 bytes or more and META_ONLY is not
 * set.  META_ONLY on the indexes kind checks magic and Version alone. */
int rgb_snapshot_validate_device(rgb_ctx *ctx, const rgb_snap_file *files, uint32_t n, const void *d_files,
                                 uint64_t files_bytes, void *d_infos, void *stream);
int rgb_snapshot_validate(rgb_ctx *ctx, const rgb_snap_file *files, uint32_t n, const void *bytes, uint64_t files_bytes,
                          rgb_snap_info *infos);

#ifdef __cplusplus
}
#endif
#endif

/*
 * rgb_segment.hip -- batched CRC-32 (zlib / erlang:crc32: reflected 0xEDB88320, init and final xor 0xFFFFFFFF)
 * for the second half of Ra's storage path (include/ra_gpu_wal.h, "segments and snapshots"):
 *   - per-entry CRC of a batch of payloads          (src/ra_log_segment.erl:277, 670, 1240-1248)
 *   - the whole segment file image in one pass      (src/ra_log_segment.erl:1118-1122, 1211-1219)
 *   - one long buffer with a starting value         (src/ra_log_snapshot.erl:57-107, 256; src/ra_snapshot.erl:1020, 1038)
 * and, behind them, major compaction: info/2 of the files of a group and the copy of their live entries into one new
 * segment (src/ra_log_segment.erl:736-790, 819-908; src/ra_log_segments.erl:741-835) -- "major compaction" below --
 * the mem-table flush, the batched reads, and the snapshot family as ragged batches: spans with their own starting
 * values, the snapshot.dat / indexes images and their validation -- "snapshots and checkpoints" below.
 *
 * The arithmetic.  With a ZERO register and no final xor the CRC is linear over GF(2): raw(M) = M(x) * x^32 mod P,
 *     raw(A ++ B) = raw(A) * x^(8 |B|)  xor  raw(B),        raw(zeros ++ M) = raw(M)
 * (zlib's crc32_combine), and the real checksum is  crc(M, init) = ~( ~init * x^(8 |M|)  xor  raw(M) ).  gfx950 has
 * no carry-less multiply, so  * x^(8 k)  is either four table lookups (k fixed: the tables of slicing-by-N are
 * exactly "byte b followed by k zero bytes") or a 32-step shift/xor loop (k varies: once per lane per payload).
 *
 * The work split.  A payload is cut into 16-byte slots that are aligned to its END: the stream is thought of as
 * padded IN FRONT with zeros (neutral for raw) up to a whole number of rounds of GROUP slots.  Lane l takes slot
 * l of every round: one 16-byte load at the payload's own alignment, sixteen lookups for the slot's raw value, four
 * more to move the lane's running value one round (16 * GROUP bytes) further:  acc = acc * x^(128 GROUP) ^ raw16(slot).
 * Because the slots are aligned to the end, every lane finishes the same fixed distance from the end of the payload
 * (lane l: 16 (GROUP - 1 - l) bytes), so the last step is one multiplication by a per-lane constant and an xor
 * butterfly.  Only the FIRST slot of a payload can be partial; its bytes are shifted up inside the 16-byte register,
 * zeros in front.  The initial value 0xFFFFFFFF is xored into the first four payload bytes.  Only the payload's own
 * bytes are read.  Payloads under 16 bytes go byte by byte on the group's first lane.
 *
 * Tables: 16 KiB slicing-by-16 + 4 KiB "one round further", copied into LDS once per workgroup; the grid is capped
 * and walks the batch, so the copy is amortised over many payloads.  ds_read_b32 lookups at data-dependent indices:
 * bank conflicts are expected (32 banks, 32 random dwords: ~3.5-way on average), see DESIGN.md for the counters.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/ra_gpu_wal.h"

static_assert(sizeof(rgb_seg_entry) == 32, "rgb_seg_entry is 32 bytes");

namespace {
namespace seg {

typedef unsigned int u32;
typedef unsigned long long u64;
typedef unsigned int v4u __attribute__((ext_vector_type(4)));
typedef v4u v4u_any __attribute__((aligned(1)));

constexpr u32 POLY = 0xEDB88320u;
constexpr u32 X0 = 0x80000000u;                 /* the polynomial 1: x^k is bit 31 - k */
constexpr int THREADS = 256;
constexpr u32 STREAM_BLOCK = 65536u;            /* bytes of a long buffer per workgroup step: 16 rounds of 256 slots */
constexpr u32 STREAM_MAX_BLOCKS = 16384u;       /* partial values the context keeps: 1 GiB per launch */
constexpr u32 GRID_CAP = 2048u;                 /* 8 workgroups (20 KiB of LDS each) on each of 256 CUs */

/* a * b mod P, both in the reflected representation (zlib's multmodp) */
constexpr u32 mulmod_c(u32 a, u32 b) {
  u32 p = 0;
  for (u32 m = X0; m; m >>= 1) {
    if (a & m) p ^= b;
    b = (b & 1u) ? (b >> 1) ^ POLY : b >> 1;
  }
  return p;
}
/* x^(8 n) mod P */
constexpr u32 xpow8_c(u64 n) {
  u32 p = X0, sq = X0 >> 8;
  while (n) {
    if (n & 1u) p = mulmod_c(sq, p);
    sq = mulmod_c(sq, sq);
    n >>= 1;
  }
  return p;
}

/* slice[k][b] = raw(byte b followed by k zero bytes); adv[s][i][b] = the same for k = D_s - 4 + i, D_s the bytes of
 * one round of 8 / 16 / 64 / 256 lanes; lanek[j] = x^(128 j); blk[j] = x^(8 STREAM_BLOCK j) */
struct alignas(16) Tables {
  u32 slice[16][256];
  u32 adv[4][4][256];
  u32 lanek[256];
  u32 blk[257];
};
constexpr int adv_set(int group) { return group == 8 ? 0 : group == 16 ? 1 : group == 64 ? 2 : 3; }
constexpr Tables make_tables() {
  Tables t{};
  for (u32 b = 0; b < 256; ++b) {
    u32 c = b;
    for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ POLY : c >> 1;
    t.slice[0][b] = c;
  }
  for (int k = 1; k < 16; ++k)
    for (u32 b = 0; b < 256; ++b) t.slice[k][b] = (t.slice[k - 1][b] >> 8) ^ t.slice[0][t.slice[k - 1][b] & 0xFFu];
  const u32 round_bytes[4] = {128u, 256u, 1024u, 4096u};
  for (int s = 0; s < 4; ++s) {
    u32 xp = xpow8_c(round_bytes[s] - 4u);
    for (int i = 0; i < 4; ++i) {
      /* linear in b: eight products, the rest by xor */
      t.adv[s][i][0] = 0;
      for (u32 bit = 1; bit < 256; bit <<= 1) t.adv[s][i][bit] = mulmod_c(t.slice[0][bit], xp);
      for (u32 b = 1; b < 256; ++b)
        if (b & (b - 1u)) t.adv[s][i][b] = t.adv[s][i][b & (b - 1u)] ^ t.adv[s][i][b & (0u - b)];
      xp = mulmod_c(xp, X0 >> 8);
    }
  }
  const u32 x128 = xpow8_c(16), xblk = xpow8_c(STREAM_BLOCK);
  t.lanek[0] = X0;
  for (int j = 1; j < 256; ++j) t.lanek[j] = mulmod_c(t.lanek[j - 1], x128);
  t.blk[0] = X0;
  for (int j = 1; j < 257; ++j) t.blk[j] = mulmod_c(t.blk[j - 1], xblk);
  return t;
}
__device__ const Tables g_tab = make_tables();

constexpr u32 LDS_WORDS = 20u * 256u;

/* the same product at run time, branch-free: ~7 instructions a bit */
__device__ __forceinline__ u32 mulmod(u32 a, u32 b) {
  u32 p = 0;
#pragma unroll 8
  for (int k = 0; k < 32; ++k) {
    p ^= b & (u32)((int)a >> 31);
    a <<= 1;
    b = (b >> 1) ^ (POLY & (0u - (b & 1u)));
  }
  return p;
}

template <int GROUP>
__device__ __forceinline__ void load_tables(u32 *lds) {
  const v4u *src_a = reinterpret_cast<const v4u *>(&g_tab.slice[0][0]);
  const v4u *src_b = reinterpret_cast<const v4u *>(&g_tab.adv[adv_set(GROUP)][0][0]);
  v4u *dst = reinterpret_cast<v4u *>(lds);
  for (u32 i = threadIdx.x; i < 1024u; i += THREADS) dst[i] = src_a[i];
  for (u32 i = threadIdx.x; i < 256u; i += THREADS) dst[1024u + i] = src_b[i];
  __syncthreads();
}

/* raw value of the 16 bytes of v (byte 0 = lowest address = first in the stream, 15 bytes behind it) */
__device__ __forceinline__ u32 raw16(const u32 *lds, const uint4 v) {
  u32 r;
  r  = lds[15 * 256 + (v.x & 0xFFu)] ^ lds[14 * 256 + ((v.x >> 8) & 0xFFu)] ^ lds[13 * 256 + ((v.x >> 16) & 0xFFu)] ^ lds[12 * 256 + (v.x >> 24)];
  r ^= lds[11 * 256 + (v.y & 0xFFu)] ^ lds[10 * 256 + ((v.y >> 8) & 0xFFu)] ^ lds[ 9 * 256 + ((v.y >> 16) & 0xFFu)] ^ lds[ 8 * 256 + (v.y >> 24)];
  r ^= lds[ 7 * 256 + (v.z & 0xFFu)] ^ lds[ 6 * 256 + ((v.z >> 8) & 0xFFu)] ^ lds[ 5 * 256 + ((v.z >> 16) & 0xFFu)] ^ lds[ 4 * 256 + (v.z >> 24)];
  r ^= lds[ 3 * 256 + (v.w & 0xFFu)] ^ lds[ 2 * 256 + ((v.w >> 8) & 0xFFu)] ^ lds[ 1 * 256 + ((v.w >> 16) & 0xFFu)] ^ lds[ 0 * 256 + (v.w >> 24)];
  return r;
}
/* s * x^(8 D), D the bytes of one round: the four bytes of s followed by D - 4 zero bytes */
__device__ __forceinline__ u32 advance(const u32 *lds, u32 s) {
  const u32 *a = lds + 16 * 256;
  return a[3 * 256 + (s & 0xFFu)] ^ a[2 * 256 + ((s >> 8) & 0xFFu)] ^ a[1 * 256 + ((s >> 16) & 0xFFu)] ^ a[s >> 24];
}

/* the 16-byte register (lo = bytes 0-7) moved up by sh bytes, 1 <= sh <= 15, zeros in front */
__device__ __forceinline__ void shift_up(u64 &lo, u64 &hi, u32 sh) {
  if (sh >= 8u) { hi = lo << (8u * (sh - 8u)); lo = 0; }
  else { hi = (hi << (8u * sh)) | (lo >> (64u - 8u * sh)); lo <<= 8u * sh; }
}

/* Slot t of a payload of `len` >= 16 bytes at `pay`, `pad` zero bytes thought in front: the slot covers payload bytes
 * [p, p + 16), p = 16 t - pad.  COPY: the bytes also go to dst + p (the first, partial slot stores [0, 16): the bytes
 * it shares with its successor are written twice with the same value).  `fold` is xored into payload bytes 0..3. */
template <bool COPY, int USER = 0>
__device__ __forceinline__ uint4 load_slot(const unsigned char *pay, unsigned char *dst, u32 t, u32 pad, u32 fold) {
  const long long p = (long long)t * 16 - (long long)pad;
  if (p <= -16) return make_uint4(0, 0, 0, 0);
  const long long q = p < 0 ? 0 : p;
  const v4u w = __builtin_nontemporal_load(reinterpret_cast<const v4u_any *>(pay + q));
  if (COPY) *reinterpret_cast<v4u_any *>(dst + q) = w;
  uint4 v = make_uint4(w.x, w.y, w.z, w.w);
  if (p < 4) {                                   /* the first slot, or the one behind a first slot of < 4 bytes */
    if (p < 0) {
      u64 lo = (u64)v.x | ((u64)v.y << 32), hi = (u64)v.z | ((u64)v.w << 32);
      u64 flo = fold, fhi = 0;
      shift_up(lo, hi, (u32)(-p));
      shift_up(flo, fhi, (u32)(-p));
      lo ^= flo; hi ^= fhi;
      v = make_uint4((u32)lo, (u32)(lo >> 32), (u32)hi, (u32)(hi >> 32));
    } else if (p == 0) {
      v.x ^= fold;
    } else {
      v.x ^= fold >> (8u * (u32)p);              /* payload bytes p..3 */
    }
  }
  return v;
}

/* USER (here and in load_slot): a caller that wants instantiations of its own, see SNAP_USER.
 * This lane's share of raw(fold-ed payload), already moved to the end of the payload: the xor over the GROUP lanes
 * is the raw value.  len >= 16 or len == 0 (nothing to do); every lane of the group makes the same number of rounds. */
template <int GROUP, int UNROLL, bool COPY, int USER = 0>
__device__ __forceinline__ u32 lane_raw(const u32 *lds, const unsigned char *pay, unsigned char *dst, u32 len,
                                        u32 lane, u32 fold) {
  const u32 slots = (u32)(((u64)len + 15u) >> 4);
  const u32 rounds = (slots + (u32)GROUP - 1u) / (u32)GROUP;
  const u32 pad = (u32)((u64)rounds * GROUP * 16u - len);            /* < 16 GROUP */
  u32 acc = 0;
  for (u32 r0 = 0; r0 < rounds; r0 += UNROLL) {
    uint4 v[UNROLL];
#pragma unroll
    for (int k = 0; k < UNROLL; ++k) {
      v[k] = make_uint4(0, 0, 0, 0);
      if (r0 + (u32)k < rounds) v[k] = load_slot<COPY, USER>(pay, dst, (r0 + (u32)k) * GROUP + lane, pad, fold);
    }
#pragma unroll
    for (int k = 0; k < UNROLL; ++k)
      if (r0 + (u32)k < rounds) acc = advance(lds, acc) ^ raw16(lds, v[k]);
  }
  if (rounds && lane != (u32)GROUP - 1u) acc = mulmod(acc, g_tab.lanek[GROUP - 1 - (int)lane]);
  return acc;
}

template <int GROUP>
__device__ __forceinline__ u32 group_xor(u32 v) {
#pragma unroll
  for (int off = (GROUP < 64 ? GROUP : 64) / 2; off > 0; off >>= 1) v ^= __shfl_xor(v, off, 64);
  return v;
}

/* byte by byte through the first slicing table (payloads under 16 bytes, buffers under 16 bytes) */
__device__ __forceinline__ u32 crc_bytes(const u32 *t0, u32 crc, const unsigned char *p, u32 n, unsigned char *copy_to) {
  crc = ~crc;
  for (u32 k = 0; k < n; ++k) {
    const u32 c = p[k];
    if (copy_to) copy_to[k] = (unsigned char)c;
    crc = (crc >> 8) ^ t0[(crc ^ c) & 0xFFu];
  }
  return ~crc;
}

/* The CRC of one entry's payload of 16 bytes or more by the GROUP lanes that share it, valid on the group's first lane.
 * Every lane of the group comes here, live or not (the butterfly needs them all); an entry that is not live, or
 * shorter, is not read.  COPY: the payload goes to dst as it is read. */
template <int GROUP, bool COPY>
__device__ __forceinline__ u32 entry_crc(const u32 *lds, const unsigned char *pay, unsigned char *dst, u32 len, bool live,
                                         u32 lane) {
  constexpr int UNROLL = GROUP == 64 ? 4 : 2;
  const bool wide = live && len >= 16u;
  const u32 part = lane_raw<GROUP, UNROLL, COPY>(lds, pay, dst, wide ? len : 0u, lane, 0xFFFFFFFFu);
  return ~group_xor<GROUP>(part);
}
/* ... and the answer, on the first lane of a live entry: payloads under 16 bytes go byte by byte here, inside the
 * caller's own lane-0 region (a region of their own in front of it costs the 8-lane build 3 to 5 % at 256-byte payloads) */
template <bool COPY>
__device__ __forceinline__ u32 lane0_crc(const u32 *lds, u32 group_crc, const unsigned char *pay, unsigned char *dst, u32 len) {
  return len >= 16u ? group_crc : crc_bytes(lds, 0u, pay, len, COPY ? dst : nullptr);
}

/* <<"RASG", 2:16, MaxCount:16>> (src/ra_log_segment.erl:1118-1122) */
__device__ __forceinline__ void put_header(unsigned char *at, u32 max_count) {
  struct __attribute__((packed)) hdr8 { u64 v; } h;
  h.v = 0x47534152ull | (0x0200ull << 32) | ((u64)((max_count >> 8) & 0xFFu) << 48) | ((u64)(max_count & 0xFFu) << 56);
  __builtin_memcpy(at, &h, 8);
}
/* <<Idx:64, Term:64, DataOffset:64, Length:32, Crc:32>> (src/ra_log_segment.erl:1211-1219), at any alignment */
__device__ __forceinline__ void put_record(unsigned char *rec, u64 idx, u64 term, u64 off, u32 len, u32 crc) {
  v4u a, b;
  a.x = __builtin_bswap32((u32)(idx >> 32));  a.y = __builtin_bswap32((u32)idx);
  a.z = __builtin_bswap32((u32)(term >> 32)); a.w = __builtin_bswap32((u32)term);
  b.x = __builtin_bswap32((u32)(off >> 32));  b.y = __builtin_bswap32((u32)off);
  b.z = __builtin_bswap32(len);               b.w = __builtin_bswap32(crc);
  *reinterpret_cast<v4u_any *>(rec) = a;
  *reinterpret_cast<v4u_any *>(rec + 16) = b;
}

/* ---- per-entry CRC, and the segment image around it ------------------------------------------------------
 * GROUP lanes per entry (8 up to a mean payload of 320 bytes, 16 up to 1 KiB, then a wavefront), as the WAL kernels.
 * BUILD: the payload is copied to out + out_offsets[e] as it is read, the group's first lane writes the index record
 * at 8 + 32 e, and the first thread of the grid the file header.
 * An entry whose payload does not lie inside the data buffer, or whose copy does not lie inside the output, is not
 * touched at all (the host-buffer forms refuse such a batch before anything is launched). */
template <int GROUP, bool BUILD>
__global__ __launch_bounds__(THREADS) void rgb_seg_crc_kernel(
    const rgb_seg_entry *__restrict__ entries, u32 n, const unsigned char *__restrict__ data, u64 data_bytes,
    u32 *__restrict__ crcs, unsigned char *__restrict__ out, u64 out_bytes, const u64 *__restrict__ out_offsets,
    u32 max_count, u32 flags) {
  __shared__ __attribute__((aligned(16))) u32 lds[LDS_WORDS];
  load_tables<GROUP>(lds);
  constexpr u32 PER_BLOCK = THREADS / GROUP;
  const u32 lane = threadIdx.x & (GROUP - 1);
  if (BUILD && blockIdx.x == 0 && threadIdx.x == 0) put_header(out, max_count);
  for (u32 base = blockIdx.x * PER_BLOCK; base < n; base += gridDim.x * PER_BLOCK) {
    const u32 e = base + threadIdx.x / GROUP;
    bool live = e < n;
    rgb_seg_entry en;
    en.index = en.term = en.data_offset = 0; en.data_len = en.crc = 0;
    if (live) en = entries[e];
    u64 dst_off = 0;
    if (BUILD && live) dst_off = out_offsets[e];
    const u32 len = en.data_len;
    if (en.data_offset > data_bytes || len > data_bytes - en.data_offset) live = false;
    if (BUILD && (dst_off > out_bytes || len > out_bytes - dst_off)) live = false;
    const unsigned char *pay = data + en.data_offset;
    unsigned char *dst = BUILD ? out + dst_off : nullptr;
    u32 crc = entry_crc<GROUP, BUILD>(lds, pay, dst, len, live, lane);
    if (live && lane == 0u) {
      crc = lane0_crc<BUILD>(lds, crc, pay, dst, len);
      if (BUILD) {
        if (flags & RGB_SEG_NO_CHECKSUMS) crc = 0u;
        put_record(out + RGB_SEG_HEADER_BYTES + (u64)RGB_SEG_RECORD_BYTES * e, en.index, en.term, dst_off, len, crc);
      }
      if (crcs) crcs[e] = crc;
    }
  }
}

/* ---- one long buffer -------------------------------------------------------------------------------------
 * The buffer is cut into blocks of STREAM_BLOCK bytes aligned to its END (the first block is the short one, so every
 * other block is a whole number of rounds and sits a multiple of STREAM_BLOCK from the end).  A workgroup is one
 * group of 256 lanes; it leaves raw(block) in partials[b].  n_bytes >= 16. */
__global__ __launch_bounds__(THREADS) void rgb_seg_stream_kernel(const unsigned char *__restrict__ data, u64 n_bytes,
                                                                 u32 n_blocks, u32 *__restrict__ partials) {
  __shared__ __attribute__((aligned(16))) u32 lds[LDS_WORDS];
  __shared__ u32 red[THREADS / 64];
  load_tables<256>(lds);
  const u64 first_len = n_bytes - (u64)(n_blocks - 1u) * STREAM_BLOCK;      /* 1 .. STREAM_BLOCK */
  for (u32 b = blockIdx.x; b < n_blocks; b += gridDim.x) {
    const u64 start = b ? first_len + (u64)(b - 1u) * STREAM_BLOCK : 0ull;
    const u32 len = b ? STREAM_BLOCK : (u32)first_len;
    /* a first block under 16 bytes: its one slot loads [0, 16), inside the buffer, and keeps its own bytes */
    const u32 part = lane_raw<256, 4, false>(lds, data + start, nullptr, len, threadIdx.x, 0u);
    const u32 w = group_xor<64>(part);
    if ((threadIdx.x & 63u) == 0u) red[threadIdx.x >> 6] = w;
    __syncthreads();
    if (threadIdx.x == 0u) partials[b] = red[0] ^ red[1] ^ red[2] ^ red[3];
    __syncthreads();
  }
}

/* One workgroup: raw(buffer) = xor_b partials[b] * x^(8 STREAM_BLOCK (n_blocks - 1 - b)), then
 * crc = ~( ~init * x^(8 n_bytes) ^ raw ), x^(8 n_bytes) computed by the host (`xn`).  init_from_crc: the starting
 * value is what *crc holds (the next gigabyte of one buffer).  n_blocks == 0: the `small_len` < 16 bytes at `small`,
 * byte by byte. */
__global__ __launch_bounds__(THREADS) void rgb_seg_combine_kernel(const u32 *__restrict__ partials, u32 n_blocks, u32 xn,
                                                                  u32 init, u32 init_from_crc, u32 *__restrict__ crc,
                                                                  const unsigned char *__restrict__ small, u32 small_len) {
  __shared__ u32 red[THREADS / 64];
  u32 acc = 0;
  const u32 k_round = g_tab.blk[256];
  for (u32 b = threadIdx.x; b < n_blocks; b += THREADS) acc = mulmod(acc, k_round) ^ partials[b];
  if (threadIdx.x < n_blocks) {
    const u32 last = threadIdx.x + ((n_blocks - 1u - threadIdx.x) / THREADS) * THREADS;
    acc = mulmod(acc, g_tab.blk[n_blocks - 1u - last]);
  }
  const u32 w = group_xor<64>(acc);
  if ((threadIdx.x & 63u) == 0u) red[threadIdx.x >> 6] = w;
  __syncthreads();
  if (threadIdx.x == 0u) {
    const u32 start = init_from_crc ? *crc : init;
    if (n_blocks) *crc = ~(mulmod(~start, xn) ^ red[0] ^ red[1] ^ red[2] ^ red[3]);
    else *crc = crc_bytes(&g_tab.slice[0][0], start, small, small_len, nullptr);
  }
}

/* ---- major compaction (include/ra_gpu_wal.h, "major compaction") -------------------------------------------
 * Three passes, each its own launch, so that no workgroup ever waits for another:
 *   resolve  one workgroup per source: the index walk, which records are effective, which of those are live; the info
 *            row, the source's counters and one plan record per selected entry, in copy order
 *   place    one thread: the sources' bases, file_bytes, the first MISSING / TRUNCATED / FULL entry in copy order, SPACE
 *   copy     GROUP lanes per plan record: the payload (with or without its CRC), the index record; nothing at all
 *            unless the status is OK
 * When the status is OK every live index was found, so the plan is dense, its position IS the record number of the new
 * file, and MaxCount records are written: there are no unused index records to zero.
 * The kernels' parameter types are the unit's own (the resource gate of tests/test_segment.py counts kernels by the
 * header's type prefix in their symbol names). */
constexpr u32 NONE32 = 0xFFFFFFFFu;
constexpr u64 NONE64 = ~0ull;
constexpr u32 CMP_MAX_RECORDS = 65536u;         /* MaxCount has 16 bits */

struct src_desc { u64 offset, n_bytes; u32 live_first, live_n, asked, plan_base; };        /* staged from the host */
struct src_done { u64 sel_bytes, miss_idx; u32 sel_count, miss_k, trunc_k, bad; };         /* resolve -> place */
struct alignas(16) plan_rec { u64 idx, term, src_off, pre; u32 len, crc, src, _pad; };     /* resolve -> place, copy */
struct work_hdr { u32 status, crc_fail, _pad[2]; };                                        /* place -> copy -> finish */
static_assert(sizeof(src_desc) == 32 && sizeof(src_done) == 32 && sizeof(plan_rec) == 48 && sizeof(work_hdr) == 16, "");

__device__ __forceinline__ void atomic_min(u32 *p, u32 v) {
  u32 old = *p;
  while (v < old) {
    const u32 seen = atomicCAS(p, old, v);
    if (seen == old) break;
    old = seen;
  }
}
__device__ __forceinline__ u64 ld_be64(const unsigned char *p) { u64 v; __builtin_memcpy(&v, p, 8); return __builtin_bswap64(v); }
__device__ __forceinline__ u32 ld_be32(const unsigned char *p) { u32 v; __builtin_memcpy(&v, p, 4); return __builtin_bswap32(v); }

struct idx_rec { u64 idx, term, off; u32 len, crc; };
/* decode_index_record/3 (src/ra_log_segment.erl:1180-1209) */
__device__ __forceinline__ idx_rec decode_rec(const unsigned char *p, bool v2) {
  idx_rec r;
  r.idx = ld_be64(p); r.term = ld_be64(p + 8);
  r.off = v2 ? ld_be64(p + 16) : (u64)ld_be32(p + 16);
  r.len = ld_be32(p + (v2 ? 24 : 20)); r.crc = ld_be32(p + (v2 ? 28 : 24));
  return r;
}
/* ra_seq:in/2 over pairs [first, first + n) of the live list; *which = the pair that holds idx */
__device__ __forceinline__ bool live_find(const u64 *live, u32 first, u32 n, u64 idx, u32 *which) {
  u32 lo = 0, hi = n;                                   /* lo = pairs whose first <= idx */
  while (lo < hi) {
    const u32 mid = (lo + hi) >> 1;
    if (live[2 * (u64)(first + mid)] <= idx) lo = mid + 1u; else hi = mid;
  }
  if (!lo) return false;
  *which = first + lo - 1u;
  return idx <= live[2 * (u64)*which + 1u];
}

/* read_header/1 (:1124-1138): version 0 = not a segment file this unit serves */
__device__ __forceinline__ void read_header(const unsigned char *f, u64 n_bytes, u32 *version, u32 *max_count) {
  *version = 0; *max_count = 0;
  if (n_bytes >= RGB_SEG_HEADER_BYTES && f[0] == 'R' && f[1] == 'A' && f[2] == 'S' && f[3] == 'G') {
    *version = ((u32)f[4] << 8) | f[5];
    *max_count = ((u32)f[6] << 8) | f[7];
  }
}

/* The index walk of one source by its workgroup (every lane comes here), for the resolve passes of compaction and of
 * the reads.  Pass A: where the walk ends -- the first all-zero record among the n_fit whole records inside the file.
 * Pass B, last chunk first: record j is effective iff Idx_j < min Idx of every later record (the last one always is)
 * -- a reverse exclusive min-scan, `carry` the minimum of the chunks already seen.  Leaves the effective bitmap in
 * s_bits, their number in *s_eff (both valid after the last barrier in here), the smallest Idx walked in *min_idx;
 * returns the records walked.  each(r) sees every walked record once, on its own lane.  The caller has a barrier
 * between its own use of the LDS arrays and this call. */
template <class F>
__device__ __forceinline__ u32 walk_effective(const unsigned char *index, u32 rec_bytes, bool v2, u32 n_fit, u64 *s_wide,
                                              u32 *s_bits, u32 *s_first_zero, u32 *s_eff, u64 *min_idx, F &&each) {
  const u32 tid = threadIdx.x;
  if (tid == 0u) { *s_first_zero = n_fit; *s_eff = 0u; }
  for (u32 i = tid; i < CMP_MAX_RECORDS / 32; i += THREADS) s_bits[i] = 0u;
  __syncthreads();
  for (u32 base = 0; base < n_fit; base += THREADS) {
    const u32 j = base + tid;
    if (j < n_fit) {
      const idx_rec r = decode_rec(index + (u64)rec_bytes * j, v2);
      if ((r.idx | r.term | r.off | r.len | r.crc) == 0ull) atomic_min(s_first_zero, j);
    }
    __syncthreads();
    const u32 z = *s_first_zero;
    __syncthreads();
    if (z != n_fit) break;
  }
  const u32 n_walk = *s_first_zero;
  const u32 n_chunks = (n_walk + THREADS - 1u) / THREADS;
  u64 carry = NONE64;
  for (u32 c = n_chunks; c-- > 0u;) {
    const u32 j = c * THREADS + tid;
    const bool valid = j < n_walk;
    idx_rec r{};
    if (valid) r = decode_rec(index + (u64)rec_bytes * j, v2);
    s_wide[tid] = valid ? r.idx : NONE64;
    __syncthreads();
    for (u32 off = 1; off < THREADS; off <<= 1) {
      u64 t = s_wide[tid];
      if (tid + off < THREADS && s_wide[tid + off] < t) t = s_wide[tid + off];
      __syncthreads();
      s_wide[tid] = t;
      __syncthreads();
    }
    u64 later = tid + 1u < THREADS ? s_wide[tid + 1u] : NONE64;
    if (carry < later) later = carry;
    const u64 chunk_min = s_wide[0];
    if (valid && (j == n_walk - 1u || r.idx < later)) {
      atomicOr(&s_bits[j >> 5], 1u << (j & 31u));
      atomicAdd(s_eff, 1u);
    }
    if (valid) each(r);
    if (chunk_min < carry) carry = chunk_min;
    __syncthreads();
  }
  *min_idx = carry;
  return n_walk;
}

__global__ __launch_bounds__(THREADS) void rgb_compact_resolve_kernel(
    const src_desc *__restrict__ srcs, const unsigned char *__restrict__ files, const u64 *__restrict__ live,
    const u32 *__restrict__ rank, u32 all_live, void *infos_v, src_done *__restrict__ done, plan_rec *__restrict__ plan) {
  __shared__ u64 s_wide[THREADS];                       /* scan buffer: suffix min of Idx, prefix sum of bytes */
  __shared__ u32 s_cnt[THREADS];                        /* scan buffer: prefix count */
  __shared__ u32 s_bits[CMP_MAX_RECORDS / 32];          /* record j is effective */
  __shared__ u32 s_first_zero, s_eff, s_miss_k, s_trunc_k;
  __shared__ u64 s_live_size;
  const u32 tid = threadIdx.x, s = blockIdx.x;
  const src_desc sd = srcs[s];
  const unsigned char *f = files + sd.offset;
  rgb_seg_info *info = infos_v ? reinterpret_cast<rgb_seg_info *>(infos_v) + s : nullptr;

  u32 version, max_count;
  read_header(f, sd.n_bytes, &version, &max_count);
  if (version < 1u || version > RGB_SEG_VERSION) {      /* the same for every lane */
    if (tid == 0u) {
      if (info) { rgb_seg_info z{}; z.status = RGB_SEG_COMPACT_BAD_SOURCE; *info = z; }
      if (done) { src_done d{}; d.miss_k = d.trunc_k = NONE32; d.bad = 1u; done[s] = d; }
    }
    return;
  }
  const bool v2 = version == 2u;
  const u32 rec_bytes = v2 ? RGB_SEG_RECORD_BYTES : RGB_SEG_RECORD_BYTES_V1;
  const u64 data_start = (u64)RGB_SEG_HEADER_BYTES + (u64)rec_bytes * max_count;
  const u64 fit = (sd.n_bytes - RGB_SEG_HEADER_BYTES) / rec_bytes;            /* whole records inside the file */
  const u32 n_fit = fit < max_count ? (u32)fit : max_count;
  const unsigned char *index = f + RGB_SEG_HEADER_BYTES;

  /* passes A and B: the walk, the effective records, and live_size over every walked record */
  if (tid == 0u) { s_miss_k = NONE32; s_trunc_k = NONE32; s_live_size = 0ull; }
  u64 carry, my_live = 0;
  const u32 n_walk = walk_effective(index, rec_bytes, v2, n_fit, s_wide, s_bits, &s_first_zero, &s_eff, &carry,
                                    [&](const idx_rec &r) {
    u32 which;
    if (all_live || live_find(live, sd.live_first, sd.live_n, r.idx, &which)) my_live += r.len;
  });
  const u32 n_chunks = (n_walk + THREADS - 1u) / THREADS;
  if (my_live) atomicAdd(&s_live_size, (unsigned long long)my_live);
  __syncthreads();

  if (info && tid == 0u) {
    rgb_seg_info o{};
    o.size = o.index_size = data_start;
    if (n_walk) {
      const idx_rec last = decode_rec(index + (u64)rec_bytes * (n_walk - 1u), v2);
      o.size = last.off + last.len;
      o.range_first = carry; o.range_last = last.idx;
    }
    o.live_size = s_live_size;
    o.num_entries = n_walk; o.num_indexes = s_eff; o.max_count = max_count; o.version = version;
    o.status = RGB_SEG_COMPACT_OK;
    *info = o;
  }
  if (!done) return;

  /* pass C, in file order: the selected records (effective and live) get their place in the source's part of the
   * plan and their running byte offset; a selected record whose rank among the source's live indexes is not its
   * place has a missing index in front of it */
  u32 run_cnt = 0;
  u64 run_bytes = 0;
  for (u32 c = 0; c < n_chunks; ++c) {
    const u32 j = c * THREADS + tid;
    idx_rec r{};
    u32 which = 0;
    bool sel = j < n_walk && ((s_bits[j >> 5] >> (j & 31u)) & 1u);
    if (sel) {
      r = decode_rec(index + (u64)rec_bytes * j, v2);
      sel = live_find(live, sd.live_first, sd.live_n, r.idx, &which);
    }
    s_cnt[tid] = sel ? 1u : 0u;
    s_wide[tid] = sel ? (u64)r.len : 0ull;
    __syncthreads();
    for (u32 off = 1; off < THREADS; off <<= 1) {
      u32 tc = s_cnt[tid];
      u64 tb = s_wide[tid];
      if (tid >= off) { tc += s_cnt[tid - off]; tb += s_wide[tid - off]; }
      __syncthreads();
      s_cnt[tid] = tc; s_wide[tid] = tb;
      __syncthreads();
    }
    if (sel) {
      const u32 k = run_cnt + s_cnt[tid] - 1u;
      if (k < sd.asked) {
        plan_rec p;
        p.idx = r.idx; p.term = r.term; p.src_off = sd.offset + r.off; p.pre = run_bytes + s_wide[tid] - r.len;
        p.len = r.len; p.crc = r.crc; p.src = s; p._pad = 0u;
        plan[sd.plan_base + k] = p;
      }
      if (rank[which] + (u32)(r.idx - live[2 * (u64)which]) != k) atomic_min(&s_miss_k, k);
      if (r.off > sd.n_bytes || r.len > sd.n_bytes - r.off) atomic_min(&s_trunc_k, k);
    }
    run_cnt += s_cnt[THREADS - 1];
    run_bytes += s_wide[THREADS - 1];
    __syncthreads();
  }
  if (tid == 0u) {
    src_done d{};
    d.sel_bytes = run_bytes; d.sel_count = run_cnt; d.trunc_k = s_trunc_k; d.miss_k = s_miss_k;
    if (d.miss_k == NONE32 && run_cnt < sd.asked) d.miss_k = run_cnt;
    if (d.miss_k != NONE32) {                           /* the live index of rank miss_k */
      u32 lo = 0, hi = sd.live_n;                       /* lo = pairs whose rank <= miss_k; at least one */
      while (lo < hi) {
        const u32 mid = (lo + hi) >> 1;
        if (rank[sd.live_first + mid] <= d.miss_k) lo = mid + 1u; else hi = mid;
      }
      const u32 i = sd.live_first + lo - 1u;
      d.miss_idx = live[2 * (u64)i] + (d.miss_k - rank[i]);
    }
    done[s] = d;
  }
}

__global__ void rgb_compact_place_kernel(const src_desc *__restrict__ srcs, u32 n_sources, const src_done *__restrict__ done,
                                         const plan_rec *__restrict__ plan, u32 max_count, u64 max_size, u64 out_bytes,
                                         u64 *__restrict__ byte_base, work_hdr *__restrict__ hdr, void *result_v) {
  if (threadIdx.x != 0u || blockIdx.x != 0u) return;
  rgb_seg_compact_result res{};
  u64 bytes = 0;
  u32 recs = 0;
  for (u32 s = 0; s < n_sources && !res.status; ++s)
    if (done[s].bad) { res.status = RGB_SEG_COMPACT_BAD_SOURCE; res.source = s; }
  for (u32 s = 0; s < n_sources && !res.status; ++s) {
    const src_done d = done[s];
    const plan_rec *p = plan + srcs[s].plan_base;
    /* append_raw refuses entry k when the payload bytes in front of it exceed max_size (is_full/1, :1250-1255) */
    u32 full_k = NONE32;
    if (d.sel_count && bytes + p[d.sel_count - 1u].pre > max_size) {
      u32 lo = 0, hi = d.sel_count - 1u;                /* the first k with bytes + pre[k] > max_size */
      while (lo < hi) {
        const u32 mid = (lo + hi) >> 1;
        if (bytes + p[mid].pre > max_size) hi = mid; else lo = mid + 1u;
      }
      full_k = lo;
    }
    /* copy order: the missing index is met before the entry that took its place; the payload is read before append_raw */
    if (d.miss_k != NONE32 && d.miss_k <= d.trunc_k && d.miss_k <= full_k) {
      res.status = RGB_SEG_COMPACT_MISSING; res.source = s; res.index = d.miss_idx;
    } else if (d.trunc_k != NONE32 && d.trunc_k <= full_k) {
      res.status = RGB_SEG_COMPACT_TRUNCATED; res.source = s; res.index = p[d.trunc_k].idx;
    } else if (full_k != NONE32) {
      res.status = RGB_SEG_COMPACT_FULL; res.source = s; res.index = p[full_k].idx;
    } else {
      byte_base[s] = bytes;
      bytes += d.sel_bytes;
      recs += d.sel_count;
    }
  }
  if (!res.status) {
    res.n_entries = recs;                               /* == max_count: every live index was found */
    res.file_bytes = (u64)RGB_SEG_HEADER_BYTES + (u64)RGB_SEG_RECORD_BYTES * max_count + bytes;
    if (out_bytes < res.file_bytes) { res.status = RGB_SEG_COMPACT_SPACE; res.n_entries = 0u; }
  }
  hdr->status = res.status;
  hdr->crc_fail = NONE32;
  __builtin_memcpy(result_v, &res, sizeof res);
}

/* plain gather-copy of a payload of len >= 16 bytes: 16-byte slots aligned to its END (as load_slot), the first one
 * moved up to the payload's start -- the bytes it shares with its successor are written twice with the same value */
template <int GROUP>
__device__ __forceinline__ void copy_plain(const unsigned char *pay, unsigned char *dst, u32 len, u32 lane) {
  const u32 slots = (u32)(((u64)len + 15u) >> 4);
  const u32 pad = (u32)(((u64)slots << 4) - len);
#pragma unroll 4
  for (u32 t = lane; t < slots; t += (u32)GROUP) {
    const u64 q = t ? ((u64)t << 4) - pad : 0ull;
    *reinterpret_cast<v4u_any *>(dst + q) = __builtin_nontemporal_load(reinterpret_cast<const v4u_any *>(pay + q));
  }
}

template <int GROUP, bool VERIFY>
__global__ __launch_bounds__(THREADS) void rgb_compact_copy_kernel(
    const plan_rec *__restrict__ plan, u32 n, const unsigned char *__restrict__ files, const u64 *__restrict__ byte_base,
    work_hdr *__restrict__ hdr, unsigned char *__restrict__ out) {
  __shared__ __attribute__((aligned(16))) u32 lds[VERIFY ? LDS_WORDS : 4u];
  if (hdr->status != RGB_SEG_COMPACT_OK) return;        /* decided before this launch: the same for every lane */
  if (VERIFY) load_tables<GROUP>(lds);
  constexpr u32 PER_BLOCK = THREADS / GROUP;
  const u32 lane = threadIdx.x & (GROUP - 1);
  const u64 data_start = (u64)RGB_SEG_HEADER_BYTES + (u64)RGB_SEG_RECORD_BYTES * n;
  if (blockIdx.x == 0 && threadIdx.x == 0) put_header(out, n);
  for (u32 base = blockIdx.x * PER_BLOCK; base < n; base += gridDim.x * PER_BLOCK) {
    const u32 e = base + threadIdx.x / GROUP;
    const bool live = e < n;
    plan_rec p{};
    u64 dst_off = 0;
    if (live) { p = plan[e]; dst_off = data_start + byte_base[p.src] + p.pre; }
    const u32 len = p.len;
    const unsigned char *pay = files + p.src_off;
    unsigned char *dst = out + dst_off;
    const bool wide = live && len >= 16u;
    u32 crc = 0;
    if (VERIFY) crc = entry_crc<GROUP, true>(lds, pay, dst, len, live, lane);
    else if (wide) copy_plain<GROUP>(pay, dst, len, lane);
    if (live && lane == 0u) {
      if (VERIFY) crc = lane0_crc<true>(lds, crc, pay, dst, len);
      else if (!wide) for (u32 k = 0; k < len; ++k) dst[k] = pay[k];
      if (VERIFY && p.crc != 0u && crc != p.crc) atomic_min(&hdr->crc_fail, e);
      /* the source's Crc, 0 included */
      put_record(out + RGB_SEG_HEADER_BYTES + (u64)RGB_SEG_RECORD_BYTES * e, p.idx, p.term, dst_off, len, p.crc);
    }
  }
}

/* VERIFY: the first mismatch in copy order, once every workgroup of the copy is done */
__global__ void rgb_compact_finish_kernel(const plan_rec *__restrict__ plan, const work_hdr *__restrict__ hdr, void *result_v) {
  if (threadIdx.x != 0u || blockIdx.x != 0u) return;
  if (hdr->status != RGB_SEG_COMPACT_OK || hdr->crc_fail == NONE32) return;
  rgb_seg_compact_result res;
  __builtin_memcpy(&res, result_v, sizeof res);
  res.status = RGB_SEG_COMPACT_CRC;
  res.n_entries = 0u;
  res.source = plan[hdr->crc_fail].src;
  res.index = plan[hdr->crc_fail].idx;
  __builtin_memcpy(result_v, &res, sizeof res);
}

/* ---- major compaction for many members (include/ra_gpu_wal.h, "... for many members in one call") ----------
 * Any number of groups in one call.  resolve is rgb_compact_resolve_kernel as it is: its source numbers and plan bases
 * are already global.  The three passes behind it, each its own launch:
 *   place    one lane per group: the walk of rgb_compact_place_kernel over the group's own sources (byte bases within
 *            the group), the group's header row and result row, and the 8 header bytes of a good image -- a header-only
 *            group has no plan entry that could write them
 *   copy     GROUP lanes per plan entry across all groups.  The entry's group is found from the groups' first plan
 *            entries alone (a binary search: groups without entries share their first entry with their successor, and
 *            the last of equals is the one that owns it) -- NOT from the plan record, which a failed group may have
 *            left unwritten.  Record number = entry - the group's first entry.  Nothing for a group that is not OK.
 *   finish   (VERIFY) one lane per group: the first mismatch of the group in copy order into a CRC status
 * The kernels' parameter types are the unit's own (see "major compaction" above). */
struct grp_desc { u64 out_offset, out_bytes; u32 src_first, src_n, plan_first, max_count; };   /* staged from the host */
static_assert(sizeof(grp_desc) == 32, "");
constexpr int GRP_LANES = 64;                           /* groups per workgroup of place and finish: one wavefront */

__global__ __launch_bounds__(GRP_LANES) void rgb_cgroups_place_kernel(
    const grp_desc *__restrict__ groups, u32 n_groups, const src_desc *__restrict__ srcs, const src_done *__restrict__ done,
    const plan_rec *__restrict__ plan, u64 max_size, u64 *__restrict__ byte_base, work_hdr *__restrict__ hdrs,
    unsigned char *__restrict__ out, void *results_v) {
  const u32 g = blockIdx.x * GRP_LANES + threadIdx.x;
  if (g >= n_groups) return;
  const grp_desc gd = groups[g];
  rgb_seg_compact_result res{};
  u64 bytes = 0;
  u32 recs = 0;
  for (u32 q = 0; q < gd.src_n && !res.status; ++q)
    if (done[gd.src_first + q].bad) { res.status = RGB_SEG_COMPACT_BAD_SOURCE; res.source = q; }
  for (u32 q = 0; q < gd.src_n && !res.status; ++q) {
    const u32 s = gd.src_first + q;
    const src_done d = done[s];
    const plan_rec *p = plan + srcs[s].plan_base;
    /* as rgb_compact_place_kernel: the first k with more than max_size payload bytes of the GROUP in front of it */
    u32 full_k = NONE32;
    if (d.sel_count && bytes + p[d.sel_count - 1u].pre > max_size) {
      u32 lo = 0, hi = d.sel_count - 1u;
      while (lo < hi) {
        const u32 mid = (lo + hi) >> 1;
        if (bytes + p[mid].pre > max_size) hi = mid; else lo = mid + 1u;
      }
      full_k = lo;
    }
    if (d.miss_k != NONE32 && d.miss_k <= d.trunc_k && d.miss_k <= full_k) {
      res.status = RGB_SEG_COMPACT_MISSING; res.source = q; res.index = d.miss_idx;
    } else if (d.trunc_k != NONE32 && d.trunc_k <= full_k) {
      res.status = RGB_SEG_COMPACT_TRUNCATED; res.source = q; res.index = p[d.trunc_k].idx;
    } else if (full_k != NONE32) {
      res.status = RGB_SEG_COMPACT_FULL; res.source = q; res.index = p[full_k].idx;
    } else {
      byte_base[s] = bytes;
      bytes += d.sel_bytes;
      recs += d.sel_count;
    }
  }
  if (!res.status) {
    res.n_entries = recs;                               /* == max_count: every live index was found */
    res.file_bytes = (u64)RGB_SEG_HEADER_BYTES + (u64)RGB_SEG_RECORD_BYTES * gd.max_count + bytes;
    if (gd.out_bytes < res.file_bytes) { res.status = RGB_SEG_COMPACT_SPACE; res.n_entries = 0u; }
  }
  if (!res.status) put_header(out + gd.out_offset, gd.max_count);
  work_hdr h{};
  h.status = res.status; h.crc_fail = NONE32;
  hdrs[g] = h;
  __builtin_memcpy(reinterpret_cast<unsigned char *>(results_v) + sizeof(res) * (u64)g, &res, sizeof res);
}

/* the group that owns plan entry e: the last g with plan_first <= e (e < the entries of the call, so there is one) */
__device__ __forceinline__ u32 group_of_entry(const grp_desc *groups, u32 n_groups, u32 e) {
  u32 lo = 0, hi = n_groups;                            /* lo = groups whose plan_first <= e, at least one */
  while (hi - lo > 1u) {
    const u32 mid = (lo + hi) >> 1;
    if (groups[mid].plan_first <= e) lo = mid; else hi = mid;
  }
  return lo;
}

template <int GROUP, bool VERIFY>
__global__ __launch_bounds__(THREADS) void rgb_cgroups_copy_kernel(
    const plan_rec *__restrict__ plan, u32 n, const grp_desc *__restrict__ groups, u32 n_groups,
    const unsigned char *__restrict__ files, const u64 *__restrict__ byte_base, work_hdr *__restrict__ hdrs,
    unsigned char *__restrict__ out) {
  __shared__ __attribute__((aligned(16))) u32 lds[VERIFY ? LDS_WORDS : 4u];
  if (VERIFY) load_tables<GROUP>(lds);
  constexpr u32 PER_BLOCK = THREADS / GROUP;
  const u32 lane = threadIdx.x & (GROUP - 1);
  for (u32 base = blockIdx.x * PER_BLOCK; base < n; base += gridDim.x * PER_BLOCK) {
    const u32 e = base + threadIdx.x / GROUP;
    bool live = e < n;
    u32 g = 0, rec = 0;
    unsigned char *image = out;
    u64 data_start = 0;
    if (live) {
      g = group_of_entry(groups, n_groups, e);
      live = hdrs[g].status == RGB_SEG_COMPACT_OK;      /* decided before this launch: the same for the whole group */
    }
    plan_rec p{};
    u64 dst_off = 0;
    if (live) {
      const grp_desc gd = groups[g];
      p = plan[e];
      rec = e - gd.plan_first;
      image = out + gd.out_offset;
      data_start = (u64)RGB_SEG_HEADER_BYTES + (u64)RGB_SEG_RECORD_BYTES * gd.max_count;
      dst_off = data_start + byte_base[p.src] + p.pre;
    }
    const u32 len = p.len;
    const unsigned char *pay = files + p.src_off;
    unsigned char *dst = image + dst_off;
    const bool wide = live && len >= 16u;
    u32 crc = 0;
    if (VERIFY) crc = entry_crc<GROUP, true>(lds, pay, dst, len, live, lane);
    else if (wide) copy_plain<GROUP>(pay, dst, len, lane);
    if (live && lane == 0u) {
      if (VERIFY) crc = lane0_crc<true>(lds, crc, pay, dst, len);
      else if (!wide) for (u32 k = 0; k < len; ++k) dst[k] = pay[k];
      if (VERIFY && p.crc != 0u && crc != p.crc) atomic_min(&hdrs[g].crc_fail, rec);
      /* the source's Crc, 0 included */
      put_record(image + RGB_SEG_HEADER_BYTES + (u64)RGB_SEG_RECORD_BYTES * rec, p.idx, p.term, dst_off, len, p.crc);
    }
  }
}

/* VERIFY: per group the first mismatch in copy order, once every workgroup of the copy is done */
__global__ __launch_bounds__(GRP_LANES) void rgb_cgroups_finish_kernel(
    const grp_desc *__restrict__ groups, u32 n_groups, const plan_rec *__restrict__ plan,
    const work_hdr *__restrict__ hdrs, void *results_v) {
  const u32 g = blockIdx.x * GRP_LANES + threadIdx.x;
  if (g >= n_groups) return;
  const work_hdr h = hdrs[g];
  if (h.status != RGB_SEG_COMPACT_OK || h.crc_fail == NONE32) return;
  const plan_rec *p = plan + groups[g].plan_first + h.crc_fail;
  unsigned char *row = reinterpret_cast<unsigned char *>(results_v) + sizeof(rgb_seg_compact_result) * (u64)g;
  rgb_seg_compact_result res;
  __builtin_memcpy(&res, row, sizeof res);
  res.status = RGB_SEG_COMPACT_CRC;
  res.n_entries = 0u;
  res.source = p->src - groups[g].src_first;
  res.index = p->idx;
  __builtin_memcpy(row, &res, sizeof res);
}

/* ---- reading entries back (include/ra_gpu_wal.h, "reading entries back") -----------------------------------
 * Passes, each its own launch, so that no workgroup ever waits for another:
 *   resolve  one workgroup per source: the walk and the effective records as in compaction (walk_effective), the
 *            effective records' numbers as one ascending table in scratch (their Idx ascend with them; a source whose
 *            records are all effective needs none: the record number IS the place), then the source's requests in steps
 *            of THREADS: a binary search each, the row, the bytes in front of it within the slice (LDS scan, carried
 *            from step to step), the first MISSING and the first TRUNCATED position
 *   place    one workgroup: the sources' first bytes in `out` (a scan in steps of THREADS, carried from step to step),
 *            their result rows, the total and SPACE
 *   copy     GROUP lanes per good row: the final data_offset and, unless the status is SPACE, the payload -- with
 *            VERIFY its CRC in the same read, and per source the first position whose CRC does not match
 *   finish   (VERIFY) one workgroup: those positions into CRC statuses
 * With NO_DATA the rows are final after resolve, and copy and finish are not launched.
 * The kernels' parameter types are the unit's own (see "major compaction" above). */
struct rd_src { u64 offset, n_bytes; u32 req_first, req_n; u64 tab_base; };                 /* staged from the host */
struct rd_done { u64 bytes, bad_idx; u32 bad_k, kind; u64 _pad; };                          /* resolve -> place */
struct alignas(16) rd_plan { u64 src_off, pre; u32 src, pos, len, crc; };                   /* resolve -> copy, per request */
struct rd_row { u64 idx, term, off; u32 len, crc; };
static_assert(sizeof(rd_src) == sizeof(rgb_seg_read_source) && sizeof(rd_done) == 32 && sizeof(rd_plan) == 32, "");
static_assert(sizeof(rd_row) == sizeof(rgb_seg_entry) && sizeof(rgb_seg_read_result) == 32 && sizeof(rgb_seg_read_total) == 16, "");

__device__ __forceinline__ rd_row missing_row(u64 idx) {
  rd_row w;
  w.idx = idx; w.term = 0ull; w.off = RGB_UNDEF; w.len = 0u; w.crc = 0u;
  return w;
}

/* the plan record of a row that has nothing to copy */
__device__ __forceinline__ rd_plan no_plan() {
  rd_plan p;
  p.src_off = p.pre = 0ull; p.src = NONE32; p.pos = p.len = p.crc = 0u;
  return p;
}

__global__ __launch_bounds__(THREADS) void rgb_read_resolve_kernel(
    const rd_src *__restrict__ srcs, const unsigned char *__restrict__ files, const u64 *__restrict__ req, u32 no_data,
    u32 *tab, void *rows_v, rd_plan *__restrict__ plan, rd_done *__restrict__ done) {
  __shared__ u64 s_wide[THREADS];                       /* scan buffer: suffix min of Idx, prefix sum of bytes */
  __shared__ u32 s_cnt[THREADS];                        /* scan buffer: prefix count */
  __shared__ u32 s_bits[CMP_MAX_RECORDS / 32];          /* record j is effective */
  __shared__ u32 s_first_zero, s_eff, s_miss_k, s_trunc_k;
  const u32 tid = threadIdx.x, s = blockIdx.x;
  const rd_src sd = srcs[s];
  const unsigned char *f = files + sd.offset;
  const u64 *asked = req + sd.req_first;
  rd_row *rows = reinterpret_cast<rd_row *>(rows_v) + sd.req_first;

  u32 version, max_count;
  read_header(f, sd.n_bytes, &version, &max_count);
  if (version < 1u || version > RGB_SEG_VERSION) {      /* the same for every lane */
    for (u32 k = tid; k < sd.req_n; k += THREADS) {
      rows[k] = missing_row(asked[k]);
      if (!no_data) plan[sd.req_first + k] = no_plan();
    }
    if (tid == 0u) { rd_done d{}; d.kind = RGB_SEG_READ_BAD_SOURCE; done[s] = d; }
    return;
  }
  const bool v2 = version == 2u;
  const u32 rec_bytes = v2 ? RGB_SEG_RECORD_BYTES : RGB_SEG_RECORD_BYTES_V1;
  const u64 fit = (sd.n_bytes - RGB_SEG_HEADER_BYTES) / rec_bytes;            /* whole records inside the file */
  const u32 n_fit = fit < max_count ? (u32)fit : max_count;
  const unsigned char *index = f + RGB_SEG_HEADER_BYTES;

  if (tid == 0u) { s_miss_k = NONE32; s_trunc_k = NONE32; }
  u64 min_idx;
  const u32 n_walk = walk_effective(index, rec_bytes, v2, n_fit, s_wide, s_bits, &s_first_zero, &s_eff, &min_idx,
                                    [](const idx_rec &) {});
  const u32 n_chunks = (n_walk + THREADS - 1u) / THREADS;
  const u32 n_eff = s_eff;
  const bool dense = n_eff == n_walk;                   /* every record effective: place k is record k */
  u32 *places = tab + sd.tab_base;

  /* in file order: the effective records' numbers, one behind the other */
  if (!dense) {
    u32 run_cnt = 0;
    for (u32 c = 0; c < n_chunks; ++c) {
      const u32 j = c * THREADS + tid;
      const bool sel = j < n_walk && ((s_bits[j >> 5] >> (j & 31u)) & 1u);
      s_cnt[tid] = sel ? 1u : 0u;
      __syncthreads();
      for (u32 off = 1; off < THREADS; off <<= 1) {
        u32 tc = s_cnt[tid];
        if (tid >= off) tc += s_cnt[tid - off];
        __syncthreads();
        s_cnt[tid] = tc;
        __syncthreads();
      }
      if (sel) places[run_cnt + s_cnt[tid] - 1u] = j;
      run_cnt += s_cnt[THREADS - 1];
      __syncthreads();
    }
  }

  /* the requests, in the caller's order */
  u64 run_bytes = 0;
  for (u32 base = 0; base < sd.req_n; base += THREADS) {
    const u32 k = base + tid;
    const bool valid = k < sd.req_n;
    idx_rec r{};
    u64 q = 0;
    u32 kind = RGB_SEG_READ_OK;
    if (valid) {
      q = asked[k];
      u32 lo = 0, hi = n_eff;                           /* lo = effective records whose Idx < q */
      while (lo < hi) {
        const u32 mid = (lo + hi) >> 1;
        if (ld_be64(index + (u64)rec_bytes * (dense ? mid : places[mid])) < q) lo = mid + 1u; else hi = mid;
      }
      if (lo < n_eff) r = decode_rec(index + (u64)rec_bytes * (dense ? lo : places[lo]), v2);
      if (lo == n_eff || r.idx != q) kind = RGB_SEG_READ_MISSING;
      else if (r.off > sd.n_bytes || r.len > sd.n_bytes - r.off) kind = RGB_SEG_READ_TRUNCATED;
    }
    const bool good = valid && kind == RGB_SEG_READ_OK;
    const u32 len = good && !no_data ? r.len : 0u;      /* the bytes of `out` the row takes */
    s_wide[tid] = len;
    __syncthreads();
    for (u32 off = 1; off < THREADS; off <<= 1) {
      u64 tb = s_wide[tid];
      if (tid >= off) tb += s_wide[tid - off];
      __syncthreads();
      s_wide[tid] = tb;
      __syncthreads();
    }
    if (good) {
      const u64 pre = run_bytes + s_wide[tid] - len;
      rd_row w;
      w.idx = r.idx; w.term = r.term; w.off = no_data ? sd.offset + r.off : pre; w.len = r.len; w.crc = r.crc;
      rows[k] = w;
      if (!no_data) {
        rd_plan p;
        p.src_off = sd.offset + r.off; p.pre = pre; p.src = s; p.pos = k; p.len = r.len; p.crc = r.crc;
        plan[sd.req_first + k] = p;
      }
    } else if (valid) {
      rows[k] = missing_row(q);
      if (!no_data) plan[sd.req_first + k] = no_plan();
      atomic_min(kind == RGB_SEG_READ_MISSING ? &s_miss_k : &s_trunc_k, k);
    }
    run_bytes += s_wide[THREADS - 1];
    __syncthreads();
  }
  if (tid == 0u) {
    rd_done d{};
    d.bytes = run_bytes;
    d.bad_k = s_miss_k < s_trunc_k ? s_miss_k : s_trunc_k;            /* the first bad row of either kind */
    if (d.bad_k != NONE32) {
      d.kind = s_miss_k < s_trunc_k ? RGB_SEG_READ_MISSING : RGB_SEG_READ_TRUNCATED;
      d.bad_idx = asked[d.bad_k];
    }
    done[s] = d;
  }
}

__global__ __launch_bounds__(THREADS) void rgb_read_place_kernel(
    const rd_src *__restrict__ srcs, u32 n_sources, const rd_done *__restrict__ done, u64 out_bytes,
    u64 *__restrict__ byte_base, u32 *__restrict__ crc_k, work_hdr *__restrict__ hdr, void *results_v, void *total_v) {
  __shared__ u64 s_wide[THREADS];
  __shared__ u32 s_bad;
  const u32 tid = threadIdx.x;
  rgb_seg_read_result *results = reinterpret_cast<rgb_seg_read_result *>(results_v);
  if (tid == 0u) s_bad = 0u;
  u64 run_bytes = 0;
  u32 my_bad = 0;
  for (u32 base = 0; base < n_sources; base += THREADS) {
    const u32 s = base + tid;
    const bool valid = s < n_sources;
    rd_done d{};
    if (valid) d = done[s];
    s_wide[tid] = d.bytes;
    __syncthreads();
    for (u32 off = 1; off < THREADS; off <<= 1) {
      u64 tb = s_wide[tid];
      if (tid >= off) tb += s_wide[tid - off];
      __syncthreads();
      s_wide[tid] = tb;
      __syncthreads();
    }
    if (valid) {
      byte_base[s] = run_bytes + s_wide[tid] - d.bytes;
      crc_k[s] = NONE32;
      rgb_seg_read_result res{};
      res.status = d.kind;
      res.n_read = d.kind == RGB_SEG_READ_OK ? srcs[s].req_n : d.bad_k;
      res.index = d.bad_idx; res.data_bytes = d.bytes;
      results[s] = res;
      if (d.kind != RGB_SEG_READ_OK) my_bad += 1u;
    }
    run_bytes += s_wide[THREADS - 1];
    __syncthreads();
  }
  if (my_bad) atomicAdd(&s_bad, my_bad);
  __syncthreads();
  if (tid == 0u) {
    rgb_seg_read_total t{};
    t.status = out_bytes < run_bytes ? RGB_SEG_READ_SPACE : RGB_SEG_READ_OK;
    t.n_bad = s_bad; t.out_bytes = run_bytes;
    hdr->status = t.status;
    hdr->crc_fail = NONE32;
    *reinterpret_cast<rgb_seg_read_total *>(total_v) = t;
  }
}

template <int GROUP, bool VERIFY>
__global__ __launch_bounds__(THREADS) void rgb_read_copy_kernel(
    const rd_plan *__restrict__ plan, u32 n, const unsigned char *__restrict__ files, const u64 *__restrict__ byte_base,
    const work_hdr *__restrict__ hdr, u32 *__restrict__ crc_k, void *rows_v, unsigned char *__restrict__ out) {
  __shared__ __attribute__((aligned(16))) u32 lds[VERIFY ? LDS_WORDS : 4u];
  const bool room = hdr->status == RGB_SEG_READ_OK;     /* decided before this launch: the same for every lane */
  if (VERIFY && room) load_tables<GROUP>(lds);
  constexpr u32 PER_BLOCK = THREADS / GROUP;
  const u32 lane = threadIdx.x & (GROUP - 1);
  rd_row *rows = reinterpret_cast<rd_row *>(rows_v);
  for (u32 base = blockIdx.x * PER_BLOCK; base < n; base += gridDim.x * PER_BLOCK) {
    const u32 e = base + threadIdx.x / GROUP;
    bool live = e < n;
    rd_plan p{};
    if (live) { p = plan[e]; live = p.src != NONE32; }  /* a request of no slice, a MISSING or TRUNCATED row */
    u64 dst_off = 0;
    if (live) dst_off = byte_base[p.src] + p.pre;
    if (live && lane == 0u) rows[e].off = dst_off;
    live = live && room;                                /* SPACE: the rows are final, `out` is not touched */
    const u32 len = p.len;
    const unsigned char *pay = files + p.src_off;
    unsigned char *dst = out + dst_off;
    const bool wide = live && len >= 16u;
    u32 crc = 0;
    if (VERIFY) crc = entry_crc<GROUP, true>(lds, pay, dst, len, live, lane);
    else if (wide) copy_plain<GROUP>(pay, dst, len, lane);
    if (live && lane == 0u) {
      if (VERIFY) crc = lane0_crc<true>(lds, crc, pay, dst, len);
      else if (!wide) for (u32 k = 0; k < len; ++k) dst[k] = pay[k];
      if (VERIFY) {
        /* the stored Crc, the source and the position are fetched again here (loads the compiler does not merge with
         * the ones above): kept in registers across the copy they take the wavefront-per-row form from 8 to 7
         * wavefronts per SIMD */
        const u32 stored = __builtin_nontemporal_load(&plan[e].crc);
        if (stored != 0u && crc != stored)
          atomic_min(&crc_k[__builtin_nontemporal_load(&plan[e].src)], __builtin_nontemporal_load(&plan[e].pos));
      }
    }
  }
}

/* VERIFY: per source the first mismatch in request order, once every workgroup of the copy is done; MISSING and
 * TRUNCATED keep their place */
__global__ __launch_bounds__(THREADS) void rgb_read_finish_kernel(
    const rd_src *__restrict__ srcs, u32 n_sources, const u64 *__restrict__ req, const u32 *__restrict__ crc_k,
    const work_hdr *__restrict__ hdr, void *results_v, void *total_v) {
  __shared__ u32 s_new;
  if (hdr->status != RGB_SEG_READ_OK) return;           /* the same for every lane */
  rgb_seg_read_result *results = reinterpret_cast<rgb_seg_read_result *>(results_v);
  if (threadIdx.x == 0u) s_new = 0u;
  __syncthreads();
  u32 mine = 0;
  for (u32 s = threadIdx.x; s < n_sources; s += THREADS) {
    const u32 k = crc_k[s];
    if (k == NONE32 || results[s].status != RGB_SEG_READ_OK) continue;
    results[s].status = RGB_SEG_READ_CRC;
    results[s].n_read = k;
    results[s].index = req[srcs[s].req_first + k];
    mine += 1u;
  }
  if (mine) atomicAdd(&s_new, mine);
  __syncthreads();
  if (threadIdx.x == 0u) reinterpret_cast<rgb_seg_read_total *>(total_v)->n_bad += s_new;
}

/* ---- mem-table flush (include/ra_gpu_wal.h, "mem-table flush") ---------------------------------------------
 * Three passes, each its own launch, so that no workgroup ever waits for another:
 *   plan   S lanes per writer (8, 16 or a wavefront, by the longest writer of the call), THREADS / S writers per step of
 *          a workgroup, every workgroup a contiguous run of writers.  A writer goes through in chunks of S entries: an
 *          LDS prefix sum of the lengths, then the sub-group's first lane walks the SEGMENTS of the chunk -- the next
 *          boundary is the count limit or, by binary search on the prefix sums, the first entry with more than max_size
 *          bytes in front of it -- with the file's and the running piece's state carried from chunk to chunk.  Every
 *          entry then finds its segment and leaves its plan record, the first lane of a segment the minimum index; a
 *          piece that ends is stored at its first entry's number.  Per writer: pieces and bytes of `out`, relative to
 *          the writer's own start; per workgroup: their sums, and the first entry whose payload lies outside the data.
 *   place  the same grid: every workgroup adds up the sums of all (the status, the result row) and of its predecessors,
 *          then scans its own writers -- each writer's first piece row and first byte of `out` -- and turns the plan
 *          record of each of their entries into places in `out` and in the file; a piece's first entry leaves the piece
 *          row and, for a successor file, the header.  Nothing unless the status is OK.
 *   copy   GROUP lanes per entry: the payload into `out` with its CRC in the same read, the index record.  Nothing
 *          unless the status is OK.
 * The kernels' parameter types are the unit's own (see "major compaction" above). */
constexpr int FL_CHUNK = 64;                    /* entries per step of a writer at the widest sub-group */
constexpr u32 FL_GRID_CAP = 1024u;              /* workgroups of plan and place: the sums every one of them adds up */

struct fl_writer { u32 entry_first, entry_n, open_count, open_max_count; u64 open_data_bytes, range_first, range_last, _pad; };
struct fl_entry { u64 idx, term, off; u32 len, crc; };
struct alignas(16) fl_row { u64 out_bytes, out_base; u32 n_pieces, piece_base, first_ord, _pad; };   /* per writer */
struct alignas(16) fl_plan { u64 pre, rel_out; u32 start, ordinal, writer, _pad; };                 /* per entry */
struct alignas(16) fl_place { u64 dst_off, file_off, rec_off; u32 writer, _pad; };              /* per entry, over its fl_plan */
struct alignas(16) fl_piece { u64 data_bytes, range_first, range_last; u32 entry_n, _pad; };        /* at a piece's first entry */
struct alignas(16) fl_total { u64 out_bytes, bad; u32 n_pieces, _pad[3]; };                         /* per workgroup of plan */
struct fl_seg { u64 rel_out, pre_base; u32 p0, p1, ordinal, start, n_before, closes; };             /* LDS: a piece's part in a chunk */
static_assert(sizeof(fl_writer) == sizeof(rgb_seg_writer) && sizeof(fl_entry) == sizeof(rgb_seg_entry), "");
static_assert(sizeof(fl_row) == 32 && sizeof(fl_plan) == 32 && sizeof(fl_place) == 32 && sizeof(fl_piece) == 32 && sizeof(fl_total) == 32, "");

__device__ __forceinline__ void atomic_min64(u64 *p, u64 v) {
  u64 old = *p;
  while (v < old) {
    const u64 seen = atomicCAS(p, old, v);
    if (seen == old) break;
    old = seen;
  }
}
/* bytes in front of entry j of a chunk, from the chunk's inclusive prefix sums */
__device__ __forceinline__ u64 fl_pex(const u64 *pre, u32 j) { return j ? pre[j - 1u] : 0ull; }

template <int S>
__global__ __launch_bounds__(THREADS) void rgb_flush_plan_kernel(
    const fl_writer *__restrict__ writers, u32 n_writers, u32 per_block, const fl_entry *__restrict__ entries,
    u64 data_bytes, u32 max_count, u64 max_size, fl_row *__restrict__ rows, fl_plan *__restrict__ plan,
    fl_piece *__restrict__ pieces, fl_total *__restrict__ totals) {
  constexpr u32 SUBS = THREADS / S;
  __shared__ u64 s_pre[THREADS];                        /* inclusive prefix sums of the lengths, per sub-group */
  __shared__ u64 s_idx[THREADS];
  __shared__ fl_seg s_seg[THREADS];                     /* at most S segments in a chunk of S entries */
  __shared__ u32 s_nseg[SUBS], s_chunks[SUBS];
  __shared__ u64 s_min[SUBS];                           /* the minimum index of a piece that goes on in the next chunk */
  __shared__ u64 s_tot_bytes, s_bad;
  __shared__ u32 s_tot_pieces;
  const u32 tid = threadIdx.x, sub = tid / (u32)S, ln = tid % (u32)S;
  const u32 wb = blockIdx.x * per_block;
  const u32 we = n_writers - wb < per_block ? n_writers : wb + per_block;
  const u64 *pre = s_pre + sub * S;
  const u64 *idxs = s_idx + sub * S;
  fl_seg *segs = s_seg + sub * S;
  if (tid == 0u) { s_tot_bytes = 0ull; s_bad = NONE64; s_tot_pieces = 0u; }
  __syncthreads();
  for (u32 r0 = wb; r0 < we; r0 += SUBS) {              /* the same for every lane */
    const u32 w = r0 + sub;
    const bool have = w < we;
    fl_writer wd{};
    if (have) wd = writers[w];
    const u32 my_chunks = wd.entry_n / (u32)S + (wd.entry_n % (u32)S ? 1u : 0u);
    if (ln == 0u) {
      s_chunks[sub] = my_chunks;
      if (have && !wd.entry_n) { fl_row z{}; rows[w] = z; }
    }
    __syncthreads();
    u32 iters = 0;
    for (u32 i = 0; i < SUBS; ++i) iters = s_chunks[i] > iters ? s_chunks[i] : iters;
    __syncthreads();                                    /* (a step without entries has no other barrier before the next) */
    /* the sub-group's first lane: the file (c, b, k, maxc), the running piece (pn entries, pb bytes, from entry pstart,
     * at prel of the writer's part of `out`), the writer (rel bytes of `out`, npieces) */
    u32 c = wd.open_count, maxc = wd.open_max_count, k = 0, pn = 0, pstart = 0, npieces = 0, first_ord = 0;
    u64 b = wd.open_data_bytes, pb = 0, prel = 0, rel = 0, carry_min = NONE64, carry_last = 0;
    for (u32 ch = 0; ch < iters; ++ch) {
      const bool active = ch < my_chunks;
      const u32 cbase = ch * (u32)S;
      const u32 n_c = !active ? 0u : (wd.entry_n - cbase < (u32)S ? wd.entry_n - cbase : (u32)S);
      const u32 e = wd.entry_first + cbase + ln;
      const bool valid = ln < n_c;
      fl_entry en{};
      if (valid) {
        en = entries[e];
        if (en.off > data_bytes || en.len > data_bytes - en.off) atomic_min64(&s_bad, ((u64)e << 32) | w);
      }
      s_pre[tid] = valid ? (u64)en.len : 0ull;
      s_idx[tid] = en.idx;
      __syncthreads();
      for (u32 off = 1; off < (u32)S; off <<= 1) {
        u64 t = s_pre[tid];
        if (ln >= off) t += s_pre[tid - off];
        __syncthreads();
        s_pre[tid] = t;
        __syncthreads();
      }
      if (ln == 0u) {
        u32 m = 0;
        if (active) {
          const bool last_chunk = ch + 1u == my_chunks;
          if (pn) carry_min = s_min[sub];
          u32 pos = 0;
          while (pos < n_c) {
            u32 bound = pos;
            if (c < maxc && b <= max_size) {            /* not full: entry pos goes in, and its successors up to ... */
              const u32 room = maxc - c;
              const u32 j1 = n_c - pos < room ? n_c : pos + room;           /* ... the count limit, or */
              const u64 lim = max_size - b, base = fl_pex(pre, pos);
              u32 lo = pos + 1u, hi = j1;               /* ... the first with more than max_size bytes in front of it */
              while (lo < hi) {
                const u32 mid = (lo + hi) >> 1;
                if (fl_pex(pre, mid) - base > lim) hi = mid; else lo = mid + 1u;
              }
              bound = lo;
            }
            if (bound > pos) {
              if (!pn) {
                pstart = wd.entry_first + cbase + pos; prel = rel;
                if (k) rel += RGB_SEG_HEADER_BYTES;
                if (!npieces) first_ord = k;
                npieces += 1u;
              }
              const u64 bytes = fl_pex(pre, bound) - fl_pex(pre, pos);
              fl_seg sg;
              sg.rel_out = prel; sg.pre_base = pb; sg.p0 = pos; sg.p1 = bound; sg.ordinal = k; sg.start = pstart;
              sg.n_before = pn; sg.closes = (bound < n_c || last_chunk) ? 1u : 0u;
              segs[m++] = sg;
              pn += bound - pos; pb += bytes; c += bound - pos; b += bytes;
              rel += (u64)RGB_SEG_RECORD_BYTES * (bound - pos) + bytes;
              if (sg.closes) { pn = 0u; pb = 0ull; }
              if (bound < n_c) { k += 1u; c = 0u; b = 0ull; maxc = max_count; }
              pos = bound;
            } else {                                    /* full before entry pos (only the chunk's first can be) */
              if (pn) {                                 /* the piece of the chunks before ends here */
                fl_piece pc;
                pc.data_bytes = pb; pc.entry_n = pn; pc._pad = 0u; pc.range_last = carry_last;
                pc.range_first = (k == 0u && wd.open_count && wd.range_first < carry_min) ? wd.range_first : carry_min;
                pieces[pstart] = pc;
                pn = 0u; pb = 0ull;
              }
              k += 1u; c = 0u; b = 0ull; maxc = max_count;
            }
          }
          carry_last = idxs[n_c - 1u];
          if (last_chunk) {
            fl_row r{};
            r.out_bytes = rel; r.n_pieces = npieces; r.first_ord = first_ord;
            rows[w] = r;
            atomicAdd(&s_tot_bytes, rel);
            atomicAdd(&s_tot_pieces, npieces);
          }
        }
        s_nseg[sub] = m;
      }
      __syncthreads();
      if (valid) {
        u32 lo = 0, hi = s_nseg[sub];                   /* lo = segments that start at or in front of this entry */
        while (lo < hi) {
          const u32 mid = (lo + hi) >> 1;
          if (segs[mid].p0 <= ln) lo = mid + 1u; else hi = mid;
        }
        const fl_seg sg = segs[lo - 1u];
        fl_plan p;
        p.pre = sg.pre_base + fl_pex(pre, ln) - fl_pex(pre, sg.p0);
        p.rel_out = sg.rel_out; p.start = sg.start; p.ordinal = sg.ordinal; p.writer = w; p._pad = 0u;
        plan[e] = p;
        if (ln == sg.p0) {
          u64 mn = NONE64;
          for (u32 j = sg.p0; j < sg.p1; ++j) mn = idxs[j] < mn ? idxs[j] : mn;
          if (sg.n_before && carry_min < mn) mn = carry_min;              /* (the sub-group's first lane) */
          if (sg.closes) {
            fl_piece pc;
            pc.data_bytes = sg.pre_base + fl_pex(pre, sg.p1) - fl_pex(pre, sg.p0);
            pc.entry_n = sg.n_before + sg.p1 - sg.p0; pc._pad = 0u;
            pc.range_last = idxs[sg.p1 - 1u];
            pc.range_first = (sg.ordinal == 0u && wd.open_count && wd.range_first < mn) ? wd.range_first : mn;
            pieces[sg.start] = pc;
          } else {
            s_min[sub] = mn;
          }
        }
      }
      __syncthreads();
    }
  }
  __syncthreads();
  if (tid == 0u) {
    fl_total t{};
    t.out_bytes = s_tot_bytes; t.bad = s_bad; t.n_pieces = s_tot_pieces;
    totals[blockIdx.x] = t;
  }
}

__global__ __launch_bounds__(THREADS) void rgb_flush_place_kernel(
    const fl_writer *__restrict__ writers, u32 n_writers, u32 per_block, u32 n_blocks, const fl_total *__restrict__ totals,
    fl_row *rows, fl_plan *plan, const fl_piece *__restrict__ pieces, u32 max_count, u32 pieces_cap, u64 out_bytes,
    work_hdr *__restrict__ hdr, void *pieces_out_v, unsigned char *__restrict__ out, void *result_v) {
  __shared__ u64 s_bytes[THREADS];
  __shared__ u32 s_cnt[THREADS];
  __shared__ u64 s_sum_bytes, s_base_bytes, s_bad;
  __shared__ u32 s_sum_pieces, s_base_pieces;
  const u32 tid = threadIdx.x;
  if (tid == 0u) { s_sum_bytes = s_base_bytes = 0ull; s_bad = NONE64; s_sum_pieces = s_base_pieces = 0u; }
  __syncthreads();
  u64 sb = 0, bb = 0, bad = NONE64;
  u32 sp = 0, bp = 0;
  for (u32 i = tid; i < n_blocks; i += THREADS) {
    const fl_total t = totals[i];
    sb += t.out_bytes; sp += t.n_pieces;
    if (i < blockIdx.x) { bb += t.out_bytes; bp += t.n_pieces; }
    if (t.bad < bad) bad = t.bad;
  }
  if (sb) atomicAdd(&s_sum_bytes, sb);
  if (bb) atomicAdd(&s_base_bytes, bb);
  if (sp) atomicAdd(&s_sum_pieces, sp);
  if (bp) atomicAdd(&s_base_pieces, bp);
  if (bad != NONE64) atomic_min64(&s_bad, bad);
  __syncthreads();
  u32 status = RGB_SEG_FLUSH_OK;
  if (s_bad != NONE64) status = RGB_SEG_FLUSH_ENTRY;
  else if (s_sum_pieces > pieces_cap || s_sum_bytes > out_bytes) status = RGB_SEG_FLUSH_SPACE;
  if (blockIdx.x == 0u && tid == 0u) {
    rgb_seg_flush_result res{};
    res.status = status;
    if (status == RGB_SEG_FLUSH_ENTRY) { res.entry = (u32)(s_bad >> 32); res.writer = (u32)s_bad; }
    else { res.n_pieces = s_sum_pieces; res.out_bytes = s_sum_bytes; }
    hdr->status = status;
    hdr->crc_fail = NONE32;
    __builtin_memcpy(result_v, &res, sizeof res);
  }
  if (status != RGB_SEG_FLUSH_OK) return;               /* the same for every lane of every workgroup */
  const u32 wb = blockIdx.x * per_block;
  if (wb >= n_writers) return;
  const u32 we = n_writers - wb < per_block ? n_writers : wb + per_block;
  u64 run_bytes = s_base_bytes;
  u32 run_cnt = s_base_pieces;
  for (u32 base = wb; base < we; base += THREADS) {
    const u32 w = base + tid;
    const bool valid = w < we;
    fl_row r{};
    if (valid) r = rows[w];
    s_bytes[tid] = r.out_bytes; s_cnt[tid] = r.n_pieces;
    __syncthreads();
    for (u32 off = 1; off < THREADS; off <<= 1) {
      u64 tb = s_bytes[tid];
      u32 tc = s_cnt[tid];
      if (tid >= off) { tb += s_bytes[tid - off]; tc += s_cnt[tid - off]; }
      __syncthreads();
      s_bytes[tid] = tb; s_cnt[tid] = tc;
      __syncthreads();
    }
    if (valid) {
      r.out_base = run_bytes + s_bytes[tid] - r.out_bytes;
      r.piece_base = run_cnt + s_cnt[tid] - r.n_pieces;
      rows[w] = r;
    }
    run_bytes += s_bytes[THREADS - 1];
    run_cnt += s_cnt[THREADS - 1];
    __syncthreads();
  }
  /* the entries of this workgroup's writers (one run of the entry array: the slices ascend): where each one's record
   * and payload go in `out`, what its record says; a piece's first entry also leaves the piece row and, for a
   * successor file, the header */
  const fl_writer w_last = writers[we - 1u];
  const u32 e_end = w_last.entry_first + w_last.entry_n;
  for (u32 e = writers[wb].entry_first + tid; e < e_end; e += THREADS) {
    const fl_plan p = plan[e];
    if (p.writer == NONE32) continue;                   /* an entry of no writer */
    const fl_row r = rows[p.writer];
    const fl_piece pc = pieces[p.start];
    const bool open_file = p.ordinal == 0u;
    u32 file_max = max_count, in_file = 0;
    u64 open_bytes = 0;
    if (open_file) {
      const fl_writer wd = writers[p.writer];
      file_max = wd.open_max_count; in_file = wd.open_count; open_bytes = wd.open_data_bytes;
    }
    const u64 piece_off = r.out_base + p.rel_out;                        /* positions in `out` ... */
    const u64 index_off = piece_off + (open_file ? 0u : RGB_SEG_HEADER_BYTES);
    const u64 data_off = index_off + (u64)RGB_SEG_RECORD_BYTES * pc.entry_n;
    const u64 file_data = (u64)RGB_SEG_HEADER_BYTES + (u64)RGB_SEG_RECORD_BYTES * file_max + open_bytes;   /* ... and in the file */
    fl_place d;
    d.dst_off = data_off + p.pre; d.file_off = file_data + p.pre;
    d.rec_off = index_off + (u64)RGB_SEG_RECORD_BYTES * (e - p.start);
    d.writer = p.writer; d._pad = 0u;
    *reinterpret_cast<fl_place *>(plan + e) = d;
    if (e == p.start) {
      if (!open_file) put_header(out + piece_off, max_count);
      rgb_seg_piece row;
      row.writer = p.writer; row.ordinal = p.ordinal; row.entry_first = e; row.entry_n = pc.entry_n;
      row.index_file_off = (u64)RGB_SEG_HEADER_BYTES + (u64)RGB_SEG_RECORD_BYTES * in_file;
      row.data_file_off = file_data;
      row.out_index_off = index_off; row.out_data_off = data_off; row.data_bytes = pc.data_bytes;
      row.range_first = pc.range_first; row.range_last = pc.range_last;
      row.max_count = file_max; row._pad = 0u;
      reinterpret_cast<rgb_seg_piece *>(pieces_out_v)[r.piece_base + (p.ordinal - r.first_ord)] = row;
    }
  }
}

template <int GROUP>
__global__ __launch_bounds__(THREADS) void rgb_flush_copy_kernel(
    const fl_entry *__restrict__ entries, u32 n, const unsigned char *__restrict__ data, const fl_place *__restrict__ placed,
    const work_hdr *__restrict__ hdr, u32 flags, unsigned char *__restrict__ out) {
  __shared__ __attribute__((aligned(16))) u32 lds[LDS_WORDS];
  if (hdr->status != RGB_SEG_FLUSH_OK) return;          /* decided before this launch: the same for every lane */
  load_tables<GROUP>(lds);
  constexpr u32 PER_BLOCK = THREADS / GROUP;
  const u32 lane = threadIdx.x & (GROUP - 1);
  for (u32 base = blockIdx.x * PER_BLOCK; base < n; base += gridDim.x * PER_BLOCK) {
    const u32 e = base + threadIdx.x / GROUP;
    bool live = e < n;
    fl_place d{};
    if (live) { d = placed[e]; live = d.writer != NONE32; }               /* an entry of no writer */
    fl_entry en{};
    if (live) en = entries[e];
    const u32 len = en.len;
    const unsigned char *pay = data + en.off;
    unsigned char *dst = out + d.dst_off;
    u32 crc = entry_crc<GROUP, true>(lds, pay, dst, len, live, lane);
    if (live && lane == 0u) {
      crc = lane0_crc<true>(lds, crc, pay, dst, len);
      if (flags & RGB_SEG_NO_CHECKSUMS) crc = 0u;
      put_record(out + d.rec_off, en.idx, en.term, d.file_off, len, crc);
    }
  }
}

/* ---- snapshots and checkpoints (include/ra_gpu_wal.h, "snapshots and checkpoints") -----------------------
 * A ragged batch: what an item checksums is a STREAM of up to two pieces at unrelated addresses, A ++ B, behind a
 * starting value `head` (in raw terms: head is multiplied by x^(8 |A ++ B|)):
 *     span      B = the span,                head = ~init
 *     image     A = Meta, B = Data,          head = raw(<<MetaSize:32>> xor 0xFFFFFFFF)    (indexes: B = Data, 0xFFFFFFFF)
 *     file      B = the bytes behind byte 9, head = 0xFFFFFFFF
 * The host knows every size, so it plans the call (snap_plan, below) and the device only walks the plan:
 *   group    a piece under SNAP_TBLOCK bytes gets 8, 16 or 64 lanes, as an entry of the per-entry kernel, one launch
 *            per width; the head of the stream is folded into the first four bytes of its first piece
 *   block    a longer piece is cut into blocks of SNAP_BLOCK bytes aligned to its END; the blocks of all such pieces
 *            are numbered through and dealt to one capped grid, a workgroup per block, the piece found by bisection
 *   finish   per item: raw(A), raw(B) joined (a workgroup for an item of several blocks, a lane for every other), then what
 *            the call is about -- the span's CRC, the image's header, the file's info row
 * Each pass is its own launch, so no workgroup ever waits for another.  A span that is one group piece needs no finish:
 * its group writes the CRC.  The kernels' parameter types are the unit's own (see "major compaction" above). */
constexpr u32 SNAP_BLOCK = STREAM_BLOCK;
constexpr u32 SNAP_T8 = 320u, SNAP_T16 = 1024u;      /* 8 lanes up to 320 bytes, 16 under 1 KiB, as group_width() */
constexpr u32 SNAP_TBLOCK = 16384u;                   /* a wavefront under 16 KiB, blocks from there */
constexpr u32 SNAP_DIRECT = 0x80000000u;              /* piece.slot: the CRC goes straight to crcs[slot & ~SNAP_DIRECT] */
constexpr int SNAP_SPANS = 0, SNAP_BUILD = 1, SNAP_VALIDATE = 2;
/* lane_raw / load_slot of their own for these kernels: the same source, but the other kernels' instantiations see the
 * starting values they always saw (constants), and so compile to what they compiled to before */
constexpr int SNAP_USER = 1;

struct snap_piece { u64 src, len, dst; u32 fold, slot; };                                  /* staged from the host */
struct snap_item { u64 off, len_a, len_b; u32 slot_a, slot_b, nblk_a, nblk_b, head, kind; };
struct snap_row { u32 status, version, stored_crc, computed_crc; u64 meta_offset; u32 meta_len, _pad; u64 data_offset, data_bytes; };
static_assert(sizeof(snap_piece) == 32 && sizeof(snap_item) == 48 && sizeof(snap_row) == sizeof(rgb_snap_info), "");

/* pow8[k] = x^(8 2^k): x^(8 n) is the product over the set bits of n */
struct Pow8 { u32 v[64]; };
constexpr Pow8 make_pow8() {
  Pow8 t{};
  u32 sq = X0 >> 8;
  for (int k = 0; k < 64; ++k) { t.v[k] = sq; sq = mulmod_c(sq, sq); }
  return t;
}
__device__ const Pow8 g_pow8 = make_pow8();
__device__ __forceinline__ u32 xpow8(u64 n) {
  u32 p = X0;
  for (int k = 0; n; ++k, n >>= 1)
    if (n & 1u) p = mulmod(p, g_pow8.v[k]);
  return p;
}

/* raws[slot] = raw(piece, its first four bytes xored with fold) = raw(piece) ^ fold * x^(8 len), for the n pieces of
 * one width; COPY: the piece goes to out + dst as it is read */
template <int GROUP, bool COPY>
__global__ __launch_bounds__(THREADS) void rgb_snap_group_kernel(const snap_piece *__restrict__ pieces, u32 n,
                                                                 const unsigned char *__restrict__ data,
                                                                 unsigned char *__restrict__ out, u32 *__restrict__ raws,
                                                                 u32 *__restrict__ crcs) {
  __shared__ __attribute__((aligned(16))) u32 lds[LDS_WORDS];
  load_tables<GROUP>(lds);
  constexpr u32 PER_BLOCK = THREADS / GROUP;
  constexpr int UNROLL = GROUP == 64 ? 4 : 2;
  const u32 lane = threadIdx.x & (GROUP - 1);
  for (u32 base = blockIdx.x * PER_BLOCK; base < n; base += gridDim.x * PER_BLOCK) {
    const u32 e = base + threadIdx.x / GROUP;
    const bool live = e < n;
    snap_piece p;
    p.src = p.len = p.dst = 0ull; p.fold = p.slot = 0u;
    if (live) p = pieces[e];
    const u32 len = (u32)p.len;                         /* < SNAP_TBLOCK */
    const unsigned char *pay = data + p.src;
    unsigned char *dst = COPY ? out + p.dst : nullptr;
    const u32 part = lane_raw<GROUP, UNROLL, COPY, SNAP_USER>(lds, pay, dst, live && len >= 16u ? len : 0u, lane, p.fold);
    u32 raw = group_xor<GROUP>(part);
    if (live && lane == 0u) {
      if (len < 16u) raw = ~crc_bytes(lds, ~p.fold, pay, len, dst);
      if (p.slot & SNAP_DIRECT) crcs[p.slot & ~SNAP_DIRECT] = ~raw;
      else raws[p.slot] = raw;
    }
  }
}

/* raws[slot + b] = raw(block b of its piece), for the n_blocks blocks of the n_big long pieces: blk_start[j] = the
 * number of the first block of piece j, blk_start[n_big] = n_blocks.  As rgb_seg_stream_kernel: the first block of a
 * piece is the short one. */
template <bool COPY>
__global__ __launch_bounds__(THREADS) void rgb_snap_block_kernel(const snap_piece *__restrict__ pieces,
                                                                 const u32 *__restrict__ blk_start, u32 n_big, u32 n_blocks,
                                                                 const unsigned char *__restrict__ data,
                                                                 unsigned char *__restrict__ out, u32 *__restrict__ raws) {
  __shared__ __attribute__((aligned(16))) u32 lds[LDS_WORDS];
  __shared__ u32 red[THREADS / 64];
  load_tables<256>(lds);
  for (u32 gb = blockIdx.x; gb < n_blocks; gb += gridDim.x) {
    u32 lo = 0, hi = n_big;                             /* the last piece whose first block is <= gb */
    while (hi - lo > 1u) {
      const u32 mid = (lo + hi) >> 1;
      if (blk_start[mid] <= gb) lo = mid; else hi = mid;
    }
    const snap_piece p = pieces[lo];
    const u32 b = gb - blk_start[lo], nb = blk_start[lo + 1u] - blk_start[lo];
    const u64 first_len = p.len - (u64)(nb - 1u) * SNAP_BLOCK;             /* 1 .. SNAP_BLOCK */
    const u64 start = b ? first_len + (u64)(b - 1u) * SNAP_BLOCK : 0ull;
    const u32 len = b ? SNAP_BLOCK : (u32)first_len;
    /* a first block under 16 bytes: its one slot loads (and copies) [0, 16) of the piece, and keeps its own bytes */
    const u32 part = lane_raw<256, 4, COPY, SNAP_USER>(lds, data + p.src + start, COPY ? out + p.dst + start : nullptr, len,
                                            threadIdx.x, 0u);
    const u32 w = group_xor<64>(part);
    if ((threadIdx.x & 63u) == 0u) red[threadIdx.x >> 6] = w;
    __syncthreads();
    if (threadIdx.x == 0u) raws[p.slot + b] = red[0] ^ red[1] ^ red[2] ^ red[3];
    __syncthreads();
  }
}

/* raw(piece) from its blocks' values, by the whole workgroup (every lane comes here and gets the answer): the sum of
 * rgb_seg_combine_kernel -- rounds of THREADS blocks, a round is x^(8 SNAP_BLOCK THREADS) */
__device__ __forceinline__ u32 snap_join_blocks(const u32 *__restrict__ partials, u32 n_blocks, u32 *red) {
  u32 acc = 0;
  const u32 k_round = g_tab.blk[256];
  for (u32 b = threadIdx.x; b < n_blocks; b += THREADS) acc = mulmod(acc, k_round) ^ partials[b];
  if (threadIdx.x < n_blocks) {
    const u32 last = threadIdx.x + ((n_blocks - 1u - threadIdx.x) / THREADS) * THREADS;
    acc = mulmod(acc, g_tab.blk[n_blocks - 1u - last]);
  }
  const u32 w = group_xor<64>(acc);
  if ((threadIdx.x & 63u) == 0u) red[threadIdx.x >> 6] = w;
  __syncthreads();
  const u32 raw = red[0] ^ red[1] ^ red[2] ^ red[3];
  __syncthreads();
  return raw;
}

__device__ __forceinline__ void put_be32(unsigned char *at, u32 v) {
  at[0] = (unsigned char)(v >> 24); at[1] = (unsigned char)(v >> 16); at[2] = (unsigned char)(v >> 8); at[3] = (unsigned char)v;
}

/* recover/1, validate/2, parse_snapshot/1 and read_meta_internal/1 of one file, whose CRC (behind byte 9) is `crc` */
__device__ __forceinline__ snap_row snap_check_file(const unsigned char *f, u64 off, u64 n, u32 kind, bool meta_only, u32 crc) {
  snap_row r{};
  const bool snapshot = kind == RGB_SNAP_KIND_SNAPSHOT;
  if (meta_only && n == 0ull) { r.status = RGB_SNAP_EOF; return r; }
  if (n < RGB_SNAP_HEADER_BYTES || f[0] != 'R' || f[1] != 'A' || f[2] != 'S' || f[3] != (snapshot ? 'N' : 'I')) {
    r.status = RGB_SNAP_INVALID_FORMAT;
    return r;
  }
  r.version = f[4];
  r.stored_crc = ld_be32(f + 5);
  if (r.version != 1u || (meta_only && snapshot && n < RGB_SNAP_META_HEADER_BYTES)) { r.status = RGB_SNAP_INVALID_VERSION; return r; }
  if (!meta_only) {
    r.computed_crc = crc;
    if (crc != r.stored_crc) { r.status = RGB_SNAP_CHECKSUM; return r; }
  }
  if (!snapshot) {
    r.data_offset = off + RGB_SNAP_HEADER_BYTES; r.data_bytes = n - RGB_SNAP_HEADER_BYTES;
    return r;
  }
  if (n < RGB_SNAP_META_HEADER_BYTES) { r.status = RGB_SNAP_BAD_META; return r; }
  const u32 meta_size = ld_be32(f + RGB_SNAP_HEADER_BYTES);
  if (meta_size > n - RGB_SNAP_META_HEADER_BYTES) { r.status = RGB_SNAP_BAD_META; return r; }
  r.meta_offset = off + RGB_SNAP_META_HEADER_BYTES; r.meta_len = meta_size;
  r.data_offset = r.meta_offset + meta_size; r.data_bytes = n - RGB_SNAP_META_HEADER_BYTES - meta_size;
  return r;
}

/* item i, its pieces' raw values known: raw(stream) = (head x^(8 |A|) ^ raw(A)) x^(8 |B|) ^ raw(B) */
template <int MODE>
__device__ __forceinline__ void snap_finish_item(const snap_item &it, u32 i, u32 raw_a, u32 raw_b,
                                                 const unsigned char *__restrict__ data, unsigned char *__restrict__ out,
                                                 u32 *__restrict__ crcs, snap_row *__restrict__ rows) {
  u32 t = raw_a;
  if (it.head) t ^= mulmod(it.head, xpow8(MODE == SNAP_VALIDATE ? 0ull : it.len_a));   /* a file has no piece A */
  u32 raw = raw_b;
  if (t) raw ^= mulmod(t, xpow8(it.len_b));
  const u32 crc = ~raw;
  if (MODE == SNAP_SPANS) {
    crcs[it.off] = crc;
  } else if (MODE == SNAP_BUILD) {
    unsigned char *o = out + it.off;
    const bool snapshot = it.kind == RGB_SNAP_KIND_SNAPSHOT;
    o[0] = 'R'; o[1] = 'A'; o[2] = 'S'; o[3] = snapshot ? 'N' : 'I'; o[4] = 1;
    put_be32(o + 5, crc);
    if (snapshot) put_be32(o + RGB_SNAP_HEADER_BYTES, (u32)it.len_a);
    if (crcs) crcs[i] = crc;
  } else {
    /* len_a = the file's n_bytes (it has no piece A) */
    rows[i] = snap_check_file(data + it.off, it.off, it.len_a, it.kind & 0xFFu, (it.kind >> 8) & RGB_SNAP_META_ONLY, crc);
  }
}

/* `big` = the n_big items that have a piece of more than one block, a workgroup each; then every other item, a lane each
 * (the items of a spans call are its long spans only: the others are DIRECT pieces) */
template <int MODE>
__global__ __launch_bounds__(THREADS) void rgb_snap_finish_kernel(const snap_item *__restrict__ items, u32 n_items,
                                                                  const u32 *__restrict__ big, u32 n_big,
                                                                  const u32 *__restrict__ raws,
                                                                  const unsigned char *__restrict__ data,
                                                                  unsigned char *__restrict__ out, u32 *__restrict__ crcs,
                                                                  snap_row *__restrict__ rows) {
  __shared__ u32 red[THREADS / 64];
  for (u32 k = blockIdx.x; k < n_big; k += gridDim.x) {
    const u32 i = big[k];
    const snap_item it = items[i];
    const u32 raw_a = snap_join_blocks(raws + it.slot_a, it.nblk_a, red);
    const u32 raw_b = snap_join_blocks(raws + it.slot_b, it.nblk_b, red);
    if (threadIdx.x == 0u) snap_finish_item<MODE>(it, i, raw_a, raw_b, data, out, crcs, rows);
  }
  for (u32 i = blockIdx.x * THREADS + threadIdx.x; i < n_items; i += gridDim.x * THREADS) {
    const snap_item it = items[i];
    if (it.nblk_a > 1u || it.nblk_b > 1u) continue;
    snap_finish_item<MODE>(it, i, it.nblk_a ? raws[it.slot_a] : 0u, it.nblk_b ? raws[it.slot_b] : 0u, data, out, crcs, rows);
  }
}

/* x^(8 n) mod P on the host */
inline u32 host_xpow8(u64 n) { return xpow8_c(n); }

}  // namespace seg
}  // namespace

extern "C" void *rgb_ctx_stream(rgb_ctx *ctx);
extern "C" int rgb_ctx_device(rgb_ctx *ctx);

#include <string.h>
#include <mutex>
#include <type_traits>
#include <unordered_map>
#include <vector>
namespace {
namespace seg {

/* ---- launching the per-entry kernels -------------------------------------------------------------------- */

/* the lanes that share an entry, from the mean payload of the call: known to the host without a sync, and a wrong guess
 * costs speed, never correctness */
inline u32 group_width(u64 mean_bytes) { return mean_bytes <= 320u ? 8u : mean_bytes < 1024u ? 16u : 64u; }
/* workgroups for n entries of `width` lanes each: capped (the kernels walk the batch), never 0 */
inline u32 entry_grid(u32 n, u32 width) {
  const u32 per = THREADS / width, grid = (n + per - 1u) / per;
  return grid > GRID_CAP ? GRID_CAP : grid ? grid : 1u;
}
/* f(std::integral_constant<int, width>), for the three widths the kernels are built for */
template <class F>
inline void with_width(u32 width, F &&f) {
  if (width == 8u) f(std::integral_constant<int, 8>{});
  else if (width == 16u) f(std::integral_constant<int, 16>{});
  else f(std::integral_constant<int, 64>{});
}

/* ---- per-context device buffers: staging of the host-buffer forms, scratch of the device forms ---------- */

/* a device block that only ever grows; gone with the context */
struct dev_buf {
  void *p = nullptr;
  size_t cap = 0;
  dev_buf() = default;
  dev_buf(const dev_buf &) = delete;
  dev_buf &operator=(const dev_buf &) = delete;
  ~dev_buf() { if (p) (void)hipFree(p); }
  int reserve(size_t need) {
    if (need <= cap) return 0;
    if (p) (void)hipFree(p);
    p = nullptr; cap = 0;
    const size_t want = need + need / 2 + 4096;
    if (hipMalloc(&p, want) != hipSuccess) return -1;
    cap = want;
    return 0;
  }
};

/* The descriptors of a device-form call on their way up: the host fills the pinned block `h`, `d` is its device copy.
 * `done` is recorded behind the upload, and the next call waits for it before it refills `h`. */
struct pinned_upload {
  void *h = nullptr;
  size_t cap_h = 0;
  dev_buf d;
  hipEvent_t done = nullptr;
  bool recorded = false;
  ~pinned_upload() {
    if (h) (void)hipHostFree(h);
    if (done) (void)hipEventDestroy(done);
  }
  /* the previous upload is over, and the pinned side holds `need` bytes: nothing on the device is touched yet, so
   * the caller can still validate (into `h`) and refuse */
  int prepare(size_t need) {
    if (!done && hipEventCreateWithFlags(&done, hipEventDisableTiming) != hipSuccess) return RGB_E_HIP;
    if (recorded && hipEventSynchronize(done) != hipSuccess) return RGB_E_HIP;
    recorded = false;
    if (need > cap_h) {
      if (h) (void)hipHostFree(h);
      h = nullptr; cap_h = 0;
      if (hipHostMalloc(&h, need * 2u, hipHostMallocDefault) != hipSuccess) return RGB_E_NOMEM;
      cap_h = need * 2u;
    }
    return RGB_OK;
  }
  int upload(size_t need, hipStream_t st) {
    if (d.reserve(need)) return RGB_E_NOMEM;
    if (hipMemcpyAsync(d.p, h, need, hipMemcpyHostToDevice, st) != hipSuccess) return RGB_E_HIP;
    if (hipEventRecord(done, st) != hipSuccess) return RGB_E_HIP;
    recorded = true;
    return RGB_OK;
  }
};

struct stage {
  dev_buf entries, data, offsets;                     /* host-buffer forms: what goes up ... */
  dev_buf crcs, out, pieces, result;                  /* ... and what comes down */
  dev_buf partials;                                   /* STREAM_MAX_BLOCKS values + the one result of the host-buffer form */
  pinned_upload compact_desc, flush_writers, read_desc;   /* device forms: the host arrays of a call ... */
  dev_buf compact_work, flush_work, read_work;        /* ... and its scratch plan */
  pinned_upload snap_plan_up;                         /* snapshots and checkpoints: the plan of a call ... */
  dev_buf snap_raws, infos;                           /* ... its pieces' raw values; the rows of the host-buffer form */
  std::vector<snap_piece> snap_pieces;                /* the plan on the host, before it is sorted into the upload */
  std::vector<snap_item> snap_items;
  std::vector<u32> snap_big;
};
std::recursive_mutex g_mu;     /* the host-buffer forms call the device forms with it held */
/* never destroyed: a context that is still open when the process ends must not free through a runtime that is gone */
std::unordered_map<rgb_ctx *, stage> &g_stages = *new std::unordered_map<rgb_ctx *, stage>;

/* the partial values of the context (allocated on the first long buffer) */
u32 *partials_of(rgb_ctx *ctx) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  stage &s = g_stages[ctx];
  if (s.partials.reserve((size_t)(STREAM_MAX_BLOCKS + 1u) * sizeof(u32))) return nullptr;
  return (u32 *)s.partials.p;
}

/* ---- the steps of a host-buffer form: stage the inputs, call the device form, fetch the answer ---------- */

inline bool slices_ok(const rgb_seg_entry *entries, u32 n, uint64_t data_bytes) {
  for (u32 i = 0; i < n; ++i)
    if (entries[i].data_offset > data_bytes || entries[i].data_len > data_bytes - entries[i].data_offset) return false;
  return true;
}
/* room for `bytes` in b, and the host's bytes in it */
int stage_in(dev_buf &b, const void *src, size_t bytes, hipStream_t st) {
  if (b.reserve(bytes)) return RGB_E_NOMEM;
  if (bytes && hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, st) != hipSuccess) return RGB_E_HIP;
  return RGB_OK;
}
int copy_down(void *dst, const dev_buf &b, size_t bytes, hipStream_t st) {
  return bytes && hipMemcpyAsync(dst, b.p, bytes, hipMemcpyDeviceToHost, st) != hipSuccess ? RGB_E_HIP : RGB_OK;
}
/* ... and the call is over */
int fetch(void *dst, const dev_buf &b, size_t bytes, hipStream_t st) {
  if (copy_down(dst, b, bytes, st)) return RGB_E_HIP;
  return hipStreamSynchronize(st) == hipSuccess ? RGB_OK : RGB_E_HIP;
}
/* The result row first; only the status `ok` brings the bulk bytes back, which bulk(row) enqueues: the caller's buffers
 * stay untouched otherwise. */
template <class Row, class F>
int fetch_result(Row *result, const dev_buf &d_row, u32 ok, hipStream_t st, F &&bulk) {
  Row row;
  if (int rc = fetch(&row, d_row, sizeof row, st)) return rc;
  if (row.status == ok) {
    if (int rc = bulk(row)) return rc;
    if (hipStreamSynchronize(st) != hipSuccess) return RGB_E_HIP;
  }
  *result = row;
  return RGB_OK;
}
}  // namespace seg
}  // namespace

extern "C" void rgb_seg_release(rgb_ctx *ctx) {      /* called by rgb_close */
  std::lock_guard<std::recursive_mutex> lk(seg::g_mu);
  seg::g_stages.erase(ctx);
}

extern "C" int rgb_crc32_device(rgb_ctx *ctx, const void *d_entries, uint32_t n, const void *d_data,
                                uint64_t data_bytes, void *d_crcs, void *stream) {
  if (!ctx || (n && (!d_entries || !d_crcs))) return RGB_E_INVAL;
  if (n == 0) return RGB_OK;
  hipStream_t st = stream ? (hipStream_t)stream : (hipStream_t)rgb_ctx_stream(ctx);
  (void)hipGetLastError();
  const seg::u32 width = seg::group_width(data_bytes / n);
  seg::with_width(width, [&](auto g) {
    hipLaunchKernelGGL((seg::rgb_seg_crc_kernel<decltype(g)::value, false>), dim3(seg::entry_grid(n, width)),
                       dim3(seg::THREADS), 0, st, (const rgb_seg_entry *)d_entries, n, (const unsigned char *)d_data,
                       data_bytes, (seg::u32 *)d_crcs, (unsigned char *)nullptr, (seg::u64)0, (const seg::u64 *)nullptr,
                       0u, 0u);
  });
  return hipGetLastError() == hipSuccess ? RGB_OK : RGB_E_HIP;
}

extern "C" int rgb_segment_build_device(rgb_ctx *ctx, const void *d_entries, uint32_t n, uint32_t max_count,
                                        const void *d_out_offsets, const void *d_data, uint64_t data_bytes,
                                        void *d_out, uint64_t out_bytes, uint32_t flags, void *stream) {
  if (!ctx || !d_out || (n && (!d_entries || !d_out_offsets)) || (flags & ~RGB_SEG_NO_CHECKSUMS)) return RGB_E_INVAL;
  if (n > max_count || max_count > 65535u) return RGB_E_INVAL;
  const uint64_t data_start = (uint64_t)RGB_SEG_HEADER_BYTES + (uint64_t)RGB_SEG_RECORD_BYTES * max_count;
  if (out_bytes < data_start) return RGB_E_INVAL;
  hipStream_t st = stream ? (hipStream_t)stream : (hipStream_t)rgb_ctx_stream(ctx);
  (void)hipGetLastError();
  /* the unused index records are zeros (the reference leaves a hole in a fresh file) */
  if (max_count > n &&
      hipMemsetAsync((unsigned char *)d_out + RGB_SEG_HEADER_BYTES + (uint64_t)RGB_SEG_RECORD_BYTES * n, 0,
                     (uint64_t)RGB_SEG_RECORD_BYTES * (max_count - n), st) != hipSuccess)
    return RGB_E_HIP;
  const seg::u32 width = seg::group_width(n ? data_bytes / n : 0);
  seg::with_width(width, [&](auto g) {
    hipLaunchKernelGGL((seg::rgb_seg_crc_kernel<decltype(g)::value, true>), dim3(seg::entry_grid(n, width)),
                       dim3(seg::THREADS), 0, st, (const rgb_seg_entry *)d_entries, n, (const unsigned char *)d_data,
                       data_bytes, (seg::u32 *)nullptr, (unsigned char *)d_out, (seg::u64)out_bytes,
                       (const seg::u64 *)d_out_offsets, max_count, flags);
  });
  return hipGetLastError() == hipSuccess ? RGB_OK : RGB_E_HIP;
}

extern "C" int rgb_crc32_stream_device(rgb_ctx *ctx, const void *d_data, uint64_t n_bytes, uint32_t init,
                                       void *d_crc, void *stream) {
  if (!ctx || !d_crc || (n_bytes && !d_data)) return RGB_E_INVAL;
  hipStream_t st = stream ? (hipStream_t)stream : (hipStream_t)rgb_ctx_stream(ctx);
  (void)hipGetLastError();
  if (n_bytes < 16u) {
    hipLaunchKernelGGL(seg::rgb_seg_combine_kernel, dim3(1), dim3(seg::THREADS), 0, st, (const seg::u32 *)nullptr, 0u,
                       0u, init, 0u, (seg::u32 *)d_crc, (const unsigned char *)d_data, (seg::u32)n_bytes);
    return hipGetLastError() == hipSuccess ? RGB_OK : RGB_E_HIP;
  }
  seg::u32 *partials = seg::partials_of(ctx);
  if (!partials) return RGB_E_NOMEM;
  /* a gigabyte per pair of launches; the pieces behind the first start from what *d_crc holds.  A last piece under
   * 16 bytes is avoided by leaving it 16 bytes of its predecessor. */
  const uint64_t piece_max = (uint64_t)seg::STREAM_MAX_BLOCKS * seg::STREAM_BLOCK;
  uint64_t done = 0;
  while (done < n_bytes) {
    uint64_t piece = n_bytes - done;
    if (piece > piece_max) piece = (piece - piece_max < 16u) ? piece_max - 16u : piece_max;
    const seg::u32 n_blocks = (seg::u32)((piece + seg::STREAM_BLOCK - 1u) / seg::STREAM_BLOCK);
    const seg::u32 grid = n_blocks < seg::GRID_CAP ? n_blocks : seg::GRID_CAP;
    hipLaunchKernelGGL(seg::rgb_seg_stream_kernel, dim3(grid), dim3(seg::THREADS), 0, st,
                       (const unsigned char *)d_data + done, (seg::u64)piece, n_blocks, partials);
    hipLaunchKernelGGL(seg::rgb_seg_combine_kernel, dim3(1), dim3(seg::THREADS), 0, st, (const seg::u32 *)partials,
                       n_blocks, seg::host_xpow8(piece), init, done ? 1u : 0u, (seg::u32 *)d_crc,
                       (const unsigned char *)nullptr, 0u);
    done += piece;
  }
  return hipGetLastError() == hipSuccess ? RGB_OK : RGB_E_HIP;
}

/* ---- host-buffer forms ---------------------------------------------------------------------------------- */

extern "C" int rgb_crc32(rgb_ctx *ctx, const rgb_seg_entry *entries, uint32_t n, const void *data,
                         uint64_t data_bytes, uint32_t *crcs) {
  if (!ctx || (n && (!entries || !crcs)) || (data_bytes && !data)) return RGB_E_INVAL;
  if (n == 0) return RGB_OK;
  if (!seg::slices_ok(entries, n, data_bytes)) return RGB_E_INVAL;
  if (hipSetDevice(rgb_ctx_device(ctx)) != hipSuccess) return RGB_E_HIP;
  std::lock_guard<std::recursive_mutex> lk(seg::g_mu);
  seg::stage &s = seg::g_stages[ctx];
  hipStream_t st = (hipStream_t)rgb_ctx_stream(ctx);
  if (s.crcs.reserve((size_t)n * 4u)) return RGB_E_NOMEM;
  int rc;
  if ((rc = seg::stage_in(s.entries, entries, (size_t)n * sizeof(rgb_seg_entry), st)) ||
      (rc = seg::stage_in(s.data, data, (size_t)data_bytes, st)))
    return rc;
  rc = rgb_crc32_device(ctx, s.entries.p, n, s.data.p, data_bytes, s.crcs.p, st);
  if (rc) return rc;
  return seg::fetch(crcs, s.crcs, (size_t)n * 4u, st);
}

extern "C" int rgb_crc32_stream(rgb_ctx *ctx, const void *data, uint64_t n_bytes, uint32_t init, uint32_t *crc_out) {
  if (!ctx || !crc_out || (n_bytes && !data)) return RGB_E_INVAL;
  if (hipSetDevice(rgb_ctx_device(ctx)) != hipSuccess) return RGB_E_HIP;
  std::lock_guard<std::recursive_mutex> lk(seg::g_mu);
  seg::u32 *partials = seg::partials_of(ctx);
  if (!partials) return RGB_E_NOMEM;
  seg::stage &s = seg::g_stages[ctx];
  hipStream_t st = (hipStream_t)rgb_ctx_stream(ctx);
  int rc = seg::stage_in(s.data, data, (size_t)n_bytes, st);
  if (rc) return rc;
  seg::u32 *d_crc = partials + seg::STREAM_MAX_BLOCKS;
  rc = rgb_crc32_stream_device(ctx, s.data.p, n_bytes, init, d_crc, st);
  if (rc) return rc;
  if (hipMemcpyAsync(crc_out, d_crc, 4u, hipMemcpyDeviceToHost, st) != hipSuccess) return RGB_E_HIP;
  return hipStreamSynchronize(st) == hipSuccess ? RGB_OK : RGB_E_HIP;
}

extern "C" int rgb_segment_build(rgb_ctx *ctx, const rgb_seg_entry *entries, uint32_t n, uint32_t max_count,
                                 const void *data, uint64_t data_bytes, void *out, uint64_t out_bytes, uint32_t flags) {
  if (!ctx || !out || (n && !entries) || (data_bytes && !data) || (flags & ~RGB_SEG_NO_CHECKSUMS)) return RGB_E_INVAL;
  if (n > max_count || max_count > 65535u) return RGB_E_INVAL;
  if (!seg::slices_ok(entries, n, data_bytes)) return RGB_E_INVAL;
  std::vector<uint64_t> offs(n ? n : 1);
  const uint64_t total = rgb_segment_layout(entries, n, max_count, offs.data());
  if (out_bytes < total) return RGB_E_INVAL;
  if (hipSetDevice(rgb_ctx_device(ctx)) != hipSuccess) return RGB_E_HIP;
  std::lock_guard<std::recursive_mutex> lk(seg::g_mu);
  seg::stage &s = seg::g_stages[ctx];
  hipStream_t st = (hipStream_t)rgb_ctx_stream(ctx);
  if (s.out.reserve((size_t)total)) return RGB_E_NOMEM;
  int rc;
  if ((rc = seg::stage_in(s.entries, entries, (size_t)n * sizeof(rgb_seg_entry), st)) ||
      (rc = seg::stage_in(s.offsets, offs.data(), (size_t)n * 8u, st)) ||
      (rc = seg::stage_in(s.data, data, (size_t)data_bytes, st)))
    return rc;
  rc = rgb_segment_build_device(ctx, s.entries.p, n, max_count, s.offsets.p, s.data.p, data_bytes, s.out.p, total, flags,
                                st);
  if (rc) return rc;
  /* only the file's own bytes come back: `out` behind them is the caller's */
  return seg::fetch(out, s.out, (size_t)total, st);
}

/* validate_checksum/2 (src/ra_log_segment.erl:1245-1248) over the records of a scanned file, in order */
extern "C" int rgb_segment_validate(rgb_ctx *ctx, const void *bytes, uint64_t n_bytes, const rgb_seg_entry *recs,
                                    uint32_t n, uint32_t *n_ok) {
  if (!ctx || !n_ok || (n && (!recs || !bytes))) return RGB_E_INVAL;
  *n_ok = n;
  if (n == 0) return RGB_OK;
  std::vector<uint32_t> sums(n);
  int rc = rgb_crc32(ctx, recs, n, bytes, n_bytes, sums.data());
  if (rc) return rc;
  for (uint32_t i = 0; i < n; ++i)
    if (recs[i].crc != 0u && recs[i].crc != sums[i]) { *n_ok = i; break; }
  return RGB_OK;
}

/* ---- major compaction: info/2 and copy/3 of a compaction group ------------------------------------------- */

extern "C" int rgb_seg_compact_check(const rgb_seg_source *sources, uint32_t n_sources, const uint64_t *live,
                                     uint32_t n_live, uint64_t files_bytes, int with_live, int limit_count,
                                     uint32_t *asked, uint32_t *rank, uint64_t *sum_bytes, uint32_t *max_count);

namespace {
namespace seg {
struct staged_call {
  const src_desc *d_srcs = nullptr;
  const u64 *d_live = nullptr;
  const u32 *d_rank = nullptr;
  src_done *d_done = nullptr;
  u64 *d_byte_base = nullptr;
  work_hdr *d_hdr = nullptr;
  plan_rec *d_plan = nullptr;
  u32 max_count = 0;
  u64 sum_bytes = 0;
};
inline size_t up16(size_t v) { return (v + 15u) & ~(size_t)15u; }

/* Validate the descriptors, put them (and the live list, and its ranks) behind each other in the context's pinned
 * buffer, upload that on `st`, size the scratch plan.  compact = false: the info form, no counts, no plan. */
int stage_call(stage &s, const rgb_seg_source *sources, u32 n_sources, const uint64_t *live, u32 n_live,
               uint64_t files_bytes, bool with_live, bool compact, hipStream_t st, staged_call *out) {
  const size_t off_live = (size_t)n_sources * sizeof(src_desc);
  const size_t off_rank = off_live + (size_t)n_live * 16u;
  const size_t need = up16(off_rank + (size_t)n_live * 4u) + 16u;
  pinned_upload &up = s.compact_desc;
  int rc = up.prepare(need);                            /* (the check leaves the ranks in the pinned block) */
  if (rc) return rc;
  unsigned char *h = (unsigned char *)up.h;
  src_desc *h_srcs = (src_desc *)h;
  u32 *h_rank = (u32 *)(h + off_rank);
  uint32_t asked[RGB_SEG_COMPACT_MAX_SOURCES];
  uint32_t max_count = 0;
  uint64_t sum = 0;
  rc = rgb_seg_compact_check(sources, n_sources, live, n_live, files_bytes, with_live ? 1 : 0, compact ? 1 : 0, asked,
                             h_rank, &sum, &max_count);
  if (rc) return rc;
  u32 plan_base = 0;
  for (u32 i = 0; i < n_sources; ++i) {
    src_desc d;
    d.offset = sources[i].offset; d.n_bytes = sources[i].n_bytes;
    d.live_first = with_live ? sources[i].live_first : 0u; d.live_n = with_live ? sources[i].live_n : 0u;
    d.asked = compact ? asked[i] : 0u; d.plan_base = plan_base;
    plan_base += d.asked;
    h_srcs[i] = d;
  }
  if (n_live && with_live) memcpy(h + off_live, live, (size_t)n_live * 16u);
  const size_t off_base = (size_t)n_sources * sizeof(src_done);
  const size_t off_hdr = up16(off_base + (size_t)n_sources * 8u);
  const size_t off_plan = off_hdr + sizeof(work_hdr);
  if (s.compact_work.reserve(off_plan + (size_t)max_count * sizeof(plan_rec) + 16u)) return RGB_E_NOMEM;
  if ((rc = up.upload(need, st))) return rc;
  unsigned char *d = (unsigned char *)up.d.p, *w = (unsigned char *)s.compact_work.p;
  out->d_srcs = (const src_desc *)d;
  out->d_live = (const u64 *)(d + off_live);
  out->d_rank = (const u32 *)(d + off_rank);
  out->d_done = (src_done *)w;
  out->d_byte_base = (u64 *)(w + off_base);
  out->d_hdr = (work_hdr *)(w + off_hdr);
  out->d_plan = (plan_rec *)(w + off_plan);
  out->max_count = max_count;
  out->sum_bytes = sum;
  return RGB_OK;
}

/* what the host-buffer forms answer RGB_E_INVAL to, where the device forms report RGB_SEG_COMPACT_BAD_SOURCE */
bool headers_ok(const rgb_seg_source *sources, u32 n_sources, const unsigned char *files) {
  for (u32 i = 0; i < n_sources; ++i) {
    const unsigned char *f = files + sources[i].offset;
    if (sources[i].n_bytes < RGB_SEG_HEADER_BYTES || f[0] != 'R' || f[1] != 'A' || f[2] != 'S' || f[3] != 'G') return false;
    const u32 version = ((u32)f[4] << 8) | f[5];
    if (version < 1u || version > RGB_SEG_VERSION) return false;
  }
  return true;
}
}  // namespace seg
}  // namespace

extern "C" int rgb_segment_info_device(rgb_ctx *ctx, const rgb_seg_source *sources, uint32_t n_sources, const void *d_files,
                                       uint64_t files_bytes, const uint64_t *live, uint32_t n_live, void *d_infos,
                                       void *stream) {
  if (!ctx || (n_sources && (!sources || !d_infos)) || (files_bytes && !d_files) || (n_live && !live)) return RGB_E_INVAL;
  if (n_sources > RGB_SEG_COMPACT_MAX_SOURCES) return RGB_E_INVAL;
  if (n_sources == 0) return RGB_OK;
  hipStream_t st = stream ? (hipStream_t)stream : (hipStream_t)rgb_ctx_stream(ctx);
  std::lock_guard<std::recursive_mutex> lk(seg::g_mu);
  seg::stage &s = seg::g_stages[ctx];
  seg::staged_call c;
  const bool with_live = live != nullptr;
  int rc = seg::stage_call(s, sources, n_sources, live, with_live ? n_live : 0u, files_bytes, with_live, false, st, &c);
  if (rc) return rc;
  (void)hipGetLastError();
  hipLaunchKernelGGL(seg::rgb_compact_resolve_kernel, dim3(n_sources), dim3(seg::THREADS), 0, st, c.d_srcs,
                     (const unsigned char *)d_files, c.d_live, (const seg::u32 *)nullptr, with_live ? 0u : 1u, d_infos,
                     (seg::src_done *)nullptr, (seg::plan_rec *)nullptr);
  return hipGetLastError() == hipSuccess ? RGB_OK : RGB_E_HIP;
}

extern "C" int rgb_segment_compact_device(rgb_ctx *ctx, const rgb_seg_source *sources, uint32_t n_sources,
                                          const void *d_files, uint64_t files_bytes, const uint64_t *live, uint32_t n_live,
                                          uint64_t max_size, uint32_t flags, void *d_out, uint64_t out_bytes,
                                          void *d_result, void *stream) {
  if (!ctx || !d_out || !d_result || (n_sources && !sources) || (files_bytes && !d_files) || (n_live && !live) ||
      (flags & ~RGB_SEG_COMPACT_VERIFY))
    return RGB_E_INVAL;
  if (n_sources > RGB_SEG_COMPACT_MAX_SOURCES) return RGB_E_INVAL;
  hipStream_t st = stream ? (hipStream_t)stream : (hipStream_t)rgb_ctx_stream(ctx);
  std::lock_guard<std::recursive_mutex> lk(seg::g_mu);
  seg::stage &s = seg::g_stages[ctx];
  seg::staged_call c;
  int rc = seg::stage_call(s, sources, n_sources, live, n_live, files_bytes, true, true, st, &c);
  if (rc) return rc;
  (void)hipGetLastError();
  if (n_sources)
    hipLaunchKernelGGL(seg::rgb_compact_resolve_kernel, dim3(n_sources), dim3(seg::THREADS), 0, st, c.d_srcs,
                       (const unsigned char *)d_files, c.d_live, c.d_rank, 0u, (void *)nullptr, c.d_done, c.d_plan);
  hipLaunchKernelGGL(seg::rgb_compact_place_kernel, dim3(1), dim3(64), 0, st, c.d_srcs, n_sources,
                     (const seg::src_done *)c.d_done, (const seg::plan_rec *)c.d_plan, c.max_count, (seg::u64)max_size,
                     (seg::u64)out_bytes, c.d_byte_base, c.d_hdr, d_result);
  /* (the mean over the sources' bytes, not the live payloads': those are not known here) */
  const uint32_t n = c.max_count;
  const seg::u32 width = seg::group_width(c.sum_bytes / (n ? n : 1u));
  const bool verify = (flags & RGB_SEG_COMPACT_VERIFY) != 0u;
  seg::with_width(width, [&](auto g) {
    constexpr int G = decltype(g)::value;
    auto *copy = verify ? seg::rgb_compact_copy_kernel<G, true> : seg::rgb_compact_copy_kernel<G, false>;
    hipLaunchKernelGGL(copy, dim3(seg::entry_grid(n, width)), dim3(seg::THREADS), 0, st, (const seg::plan_rec *)c.d_plan,
                       n, (const unsigned char *)d_files, (const seg::u64 *)c.d_byte_base, c.d_hdr,
                       (unsigned char *)d_out);
  });
  if (verify)
    hipLaunchKernelGGL(seg::rgb_compact_finish_kernel, dim3(1), dim3(64), 0, st, (const seg::plan_rec *)c.d_plan,
                       (const seg::work_hdr *)c.d_hdr, d_result);
  return hipGetLastError() == hipSuccess ? RGB_OK : RGB_E_HIP;
}

extern "C" int rgb_segment_info(rgb_ctx *ctx, const rgb_seg_source *sources, uint32_t n_sources, const void *files,
                                uint64_t files_bytes, const uint64_t *live, uint32_t n_live, rgb_seg_info *infos) {
  if (!ctx || (n_sources && (!sources || !infos)) || (files_bytes && !files) || (n_live && !live)) return RGB_E_INVAL;
  int rc = rgb_seg_compact_check(sources, n_sources, live, live ? n_live : 0u, files_bytes, live ? 1 : 0, 0, nullptr,
                                 nullptr, nullptr, nullptr);
  if (rc) return rc;
  if (!seg::headers_ok(sources, n_sources, (const unsigned char *)files)) return RGB_E_INVAL;
  if (n_sources == 0) return RGB_OK;
  if (hipSetDevice(rgb_ctx_device(ctx)) != hipSuccess) return RGB_E_HIP;
  std::lock_guard<std::recursive_mutex> lk(seg::g_mu);
  seg::stage &s = seg::g_stages[ctx];
  const size_t need_i = (size_t)n_sources * sizeof(rgb_seg_info);
  hipStream_t st = (hipStream_t)rgb_ctx_stream(ctx);
  if (s.result.reserve(need_i)) return RGB_E_NOMEM;
  if ((rc = seg::stage_in(s.data, files, (size_t)files_bytes, st))) return rc;
  rc = rgb_segment_info_device(ctx, sources, n_sources, s.data.p, files_bytes, live, n_live, s.result.p, st);
  if (rc) return rc;
  return seg::fetch(infos, s.result, need_i, st);
}

extern "C" int rgb_segment_compact(rgb_ctx *ctx, const rgb_seg_source *sources, uint32_t n_sources, const void *files,
                                   uint64_t files_bytes, const uint64_t *live, uint32_t n_live, uint64_t max_size,
                                   uint32_t flags, void *out, uint64_t out_bytes, rgb_seg_compact_result *result) {
  if (!ctx || !out || !result || (files_bytes && !files) || (flags & ~RGB_SEG_COMPACT_VERIFY)) return RGB_E_INVAL;
  uint64_t bound = 0;
  uint32_t max_count = 0;
  int rc = rgb_segment_compact_bound(sources, n_sources, live, n_live, files_bytes, &bound, &max_count);
  if (rc) return rc;
  if (!seg::headers_ok(sources, n_sources, (const unsigned char *)files)) return RGB_E_INVAL;
  if (hipSetDevice(rgb_ctx_device(ctx)) != hipSuccess) return RGB_E_HIP;
  std::lock_guard<std::recursive_mutex> lk(seg::g_mu);
  seg::stage &s = seg::g_stages[ctx];
  const uint64_t room = out_bytes < bound ? out_bytes : bound;         /* the image never needs more than the bound */
  hipStream_t st = (hipStream_t)rgb_ctx_stream(ctx);
  if (s.out.reserve((size_t)room + 16u) || s.result.reserve(sizeof(rgb_seg_compact_result))) return RGB_E_NOMEM;
  if ((rc = seg::stage_in(s.data, files, (size_t)files_bytes, st))) return rc;
  rc = rgb_segment_compact_device(ctx, sources, n_sources, s.data.p, files_bytes, live, n_live, max_size, flags, s.out.p,
                                  room, s.result.p, st);
  if (rc) return rc;
  /* only the image's own bytes come back, and only a good image */
  return seg::fetch_result(result, s.result, RGB_SEG_COMPACT_OK, st, [&](const rgb_seg_compact_result &res) {
    return seg::copy_down(out, s.out, (size_t)res.file_bytes, st);
  });
}

/* ---- major compaction for many members: any number of groups in one call ---------------------------------- */

extern "C" int rgb_seg_compact_groups_check(const rgb_seg_group *groups, uint32_t n_groups, const rgb_seg_source *sources,
                                            uint32_t n_sources, const uint64_t *live, uint32_t n_live, uint64_t files_bytes,
                                            int with_out, uint64_t out_bytes, uint32_t *order, uint32_t *asked,
                                            uint32_t *group_of_src, uint32_t *rank, uint32_t *max_counts,
                                            uint64_t *sum_bytes, uint64_t *total_count);

extern "C" int rgb_segment_compact_groups_device(rgb_ctx *ctx, const rgb_seg_group *groups, uint32_t n_groups,
                                                 const rgb_seg_source *sources, uint32_t n_sources, const void *d_files,
                                                 uint64_t files_bytes, const uint64_t *live, uint32_t n_live,
                                                 uint64_t max_size, uint32_t flags, void *d_out, uint64_t out_bytes,
                                                 void *d_results, void *stream) {
  if (!ctx || (n_groups && (!groups || !d_out || !d_results)) || (n_sources && !sources) || (files_bytes && !d_files) ||
      (n_live && !live) || (flags & ~RGB_SEG_COMPACT_VERIFY))
    return RGB_E_INVAL;
  hipStream_t st = stream ? (hipStream_t)stream : (hipStream_t)rgb_ctx_stream(ctx);
  std::lock_guard<std::recursive_mutex> lk(seg::g_mu);
  seg::stage &s = seg::g_stages[ctx];
  /* the pinned block: what goes up (sources, groups, live list, ranks), and behind it the host's own tables */
  const size_t off_grps = (size_t)n_sources * sizeof(seg::src_desc);
  const size_t off_live = off_grps + (size_t)n_groups * sizeof(seg::grp_desc);
  const size_t off_rank = off_live + (size_t)n_live * 16u;
  const size_t need = seg::up16(off_rank + (size_t)n_live * 4u) + 16u;
  const size_t off_asked = need, off_order = off_asked + (size_t)n_sources * 4u, off_counts = off_order + (size_t)n_groups * 4u;
  seg::pinned_upload &up = s.compact_desc;
  int rc = up.prepare(off_counts + (size_t)n_groups * 4u + 16u);
  if (rc) return rc;
  unsigned char *h = (unsigned char *)up.h;
  seg::src_desc *h_srcs = (seg::src_desc *)h;
  seg::grp_desc *h_grps = (seg::grp_desc *)(h + off_grps);
  uint32_t *h_asked = (uint32_t *)(h + off_asked), *h_counts = (uint32_t *)(h + off_counts);
  uint64_t sum = 0, total = 0;
  rc = rgb_seg_compact_groups_check(groups, n_groups, sources, n_sources, live, n_live, files_bytes, 1, out_bytes,
                                    (uint32_t *)(h + off_order), h_asked, nullptr, (uint32_t *)(h + off_rank), h_counts,
                                    &sum, &total);
  if (rc) return rc;
  if (n_groups == 0) return RGB_OK;
  seg::u32 plan_base = 0;
  for (seg::u32 i = 0; i < n_sources; ++i) {            /* (a source no group names asks for nothing) */
    seg::src_desc d;
    d.offset = sources[i].offset; d.n_bytes = sources[i].n_bytes;
    d.live_first = sources[i].live_first; d.live_n = sources[i].live_n;
    d.asked = h_asked[i]; d.plan_base = plan_base;
    if (!d.asked) { d.live_first = 0u; d.live_n = 0u; }
    plan_base += d.asked;
    h_srcs[i] = d;
  }
  for (seg::u32 g = 0; g < n_groups; ++g) {
    seg::grp_desc d;
    d.out_offset = groups[g].out_offset; d.out_bytes = groups[g].out_bytes;
    d.src_first = groups[g].src_first; d.src_n = groups[g].src_n;
    d.plan_first = 0u; d.max_count = h_counts[g];
    h_grps[g] = d;
  }
  /* a group's first plan entry: that of its first source; without sources, its successor's (the end for the last) */
  for (seg::u32 g = n_groups, behind = (seg::u32)total; g-- > 0u;) {
    if (h_grps[g].src_n) behind = h_srcs[h_grps[g].src_first].plan_base;
    h_grps[g].plan_first = behind;
  }
  if (n_live) memcpy(h + off_live, live, (size_t)n_live * 16u);
  const size_t off_base = (size_t)n_sources * sizeof(seg::src_done);
  const size_t off_hdr = seg::up16(off_base + (size_t)n_sources * 8u);
  const size_t off_plan = off_hdr + (size_t)n_groups * sizeof(seg::work_hdr);
  if (s.compact_work.reserve(off_plan + (size_t)total * sizeof(seg::plan_rec) + 16u)) return RGB_E_NOMEM;
  if ((rc = up.upload(need, st))) return rc;
  unsigned char *d = (unsigned char *)up.d.p, *w = (unsigned char *)s.compact_work.p;
  const seg::src_desc *d_srcs = (const seg::src_desc *)d;
  const seg::grp_desc *d_grps = (const seg::grp_desc *)(d + off_grps);
  const seg::plan_rec *d_plan = (const seg::plan_rec *)(w + off_plan);
  seg::u64 *d_base = (seg::u64 *)(w + off_base);
  seg::work_hdr *d_hdrs = (seg::work_hdr *)(w + off_hdr);
  (void)hipGetLastError();
  if (n_sources)
    hipLaunchKernelGGL(seg::rgb_compact_resolve_kernel, dim3(n_sources), dim3(seg::THREADS), 0, st, d_srcs,
                       (const unsigned char *)d_files, (const seg::u64 *)(d + off_live), (const seg::u32 *)(d + off_rank),
                       0u, (void *)nullptr, (seg::src_done *)w, (seg::plan_rec *)(w + off_plan));
  const seg::u32 grp_grid = (n_groups + seg::GRP_LANES - 1u) / seg::GRP_LANES;
  hipLaunchKernelGGL(seg::rgb_cgroups_place_kernel, dim3(grp_grid), dim3(seg::GRP_LANES), 0, st, d_grps, n_groups, d_srcs,
                     (const seg::src_done *)w, d_plan, (seg::u64)max_size, d_base, d_hdrs, (unsigned char *)d_out,
                     d_results);
  const seg::u32 n = (seg::u32)total;
  if (n == 0u) return hipGetLastError() == hipSuccess ? RGB_OK : RGB_E_HIP;     /* header-only images: place wrote them */
  /* (the mean over the sources' bytes, as the single-group call) */
  const seg::u32 width = seg::group_width(sum / n);
  const bool verify = (flags & RGB_SEG_COMPACT_VERIFY) != 0u;
  seg::with_width(width, [&](auto gw) {
    constexpr int G = decltype(gw)::value;
    auto *copy = verify ? seg::rgb_cgroups_copy_kernel<G, true> : seg::rgb_cgroups_copy_kernel<G, false>;
    hipLaunchKernelGGL(copy, dim3(seg::entry_grid(n, width)), dim3(seg::THREADS), 0, st, d_plan, n, d_grps, n_groups,
                       (const unsigned char *)d_files, (const seg::u64 *)d_base, d_hdrs, (unsigned char *)d_out);
  });
  if (verify)
    hipLaunchKernelGGL(seg::rgb_cgroups_finish_kernel, dim3(grp_grid), dim3(seg::GRP_LANES), 0, st, d_grps, n_groups,
                       d_plan, (const seg::work_hdr *)d_hdrs, d_results);
  return hipGetLastError() == hipSuccess ? RGB_OK : RGB_E_HIP;
}

extern "C" int rgb_segment_compact_groups(rgb_ctx *ctx, const rgb_seg_group *groups, uint32_t n_groups,
                                          const rgb_seg_source *sources, uint32_t n_sources, const void *files,
                                          uint64_t files_bytes, const uint64_t *live, uint32_t n_live, uint64_t max_size,
                                          uint32_t flags, void *out, uint64_t out_bytes, rgb_seg_compact_result *results) {
  if (!ctx || (n_groups && (!groups || !out || !results)) || (files_bytes && !files) ||
      (flags & ~RGB_SEG_COMPACT_VERIFY))
    return RGB_E_INVAL;
  /* the device's copy of `out` ends with the last image: the room behind it is the caller's alone */
  uint64_t room = 0;
  for (uint32_t g = 0; g < n_groups; ++g) {
    if (groups[g].out_offset > out_bytes || groups[g].out_bytes > out_bytes - groups[g].out_offset) return RGB_E_INVAL;
    if (groups[g].out_offset + groups[g].out_bytes > room) room = groups[g].out_offset + groups[g].out_bytes;
  }
  std::vector<uint32_t> order(n_groups ? n_groups : 1u);
  int rc = rgb_seg_compact_groups_check(groups, n_groups, sources, n_sources, live, n_live, files_bytes, 1, out_bytes,
                                        order.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
  if (rc) return rc;
  if (n_groups == 0) return RGB_OK;
  if (hipSetDevice(rgb_ctx_device(ctx)) != hipSuccess) return RGB_E_HIP;
  std::lock_guard<std::recursive_mutex> lk(seg::g_mu);
  seg::stage &s = seg::g_stages[ctx];
  hipStream_t st = (hipStream_t)rgb_ctx_stream(ctx);
  const size_t rows = (size_t)n_groups * sizeof(rgb_seg_compact_result);
  if (s.out.reserve((size_t)room + 16u) || s.result.reserve(rows)) return RGB_E_NOMEM;
  if ((rc = seg::stage_in(s.data, files, (size_t)files_bytes, st))) return rc;
  rc = rgb_segment_compact_groups_device(ctx, groups, n_groups, sources, n_sources, s.data.p, files_bytes, live, n_live,
                                         max_size, flags, s.out.p, room, s.result.p, st);
  if (rc) return rc;
  std::vector<rgb_seg_compact_result> got(n_groups);
  if ((rc = seg::fetch(got.data(), s.result, rows, st))) return rc;
  /* only the good images' own bytes come back; neighbours that touch travel in one piece */
  uint64_t run_first = 0, run_end = 0;
  auto flush = [&]() -> int {
    if (run_end == run_first) return RGB_OK;
    return hipMemcpyAsync((unsigned char *)out + run_first, (const unsigned char *)s.out.p + run_first,
                          (size_t)(run_end - run_first), hipMemcpyDeviceToHost, st) == hipSuccess ? RGB_OK : RGB_E_HIP;
  };
  for (uint32_t g = 0; g < n_groups; ++g) {
    if (got[g].status != RGB_SEG_COMPACT_OK) continue;
    const uint64_t first = groups[g].out_offset, end = first + got[g].file_bytes;
    if (first != run_end || run_end == run_first) {
      if ((rc = flush())) return rc;
      run_first = first;
    }
    run_end = end;
  }
  if ((rc = flush())) return rc;
  if (hipStreamSynchronize(st) != hipSuccess) return RGB_E_HIP;
  memcpy(results, got.data(), rows);
  return RGB_OK;
}

/* ---- mem-table flush: the entries of many writers into their segment files ------------------------------ */

extern "C" int rgb_seg_flush_check(const rgb_seg_writer *writers, uint32_t n_writers, uint32_t n_entries,
                                   uint32_t *covered, uint32_t *longest);

extern "C" int rgb_segment_flush_device(rgb_ctx *ctx, const rgb_seg_writer *writers, uint32_t n_writers,
                                        const void *d_entries, uint32_t n_entries, const void *d_data, uint64_t data_bytes,
                                        uint32_t max_count, uint64_t max_size, uint32_t flags, void *d_pieces,
                                        uint32_t pieces_cap, void *d_out, uint64_t out_bytes, void *d_result, void *stream) {
  if (!ctx || !d_result || (n_writers && !writers) || (n_entries && !d_entries) || (data_bytes && !d_data) ||
      (pieces_cap && !d_pieces) || (out_bytes && !d_out) || (flags & ~RGB_SEG_NO_CHECKSUMS))
    return RGB_E_INVAL;
  if (max_count < 1u || max_count > 65535u) return RGB_E_INVAL;
  uint32_t covered = 0, longest = 0;
  int rc = rgb_seg_flush_check(writers, n_writers, n_entries, &covered, &longest);
  if (rc) return rc;
  hipStream_t st = stream ? (hipStream_t)stream : (hipStream_t)rgb_ctx_stream(ctx);
  std::lock_guard<std::recursive_mutex> lk(seg::g_mu);
  seg::stage &s = seg::g_stages[ctx];
  /* the sub-group of the plan, by the longest writer; every workgroup a whole number of steps of it */
  const seg::u32 plan_width = longest <= 8u ? 8u : longest <= 16u ? 16u : (seg::u32)seg::FL_CHUNK;
  const seg::u32 subs = seg::THREADS / plan_width;
  seg::u32 grid = (n_writers + subs - 1u) / subs;
  if (grid > seg::FL_GRID_CAP) grid = seg::FL_GRID_CAP;
  if (grid == 0u) grid = 1u;
  seg::u32 per_block = (n_writers + grid - 1u) / grid;
  per_block = (per_block + subs - 1u) / subs * subs;
  if (per_block == 0u) per_block = subs;
  const seg::u32 n_blocks = (n_writers + per_block - 1u) / per_block;      /* 0 without writers */
  /* the writers, through the context's pinned buffer */
  const size_t need = (size_t)n_writers * sizeof(seg::fl_writer) + 16u;
  seg::pinned_upload &up = s.flush_writers;
  if ((rc = up.prepare(need))) return rc;
  if (n_writers) memcpy(up.h, writers, (size_t)n_writers * sizeof(seg::fl_writer));
  /* the scratch: a row per writer, the sums of the plan's workgroups, the status, a plan record and a piece per entry */
  const size_t off_tot = (size_t)n_writers * sizeof(seg::fl_row);
  const size_t off_hdr = off_tot + (size_t)seg::FL_GRID_CAP * sizeof(seg::fl_total);
  const size_t off_plan = off_hdr + sizeof(seg::work_hdr);
  const size_t off_pieces = off_plan + (size_t)n_entries * sizeof(seg::fl_plan);
  const size_t work = off_pieces + (size_t)n_entries * sizeof(seg::fl_piece) + 16u;
  if (s.flush_work.reserve(work)) return RGB_E_NOMEM;
  if ((rc = up.upload(need, st))) return rc;
  unsigned char *w = (unsigned char *)s.flush_work.p;
  const seg::fl_writer *d_writers = (const seg::fl_writer *)up.d.p;
  seg::fl_row *d_rows = (seg::fl_row *)w;
  seg::fl_total *d_totals = (seg::fl_total *)(w + off_tot);
  seg::work_hdr *d_hdr = (seg::work_hdr *)(w + off_hdr);
  seg::fl_plan *d_plan = (seg::fl_plan *)(w + off_plan);
  seg::fl_piece *d_pc = (seg::fl_piece *)(w + off_pieces);
  /* entries that no writer names keep writer = NONE32 in their plan record: the copy passes them by */
  if (covered != n_entries &&
      hipMemsetAsync(d_plan, 0xFF, (size_t)n_entries * sizeof(seg::fl_plan), st) != hipSuccess)
    return RGB_E_HIP;
  (void)hipGetLastError();
  if (n_blocks)
    seg::with_width(plan_width, [&](auto g) {
      hipLaunchKernelGGL((seg::rgb_flush_plan_kernel<decltype(g)::value>), dim3(n_blocks), dim3(seg::THREADS), 0, st,
                         d_writers, n_writers, per_block, (const seg::fl_entry *)d_entries, (seg::u64)data_bytes,
                         max_count, (seg::u64)max_size, d_rows, d_plan, d_pc, d_totals);
    });
  hipLaunchKernelGGL(seg::rgb_flush_place_kernel, dim3(n_blocks ? n_blocks : 1u), dim3(seg::THREADS), 0, st, d_writers,
                     n_writers, per_block, n_blocks, (const seg::fl_total *)d_totals, d_rows, d_plan,
                     (const seg::fl_piece *)d_pc, max_count, pieces_cap, (seg::u64)out_bytes, d_hdr, d_pieces,
                     (unsigned char *)d_out, d_result);
  if (n_entries && n_writers) {
    const seg::u32 width = seg::group_width(data_bytes / n_entries);
    seg::with_width(width, [&](auto g) {
      hipLaunchKernelGGL((seg::rgb_flush_copy_kernel<decltype(g)::value>), dim3(seg::entry_grid(n_entries, width)),
                         dim3(seg::THREADS), 0, st, (const seg::fl_entry *)d_entries, n_entries,
                         (const unsigned char *)d_data, (const seg::fl_place *)d_plan, (const seg::work_hdr *)d_hdr, flags,
                         (unsigned char *)d_out);
    });
  }
  return hipGetLastError() == hipSuccess ? RGB_OK : RGB_E_HIP;
}

extern "C" int rgb_segment_flush(rgb_ctx *ctx, const rgb_seg_writer *writers, uint32_t n_writers,
                                 const rgb_seg_entry *entries, uint32_t n_entries, const void *data, uint64_t data_bytes,
                                 uint32_t max_count, uint64_t max_size, uint32_t flags, rgb_seg_piece *pieces,
                                 uint32_t pieces_cap, void *out, uint64_t out_bytes, rgb_seg_flush_result *result) {
  if (!ctx || !result || (n_entries && !entries) || (data_bytes && !data) || (pieces_cap && !pieces) ||
      (out_bytes && !out) || (flags & ~RGB_SEG_NO_CHECKSUMS))
    return RGB_E_INVAL;
  if (max_count < 1u || max_count > 65535u) return RGB_E_INVAL;
  uint64_t bound = 0;
  uint32_t pieces_bound = 0;
  int rc = rgb_segment_flush_bound(writers, n_writers, n_entries, data_bytes, &bound, &pieces_bound);
  if (rc) return rc;
  for (uint32_t w = 0; w < n_writers; ++w)
    if (!seg::slices_ok(entries + writers[w].entry_first, writers[w].entry_n, data_bytes)) return RGB_E_INVAL;
  if (hipSetDevice(rgb_ctx_device(ctx)) != hipSuccess) return RGB_E_HIP;
  std::lock_guard<std::recursive_mutex> lk(seg::g_mu);
  seg::stage &s = seg::g_stages[ctx];
  const uint64_t room = out_bytes < bound ? out_bytes : bound;             /* the call never needs more than the bounds */
  const uint32_t rows = pieces_cap < pieces_bound ? pieces_cap : pieces_bound;
  hipStream_t st = (hipStream_t)rgb_ctx_stream(ctx);
  if (s.out.reserve((size_t)room + 16u) || s.pieces.reserve((size_t)rows * sizeof(rgb_seg_piece) + 16u) ||
      s.result.reserve(sizeof(rgb_seg_flush_result)))
    return RGB_E_NOMEM;
  if ((rc = seg::stage_in(s.entries, entries, (size_t)n_entries * sizeof(rgb_seg_entry), st)) ||
      (rc = seg::stage_in(s.data, data, (size_t)data_bytes, st)))
    return rc;
  rc = rgb_segment_flush_device(ctx, writers, n_writers, s.entries.p, n_entries, s.data.p, data_bytes, max_count, max_size,
                                flags, s.pieces.p, rows, s.out.p, room, s.result.p, st);
  if (rc) return rc;
  /* only the rows and bytes of the answer come back, and only a good answer */
  return seg::fetch_result(result, s.result, RGB_SEG_FLUSH_OK, st, [&](const rgb_seg_flush_result &res) {
    const int rc_rows = seg::copy_down(pieces, s.pieces, (size_t)res.n_pieces * sizeof(rgb_seg_piece), st);
    return rc_rows ? rc_rows : seg::copy_down(out, s.out, (size_t)res.out_bytes, st);
  });
}

/* ---- reading entries back: read plans, folds and term queries over many segment files ------------------- */

extern "C" int rgb_seg_read_check(const rgb_seg_read_source *sources, uint32_t n_sources, uint64_t files_bytes,
                                  uint32_t n_req, uint32_t flags, uint32_t *covered, uint64_t *sum_bytes,
                                  uint64_t *out_bound);

extern "C" int rgb_segment_read_device(rgb_ctx *ctx, const rgb_seg_read_source *sources, uint32_t n_sources,
                                       const void *d_files, uint64_t files_bytes, const uint64_t *req, uint32_t n_req,
                                       uint32_t flags, void *d_rows, void *d_out, uint64_t out_bytes, void *d_results,
                                       void *d_total, void *stream) {
  if (!ctx || !d_total || (n_sources && (!sources || !d_results)) || (files_bytes && !d_files) || (n_req && !req) ||
      (out_bytes && !d_out))
    return RGB_E_INVAL;
  uint32_t covered = 0;
  uint64_t sum_bytes = 0;
  int rc = rgb_seg_read_check(sources, n_sources, files_bytes, n_req, flags, &covered, &sum_bytes, nullptr);
  if (rc) return rc;
  if (covered && !d_rows) return RGB_E_INVAL;
  const bool no_data = (flags & RGB_SEG_READ_NO_DATA) != 0u, verify = (flags & RGB_SEG_READ_VERIFY) != 0u;
  hipStream_t st = stream ? (hipStream_t)stream : (hipStream_t)rgb_ctx_stream(ctx);
  std::lock_guard<std::recursive_mutex> lk(seg::g_mu);
  seg::stage &s = seg::g_stages[ctx];
  /* the sources and the requests, through the context's pinned buffer */
  const size_t off_req = (size_t)n_sources * sizeof(seg::rd_src);
  const size_t need = off_req + (size_t)n_req * 8u + 16u;
  seg::pinned_upload &up = s.read_desc;
  if ((rc = up.prepare(need))) return rc;
  seg::rd_src *h_srcs = (seg::rd_src *)up.h;
  uint64_t tab_total = 0;                               /* a source walks at most (n_bytes - 8) / 28 records */
  for (uint32_t i = 0; i < n_sources; ++i) {
    seg::rd_src d;
    d.offset = sources[i].offset; d.n_bytes = sources[i].n_bytes;
    d.req_first = sources[i].req_first; d.req_n = sources[i].req_n; d.tab_base = tab_total;
    h_srcs[i] = d;
    const uint64_t fit = d.n_bytes < RGB_SEG_HEADER_BYTES ? 0u : (d.n_bytes - RGB_SEG_HEADER_BYTES) / RGB_SEG_RECORD_BYTES_V1;
    tab_total += fit < 65535u ? fit : 65535u;
  }
  if (n_req) memcpy((unsigned char *)up.h + off_req, req, (size_t)n_req * 8u);
  /* the scratch: what resolve leaves per source, the sources' first bytes and first mismatches, the status, a plan
   * record per request, the tables of effective records */
  const size_t off_base = (size_t)n_sources * sizeof(seg::rd_done);
  const size_t off_crc = off_base + (size_t)n_sources * 8u;
  const size_t off_hdr = seg::up16(off_crc + (size_t)n_sources * 4u);
  const size_t off_plan = off_hdr + sizeof(seg::work_hdr);
  const size_t off_tab = off_plan + (no_data ? 0u : (size_t)n_req * sizeof(seg::rd_plan));
  if (s.read_work.reserve(off_tab + (size_t)tab_total * 4u + 16u)) return RGB_E_NOMEM;
  if ((rc = up.upload(need, st))) return rc;
  unsigned char *w = (unsigned char *)s.read_work.p;
  const seg::rd_src *d_srcs = (const seg::rd_src *)up.d.p;
  const seg::u64 *d_req = (const seg::u64 *)((unsigned char *)up.d.p + off_req);
  seg::rd_done *d_done = (seg::rd_done *)w;
  seg::u64 *d_base = (seg::u64 *)(w + off_base);
  seg::u32 *d_crc_k = (seg::u32 *)(w + off_crc);
  seg::work_hdr *d_hdr = (seg::work_hdr *)(w + off_hdr);
  seg::rd_plan *d_plan = (seg::rd_plan *)(w + off_plan);
  seg::u32 *d_tab = (seg::u32 *)(w + off_tab);
  /* requests that no slice names keep src = NONE32 in their plan record: the copy passes them by */
  if (!no_data && covered != n_req &&
      hipMemsetAsync(d_plan, 0xFF, (size_t)n_req * sizeof(seg::rd_plan), st) != hipSuccess)
    return RGB_E_HIP;
  (void)hipGetLastError();
  if (n_sources)
    hipLaunchKernelGGL(seg::rgb_read_resolve_kernel, dim3(n_sources), dim3(seg::THREADS), 0, st, d_srcs,
                       (const unsigned char *)d_files, d_req, no_data ? 1u : 0u, d_tab, d_rows, d_plan, d_done);
  hipLaunchKernelGGL(seg::rgb_read_place_kernel, dim3(1), dim3(seg::THREADS), 0, st, d_srcs, n_sources,
                     (const seg::rd_done *)d_done, (seg::u64)out_bytes, d_base, d_crc_k, d_hdr, d_results, d_total);
  if (no_data || !covered) return hipGetLastError() == hipSuccess ? RGB_OK : RGB_E_HIP;
  const seg::u32 width = seg::group_width(sum_bytes / (n_req ? n_req : 1u));
  seg::with_width(width, [&](auto g) {
    constexpr int G = decltype(g)::value;
    auto *copy = verify ? seg::rgb_read_copy_kernel<G, true> : seg::rgb_read_copy_kernel<G, false>;
    hipLaunchKernelGGL(copy, dim3(seg::entry_grid(n_req, width)), dim3(seg::THREADS), 0, st, (const seg::rd_plan *)d_plan,
                       n_req, (const unsigned char *)d_files, (const seg::u64 *)d_base, (const seg::work_hdr *)d_hdr,
                       d_crc_k, d_rows, (unsigned char *)d_out);
  });
  if (verify)
    hipLaunchKernelGGL(seg::rgb_read_finish_kernel, dim3(1), dim3(seg::THREADS), 0, st, d_srcs, n_sources, d_req,
                       (const seg::u32 *)d_crc_k, (const seg::work_hdr *)d_hdr, d_results, d_total);
  return hipGetLastError() == hipSuccess ? RGB_OK : RGB_E_HIP;
}

extern "C" int rgb_segment_read(rgb_ctx *ctx, const rgb_seg_read_source *sources, uint32_t n_sources, const void *files,
                                uint64_t files_bytes, const uint64_t *req, uint32_t n_req, uint32_t flags,
                                rgb_seg_entry *rows, void *out, uint64_t out_bytes, rgb_seg_read_result *results,
                                rgb_seg_read_total *total) {
  if (!ctx || !total || (n_sources && (!sources || !results)) || (files_bytes && !files) || (n_req && !req) ||
      (out_bytes && !out))
    return RGB_E_INVAL;
  uint32_t covered = 0;
  uint64_t bound = 0;
  int rc = rgb_seg_read_check(sources, n_sources, files_bytes, n_req, flags, &covered, nullptr, &bound);
  if (rc) return rc;
  if (covered && !rows) return RGB_E_INVAL;
  if (hipSetDevice(rgb_ctx_device(ctx)) != hipSuccess) return RGB_E_HIP;
  std::lock_guard<std::recursive_mutex> lk(seg::g_mu);
  seg::stage &s = seg::g_stages[ctx];
  const uint64_t room = out_bytes < bound ? out_bytes : bound;             /* the call never needs more than the bound */
  const size_t res_bytes = (size_t)n_sources * sizeof(rgb_seg_read_result), off_total = seg::up16(res_bytes);
  hipStream_t st = (hipStream_t)rgb_ctx_stream(ctx);
  if (s.out.reserve((size_t)room + 16u) || s.entries.reserve((size_t)n_req * sizeof(rgb_seg_entry) + 16u) ||
      s.result.reserve(off_total + sizeof(rgb_seg_read_total)))
    return RGB_E_NOMEM;
  if ((rc = seg::stage_in(s.data, files, (size_t)files_bytes, st))) return rc;
  unsigned char *d_res = (unsigned char *)s.result.p;
  rc = rgb_segment_read_device(ctx, sources, n_sources, s.data.p, files_bytes, req, n_req, flags, s.entries.p,
                               room ? s.out.p : nullptr, room, d_res, d_res + off_total, st);
  if (rc) return rc;
  rgb_seg_read_total t;
  if (hipMemcpyAsync(&t, d_res + off_total, sizeof t, hipMemcpyDeviceToHost, st) != hipSuccess) return RGB_E_HIP;
  if ((rc = seg::fetch(results, s.result, res_bytes, st))) return rc;
  /* only the rows that slices name come back (neighbouring slices in one copy), and only the bytes of a good answer */
  for (uint32_t i = 0; i < n_sources;) {
    const uint32_t first = sources[i].req_first;
    uint32_t end = first + sources[i].req_n;
    for (++i; i < n_sources && sources[i].req_first == end; ++i) end += sources[i].req_n;
    if (end > first && hipMemcpyAsync(rows + first, (const rgb_seg_entry *)s.entries.p + first,
                                      (size_t)(end - first) * sizeof(rgb_seg_entry), hipMemcpyDeviceToHost,
                                      st) != hipSuccess)
      return RGB_E_HIP;
  }
  if (t.status == RGB_SEG_READ_OK && (rc = seg::copy_down(out, s.out, (size_t)t.out_bytes, st))) return rc;
  if (hipStreamSynchronize(st) != hipSuccess) return RGB_E_HIP;
  *total = t;
  return RGB_OK;
}

/* ---- snapshots and checkpoints: ragged CRC batches, images, validation ---------------------------------- */

extern "C" int rgb_snapshot_spans_check(const rgb_crc_span *spans, uint32_t n, uint64_t data_bytes, uint64_t *sum_bytes);
extern "C" int rgb_snapshot_build_check(const rgb_snap_item *items, uint32_t n, uint64_t data_bytes, uint64_t out_bytes,
                                        uint64_t *sum_bytes);
extern "C" int rgb_snapshot_files_check(const rgb_snap_file *files, uint32_t n, uint64_t files_bytes, uint64_t *sum_bytes);

namespace {
namespace seg {

/* the pass that takes a piece: 8, 16 or 64 lanes, or blocks */
inline int snap_tier(u64 len) { return len <= SNAP_T8 ? 0 : len < SNAP_T16 ? 1 : len < SNAP_TBLOCK ? 2 : 3; }

/* erlang:crc32(<<V:32>>) before its final xor: raw(<<V:32>> xor 0xFFFFFFFF), the head of an image's stream */
inline u32 snap_head_of_be32(u32 v) {
  u32 crc = 0xFFFFFFFFu;
  for (int k = 3; k >= 0; --k) {
    crc ^= (v >> (8 * k)) & 0xFFu;
    for (int b = 0; b < 8; ++b) crc = (crc & 1u) ? (crc >> 1) ^ POLY : crc >> 1;
  }
  return crc;
}

/* The plan of one call, built on the host (in the context's vectors), sorted by pass into the pinned block and sent up:
 *   [ pieces: 8 lanes | 16 | 64 | blocks ] [ blk_start: a value per long piece, and the total ] [ items ] [ big ] */
struct snap_plan {
  stage &s;
  u64 slots = 0, blocks = 0;                            /* raw values / blocks the call leaves */
  u32 count[4] = {0u, 0u, 0u, 0u};
  bool too_large = false;
  explicit snap_plan(stage &st) : s(st) { s.snap_pieces.clear(); s.snap_items.clear(); s.snap_big.clear(); }

  /* one piece -> the raw values it leaves, from *slot on; `direct`: SNAP_DIRECT | the span a group piece answers */
  u32 piece(u64 src, u64 len, u64 dst, u32 fold, u32 direct, u32 *slot) {
    const int t = snap_tier(len);
    snap_piece p;
    p.src = src; p.len = len; p.dst = dst; p.fold = fold; p.slot = direct;
    u64 n_raw = 1;
    if (!direct) {
      if (t == 3) { n_raw = (len + SNAP_BLOCK - 1u) / SNAP_BLOCK; blocks += n_raw; }
      if (n_raw > 0x7FFFFFFFull || slots + n_raw > 0x7FFFFFFFull) { too_large = true; n_raw = 1; }
      p.slot = (u32)slots;
      slots += n_raw;
    }
    if (slot) *slot = p.slot;
    count[t] += 1u;
    s.snap_pieces.push_back(p);
    return (u32)n_raw;
  }
  /* item `it` (off and kind are the caller's) checksums A ++ B behind `head`: the head goes into the stream's first
   * piece when that is a group piece, and stays with the item otherwise */
  void stream(snap_item it, u64 a_src, u64 a_len, u64 a_dst, u64 b_src, u64 b_len, u64 b_dst, u32 head) {
    it.len_a = a_len; it.len_b = b_len; it.head = head;
    it.slot_a = it.slot_b = it.nblk_a = it.nblk_b = 0u;
    if (a_len) {
      const bool folds = snap_tier(a_len) < 3;
      it.nblk_a = piece(a_src, a_len, a_dst, folds ? head : 0u, 0u, &it.slot_a);
      if (folds) it.head = 0u;
    }
    if (b_len) {
      const bool folds = !a_len && snap_tier(b_len) < 3;
      it.nblk_b = piece(b_src, b_len, b_dst, folds ? head : 0u, 0u, &it.slot_b);
      if (folds) it.head = 0u;
    }
    if (it.nblk_a > 1u || it.nblk_b > 1u) s.snap_big.push_back((u32)s.snap_items.size());
    s.snap_items.push_back(it);
  }

  /* Upload and run: the group and block passes, then finish<MODE> (COPY with SNAP_BUILD).  Nothing is enqueued unless
   * the plan fits. */
  template <int MODE>
  int run(const void *d_data, void *d_out, void *d_crcs, void *d_rows, hipStream_t st) {
    constexpr bool COPY = MODE == SNAP_BUILD;
    if (too_large) return RGB_E_NOMEM;
    const size_t n_pieces = s.snap_pieces.size(), n_items = s.snap_items.size(), n_big = s.snap_big.size();
    if (!n_pieces && !n_items) return RGB_OK;
    const size_t off_blk = n_pieces * sizeof(snap_piece);
    const size_t off_items = up16(off_blk + ((size_t)count[3] + 1u) * 4u);
    const size_t off_big = off_items + n_items * sizeof(snap_item);
    const size_t need = off_big + n_big * 4u + 16u;
    pinned_upload &up = s.snap_plan_up;
    int rc;
    if ((rc = up.prepare(need))) return rc;
    unsigned char *h = (unsigned char *)up.h;
    snap_piece *h_pieces = (snap_piece *)h;
    u32 *h_blk = (u32 *)(h + off_blk);
    u32 first[4], at[4];
    first[0] = 0u;
    for (int t = 1; t < 4; ++t) first[t] = first[t - 1] + count[t - 1];
    for (int t = 0; t < 4; ++t) at[t] = first[t];
    u32 blk = 0;
    for (const snap_piece &p : s.snap_pieces) {
      const int t = snap_tier(p.len);
      if (t == 3) { h_blk[at[3] - first[3]] = blk; blk += (u32)((p.len + SNAP_BLOCK - 1u) / SNAP_BLOCK); }
      h_pieces[at[t]++] = p;
    }
    h_blk[count[3]] = blk;
    if (n_items) memcpy(h + off_items, s.snap_items.data(), n_items * sizeof(snap_item));
    if (n_big) memcpy(h + off_big, s.snap_big.data(), n_big * 4u);
    if (s.snap_raws.reserve((size_t)slots * 4u + 16u)) return RGB_E_NOMEM;
    if ((rc = up.upload(need, st))) return rc;
    const unsigned char *d = (const unsigned char *)up.d.p;
    const snap_piece *d_pieces = (const snap_piece *)d;
    const unsigned char *data = (const unsigned char *)d_data;
    unsigned char *out = (unsigned char *)d_out;
    u32 *raws = (u32 *)s.snap_raws.p, *crcs = (u32 *)d_crcs;
    (void)hipGetLastError();
    const u32 widths[3] = {8u, 16u, 64u};
    for (int t = 0; t < 3; ++t) {
      if (!count[t]) continue;
      with_width(widths[t], [&](auto g) {
        hipLaunchKernelGGL((rgb_snap_group_kernel<decltype(g)::value, COPY>), dim3(entry_grid(count[t], widths[t])),
                           dim3(THREADS), 0, st, d_pieces + first[t], count[t], data, out, raws, crcs);
      });
    }
    if (count[3])
      hipLaunchKernelGGL(rgb_snap_block_kernel<COPY>, dim3(blk < GRID_CAP ? blk : GRID_CAP), dim3(THREADS), 0, st,
                         d_pieces + first[3], (const u32 *)(d + off_blk), count[3], blk, data, out, raws);
    const size_t by_lane = (n_items + THREADS - 1u) / THREADS;
    const size_t grid = n_big > by_lane ? n_big : by_lane;
    if (grid)
      hipLaunchKernelGGL(rgb_snap_finish_kernel<MODE>, dim3((u32)(grid < GRID_CAP ? grid : GRID_CAP)), dim3(THREADS), 0, st,
                         (const snap_item *)(d + off_items), (u32)n_items, (const u32 *)(d + off_big), (u32)n_big,
                         (const u32 *)raws, data, out, crcs, (snap_row *)d_rows);
    return hipGetLastError() == hipSuccess ? RGB_OK : RGB_E_HIP;
  }
};

inline snap_item snap_item_of(u64 off, u32 kind) {
  snap_item it;
  memset(&it, 0, sizeof it);
  it.off = off; it.kind = kind;
  return it;
}
}  // namespace seg
}  // namespace

extern "C" int rgb_crc32_spans_device(rgb_ctx *ctx, const rgb_crc_span *spans, uint32_t n, const void *d_data,
                                      uint64_t data_bytes, void *d_crcs, void *stream) {
  if (!ctx || (n && (!spans || !d_crcs)) || (data_bytes && !d_data)) return RGB_E_INVAL;
  if (int rc = rgb_snapshot_spans_check(spans, n, data_bytes, nullptr)) return rc;
  hipStream_t st = stream ? (hipStream_t)stream : (hipStream_t)rgb_ctx_stream(ctx);
  std::lock_guard<std::recursive_mutex> lk(seg::g_mu);
  seg::snap_plan plan(seg::g_stages[ctx]);
  for (uint32_t i = 0; i < n; ++i) {
    const rgb_crc_span &sp = spans[i];
    if (seg::snap_tier(sp.n_bytes) < 3) plan.piece(sp.offset, sp.n_bytes, 0u, ~sp.init, seg::SNAP_DIRECT | i, nullptr);
    else plan.stream(seg::snap_item_of(i, 0u), 0u, 0u, 0u, sp.offset, sp.n_bytes, 0u, ~sp.init);
  }
  return plan.run<seg::SNAP_SPANS>(d_data, nullptr, d_crcs, nullptr, st);
}

extern "C" int rgb_snapshot_build_device(rgb_ctx *ctx, const rgb_snap_item *items, uint32_t n, const void *d_data,
                                         uint64_t data_bytes, void *d_out, uint64_t out_bytes, void *d_crcs, void *stream) {
  if (!ctx || (n && (!items || !d_out)) || (data_bytes && !d_data)) return RGB_E_INVAL;
  if (int rc = rgb_snapshot_build_check(items, n, data_bytes, out_bytes, nullptr)) return rc;
  hipStream_t st = stream ? (hipStream_t)stream : (hipStream_t)rgb_ctx_stream(ctx);
  std::lock_guard<std::recursive_mutex> lk(seg::g_mu);
  seg::snap_plan plan(seg::g_stages[ctx]);
  for (uint32_t i = 0; i < n; ++i) {
    const rgb_snap_item &it = items[i];
    if (it.kind == RGB_SNAP_KIND_SNAPSHOT) {
      const uint64_t meta_at = it.out_offset + RGB_SNAP_META_HEADER_BYTES;
      plan.stream(seg::snap_item_of(it.out_offset, it.kind), it.meta_offset, it.meta_len, meta_at, it.data_offset,
                  it.data_bytes, meta_at + it.meta_len, seg::snap_head_of_be32(it.meta_len));
    } else {
      plan.stream(seg::snap_item_of(it.out_offset, it.kind), 0u, 0u, 0u, it.data_offset, it.data_bytes,
                  it.out_offset + RGB_SNAP_HEADER_BYTES, 0xFFFFFFFFu);
    }
  }
  return plan.run<seg::SNAP_BUILD>(d_data, d_out, d_crcs, nullptr, st);
}

extern "C" int rgb_snapshot_validate_device(rgb_ctx *ctx, const rgb_snap_file *files, uint32_t n, const void *d_files,
                                            uint64_t files_bytes, void *d_infos, void *stream) {
  if (!ctx || (n && (!files || !d_infos)) || (files_bytes && !d_files)) return RGB_E_INVAL;
  if (int rc = rgb_snapshot_files_check(files, n, files_bytes, nullptr)) return rc;
  hipStream_t st = stream ? (hipStream_t)stream : (hipStream_t)rgb_ctx_stream(ctx);
  std::lock_guard<std::recursive_mutex> lk(seg::g_mu);
  seg::snap_plan plan(seg::g_stages[ctx]);
  for (uint32_t i = 0; i < n; ++i) {
    const rgb_snap_file &f = files[i];
    const bool sums = !(f.flags & RGB_SNAP_META_ONLY) && f.n_bytes > RGB_SNAP_HEADER_BYTES;
    seg::snap_item it = seg::snap_item_of(f.offset, f.kind | (f.flags << 8));
    /* the item has no piece A: len_a carries the file's size to the finish pass */
    plan.stream(it, 0u, 0u, 0u, f.offset + RGB_SNAP_HEADER_BYTES, sums ? f.n_bytes - RGB_SNAP_HEADER_BYTES : 0u, 0u,
                0xFFFFFFFFu);
    plan.s.snap_items.back().len_a = f.n_bytes;
  }
  return plan.run<seg::SNAP_VALIDATE>(d_files, nullptr, nullptr, d_infos, st);
}

extern "C" int rgb_crc32_spans(rgb_ctx *ctx, const rgb_crc_span *spans, uint32_t n, const void *data, uint64_t data_bytes,
                               uint32_t *crcs) {
  if (!ctx || (n && (!spans || !crcs)) || (data_bytes && !data)) return RGB_E_INVAL;
  if (int rc = rgb_snapshot_spans_check(spans, n, data_bytes, nullptr)) return rc;
  if (n == 0) return RGB_OK;
  if (hipSetDevice(rgb_ctx_device(ctx)) != hipSuccess) return RGB_E_HIP;
  std::lock_guard<std::recursive_mutex> lk(seg::g_mu);
  seg::stage &s = seg::g_stages[ctx];
  hipStream_t st = (hipStream_t)rgb_ctx_stream(ctx);
  if (s.crcs.reserve((size_t)n * 4u)) return RGB_E_NOMEM;
  int rc;
  if ((rc = seg::stage_in(s.data, data, (size_t)data_bytes, st))) return rc;
  if ((rc = rgb_crc32_spans_device(ctx, spans, n, s.data.p, data_bytes, s.crcs.p, st))) return rc;
  return seg::fetch(crcs, s.crcs, (size_t)n * 4u, st);
}

extern "C" int rgb_snapshot_build(rgb_ctx *ctx, const rgb_snap_item *items, uint32_t n, const void *data,
                                  uint64_t data_bytes, void *out, uint64_t out_bytes, uint32_t *crcs) {
  if (!ctx || (n && (!items || !out)) || (data_bytes && !data)) return RGB_E_INVAL;
  uint64_t sum = 0;
  if (int rc = rgb_snapshot_build_check(items, n, data_bytes, out_bytes, &sum)) return rc;
  if (n == 0) return RGB_OK;
  /* the images are packed on the device in the caller's order, wherever they go in `out` */
  std::vector<rgb_snap_item> packed(items, items + n);
  const uint64_t total = rgb_snapshot_layout(packed.data(), n, 0u);
  if (hipSetDevice(rgb_ctx_device(ctx)) != hipSuccess) return RGB_E_HIP;
  std::lock_guard<std::recursive_mutex> lk(seg::g_mu);
  seg::stage &s = seg::g_stages[ctx];
  hipStream_t st = (hipStream_t)rgb_ctx_stream(ctx);
  if (s.out.reserve((size_t)total) || s.crcs.reserve((size_t)n * 4u)) return RGB_E_NOMEM;
  int rc;
  if ((rc = seg::stage_in(s.data, data, (size_t)data_bytes, st))) return rc;
  if ((rc = rgb_snapshot_build_device(ctx, packed.data(), n, s.data.p, data_bytes, s.out.p, total, s.crcs.p, st))) return rc;
  /* only the images' own bytes come back: neighbours in `out` in one copy */
  for (uint32_t i = 0; i < n;) {
    const uint64_t from = packed[i].out_offset, to = items[i].out_offset;
    uint64_t bytes = 0;
    for (; i < n && items[i].out_offset == to + bytes; ++i)
      bytes += (i + 1u < n ? packed[i + 1u].out_offset : total) - packed[i].out_offset;
    if (bytes && hipMemcpyAsync((unsigned char *)out + to, (const unsigned char *)s.out.p + from, (size_t)bytes,
                                hipMemcpyDeviceToHost, st) != hipSuccess)
      return RGB_E_HIP;
  }
  if (crcs) return seg::fetch(crcs, s.crcs, (size_t)n * 4u, st);
  return hipStreamSynchronize(st) == hipSuccess ? RGB_OK : RGB_E_HIP;
}

extern "C" int rgb_snapshot_validate(rgb_ctx *ctx, const rgb_snap_file *files, uint32_t n, const void *bytes,
                                     uint64_t files_bytes, rgb_snap_info *infos) {
  if (!ctx || (n && (!files || !infos)) || (files_bytes && !bytes)) return RGB_E_INVAL;
  if (int rc = rgb_snapshot_files_check(files, n, files_bytes, nullptr)) return rc;
  if (n == 0) return RGB_OK;
  if (hipSetDevice(rgb_ctx_device(ctx)) != hipSuccess) return RGB_E_HIP;
  std::lock_guard<std::recursive_mutex> lk(seg::g_mu);
  seg::stage &s = seg::g_stages[ctx];
  hipStream_t st = (hipStream_t)rgb_ctx_stream(ctx);
  if (s.infos.reserve((size_t)n * sizeof(rgb_snap_info))) return RGB_E_NOMEM;
  int rc;
  if ((rc = seg::stage_in(s.data, bytes, (size_t)files_bytes, st))) return rc;
  if ((rc = rgb_snapshot_validate_device(ctx, files, n, s.data.p, files_bytes, s.infos.p, st))) return rc;
  return seg::fetch(infos, s.infos, (size_t)n * sizeof(rgb_snap_info), st);
}

/*
 * rgb_wal.hip -- Adler-32 of a batch of WAL entries (include/ra_gpu_wal.h; reference
 * src/ra_log_wal.erl:528-534, 861, 873, 1028).  One wavefront (or a quarter of one) per entry; bytes
 * stream through 16-byte lane loads, sums through v_dot4_u32_u8.  HBM-bound: every payload byte is read once.
 *
 * Adler-32 (RFC 1950 8.2) of bytes d_0..d_{n-1}:  A = 1 + sum d_i,  B = n + sum (n - i) d_i,
 * both mod 65521, checksum = B << 16 | A.  The weighted sum is additive over any partition of the
 * bytes, so each lane handles whole 16-byte aligned chunks with local sums
 *     a = sum d_j,  b = sum (16 - j) d_j        (j = 0..15 inside the chunk)
 * and a chunk that starts s bytes into the stream contributes  (W - s - 16) * a + b  where W is
 * the weight of the stream's first byte.  Bytes outside the payload are masked to zero, which
 * makes the entry's alignment irrelevant.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/ra_gpu_wal.h"

namespace {

typedef unsigned int u32;
typedef unsigned long long u64;
#define ADLER_MOD 65521u
#ifndef WAL_WAVES_PER_BLOCK
#define WAL_WAVES_PER_BLOCK 4
#endif
#define WAL_UNROLL 4            /* 16-byte loads in flight per lane: 4 KiB per wavefront iteration */
/* a lane's running sums are reduced mod 65521 once they reach this value.  A sum is below it (or below 65521, just
 * reduced) when a piece is added, and the largest single addition is the (wq a + b) mod 65521 <= 65520 of the loops
 * (a <= 4080 there; the frame kernel's tail piece adds an unreduced b <= 136 * 255 = 34680 and a <= 15 * 255 = 3825),
 * so no sum ever exceeds WAL_FOLD_AT - 1 + 65520: that has to fit 32 bits */
#ifndef WAL_FOLD_AT
#define WAL_FOLD_AT 0x7FFF0000u
#endif
static_assert((unsigned long long)(WAL_FOLD_AT) >= 65521ull && (unsigned long long)(WAL_FOLD_AT) + 65520ull <= 0xFFFFFFFFull,
              "WAL_FOLD_AT: a reduced sum lies below it, and WAL_FOLD_AT - 1 + 65520 fits a u32");
typedef unsigned int v4u __attribute__((ext_vector_type(4)));

__device__ __forceinline__ u32 dot4(u32 a, u32 b, u32 c) { return __builtin_amdgcn_udot4(a, b, c, false); }

/* local sums of one 16-byte chunk (little-endian dwords, byte 0 = lowest address) */
__device__ __forceinline__ void chunk_sums(const uint4 v, u32 &a, u32 &b) {
  a = dot4(v.x, 0x01010101u, 0); a = dot4(v.y, 0x01010101u, a);
  a = dot4(v.z, 0x01010101u, a); a = dot4(v.w, 0x01010101u, a);
  b = dot4(v.x, 0x0D0E0F10u, 0); b = dot4(v.y, 0x090A0B0Cu, b);
  b = dot4(v.z, 0x05060708u, b); b = dot4(v.w, 0x01020304u, b);
}

/* 0xFF for every byte of the dword at chunk bytes [first, first+4) that lies inside [lo, hi) */
__device__ __forceinline__ u32 byte_mask(u32 first, u32 lo, u32 hi) {
  u32 m = 0;
#pragma unroll
  for (u32 b = 0; b < 4; ++b) if (first + b >= lo && first + b < hi) m |= 0xFFu << (8 * b);
  return m;
}
/* the same for a whole 16-byte chunk, from two 64-bit shifts per half instead of sixteen byte tests */
__device__ __forceinline__ u64 ones64(u32 nbytes) { return nbytes >= 8u ? ~0ull : ((1ull << (8u * nbytes)) - 1ull); }
__device__ __forceinline__ uint4 keep_bytes(const uint4 w, u32 lo, u32 hi) {
  const u32 lo_a = lo < 8u ? lo : 8u, hi_a = hi < 8u ? hi : 8u;
  const u32 lo_b = lo > 8u ? lo - 8u : 0u, hi_b = hi > 8u ? hi - 8u : 0u;
  const u64 ma = ones64(hi_a) & ~ones64(lo_a), mb = ones64(hi_b) & ~ones64(lo_b);
  return make_uint4(w.x & (u32)ma, w.y & (u32)(ma >> 32), w.z & (u32)mb, w.w & (u32)(mb >> 32));
}

/* sum over the GROUP lanes that share a record (xor butterflies stay inside aligned groups) */
template <int GROUP>
__device__ __forceinline__ u32 group_sum(u32 v) {
#pragma unroll
  for (int off = GROUP / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

/* GROUP lanes per entry: 64 (one wavefront per entry) for KiB-sized payloads, 16 (four entries per
 * wavefront) for small ones -- the host picks by the batch's mean payload size. */
template <int GROUP>
__global__ __launch_bounds__(WAL_WAVES_PER_BLOCK * 64) void rgb_wal_adler32_kernel(
    const rgb_wal_entry *__restrict__ entries, u32 n, const unsigned char *__restrict__ data,
    u32 *__restrict__ out) {
  constexpr u32 PER_BLOCK = WAL_WAVES_PER_BLOCK * 64 / GROUP;
  const u32 lane = threadIdx.x & (GROUP - 1);
  const u32 e = blockIdx.x * PER_BLOCK + threadIdx.x / GROUP;
  const bool live = e < n;
  rgb_wal_entry en;
  en.index = en.term = en.data_offset = 0; en.data_len = 0; en._pad = 0;
  if (live) en = entries[e];
  const u64 off = en.data_offset;
  const u32 len = en.data_len;
  const u32 lead = (u32)(off & 15ull);                 /* masked bytes in front of the payload */
  const v4u *base = reinterpret_cast<const v4u *>(data + (off - lead));
  const u32 span = lead + len;                         /* aligned stream: [0, span) */
  const u32 n_chunks = live ? (span + 15u) >> 4 : 0u;
  const u32 span_q = span % ADLER_MOD;
  /* weight of stream byte j is (len + lead) - j: the last payload byte weighs 1 */
  u32 a_acc = 0, b_acc = 0;                            /* per lane, folded before they can wrap */
  for (u32 c0 = 0; c0 < n_chunks; c0 += GROUP * WAL_UNROLL) {
    uint4 v[WAL_UNROLL];
#pragma unroll
    for (int k = 0; k < WAL_UNROLL; ++k) {
      const u32 c = c0 + (u32)k * GROUP + lane;
      v[k] = make_uint4(0, 0, 0, 0);
      if (c < n_chunks) { const v4u t = __builtin_nontemporal_load(base + c); v[k] = make_uint4(t.x, t.y, t.z, t.w); }
    }
#pragma unroll
    for (int k = 0; k < WAL_UNROLL; ++k) {
      const u32 c = c0 + (u32)k * GROUP + lane;
      if (c >= n_chunks) continue;
      const u32 s = c << 4;
      uint4 w = v[k];
      /* mask the bytes before the payload (first chunk) and after it (last chunk) */
      if (s < lead || s + 16u > span) {
        const u32 lo = s < lead ? lead - s : 0u, hi = span - s < 16u ? span - s : 16u;
        w.x &= byte_mask(0, lo, hi); w.y &= byte_mask(4, lo, hi);
        w.z &= byte_mask(8, lo, hi); w.w &= byte_mask(12, lo, hi);
      }
      u32 a, b;
      chunk_sums(w, a, b);
      /* (W - s - 16) may be negative on the last chunk: work modulo 65521 */
      const u32 wq = (span_q + 2u * ADLER_MOD - (s % ADLER_MOD) - 16u) % ADLER_MOD;
      a_acc += a;                                      /* <= 4080 per chunk */
      b_acc += (wq * a + b) % ADLER_MOD;
      if (b_acc >= WAL_FOLD_AT) b_acc %= ADLER_MOD;
      if (a_acc >= WAL_FOLD_AT) a_acc %= ADLER_MOD;
    }
  }
  const u32 a_sum = group_sum<GROUP>(a_acc % ADLER_MOD);   /* GROUP * 65520 fits */
  const u32 b_sum = group_sum<GROUP>(b_acc % ADLER_MOD);
  if (live && lane == 0) {
    /* the 16 framed bytes <<Idx:64, Term:64>> in front are one more chunk whose byte k weighs
     * n - k = len + (16 - k): big-endian words, so the dot4 weight vectors run the other way */
    const u32 ih = (u32)(en.index >> 32), il = (u32)en.index, th = (u32)(en.term >> 32), tl = (u32)en.term;
    u32 pa = dot4(ih, 0x01010101u, 0); pa = dot4(il, 0x01010101u, pa);
    pa = dot4(th, 0x01010101u, pa); pa = dot4(tl, 0x01010101u, pa);
    u32 pb = dot4(ih, 0x100F0E0Du, 0); pb = dot4(il, 0x0C0B0A09u, pb);
    pb = dot4(th, 0x08070605u, pb); pb = dot4(tl, 0x04030201u, pb);
    const u32 len_q = len % ADLER_MOD;
    const u32 A = (1u + pa + a_sum) % ADLER_MOD;
    const u32 B = ((16u + len_q) + (len_q * pa + pb) % ADLER_MOD + b_sum) % ADLER_MOD;
    out[e] = (B << 16) | A;
  }
}


/* ---- record framing: checksum + header + payload copy in one pass (src/ra_log_wal.erl:513-537) ----
 *
 * A record is  HeaderData ++ <<Checksum:32, EntryDataLen:32, Idx:64, Term:64>> ++ Payload  at out + out_offset.
 * GROUP lanes per record (8 up to a mean payload of 320 bytes, 16 up to 1 KiB, then a wavefront); lane j handles
 * payload bytes [16 j, 16 j + 16) AS THEY LIE: one 16-byte load at the payload's own alignment (non-temporal), the
 * checksum on exactly those bytes (the piece that starts p bytes into the payload weighs (len - p - 16) a + b, no
 * masks), one 16-byte store at the destination's own alignment -- gfx950 global loads and stores take any byte
 * alignment.  A payload that does not end on a piece boundary ends with the piece [len - 16, len), which overlaps its
 * predecessor: the overlapped bytes are masked out of the sums (what is left weighs exactly b) and are stored twice
 * with the same value.  Payloads under 16 bytes go byte by byte.  The 24 fixed bytes are two unaligned vector stores by
 * the group's first lane once the checksum is known; HeaderData is copied byte per lane (3 bytes for a known writer).
 *
 * Rounds 1-3 framed through a FUNNEL (source-aligned loads, destination-aligned stores, the byte shift through DPP
 * and v_alignbyte, partial chunks as power-of-two store chains) because a first version with misaligned loads was
 * 30 % slower on 4 KiB payloads.  Measured again in round 4 with the funnel's instruction count out of the way
 * (profiles/EXPERIMENTS.md): this form is 24 % faster on 256-byte payloads (the funnel was vector-issue bound: ~900
 * instructions per eight records), 4 % faster on 4 KiB payloads and the same on 0.4-16 KiB mixes, at a third of the code. */

/* mean payload up to which a batch is framed with eight lanes per record (then sixteen up to 1 KiB, then a wavefront) */
#ifndef WAL_FRAME_EIGHT_MAX
#define WAL_FRAME_EIGHT_MAX 320u
#endif
typedef v4u v4u_any __attribute__((aligned(1)));
template <int GROUP>
__global__ __launch_bounds__(WAL_WAVES_PER_BLOCK * 64) void rgb_wal_frame_kernel(
    const rgb_wal_record *__restrict__ recs, u32 n, const unsigned char *__restrict__ data,
    unsigned char *__restrict__ out, u32 *__restrict__ sums_out, u32 flags) {
  constexpr u32 PER_BLOCK = WAL_WAVES_PER_BLOCK * 64 / GROUP;
  constexpr bool UNI = GROUP == 64;                     /* one record per wavefront: descriptor in scalar registers */
  constexpr int UNROLL = GROUP == 64 ? WAL_UNROLL : 2;
  const u32 lane = threadIdx.x & (GROUP - 1);
  u32 e = blockIdx.x * PER_BLOCK + threadIdx.x / GROUP;
#ifndef RGB_HOST_EMULATION
  if (UNI) e = (u32)__builtin_amdgcn_readfirstlane((int)e);
#endif
  const bool live = e < n;
  rgb_wal_record r;
  r.index = r.term = r.data_offset = r.hdr_offset = r.out_offset = 0; r.data_len = r.hdr_len = 0;
  if (live) r = recs[e];
  const u32 len = r.data_len;
  unsigned char *rec = out + r.out_offset;
  unsigned char *dst = rec + r.hdr_len + 24u;           /* the payload's place in the record */
  const unsigned char *pay = data + r.data_offset;
  const unsigned char *hdr = data + r.hdr_offset;
  u32 hbyte = 0;
  if (live && lane < r.hdr_len) hbyte = hdr[lane];
  const u32 n_full = live ? len >> 4 : 0u, rem = live ? len & 15u : 0u;
  const u32 len_q = len % ADLER_MOD;
  u32 a_acc = 0, b_acc = 0;
  constexpr u32 STEP = (16u * GROUP) % ADLER_MOD;
  /* weight of the byte behind piece j: (len - 16 j - 16) mod 65521, stepped down per round */
  u32 wq = (len_q + 2u * ADLER_MOD - ((lane << 4) % ADLER_MOD) - 16u) % ADLER_MOD;
  for (u32 j0 = 0; j0 < n_full; j0 += GROUP * UNROLL) {
    uint4 v[UNROLL];
#pragma unroll
    for (int k = 0; k < UNROLL; ++k) {
      const u32 j = j0 + (u32)k * GROUP + lane;
      v[k] = make_uint4(0, 0, 0, 0);
      if (j < n_full) {
        const v4u t = __builtin_nontemporal_load(reinterpret_cast<const v4u_any *>(pay + ((size_t)j << 4)));
        v[k] = make_uint4(t.x, t.y, t.z, t.w);
      }
    }
#pragma unroll
    for (int k = 0; k < UNROLL; ++k) {
      const u32 j = j0 + (u32)k * GROUP + lane;
      if (j < n_full) {
        v4u t; t.x = v[k].x; t.y = v[k].y; t.z = v[k].z; t.w = v[k].w;
#if defined(RGB_HOST_EMULATION)
        *reinterpret_cast<v4u_any *>(dst + ((size_t)j << 4)) = t;
#else
        /* streamed past the caches for a record per wavefront.  Small records: a plain store -- every other 128-byte
         * line of the output holds a record boundary whose bytes arrive from other instructions, and a line a
         * non-temporal store pushed out early is written to memory twice (round 3: 396 -> 360 us per 2 M records) */
        if (UNI) __builtin_nontemporal_store(t, reinterpret_cast<v4u_any *>(dst + ((size_t)j << 4)));
        else *reinterpret_cast<v4u_any *>(dst + ((size_t)j << 4)) = t;
#endif
        u32 a, b;
        chunk_sums(v[k], a, b);
        a_acc += a;
        b_acc += (wq * a + b) % ADLER_MOD;
        if (b_acc >= WAL_FOLD_AT) b_acc %= ADLER_MOD;
        if (a_acc >= WAL_FOLD_AT) a_acc %= ADLER_MOD;
      }
      wq = wq >= STEP ? wq - STEP : wq + (ADLER_MOD - STEP);
    }
  }
  if (rem && lane == (n_full & (GROUP - 1))) {           /* the last len mod 16 bytes: they weigh rem .. 1 */
    uint4 w = make_uint4(0, 0, 0, 0);
    if (n_full) {
      const v4u t = __builtin_nontemporal_load(reinterpret_cast<const v4u_any *>(pay + (len - 16u)));
      *reinterpret_cast<v4u_any *>(dst + (len - 16u)) = t;
      w = keep_bytes(make_uint4(t.x, t.y, t.z, t.w), 16u - rem, 16u);
    } else {
      u64 lo = 0, hi = 0;                                /* bytes at chunk positions [16 - rem, 16) */
      for (u32 k = 0; k < rem; ++k) {
        const u32 c = pay[k], q = 16u - rem + k;
        dst[k] = (unsigned char)c;
        if (q < 8u) lo |= (u64)c << (8u * q); else hi |= (u64)c << (8u * (q - 8u));
      }
      w = make_uint4((u32)lo, (u32)(lo >> 32), (u32)hi, (u32)(hi >> 32));
    }
    u32 a, b;
    chunk_sums(w, a, b);
    a_acc += a; b_acc += b;                              /* both far from wrapping: one piece */
  }
  const u32 a_sum = group_sum<GROUP>(a_acc % ADLER_MOD);
  const u32 b_sum = group_sum<GROUP>(b_acc % ADLER_MOD);
  if (!live) return;
  const u32 ih = (u32)(r.index >> 32), il = (u32)r.index, th = (u32)(r.term >> 32), tl = (u32)r.term;
  u32 pa = dot4(ih, 0x01010101u, 0); pa = dot4(il, 0x01010101u, pa);
  pa = dot4(th, 0x01010101u, pa); pa = dot4(tl, 0x01010101u, pa);
  u32 pb = dot4(ih, 0x100F0E0Du, 0); pb = dot4(il, 0x0C0B0A09u, pb);
  pb = dot4(th, 0x08070605u, pb); pb = dot4(tl, 0x04030201u, pb);
  const u32 A = (1u + pa + a_sum) % ADLER_MOD;
  const u32 B = ((16u + len_q) + (len_q * pa + pb) % ADLER_MOD + b_sum) % ADLER_MOD;
  const u32 cs = (flags & RGB_WAL_NO_CHECKSUMS) ? 0u : ((B << 16) | A);
  if (lane < r.hdr_len) rec[lane] = (unsigned char)hbyte;
  for (u32 j = GROUP + lane; j < r.hdr_len; j += GROUP) rec[j] = hdr[j];
  if (lane == 0u) {
    if (sums_out) sums_out[e] = cs;
    struct __attribute__((packed)) fixed24 { v4u a; u64 b; };
    fixed24 fx;
    fx.a.x = __builtin_bswap32(cs); fx.a.y = __builtin_bswap32(len);
    fx.a.z = __builtin_bswap32(ih); fx.a.w = __builtin_bswap32(il);
    fx.b = (u64)__builtin_bswap32(th) | ((u64)__builtin_bswap32(tl) << 32);
    __builtin_memcpy(rec + r.hdr_len, &fx, 24);
  }
}

/* ---- WAL batch (include/ra_gpu_wal.h, "WAL batch"): handle_batch/2 for a batch of append commands --------------
 * Seven launches, each its own, so that no workgroup ever waits for another:
 *   verdict  S lanes per writer (8, 16 or a wavefront, by the longest writer of the call), every workgroup a contiguous
 *            run of writers.  A writer's commands (the host's per-writer order) go through LDS in chunks of S; the
 *            sub-group's first lane walks the chain of handle_msg/2 and leaves per command the verdict, the Trunc and
 *            first-appearance bits, whether a run of equal (term, tid) starts here, and the state behind it.
 *   sum      mailbox order, every workgroup a contiguous run of tiles: the sums of (accounted bytes, real bytes,
 *            WRITEs, first appearances) of its commands.
 *   place    the same grid: the sums of the workgroups in front, an LDS scan per tile, the exclusive prefixes of every
 *            command, and the minimum over "WRITE command that finds the roll test true" -- both limits are monotone
 *            in the prefixes.
 *   rows     per command, clipped to n_consumed: the result row, and for a WRITE its frame record at its rank.
 *   events   per writer as in verdict: the walker keeps the ra_seq of the running run as a stack of (first, last) pairs
 *            in the writer's own part of the scratch (its top in registers), closes a run with the floor, and leaves
 *            the writer's row; per workgroup the event and pair counts.
 *   gather   the same grid: totals, the status and the total row; the base of every writer by LDS scan; events and
 *            pairs move to their dense, sorted places.
 *   frame    the body of rgb_wal_frame_kernel over the frame records, the header made in registers. */
#define WB_THREADS 256
#define WB_GRID_CAP 1024u
#define WB_NONE32 0xFFFFFFFFu
/* bits of wb_v.bits above the public RGB_WAL_V_* ones */
#define WB_RUN 0x400u                                   /* WRITE: (term, tid) differ from the writer's previous WRITE */
#define WB_KIND_SHIFT 16                                /* the state kind behind the command */

struct wb_hdr {                                         /* one per call, in the scratch */
  u32 n_consumed, n_written, store, status;
  u64 out_bytes, file_size, entry_count;
  u32 next_id_ref, _pad;
};
struct wb_v { u64 value, post_prev; u32 bits, _pad; };              /* per command: verdict */
struct wb_pre { u64 acc, real; u32 writes, firsts; };               /* per command: exclusive prefixes; per workgroup: sums */
struct wb_frec { u64 index, term, data_offset, uid_offset, out_offset; u32 data_len, hdr3, uid_len, cmd; u64 _pad; };
struct wb_ev { u64 term, tid; u32 pair_first, pair_n; };            /* per writer part: an event before it is placed */
struct wb_cnt { u32 events, pairs; };
static_assert(sizeof(wb_v) == 24 && sizeof(wb_pre) == 24 && sizeof(wb_frec) == 64 && sizeof(wb_ev) == 24, "");

__device__ __forceinline__ void wb_atomic_min32(u32 *p, u32 v) {
  u32 old = *p;
  while (v < old) {
    const u32 seen = atomicCAS(p, old, v);
    if (seen == old) break;
    old = seen;
  }
}

/* what command i adds to the file: (accounted, real) bytes, a WRITE, a first appearance */
__device__ __forceinline__ wb_pre wb_elem(const rgb_wal_cmd *cmds, const rgb_wal_writer *writers, const wb_v *vd, u32 i) {
  wb_pre e; e.acc = e.real = 0ull; e.writes = e.firsts = 0u;
  const u32 bits = vd[i].bits;
  if ((bits & RGB_WAL_V_MASK) != RGB_WAL_V_WRITE) return e;
  const u64 body = 24ull + cmds[i].data_len;
  e.writes = 1u;
  if (bits & RGB_WAL_V_FIRST) {
    e.firsts = 1u;
    e.acc = e.real = body + 5u + writers[cmds[i].writer].uid_len;
  } else {
    e.real = body + 3u;
    e.acc = body + ((bits & RGB_WAL_V_TRUNC) ? 2u : 3u);   /* the reference's HeaderLen of a cached header with Trunc */
  }
  return e;
}

template <int S>
__global__ __launch_bounds__(WB_THREADS) void rgb_wal_batch_verdict_kernel(
    const rgb_wal_cmd *__restrict__ cmds, const rgb_wal_writer *__restrict__ writers, u32 n_writers, u32 per_block,
    const u32 *__restrict__ order, const u32 *__restrict__ wstart, wb_v *__restrict__ vd, u32 *__restrict__ wfirst) {
  constexpr u32 SUBS = WB_THREADS / S;
  __shared__ u64 s_idx[WB_THREADS], s_prev[WB_THREADS], s_small[WB_THREADS], s_term[WB_THREADS], s_tid[WB_THREADS];
  __shared__ u64 s_value[WB_THREADS], s_post[WB_THREADS];
  __shared__ u32 s_bits[WB_THREADS];
  __shared__ u32 s_chunks[SUBS];
  const u32 tid = threadIdx.x, sub = tid / (u32)S, ln = tid % (u32)S, s0 = sub * (u32)S;
  const u32 wb = blockIdx.x * per_block;
  const u32 we = n_writers - wb < per_block ? n_writers : wb + per_block;
  for (u32 r0 = wb; r0 < we; r0 += SUBS) {                /* the same for every lane */
    const u32 w = r0 + sub;
    const bool have = w < we;
    u32 first = 0, count = 0;
    rgb_wal_writer wd{};
    if (have) { wd = writers[w]; first = wstart[w]; count = wstart[w + 1u] - first; }
    const u32 my_chunks = count / (u32)S + (count % (u32)S ? 1u : 0u);
    if (ln == 0u) s_chunks[sub] = my_chunks;
    __syncthreads();
    u32 iters = 0;
    for (u32 i = 0; i < SUBS; ++i) iters = s_chunks[i] > iters ? s_chunks[i] : iters;
    __syncthreads();
    /* the sub-group's first lane: the writer's state, whether it is named in the file, its last WRITE's (term, tid) */
    u32 kind = wd.state, first_cmd = WB_NONE32;
    u64 P = wd.prev_index, run_term = 0, run_tid = 0;
    bool named = wd.id_ref != RGB_WAL_NO_ID_REF, wrote = false;
    for (u32 ch = 0; ch < iters; ++ch) {
      const u32 cbase = ch * (u32)S;
      const u32 n_c = ch >= my_chunks ? 0u : (count - cbase < (u32)S ? count - cbase : (u32)S);
      const bool valid = ln < n_c;
      u32 c = 0;
      if (valid) {
        c = order[first + cbase + ln];
        const rgb_wal_cmd cm = cmds[c];
        s_idx[tid] = cm.index; s_prev[tid] = cm.prev_index; s_small[tid] = cm.smallest_index;
        s_term[tid] = cm.term; s_tid[tid] = cm.tid;
      }
      __syncthreads();
      if (ln == 0u) {
        for (u32 j = 0; j < n_c; ++j) {
          const u64 idx = s_idx[s0 + j], small = s_small[s0 + j];
          const bool trunc = idx == small;
          u32 bits;
          u64 value = 0;
          if (idx < small) {
            bits = RGB_WAL_V_DROP; kind = RGB_WAL_W_IN_SEQ; P = small - 1ull;
          } else if (kind == RGB_WAL_W_UNDEFINED || s_prev[s0 + j] <= P || trunc) {
            bits = RGB_WAL_V_WRITE;
            if (trunc && kind != RGB_WAL_W_UNDEFINED) bits |= RGB_WAL_V_TRUNC;
            if (!named) { bits |= RGB_WAL_V_FIRST; named = true; first_cmd = order[first + cbase + j]; }
            if (!wrote || s_term[s0 + j] != run_term || s_tid[s0 + j] != run_tid) bits |= WB_RUN;
            wrote = true; run_term = s_term[s0 + j]; run_tid = s_tid[s0 + j];
            kind = RGB_WAL_W_IN_SEQ; P = idx;
          } else if (kind == RGB_WAL_W_OUT_OF_SEQ) {
            bits = RGB_WAL_V_IGNORE;
          } else {
            bits = RGB_WAL_V_RESEND; value = P + 1ull; kind = RGB_WAL_W_OUT_OF_SEQ;
          }
          s_bits[s0 + j] = bits | (kind << WB_KIND_SHIFT); s_value[s0 + j] = value; s_post[s0 + j] = P;
        }
      }
      __syncthreads();
      if (valid) {
        wb_v v; v.value = s_value[tid]; v.post_prev = s_post[tid]; v.bits = s_bits[tid]; v._pad = 0u;
        vd[c] = v;
      }
      __syncthreads();
    }
    if (have && ln == 0u) wfirst[w] = first_cmd;
  }
}

__global__ __launch_bounds__(WB_THREADS) void rgb_wal_batch_sum_kernel(
    const rgb_wal_cmd *__restrict__ cmds, u32 n, const rgb_wal_writer *__restrict__ writers, const wb_v *__restrict__ vd,
    u32 per_block, wb_pre *__restrict__ blk, wb_hdr *__restrict__ hdr) {
  __shared__ u64 s_acc, s_real;
  __shared__ u32 s_writes, s_firsts;
  const u32 tid = threadIdx.x;
  if (tid == 0u) { s_acc = s_real = 0ull; s_writes = s_firsts = 0u; }
  __syncthreads();
  const u64 b0 = (u64)blockIdx.x * per_block, b1 = b0 + per_block < n ? b0 + per_block : n;
  wb_pre t; t.acc = t.real = 0ull; t.writes = t.firsts = 0u;
  for (u64 i = b0 + tid; i < b1; i += WB_THREADS) {
    const wb_pre e = wb_elem(cmds, writers, vd, (u32)i);
    t.acc += e.acc; t.real += e.real; t.writes += e.writes; t.firsts += e.firsts;
  }
  if (t.writes) { atomicAdd(&s_acc, t.acc); atomicAdd(&s_real, t.real); atomicAdd(&s_writes, t.writes); }
  if (t.firsts) atomicAdd(&s_firsts, t.firsts);
  __syncthreads();
  if (tid == 0u) {
    wb_pre r; r.acc = s_acc; r.real = s_real; r.writes = s_writes; r.firsts = s_firsts;
    blk[blockIdx.x] = r;
    if (blockIdx.x == 0u) hdr->n_consumed = n;            /* place takes the minimum into it */
  }
}

__global__ __launch_bounds__(WB_THREADS) void rgb_wal_batch_place_kernel(
    const rgb_wal_cmd *__restrict__ cmds, u32 n, const rgb_wal_writer *__restrict__ writers, const wb_v *__restrict__ vd,
    u32 per_block, const wb_pre *__restrict__ blk, const rgb_wal_file *__restrict__ file, wb_pre *__restrict__ pre,
    wb_hdr *hdr) {
  __shared__ u64 s_a[WB_THREADS], s_r[WB_THREADS];
  __shared__ u32 s_w[WB_THREADS], s_f[WB_THREADS];
  __shared__ u64 s_acc, s_real;
  __shared__ u32 s_writes, s_firsts, s_roll;
  const u32 tid = threadIdx.x;
  if (tid == 0u) { s_acc = s_real = 0ull; s_writes = s_firsts = 0u; s_roll = WB_NONE32; }
  __syncthreads();
  wb_pre t; t.acc = t.real = 0ull; t.writes = t.firsts = 0u;
  for (u32 i = tid; i < blockIdx.x; i += WB_THREADS) {
    const wb_pre e = blk[i];
    t.acc += e.acc; t.real += e.real; t.writes += e.writes; t.firsts += e.firsts;
  }
  if (t.writes) { atomicAdd(&s_acc, t.acc); atomicAdd(&s_real, t.real); atomicAdd(&s_writes, t.writes); }
  if (t.firsts) atomicAdd(&s_firsts, t.firsts);
  __syncthreads();
  wb_pre run; run.acc = s_acc; run.real = s_real; run.writes = s_writes; run.firsts = s_firsts;
  const rgb_wal_file fl = *file;
  const u64 b0 = (u64)blockIdx.x * per_block, b1 = b0 + per_block < n ? b0 + per_block : n;
  for (u64 base = b0; base < b1; base += WB_THREADS) {    /* the same for every lane */
    const u64 i = base + tid;
    const bool valid = i < b1;
    wb_pre e; e.acc = e.real = 0ull; e.writes = e.firsts = 0u;
    if (valid) e = wb_elem(cmds, writers, vd, (u32)i);
    s_a[tid] = e.acc; s_r[tid] = e.real; s_w[tid] = e.writes; s_f[tid] = e.firsts;
    __syncthreads();
    for (u32 off = 1; off < WB_THREADS; off <<= 1) {
      u64 ta = s_a[tid], tr = s_r[tid];
      u32 tw = s_w[tid], tf = s_f[tid];
      if (tid >= off) { ta += s_a[tid - off]; tr += s_r[tid - off]; tw += s_w[tid - off]; tf += s_f[tid - off]; }
      __syncthreads();
      s_a[tid] = ta; s_r[tid] = tr; s_w[tid] = tw; s_f[tid] = tf;
      __syncthreads();
    }
    if (valid) {
      wb_pre p;                                           /* what the commands in front of i added */
      p.acc = run.acc + s_a[tid] - e.acc; p.real = run.real + s_r[tid] - e.real;
      p.writes = run.writes + s_w[tid] - e.writes; p.firsts = run.firsts + s_f[tid] - e.firsts;
      pre[i] = p;
      if (e.writes) {                                     /* should_roll_wal/1 in front of this WRITE */
        const bool roll = fl.file_size + p.acc > fl.max_size ||
                          (fl.max_entries != 0ull && fl.entry_count + p.writes >= fl.max_entries);
        if (roll) wb_atomic_min32(&s_roll, (u32)i);
      }
      if (i + 1ull == n) {                                /* pre[n]: the whole batch */
        p.acc += e.acc; p.real += e.real; p.writes += e.writes; p.firsts += e.firsts;
        pre[n] = p;
      }
    }
    run.acc += s_a[WB_THREADS - 1]; run.real += s_r[WB_THREADS - 1];
    run.writes += s_w[WB_THREADS - 1]; run.firsts += s_f[WB_THREADS - 1];
    __syncthreads();
  }
  __syncthreads();
  if (tid == 0u && s_roll != WB_NONE32) wb_atomic_min32(&hdr->n_consumed, s_roll);
}

__global__ __launch_bounds__(WB_THREADS) void rgb_wal_batch_rows_kernel(
    const rgb_wal_cmd *__restrict__ cmds, u32 n, const rgb_wal_writer *__restrict__ writers, const wb_v *__restrict__ vd,
    const wb_pre *__restrict__ pre, const u32 *__restrict__ wfirst, const rgb_wal_file *__restrict__ file, u64 out_bytes,
    wb_hdr *hdr, wb_frec *__restrict__ frecs, rgb_wal_cmd_result *__restrict__ results) {
  const u32 nc = hdr->n_consumed;                         /* settled before this launch; not written here */
  const rgb_wal_file fl = *file;
  if (blockIdx.x == 0u && threadIdx.x == 0u) {
    const wb_pre t = pre[nc];
    hdr->n_written = t.writes; hdr->out_bytes = t.real; hdr->store = t.real <= out_bytes ? 1u : 0u;
    hdr->file_size = fl.file_size + t.acc; hdr->entry_count = fl.entry_count + t.writes;
    hdr->next_id_ref = fl.next_id_ref + t.firsts;
  }
  for (u64 i = (u64)blockIdx.x * WB_THREADS + threadIdx.x; i < n; i += (u64)gridDim.x * WB_THREADS) {
    rgb_wal_cmd_result r; r.verdict = RGB_WAL_V_NOT_CONSUMED; r.checksum = 0u; r.value = 0ull;
    if (i < nc) {
      const wb_v v = vd[i];
      r.verdict = v.bits & (RGB_WAL_V_MASK | RGB_WAL_V_TRUNC | RGB_WAL_V_FIRST);
      r.value = v.value;
      if ((v.bits & RGB_WAL_V_MASK) == RGB_WAL_V_WRITE) {
        const rgb_wal_cmd cm = cmds[i];
        const rgb_wal_writer wd = writers[cm.writer];
        const wb_pre p = pre[i];
        const bool first = (v.bits & RGB_WAL_V_FIRST) != 0u;
        u32 id_ref = wd.id_ref;
        if (first) id_ref = fl.next_id_ref + p.firsts;
        else if (id_ref == RGB_WAL_NO_ID_REF) id_ref = fl.next_id_ref + pre[wfirst[cm.writer]].firsts;
        wb_frec f;
        f.index = cm.index; f.term = cm.term; f.data_offset = cm.data_offset; f.data_len = cm.data_len;
        f.uid_offset = wd.uid_offset; f.uid_len = first ? wd.uid_len : 0u; f.out_offset = p.real; f.cmd = (u32)i;
        f.hdr3 = ((v.bits & RGB_WAL_V_TRUNC) ? 1u << 23 : 0u) | (first ? 0u : 1u << 22) | (id_ref & 0x3FFFFFu);
        f._pad = 0ull;
        frecs[p.writes] = f;
        r.value = p.real;
      }
    }
    results[i] = r;
  }
}

template <int S>
__global__ __launch_bounds__(WB_THREADS) void rgb_wal_batch_events_kernel(
    const rgb_wal_cmd *__restrict__ cmds, const rgb_wal_writer *__restrict__ writers, u32 n_writers, u32 per_block,
    const u32 *__restrict__ order, const u32 *__restrict__ wstart, const wb_v *__restrict__ vd,
    const wb_pre *__restrict__ pre, const u32 *__restrict__ wfirst, const rgb_wal_file *__restrict__ file,
    const wb_hdr *__restrict__ hdr, ulonglong2 *pairs, wb_ev *__restrict__ evs, wb_cnt *__restrict__ counts,
    wb_cnt *__restrict__ blk, rgb_wal_writer *__restrict__ writers_out) {
  constexpr u32 SUBS = WB_THREADS / S;
  __shared__ u64 s_idx[WB_THREADS], s_small[WB_THREADS], s_term[WB_THREADS], s_tid[WB_THREADS], s_post[WB_THREADS];
  __shared__ u32 s_bits[WB_THREADS];
  __shared__ u32 s_chunks[SUBS];
  __shared__ u32 s_events, s_pairs;
  const u32 tid = threadIdx.x, sub = tid / (u32)S, ln = tid % (u32)S, s0 = sub * (u32)S;
  const u32 nc = hdr->n_consumed;
  const u32 wb = blockIdx.x * per_block;
  const u32 we = n_writers - wb < per_block ? n_writers : wb + per_block;
  if (tid == 0u) { s_events = 0u; s_pairs = 0u; }
  __syncthreads();
  for (u32 r0 = wb; r0 < we; r0 += SUBS) {                /* the same for every lane */
    const u32 w = r0 + sub;
    const bool have = w < we;
    u32 first = 0, count = 0;
    if (have) { first = wstart[w]; count = wstart[w + 1u] - first; }
    const u32 my_chunks = count / (u32)S + (count % (u32)S ? 1u : 0u);
    if (ln == 0u) s_chunks[sub] = my_chunks;
    __syncthreads();
    u32 iters = 0;
    for (u32 i = 0; i < SUBS; ++i) iters = s_chunks[i] > iters ? s_chunks[i] : iters;
    __syncthreads();
    /* the sub-group's first lane: the running run -- its pairs are p[run_base .. run_base + depth), the top one in
     * (top_f, top_l) until it is pushed down or the run closes -- and the writer's events and pairs so far */
    ulonglong2 *p = pairs + first;
    wb_ev *ev = evs + first;
    u32 n_ev = 0, run_base = 0, depth = 0, last_kind = WB_NONE32;
    u64 top_f = 0, top_l = 0, run_term = 0, run_tid = 0, floor_at = 0, last_post = 0;
    auto close_run = [&]() {
      p[run_base + depth - 1u] = make_ulonglong2(top_f, top_l);
      u32 b = 0;                                          /* ra_seq:floor/2: the run's last index is never below it */
      while (p[run_base + b].y < floor_at) b += 1u;
      if (p[run_base + b].x < floor_at) p[run_base + b].x = floor_at;
      if (b) for (u32 k = 0; k + b < depth; ++k) p[run_base + k] = p[run_base + b + k];
      wb_ev e; e.term = run_term; e.tid = run_tid; e.pair_first = run_base; e.pair_n = depth - b;
      ev[n_ev++] = e;
      run_base += depth - b; depth = 0u;
    };
    for (u32 ch = 0; ch < iters; ++ch) {
      const u32 cbase = ch * (u32)S;
      const u32 n_c = ch >= my_chunks ? 0u : (count - cbase < (u32)S ? count - cbase : (u32)S);
      s_bits[tid] = 0u;                                   /* not consumed */
      if (ln < n_c) {
        const u32 c = order[first + cbase + ln];
        if (c < nc) {
          const rgb_wal_cmd cm = cmds[c];
          const wb_v v = vd[c];
          s_idx[tid] = cm.index; s_small[tid] = cm.smallest_index; s_term[tid] = cm.term; s_tid[tid] = cm.tid;
          s_post[tid] = v.post_prev; s_bits[tid] = v.bits;
        }
      }
      __syncthreads();
      if (ln == 0u) {
        for (u32 j = 0; j < n_c; ++j) {
          const u32 bits = s_bits[s0 + j];
          if (!bits) break;                               /* the consumed commands are a prefix of the writer's */
          last_kind = bits >> WB_KIND_SHIFT; last_post = s_post[s0 + j];
          if ((bits & RGB_WAL_V_MASK) != RGB_WAL_V_WRITE) continue;
          const u64 idx = s_idx[s0 + j];
          if (bits & WB_RUN) {
            if (depth) close_run();
            run_term = s_term[s0 + j]; run_tid = s_tid[s0 + j];
          }
          /* ra_seq:append(Idx, ra_seq:limit(Idx - 1, Seq)) */
          while (depth && top_f >= idx) {
            depth -= 1u;
            if (depth) { const ulonglong2 t = p[run_base + depth - 1u]; top_f = t.x; top_l = t.y; }
          }
          if (depth && top_l >= idx) top_l = idx - 1ull;
          if (depth && top_l + 1ull == idx) {
            top_l = idx;
          } else {
            if (depth) p[run_base + depth - 1u] = make_ulonglong2(top_f, top_l);
            depth += 1u; top_f = top_l = idx;
          }
          floor_at = s_small[s0 + j];
        }
      }
      __syncthreads();
    }
    if (have && ln == 0u) {
      if (depth) close_run();
      wb_cnt c; c.events = n_ev; c.pairs = run_base;
      counts[w] = c;
      if (n_ev) { atomicAdd(&s_events, n_ev); atomicAdd(&s_pairs, run_base); }
      rgb_wal_writer wd = writers[w];
      if (last_kind != WB_NONE32) { wd.state = last_kind; wd.prev_index = last_post; }
      const u32 fc = wfirst[w];
      if (fc < nc) wd.id_ref = file->next_id_ref + pre[fc].firsts;      /* WB_NONE32 is never below nc */
      writers_out[w] = wd;
    }
  }
  __syncthreads();
  if (tid == 0u) { wb_cnt c; c.events = s_events; c.pairs = s_pairs; blk[blockIdx.x] = c; }
}

__global__ __launch_bounds__(WB_THREADS) void rgb_wal_batch_gather_kernel(
    const rgb_wal_cmd *__restrict__ cmds, u32 n, u32 n_writers, u32 per_block, u32 n_blocks,
    const u32 *__restrict__ order, const u32 *__restrict__ wstart, const ulonglong2 *__restrict__ pairs,
    const wb_ev *__restrict__ evs, const wb_cnt *__restrict__ counts, const wb_cnt *__restrict__ blk, wb_cnt *bases,
    u32 events_cap, u32 ranges_cap, wb_hdr *hdr, rgb_wal_event *__restrict__ events_out,
    ulonglong2 *__restrict__ ranges_out, rgb_wal_batch_total *__restrict__ total) {
  __shared__ u32 s_e[WB_THREADS], s_p[WB_THREADS];
  __shared__ u32 s_sum_e, s_sum_p, s_base_e, s_base_p;
  const u32 tid = threadIdx.x;
  if (tid == 0u) s_sum_e = s_sum_p = s_base_e = s_base_p = 0u;
  __syncthreads();
  u32 se = 0, sp = 0, be = 0, bp = 0;
  for (u32 i = tid; i < n_blocks; i += WB_THREADS) {
    const wb_cnt c = blk[i];
    se += c.events; sp += c.pairs;
    if (i < blockIdx.x) { be += c.events; bp += c.pairs; }
  }
  if (se) { atomicAdd(&s_sum_e, se); atomicAdd(&s_sum_p, sp); }
  if (be) { atomicAdd(&s_base_e, be); atomicAdd(&s_base_p, bp); }
  __syncthreads();
  const bool fit = s_sum_e <= events_cap && s_sum_p <= ranges_cap;
  if (blockIdx.x == 0u && tid == 0u) {
    const u32 nc = hdr->n_consumed;
    rgb_wal_batch_total t;
    t.status = !fit || !hdr->store ? RGB_WAL_BATCH_SPACE : nc < n ? RGB_WAL_BATCH_ROLL : RGB_WAL_BATCH_OK;
    t.n_consumed = nc; t.n_written = hdr->n_written; t.n_events = s_sum_e; t.n_ranges = s_sum_p;
    t.next_id_ref = hdr->next_id_ref; t.out_bytes = hdr->out_bytes; t.file_size = hdr->file_size;
    t.entry_count = hdr->entry_count; t._pad[0] = t._pad[1] = 0ull;
    *total = t;
    hdr->status = t.status;
    if (!fit) hdr->store = 0u;                            /* frame follows this launch */
  }
  if (!fit) return;                                       /* the same for every lane of every workgroup */
  const u32 wb = blockIdx.x * per_block;
  if (wb >= n_writers) return;
  const u32 we = n_writers - wb < per_block ? n_writers : wb + per_block;
  u32 run_e = s_base_e, run_p = s_base_p;
  for (u32 base = wb; base < we; base += WB_THREADS) {
    const u32 w = base + tid;
    const bool valid = w < we;
    wb_cnt c; c.events = c.pairs = 0u;
    if (valid) c = counts[w];
    s_e[tid] = c.events; s_p[tid] = c.pairs;
    __syncthreads();
    for (u32 off = 1; off < WB_THREADS; off <<= 1) {
      u32 te = s_e[tid], tp = s_p[tid];
      if (tid >= off) { te += s_e[tid - off]; tp += s_p[tid - off]; }
      __syncthreads();
      s_e[tid] = te; s_p[tid] = tp;
      __syncthreads();
    }
    if (valid) { wb_cnt b; b.events = run_e + s_e[tid] - c.events; b.pairs = run_p + s_p[tid] - c.pairs; bases[w] = b; }
    run_e += s_e[WB_THREADS - 1]; run_p += s_p[WB_THREADS - 1];
    __syncthreads();
  }
  /* the writers' parts of the scratch are one run of positions (the per-writer order): position k belongs to the
   * writer of command order[k] and is the (k - wstart[w])-th event and pair of that writer, if it has that many */
  for (u32 k = wstart[wb] + tid; k < wstart[we]; k += WB_THREADS) {
    const u32 w = cmds[order[k]].writer, rel = k - wstart[w];
    const wb_cnt c = counts[w], b = bases[w];
    if (rel < c.events) {
      const wb_ev e = evs[k];
      rgb_wal_event r;
      r.writer = w; r.range_first = b.pairs + e.pair_first; r.term = e.term; r.tid = e.tid; r.range_n = e.pair_n; r._pad = 0u;
      events_out[b.events + rel] = r;
    }
    if (rel < c.pairs) ranges_out[b.pairs + rel] = pairs[k];
  }
}

/* rgb_wal_frame_kernel's body over the frame records of the consumed WRITE commands.  HeaderData is made in registers:
 * three bytes <<Trunc:1, Form:1, IdRef:22>>, and on a first appearance <<IdDataLen:16>> and the uid copied from the
 * data buffer.  store == 0 (SPACE): everything but the stores into `out`, so that the checksums still come out. */
template <int GROUP>
__global__ __launch_bounds__(WAL_WAVES_PER_BLOCK * 64) void rgb_wal_batch_frame_kernel(
    const wb_frec *__restrict__ recs, const wb_hdr *__restrict__ hdr, const unsigned char *__restrict__ data,
    unsigned char *__restrict__ out, rgb_wal_cmd_result *__restrict__ results, u32 flags) {
  constexpr u32 PER_BLOCK = WAL_WAVES_PER_BLOCK * 64 / GROUP;
  constexpr bool UNI = GROUP == 64;
  constexpr int UNROLL = GROUP == 64 ? WAL_UNROLL : 2;
  const u32 n = hdr->n_written;
  const bool store = hdr->store != 0u;                    /* the same for every lane of every workgroup */
  const u32 lane = threadIdx.x & (GROUP - 1);
  u32 e = blockIdx.x * PER_BLOCK + threadIdx.x / GROUP;
#ifndef RGB_HOST_EMULATION
  if (UNI) e = (u32)__builtin_amdgcn_readfirstlane((int)e);
#endif
  const bool live = e < n;
  wb_frec r;
  r.index = r.term = r.data_offset = r.uid_offset = r.out_offset = 0; r.data_len = r.hdr3 = r.uid_len = r.cmd = 0;
  if (live) r = recs[e];
  const u32 len = r.data_len;
  const u32 hdr_len = (r.hdr3 & (1u << 22)) ? 3u : 5u + r.uid_len;
  unsigned char *rec = out + r.out_offset;
  unsigned char *dst = rec + hdr_len + 24u;
  const unsigned char *pay = data + r.data_offset;
  const unsigned char *uid = data + r.uid_offset;
  const u32 n_full = live ? len >> 4 : 0u, rem = live ? len & 15u : 0u;
  const u32 len_q = len % ADLER_MOD;
  u32 a_acc = 0, b_acc = 0;
  constexpr u32 STEP = (16u * GROUP) % ADLER_MOD;
  u32 wq = (len_q + 2u * ADLER_MOD - ((lane << 4) % ADLER_MOD) - 16u) % ADLER_MOD;
  for (u32 j0 = 0; j0 < n_full; j0 += GROUP * UNROLL) {
    uint4 v[UNROLL];
#pragma unroll
    for (int k = 0; k < UNROLL; ++k) {
      const u32 j = j0 + (u32)k * GROUP + lane;
      v[k] = make_uint4(0, 0, 0, 0);
      if (j < n_full) {
        const v4u t = __builtin_nontemporal_load(reinterpret_cast<const v4u_any *>(pay + ((size_t)j << 4)));
        v[k] = make_uint4(t.x, t.y, t.z, t.w);
      }
    }
#pragma unroll
    for (int k = 0; k < UNROLL; ++k) {
      const u32 j = j0 + (u32)k * GROUP + lane;
      if (j < n_full) {
        v4u t; t.x = v[k].x; t.y = v[k].y; t.z = v[k].z; t.w = v[k].w;
        if (store) {
#if defined(RGB_HOST_EMULATION)
          *reinterpret_cast<v4u_any *>(dst + ((size_t)j << 4)) = t;
#else
          if (UNI) __builtin_nontemporal_store(t, reinterpret_cast<v4u_any *>(dst + ((size_t)j << 4)));
          else *reinterpret_cast<v4u_any *>(dst + ((size_t)j << 4)) = t;
#endif
        }
        u32 a, b;
        chunk_sums(v[k], a, b);
        a_acc += a;
        b_acc += (wq * a + b) % ADLER_MOD;
        if (b_acc >= WAL_FOLD_AT) b_acc %= ADLER_MOD;
        if (a_acc >= WAL_FOLD_AT) a_acc %= ADLER_MOD;
      }
      wq = wq >= STEP ? wq - STEP : wq + (ADLER_MOD - STEP);
    }
  }
  if (rem && lane == (n_full & (GROUP - 1))) {
    uint4 w = make_uint4(0, 0, 0, 0);
    if (n_full) {
      const v4u t = __builtin_nontemporal_load(reinterpret_cast<const v4u_any *>(pay + (len - 16u)));
      if (store) *reinterpret_cast<v4u_any *>(dst + (len - 16u)) = t;
      w = keep_bytes(make_uint4(t.x, t.y, t.z, t.w), 16u - rem, 16u);
    } else {
      u64 lo = 0, hi = 0;
      for (u32 k = 0; k < rem; ++k) {
        const u32 c = pay[k], q = 16u - rem + k;
        if (store) dst[k] = (unsigned char)c;
        if (q < 8u) lo |= (u64)c << (8u * q); else hi |= (u64)c << (8u * (q - 8u));
      }
      w = make_uint4((u32)lo, (u32)(lo >> 32), (u32)hi, (u32)(hi >> 32));
    }
    u32 a, b;
    chunk_sums(w, a, b);
    a_acc += a; b_acc += b;
  }
  const u32 a_sum = group_sum<GROUP>(a_acc % ADLER_MOD);
  const u32 b_sum = group_sum<GROUP>(b_acc % ADLER_MOD);
  if (!live) return;
  const u32 ih = (u32)(r.index >> 32), il = (u32)r.index, th = (u32)(r.term >> 32), tl = (u32)r.term;
  u32 pa = dot4(ih, 0x01010101u, 0); pa = dot4(il, 0x01010101u, pa);
  pa = dot4(th, 0x01010101u, pa); pa = dot4(tl, 0x01010101u, pa);
  u32 pb = dot4(ih, 0x100F0E0Du, 0); pb = dot4(il, 0x0C0B0A09u, pb);
  pb = dot4(th, 0x08070605u, pb); pb = dot4(tl, 0x04030201u, pb);
  const u32 A = (1u + pa + a_sum) % ADLER_MOD;
  const u32 B = ((16u + len_q) + (len_q * pa + pb) % ADLER_MOD + b_sum) % ADLER_MOD;
  const u32 cs = (flags & RGB_WAL_NO_CHECKSUMS) ? 0u : ((B << 16) | A);
  if (lane == 0u) results[r.cmd].checksum = cs;
  if (!store) return;
  /* the header bytes: lanes 0..2 the three, lanes 3..4 the uid's length, then the uid a byte per lane */
  const u64 head = ((u64)(r.hdr3 & 0xFFFFFFu) << 16) | (r.uid_len & 0xFFFFu);   /* the five bytes, big endian */
  if (lane < (hdr_len < 5u ? hdr_len : 5u)) rec[lane] = (unsigned char)(head >> (8u * (4u - lane)));
  for (u32 j = lane; j < r.uid_len; j += GROUP) rec[5u + j] = uid[j];
  if (lane == 0u) {
    struct __attribute__((packed)) fixed24 { v4u a; u64 b; };
    fixed24 fx;
    fx.a.x = __builtin_bswap32(cs); fx.a.y = __builtin_bswap32(len);
    fx.a.z = __builtin_bswap32(ih); fx.a.w = __builtin_bswap32(il);
    fx.b = (u64)__builtin_bswap32(th) | ((u64)__builtin_bswap32(tl) << 32);
    __builtin_memcpy(rec + hdr_len, &fx, 24);
  }
}

}  // namespace

/* the context only supplies the default stream; rgb_api.hip exports the accessor */
extern "C" void *rgb_ctx_stream(rgb_ctx *ctx);
extern "C" int rgb_ctx_device(rgb_ctx *ctx);          /* the HIP device the context (and its stream) lives on */

/* off + len <= bytes without the u64 wrap-around of the sum (descriptors come from the caller) */
static inline bool wal_slice_ok(uint64_t off, uint64_t len, uint64_t bytes) { return off <= bytes && len <= bytes - off; }

extern "C" int rgb_wal_adler32_device(rgb_ctx *ctx, const void *d_entries, uint32_t n, const void *d_data,
                                      uint64_t data_bytes, void *d_checksums, void *stream) {
  if (!ctx || (n && (!d_entries || !d_checksums))) return RGB_E_INVAL;
  if (n == 0) return RGB_OK;
  hipStream_t st = stream ? (hipStream_t)stream : (hipStream_t)rgb_ctx_stream(ctx);
  (void)hipGetLastError();   /* a stale error of an earlier call in this thread is not this launch's */
  /* lanes per entry by the batch's mean payload: four entries per wavefront below 1 KiB */
  if (data_bytes / n < 1024u) {
    const u32 per = WAL_WAVES_PER_BLOCK * 64 / 16;
    hipLaunchKernelGGL(rgb_wal_adler32_kernel<16>, dim3((n + per - 1) / per), dim3(WAL_WAVES_PER_BLOCK * 64), 0, st,
                       (const rgb_wal_entry *)d_entries, n, (const unsigned char *)d_data, (u32 *)d_checksums);
  } else {
    const u32 per = WAL_WAVES_PER_BLOCK;
    hipLaunchKernelGGL(rgb_wal_adler32_kernel<64>, dim3((n + per - 1) / per), dim3(WAL_WAVES_PER_BLOCK * 64), 0, st,
                       (const rgb_wal_entry *)d_entries, n, (const unsigned char *)d_data, (u32 *)d_checksums);
  }
  return hipGetLastError() == hipSuccess ? RGB_OK : RGB_E_HIP;
}

extern "C" int rgb_wal_frame_device(rgb_ctx *ctx, const void *d_records, uint32_t n, const void *d_data,
                                    uint64_t data_bytes, void *d_out, uint64_t out_bytes, void *d_checksums,
                                    uint32_t flags, void *stream) {
  if (!ctx || (n && (!d_records || !d_out)) || (flags & ~RGB_WAL_NO_CHECKSUMS)) return RGB_E_INVAL;
  if (n == 0) return RGB_OK;
  if (out_bytes < 27ull * n) return RGB_E_INVAL;       /* the shortest record is 3 + 24 bytes */
  hipStream_t st = stream ? (hipStream_t)stream : (hipStream_t)rgb_ctx_stream(ctx);
  (void)hipGetLastError();   /* a stale error of an earlier call in this thread is not this launch's */
  /* lanes per record by the batch's mean payload: the per-record work that does not shrink with the payload --
   * descriptor, reduction, prefix -- is paid per WAVEFRONT instruction */
#define WAL_LAUNCH_FRAME(G)                                                                                          \
  hipLaunchKernelGGL(rgb_wal_frame_kernel<G>, dim3((n + (WAL_WAVES_PER_BLOCK * 64 / G) - 1) / (WAL_WAVES_PER_BLOCK * 64 / G)), \
                     dim3(WAL_WAVES_PER_BLOCK * 64), 0, st, (const rgb_wal_record *)d_records, n,                   \
                     (const unsigned char *)d_data, (unsigned char *)d_out, (u32 *)d_checksums, flags)
  if (data_bytes / n <= WAL_FRAME_EIGHT_MAX) WAL_LAUNCH_FRAME(8);
  else if (data_bytes / n < 1024u) WAL_LAUNCH_FRAME(16);
  else WAL_LAUNCH_FRAME(64);
#undef WAL_LAUNCH_FRAME
  return hipGetLastError() == hipSuccess ? RGB_OK : RGB_E_HIP;
}

/* ---- host-buffer form: staging buffers live beside the context (keyed by it), grown on demand ---- */
#include <string.h>
#include <mutex>
#include <unordered_map>
#include <vector>
namespace {
struct wal_stage {
  void *d_entries = nullptr; void *d_data = nullptr; void *d_out = nullptr; size_t cap_e = 0, cap_d = 0;
  void *d_records = nullptr; void *d_frame = nullptr; size_t cap_r = 0, cap_f = 0;   /* rgb_wal_frame */
  /* rgb_wal_batch: the host arrays of a call on their way up (`h` pinned, `d_up` its device copy; `done` is recorded
   * behind the upload and the next call waits for it before it refills `h`), the scratch, the host-buffer form's rows */
  void *h = nullptr; void *d_up = nullptr; void *d_work = nullptr; void *d_rows = nullptr;
  size_t cap_h = 0, cap_up = 0, cap_work = 0, cap_rows = 0;
  hipEvent_t done = nullptr;
  bool recorded = false;
};
std::mutex g_stage_mu;
std::unordered_map<rgb_ctx *, wal_stage> g_stage;
int grow(void **p, size_t *cap, size_t need) {
  if (need <= *cap) return 0;
  if (*p) (void)hipFree(*p);
  *p = nullptr; *cap = 0;
  const size_t want = need + need / 2 + 4096;
  if (hipMalloc(p, want) != hipSuccess) return -1;
  *cap = want;
  return 0;
}
}  // namespace

extern "C" void rgb_wal_release(rgb_ctx *ctx) {      /* called by rgb_close */
  std::lock_guard<std::mutex> lk(g_stage_mu);
  auto it = g_stage.find(ctx);
  if (it == g_stage.end()) return;
  if (it->second.d_entries) (void)hipFree(it->second.d_entries);
  if (it->second.d_data) (void)hipFree(it->second.d_data);
  if (it->second.d_out) (void)hipFree(it->second.d_out);
  if (it->second.d_records) (void)hipFree(it->second.d_records);
  if (it->second.d_frame) (void)hipFree(it->second.d_frame);
  if (it->second.d_up) (void)hipFree(it->second.d_up);
  if (it->second.d_work) (void)hipFree(it->second.d_work);
  if (it->second.d_rows) (void)hipFree(it->second.d_rows);
  if (it->second.h) (void)hipHostFree(it->second.h);
  if (it->second.done) (void)hipEventDestroy(it->second.done);
  g_stage.erase(it);
}

extern "C" int rgb_wal_adler32(rgb_ctx *ctx, const rgb_wal_entry *entries, uint32_t n, const void *data,
                               uint64_t data_bytes, uint32_t *checksums) {
  if (!ctx || (n && (!entries || !checksums)) || (data_bytes && !data)) return RGB_E_INVAL;
  if (n == 0) return RGB_OK;
  for (uint32_t i = 0; i < n; ++i)
    if (!wal_slice_ok(entries[i].data_offset, entries[i].data_len, data_bytes)) return RGB_E_INVAL;
  /* a dirty-scheduler thread or a multi-context process: allocations must land on the context's device */
  if (hipSetDevice(rgb_ctx_device(ctx)) != hipSuccess) return RGB_E_HIP;
  std::lock_guard<std::mutex> lk(g_stage_mu);
  wal_stage &s = g_stage[ctx];
  size_t cap_o = s.cap_e / sizeof(rgb_wal_entry) * sizeof(u32);
  const size_t need_e = (size_t)n * sizeof(rgb_wal_entry);
  if (need_e > s.cap_e) {
    if (s.d_out) { (void)hipFree(s.d_out); s.d_out = nullptr; }
    if (grow(&s.d_entries, &s.cap_e, need_e)) return RGB_E_NOMEM;
    cap_o = s.cap_e / sizeof(rgb_wal_entry) * sizeof(u32);
    if (hipMalloc(&s.d_out, cap_o) != hipSuccess) return RGB_E_NOMEM;
  }
  if (grow(&s.d_data, &s.cap_d, (size_t)data_bytes + 16)) return RGB_E_NOMEM;
  hipStream_t st = (hipStream_t)rgb_ctx_stream(ctx);
  if (hipMemcpyAsync(s.d_entries, entries, need_e, hipMemcpyHostToDevice, st) != hipSuccess) return RGB_E_HIP;
  if (data_bytes && hipMemcpyAsync(s.d_data, data, data_bytes, hipMemcpyHostToDevice, st) != hipSuccess) return RGB_E_HIP;
  int rc = rgb_wal_adler32_device(ctx, s.d_entries, n, s.d_data, data_bytes, s.d_out, st);
  if (rc) return rc;
  if (hipMemcpyAsync(checksums, s.d_out, (size_t)n * sizeof(u32), hipMemcpyDeviceToHost, st) != hipSuccess) return RGB_E_HIP;
  return hipStreamSynchronize(st) == hipSuccess ? RGB_OK : RGB_E_HIP;
}

extern "C" int rgb_wal_frame(rgb_ctx *ctx, const rgb_wal_record *records, uint32_t n, const void *data,
                             uint64_t data_bytes, void *out, uint64_t out_bytes, uint32_t flags) {
  if (!ctx || (n && (!records || !out)) || (data_bytes && !data)) return RGB_E_INVAL;
  if (n == 0) return RGB_OK;
  /* every slice inside its buffer, records ascending and disjoint in the output */
  uint64_t floor_off = 0;
  for (uint32_t i = 0; i < n; ++i) {
    const rgb_wal_record &r = records[i];
    if (!wal_slice_ok(r.data_offset, r.data_len, data_bytes) || !wal_slice_ok(r.hdr_offset, r.hdr_len, data_bytes))
      return RGB_E_INVAL;
    if (r.hdr_len < 3u || r.out_offset < floor_off) return RGB_E_INVAL;
    const uint64_t rec_len = (uint64_t)r.hdr_len + 24u + (uint64_t)r.data_len;   /* u32 + u32 + 24: no wrap */
    if (!wal_slice_ok(r.out_offset, rec_len, out_bytes)) return RGB_E_INVAL;
    floor_off = r.out_offset + rec_len;
  }
  if (hipSetDevice(rgb_ctx_device(ctx)) != hipSuccess) return RGB_E_HIP;
  std::lock_guard<std::mutex> lk(g_stage_mu);
  wal_stage &s = g_stage[ctx];
  const size_t need_r = (size_t)n * sizeof(rgb_wal_record);
  if (grow(&s.d_records, &s.cap_r, need_r)) return RGB_E_NOMEM;
  if (grow(&s.d_data, &s.cap_d, (size_t)data_bytes + 16)) return RGB_E_NOMEM;
  if (grow(&s.d_frame, &s.cap_f, (size_t)out_bytes + 16)) return RGB_E_NOMEM;
  hipStream_t st = (hipStream_t)rgb_ctx_stream(ctx);
  if (hipMemcpyAsync(s.d_records, records, need_r, hipMemcpyHostToDevice, st) != hipSuccess) return RGB_E_HIP;
  if (data_bytes && hipMemcpyAsync(s.d_data, data, data_bytes, hipMemcpyHostToDevice, st) != hipSuccess) return RGB_E_HIP;
  /* gaps between records (none when laid out by rgb_wal_layout) read back as zeros */
  if (hipMemsetAsync(s.d_frame, 0, out_bytes, st) != hipSuccess) return RGB_E_HIP;
  int rc = rgb_wal_frame_device(ctx, s.d_records, n, s.d_data, data_bytes, s.d_frame, out_bytes, nullptr, flags, st);
  if (rc) return rc;
  if (hipMemcpyAsync(out, s.d_frame, out_bytes, hipMemcpyDeviceToHost, st) != hipSuccess) return RGB_E_HIP;
  return hipStreamSynchronize(st) == hipSuccess ? RGB_OK : RGB_E_HIP;
}

/* ---- WAL batch: staging, scratch and the seven launches ------------------------------------------------------ */
extern "C" int rgb_wal_batch_check(const rgb_wal_cmd *cmds, uint32_t n, const rgb_wal_writer *writers, uint32_t n_writers,
                                   const rgb_wal_file *file, uint64_t data_bytes, uint32_t flags, uint32_t *order,
                                   uint32_t *wstart, uint64_t *payload_bytes, uint64_t *header_bytes, uint32_t *longest);
namespace {
inline size_t wb_align(size_t v) { return (v + 15u) & ~(size_t)15u; }

/* called with g_stage_mu held; every pointer but cmds / writers / file is device memory */
int wal_batch_enqueue(wal_stage &s, const rgb_wal_cmd *cmds, u32 n, const rgb_wal_writer *writers, u32 n_writers,
                      const rgb_wal_file *file, const void *d_data, u64 data_bytes, u32 flags, void *d_results,
                      void *d_writers_out, void *d_out, u64 out_bytes, void *d_events, u32 events_cap, void *d_ranges,
                      u32 ranges_cap, void *d_total, hipStream_t st) {
  if (!d_total || !file || (n && (!cmds || !d_results)) || (n_writers && (!writers || !d_writers_out)) ||
      (out_bytes && !d_out) || (events_cap && !d_events) || (ranges_cap && !d_ranges) || (data_bytes && !d_data))
    return RGB_E_INVAL;
  /* the upload: commands, writers, file, the per-writer order, the writers' starts, and (n == 0) the total row */
  const size_t o_cmds = 0, o_writers = o_cmds + wb_align((size_t)n * sizeof(rgb_wal_cmd));
  const size_t o_file = o_writers + wb_align((size_t)n_writers * sizeof(rgb_wal_writer));
  const size_t o_order = o_file + wb_align(sizeof(rgb_wal_file));
  const size_t o_wstart = o_order + wb_align((size_t)n * sizeof(u32));
  const size_t o_total = o_wstart + wb_align(((size_t)n_writers + 1u) * sizeof(u32));
  const size_t up_bytes = o_total + wb_align(sizeof(rgb_wal_batch_total));
  if (!s.done && hipEventCreateWithFlags(&s.done, hipEventDisableTiming) != hipSuccess) return RGB_E_HIP;
  if (s.recorded && hipEventSynchronize(s.done) != hipSuccess) return RGB_E_HIP;
  s.recorded = false;
  if (up_bytes > s.cap_h) {
    if (s.h) (void)hipHostFree(s.h);
    s.h = nullptr; s.cap_h = 0;
    if (hipHostMalloc(&s.h, up_bytes * 2u, hipHostMallocDefault) != hipSuccess) return RGB_E_NOMEM;
    s.cap_h = up_bytes * 2u;
  }
  unsigned char *h = (unsigned char *)s.h;
  uint64_t payload = 0;
  uint32_t longest = 0;
  const int rc = rgb_wal_batch_check(cmds, n, writers, n_writers, file, data_bytes, flags, (u32 *)(h + o_order),
                                     (u32 *)(h + o_wstart), &payload, nullptr, &longest);
  if (rc) return rc;                                     /* nothing has been enqueued */
  if (n) memcpy(h + o_cmds, cmds, (size_t)n * sizeof(rgb_wal_cmd));
  if (n_writers) memcpy(h + o_writers, writers, (size_t)n_writers * sizeof(rgb_wal_writer));
  memcpy(h + o_file, file, sizeof(rgb_wal_file));
  rgb_wal_batch_total empty;
  memset(&empty, 0, sizeof empty);
  empty.status = RGB_WAL_BATCH_OK; empty.next_id_ref = file->next_id_ref;
  empty.file_size = file->file_size; empty.entry_count = file->entry_count;
  memcpy(h + o_total, &empty, sizeof empty);
  if (grow(&s.d_up, &s.cap_up, up_bytes)) return RGB_E_NOMEM;
  if (hipMemcpyAsync(s.d_up, h, up_bytes, hipMemcpyHostToDevice, st) != hipSuccess) return RGB_E_HIP;
  if (hipEventRecord(s.done, st) != hipSuccess) return RGB_E_HIP;
  s.recorded = true;
  unsigned char *up = (unsigned char *)s.d_up;
  const rgb_wal_cmd *d_cmds = (const rgb_wal_cmd *)(up + o_cmds);
  const rgb_wal_writer *d_writers = (const rgb_wal_writer *)(up + o_writers);
  const rgb_wal_file *d_file = (const rgb_wal_file *)(up + o_file);
  const u32 *d_order = (const u32 *)(up + o_order), *d_wstart = (const u32 *)(up + o_wstart);
  if (n == 0) {                                          /* nothing to decide: the writers and the file as they came */
    if (n_writers && hipMemcpyAsync(d_writers_out, d_writers, (size_t)n_writers * sizeof(rgb_wal_writer),
                                    hipMemcpyDeviceToDevice, st) != hipSuccess) return RGB_E_HIP;
    if (hipMemcpyAsync(d_total, up + o_total, sizeof(rgb_wal_batch_total), hipMemcpyDeviceToDevice, st) != hipSuccess)
      return RGB_E_HIP;
    return RGB_OK;
  }
  /* the grids: writers S lanes each by the longest writer, commands in tiles of WB_THREADS */
  const u32 S = longest <= 8u ? 8u : longest <= 16u ? 16u : 64u;
  const u32 subs = WB_THREADS / S;
  u32 w_blocks = (n_writers + subs - 1u) / subs;
  if (w_blocks > WB_GRID_CAP) w_blocks = WB_GRID_CAP;
  const u32 w_per = (n_writers + w_blocks - 1u) / w_blocks;
  w_blocks = (n_writers + w_per - 1u) / w_per;
  const u32 tiles = (n + WB_THREADS - 1u) / WB_THREADS;
  u32 c_blocks = tiles > WB_GRID_CAP ? WB_GRID_CAP : tiles;
  const u32 c_per = (tiles + c_blocks - 1u) / c_blocks * WB_THREADS;       /* commands per workgroup: whole tiles */
  c_blocks = (u32)(((u64)n + c_per - 1u) / c_per);
  /* the scratch */
  const size_t k_hdr = 0, k_vd = k_hdr + wb_align(sizeof(wb_hdr)), k_pre = k_vd + wb_align((size_t)n * sizeof(wb_v));
  const size_t k_blk = k_pre + wb_align(((size_t)n + 1u) * sizeof(wb_pre));
  const size_t k_wfirst = k_blk + wb_align((size_t)c_blocks * sizeof(wb_pre));
  const size_t k_frec = k_wfirst + wb_align((size_t)n_writers * sizeof(u32));
  const size_t k_pairs = k_frec + wb_align((size_t)n * sizeof(wb_frec));
  const size_t k_evs = k_pairs + wb_align((size_t)n * sizeof(ulonglong2));
  const size_t k_counts = k_evs + wb_align((size_t)n * sizeof(wb_ev));
  const size_t k_bases = k_counts + wb_align((size_t)n_writers * sizeof(wb_cnt));
  const size_t k_wblk = k_bases + wb_align((size_t)n_writers * sizeof(wb_cnt));
  const size_t work_bytes = k_wblk + wb_align((size_t)w_blocks * sizeof(wb_cnt));
  if (grow(&s.d_work, &s.cap_work, work_bytes)) return RGB_E_NOMEM;
  unsigned char *k = (unsigned char *)s.d_work;
  wb_hdr *hdr = (wb_hdr *)(k + k_hdr);
  wb_v *vd = (wb_v *)(k + k_vd);
  wb_pre *pre = (wb_pre *)(k + k_pre), *blk = (wb_pre *)(k + k_blk);
  u32 *wfirst = (u32 *)(k + k_wfirst);
  wb_frec *frecs = (wb_frec *)(k + k_frec);
  ulonglong2 *pairs = (ulonglong2 *)(k + k_pairs);
  wb_ev *evs = (wb_ev *)(k + k_evs);
  wb_cnt *counts = (wb_cnt *)(k + k_counts), *bases = (wb_cnt *)(k + k_bases), *wblk = (wb_cnt *)(k + k_wblk);
  (void)hipGetLastError();   /* a stale error of an earlier call in this thread is not this launch's */
#define WB_BY_WIDTH(W, LAUNCH) do { if ((W) == 8u) { LAUNCH(8); } else if ((W) == 16u) { LAUNCH(16); } else { LAUNCH(64); } } while (0)
#define WB_VERDICT(SS)                                                                                                \
  hipLaunchKernelGGL(rgb_wal_batch_verdict_kernel<SS>, dim3(w_blocks), dim3(WB_THREADS), 0, st, d_cmds, d_writers,    \
                     n_writers, w_per, d_order, d_wstart, vd, wfirst)
  WB_BY_WIDTH(S, WB_VERDICT);
  hipLaunchKernelGGL(rgb_wal_batch_sum_kernel, dim3(c_blocks), dim3(WB_THREADS), 0, st, d_cmds, n, d_writers,
                     (const wb_v *)vd, c_per, blk, hdr);
  hipLaunchKernelGGL(rgb_wal_batch_place_kernel, dim3(c_blocks), dim3(WB_THREADS), 0, st, d_cmds, n, d_writers,
                     (const wb_v *)vd, c_per, (const wb_pre *)blk, d_file, pre, hdr);
  hipLaunchKernelGGL(rgb_wal_batch_rows_kernel, dim3(tiles > WB_GRID_CAP ? WB_GRID_CAP : tiles), dim3(WB_THREADS), 0, st,
                     d_cmds, n, d_writers, (const wb_v *)vd, (const wb_pre *)pre, (const u32 *)wfirst, d_file,
                     (u64)out_bytes, hdr, frecs, (rgb_wal_cmd_result *)d_results);
#define WB_EVENTS(SS)                                                                                                 \
  hipLaunchKernelGGL(rgb_wal_batch_events_kernel<SS>, dim3(w_blocks), dim3(WB_THREADS), 0, st, d_cmds, d_writers,     \
                     n_writers, w_per, d_order, d_wstart, (const wb_v *)vd, (const wb_pre *)pre, (const u32 *)wfirst,  \
                     d_file, (const wb_hdr *)hdr, pairs, evs, counts, wblk, (rgb_wal_writer *)d_writers_out)
  WB_BY_WIDTH(S, WB_EVENTS);
  hipLaunchKernelGGL(rgb_wal_batch_gather_kernel, dim3(w_blocks), dim3(WB_THREADS), 0, st, d_cmds, n, n_writers, w_per,
                     w_blocks, d_order, d_wstart, (const ulonglong2 *)pairs, (const wb_ev *)evs, (const wb_cnt *)counts,
                     (const wb_cnt *)wblk, bases, events_cap, ranges_cap, hdr, (rgb_wal_event *)d_events,
                     (ulonglong2 *)d_ranges, (rgb_wal_batch_total *)d_total);
  /* lanes per record by the batch's mean payload, as rgb_wal_frame_device chooses */
  const u64 mean = payload / n;
  const u32 G = mean <= WAL_FRAME_EIGHT_MAX ? 8u : mean < 1024u ? 16u : 64u;
#define WB_FRAME(GG)                                                                                                  \
  hipLaunchKernelGGL(rgb_wal_batch_frame_kernel<GG>,                                                                  \
                     dim3((n + (WAL_WAVES_PER_BLOCK * 64 / GG) - 1) / (WAL_WAVES_PER_BLOCK * 64 / GG)),              \
                     dim3(WAL_WAVES_PER_BLOCK * 64), 0, st, (const wb_frec *)frecs, (const wb_hdr *)hdr,              \
                     (const unsigned char *)d_data, (unsigned char *)d_out, (rgb_wal_cmd_result *)d_results, flags)
  WB_BY_WIDTH(G, WB_FRAME);
#undef WB_FRAME
#undef WB_EVENTS
#undef WB_VERDICT
#undef WB_BY_WIDTH
  return hipGetLastError() == hipSuccess ? RGB_OK : RGB_E_HIP;
}
}  // namespace

extern "C" int rgb_wal_batch_device(rgb_ctx *ctx, const rgb_wal_cmd *cmds, uint32_t n, const rgb_wal_writer *writers,
                                    uint32_t n_writers, const rgb_wal_file *file, const void *d_data, uint64_t data_bytes,
                                    uint32_t flags, void *d_results, void *d_writers_out, void *d_out, uint64_t out_bytes,
                                    void *d_events, uint32_t events_cap, void *d_ranges, uint32_t ranges_cap,
                                    void *d_total, void *stream) {
  if (!ctx) return RGB_E_INVAL;
  if (hipSetDevice(rgb_ctx_device(ctx)) != hipSuccess) return RGB_E_HIP;
  hipStream_t st = stream ? (hipStream_t)stream : (hipStream_t)rgb_ctx_stream(ctx);
  std::lock_guard<std::mutex> lk(g_stage_mu);
  return wal_batch_enqueue(g_stage[ctx], cmds, n, writers, n_writers, file, d_data, data_bytes, flags, d_results,
                           d_writers_out, d_out, out_bytes, d_events, events_cap, d_ranges, ranges_cap, d_total, st);
}

extern "C" int rgb_wal_batch(rgb_ctx *ctx, const rgb_wal_cmd *cmds, uint32_t n, const rgb_wal_writer *writers,
                             uint32_t n_writers, const rgb_wal_file *file, const void *data, uint64_t data_bytes,
                             uint32_t flags, rgb_wal_cmd_result *results, rgb_wal_writer *writers_out, void *out,
                             uint64_t out_bytes, rgb_wal_event *events, uint32_t events_cap, uint64_t *ranges,
                             uint32_t ranges_cap, rgb_wal_batch_total *total) {
  if (!ctx || !total || !file || (n && (!cmds || !results)) || (n_writers && (!writers || !writers_out)) ||
      (out_bytes && !out) || (events_cap && !events) || (ranges_cap && !ranges) || (data_bytes && !data))
    return RGB_E_INVAL;
  /* refuse before anything is staged (the device form validates again, into its upload) */
  int rc = rgb_wal_batch_check(cmds, n, writers, n_writers, file, data_bytes, flags, nullptr, nullptr, nullptr, nullptr,
                               nullptr);
  if (rc) return rc;
  if (hipSetDevice(rgb_ctx_device(ctx)) != hipSuccess) return RGB_E_HIP;
  std::lock_guard<std::mutex> lk(g_stage_mu);
  wal_stage &s = g_stage[ctx];
  hipStream_t st = (hipStream_t)rgb_ctx_stream(ctx);
  /* the rows that come down, in one block: total, results, writers, events, ranges */
  const size_t r_total = 0, r_results = r_total + wb_align(sizeof(rgb_wal_batch_total));
  const size_t r_writers = r_results + wb_align((size_t)n * sizeof(rgb_wal_cmd_result));
  const size_t r_events = r_writers + wb_align((size_t)n_writers * sizeof(rgb_wal_writer));
  const size_t r_ranges = r_events + wb_align((size_t)events_cap * sizeof(rgb_wal_event));
  const size_t rows_bytes = r_ranges + wb_align((size_t)ranges_cap * 16u);
  if (grow(&s.d_rows, &s.cap_rows, rows_bytes)) return RGB_E_NOMEM;
  if (grow(&s.d_data, &s.cap_d, (size_t)data_bytes + 16)) return RGB_E_NOMEM;
  if (grow(&s.d_frame, &s.cap_f, (size_t)out_bytes + 16)) return RGB_E_NOMEM;
  if (data_bytes && hipMemcpyAsync(s.d_data, data, data_bytes, hipMemcpyHostToDevice, st) != hipSuccess) return RGB_E_HIP;
  unsigned char *d = (unsigned char *)s.d_rows;
  rc = wal_batch_enqueue(s, cmds, n, writers, n_writers, file, s.d_data, data_bytes, flags, d + r_results, d + r_writers,
                         s.d_frame, out_bytes, d + r_events, events_cap, d + r_ranges, ranges_cap, d + r_total, st);
  if (rc) return rc;
  rgb_wal_batch_total t;
  if (hipMemcpyAsync(&t, d + r_total, sizeof t, hipMemcpyDeviceToHost, st) != hipSuccess) return RGB_E_HIP;
  if (hipStreamSynchronize(st) != hipSuccess) return RGB_E_HIP;
  if (n && hipMemcpyAsync(results, d + r_results, (size_t)n * sizeof(rgb_wal_cmd_result), hipMemcpyDeviceToHost, st) != hipSuccess)
    return RGB_E_HIP;
  if (n_writers && hipMemcpyAsync(writers_out, d + r_writers, (size_t)n_writers * sizeof(rgb_wal_writer),
                                  hipMemcpyDeviceToHost, st) != hipSuccess) return RGB_E_HIP;
  if (t.n_events <= events_cap && t.n_ranges <= ranges_cap) {
    if (t.n_events && hipMemcpyAsync(events, d + r_events, (size_t)t.n_events * sizeof(rgb_wal_event),
                                     hipMemcpyDeviceToHost, st) != hipSuccess) return RGB_E_HIP;
    if (t.n_ranges && hipMemcpyAsync(ranges, d + r_ranges, (size_t)t.n_ranges * 16u, hipMemcpyDeviceToHost, st) != hipSuccess)
      return RGB_E_HIP;
  }
  if (t.status != RGB_WAL_BATCH_SPACE && t.out_bytes &&
      hipMemcpyAsync(out, s.d_frame, t.out_bytes, hipMemcpyDeviceToHost, st) != hipSuccess) return RGB_E_HIP;
  if (hipStreamSynchronize(st) != hipSuccess) return RGB_E_HIP;
  *total = t;
  return RGB_OK;
}

/* rgb_wal_layout and rgb_wal_scan are plain host code: rgb_wal_host.cpp */

extern "C" int rgb_wal_validate(rgb_ctx *ctx, const void *bytes, uint64_t n_bytes, const rgb_wal_scanned *recs,
                                uint32_t n, uint32_t *n_ok, uint32_t *status) {
  if (!ctx || !n_ok || !status || (n && (!recs || !bytes))) return RGB_E_INVAL;
  *n_ok = n;
  *status = RGB_WAL_CLEAN;
  if (n == 0) return RGB_OK;
  std::vector<rgb_wal_entry> entries(n);
  std::vector<uint32_t> sums(n);
  for (uint32_t i = 0; i < n; ++i) {
    entries[i].index = recs[i].index; entries[i].term = recs[i].term;
    entries[i].data_offset = recs[i].data_offset; entries[i].data_len = recs[i].data_len; entries[i]._pad = 0;
  }
  int rc = rgb_wal_adler32(ctx, entries.data(), n, bytes, n_bytes, sums.data());
  if (rc) return rc;
  const unsigned char *b = (const unsigned char *)bytes;
  for (uint32_t i = 0; i < n; ++i) {
    if (!(recs[i].flags & RGB_WAL_REC_VALIDATE)) continue;
    if (recs[i].checksum == 0 || recs[i].checksum == sums[i]) continue;   /* validate_checksum/4 :1022-1033 */
    /* is_last_record/3 (:994-1010): 104 zero bits behind it, or fewer than 13 bytes to the end */
    *n_ok = i;
    const uint64_t rest = recs[i].next_offset;
    if (rest > n_bytes) return RGB_E_INVAL;               /* a descriptor that points past the file */
    bool last = true;
    if (n_bytes - rest >= 13) {
      for (int k = 0; k < 13; ++k) if (b[rest + k] != 0) { last = false; break; }
    }
    *status = last ? RGB_WAL_DROPPED_LAST : RGB_WAL_CORRUPT;
    return RGB_OK;
  }
  return RGB_OK;
}

/*
 * rgb_segment.hip -- batched CRC-32 (zlib / erlang:crc32: reflected 0xEDB88320, init and final xor 0xFFFFFFFF)
 * for the second half of Ra's storage path (include/ra_gpu_wal.h, "segments and snapshots"):
 *   - per-entry CRC of a batch of payloads          (src/ra_log_segment.erl:277, 670, 1240-1248)
 *   - the whole segment file image in one pass      (src/ra_log_segment.erl:1118-1122, 1211-1219)
 *   - one long buffer with a starting value         (src/ra_log_snapshot.erl:57-107, 256; src/ra_snapshot.erl:1020, 1038)
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
template <bool COPY>
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

/* This lane's share of raw(fold-ed payload), already moved to the end of the payload: the xor over the GROUP lanes
 * is the raw value.  len >= 16 or len == 0 (nothing to do); every lane of the group makes the same number of rounds. */
template <int GROUP, int UNROLL, bool COPY>
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
      if (r0 + (u32)k < rounds) v[k] = load_slot<COPY>(pay, dst, (r0 + (u32)k) * GROUP + lane, pad, fold);
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

/* ---- per-entry CRC, and the segment image around it ------------------------------------------------------
 * GROUP lanes per entry (8 up to a mean payload of 320 bytes, 16 up to 1 KiB, then a wavefront), as the WAL kernels.
 * BUILD: the payload is copied to out + out_offsets[e] as it is read, the group's first lane writes the index record
 * <<Idx:64, Term:64, DataOffset:64, Length:32, Crc:32>> at 8 + 32 e, and the first thread of the grid the file header.
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
  constexpr int UNROLL = GROUP == 64 ? 4 : 2;
  const u32 lane = threadIdx.x & (GROUP - 1);
  if (BUILD && blockIdx.x == 0 && threadIdx.x == 0) {
    /* <<"RASG", 2:16, MaxCount:16>> (src/ra_log_segment.erl:1118-1122) */
    struct __attribute__((packed)) hdr8 { u64 v; } h;
    h.v = 0x47534152ull | (0x0200ull << 32) | ((u64)((max_count >> 8) & 0xFFu) << 48) | ((u64)(max_count & 0xFFu) << 56);
    __builtin_memcpy(out, &h, 8);
  }
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
    const bool wide = live && len >= 16u;
    const u32 part = lane_raw<GROUP, UNROLL, BUILD>(lds, pay, dst, wide ? len : 0u, lane, 0xFFFFFFFFu);
    u32 crc = ~group_xor<GROUP>(part);
    if (live && lane == 0u) {
      if (!wide) crc = crc_bytes(lds, 0u, pay, len, dst);
      if (BUILD) {
        if (flags & RGB_SEG_NO_CHECKSUMS) crc = 0u;
        v4u a, b;
        a.x = __builtin_bswap32((u32)(en.index >> 32)); a.y = __builtin_bswap32((u32)en.index);
        a.z = __builtin_bswap32((u32)(en.term >> 32));  a.w = __builtin_bswap32((u32)en.term);
        b.x = __builtin_bswap32((u32)(dst_off >> 32));  b.y = __builtin_bswap32((u32)dst_off);
        b.z = __builtin_bswap32(len);                   b.w = __builtin_bswap32(crc);
        unsigned char *rec = out + RGB_SEG_HEADER_BYTES + (u64)RGB_SEG_RECORD_BYTES * e;
        *reinterpret_cast<v4u_any *>(rec) = a;
        *reinterpret_cast<v4u_any *>(rec + 16) = b;
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

/* x^(8 n) mod P on the host */
inline u32 host_xpow8(u64 n) { return xpow8_c(n); }

inline bool slice_ok(uint64_t off, uint64_t len, uint64_t bytes) { return off <= bytes && len <= bytes - off; }

}  // namespace seg
}  // namespace

extern "C" void *rgb_ctx_stream(rgb_ctx *ctx);
extern "C" int rgb_ctx_device(rgb_ctx *ctx);

/* ---- per-context device buffers: staging of the host-buffer forms, partial values of the stream form ---- */
#include <mutex>
#include <memory>
#include <unordered_map>
#include <vector>
namespace {
namespace seg {
struct stage {
  void *d_entries = nullptr, *d_data = nullptr, *d_crcs = nullptr, *d_offsets = nullptr, *d_out = nullptr;
  size_t cap_e = 0, cap_d = 0, cap_c = 0, cap_o = 0, cap_out = 0;
  void *d_partials = nullptr;     /* STREAM_MAX_BLOCKS values + the one result of the host-buffer form */
};
std::recursive_mutex g_mu;     /* the host-buffer forms call the device forms with it held */
std::unordered_map<rgb_ctx *, stage> g_stages;
int grow(void **p, size_t *cap, size_t need) {
  if (need <= *cap) return 0;
  if (*p) (void)hipFree(*p);
  *p = nullptr; *cap = 0;
  const size_t want = need + need / 2 + 4096;
  if (hipMalloc(p, want) != hipSuccess) return -1;
  *cap = want;
  return 0;
}
/* the partial values of the context (allocated on the first long buffer) */
u32 *partials_of(rgb_ctx *ctx) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  stage &s = g_stages[ctx];
  if (!s.d_partials && hipMalloc(&s.d_partials, (size_t)(STREAM_MAX_BLOCKS + 1u) * sizeof(u32)) != hipSuccess)
    s.d_partials = nullptr;
  return (u32 *)s.d_partials;
}
}  // namespace seg
}  // namespace

extern "C" void rgb_seg_release(rgb_ctx *ctx) {      /* called by rgb_close */
  std::lock_guard<std::recursive_mutex> lk(seg::g_mu);
  auto it = seg::g_stages.find(ctx);
  if (it == seg::g_stages.end()) return;
  seg::stage &s = it->second;
  void *all[] = {s.d_entries, s.d_data, s.d_crcs, s.d_offsets, s.d_out, s.d_partials};
  for (void *p : all) if (p) (void)hipFree(p);
  seg::g_stages.erase(it);
}

#define SEG_LAUNCH(G, BUILD, ...)                                                                                    \
  do {                                                                                                               \
    const seg::u32 per = seg::THREADS / (G);                                                                         \
    seg::u32 grid = (n + per - 1) / per;                                                                             \
    if (grid > seg::GRID_CAP) grid = seg::GRID_CAP;                                                                  \
    if (grid == 0) grid = 1;                                                                                         \
    hipLaunchKernelGGL((seg::rgb_seg_crc_kernel<G, BUILD>), dim3(grid), dim3(seg::THREADS), 0, st, __VA_ARGS__);     \
  } while (0)

extern "C" int rgb_crc32_device(rgb_ctx *ctx, const void *d_entries, uint32_t n, const void *d_data,
                                uint64_t data_bytes, void *d_crcs, void *stream) {
  if (!ctx || (n && (!d_entries || !d_crcs))) return RGB_E_INVAL;
  if (n == 0) return RGB_OK;
  hipStream_t st = stream ? (hipStream_t)stream : (hipStream_t)rgb_ctx_stream(ctx);
  (void)hipGetLastError();
  const uint64_t mean = data_bytes / n;
#define SEG_CRC_ARGS (const rgb_seg_entry *)d_entries, n, (const unsigned char *)d_data, data_bytes, (seg::u32 *)d_crcs, \
                     (unsigned char *)nullptr, (seg::u64)0, (const seg::u64 *)nullptr, 0u, 0u
  if (mean <= 320u) SEG_LAUNCH(8, false, SEG_CRC_ARGS);
  else if (mean < 1024u) SEG_LAUNCH(16, false, SEG_CRC_ARGS);
  else SEG_LAUNCH(64, false, SEG_CRC_ARGS);
#undef SEG_CRC_ARGS
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
  const uint64_t mean = n ? data_bytes / n : 0;
#define SEG_BUILD_ARGS (const rgb_seg_entry *)d_entries, n, (const unsigned char *)d_data, data_bytes, (seg::u32 *)nullptr, \
                       (unsigned char *)d_out, (seg::u64)out_bytes, (const seg::u64 *)d_out_offsets, max_count, flags
  if (mean <= 320u) SEG_LAUNCH(8, true, SEG_BUILD_ARGS);
  else if (mean < 1024u) SEG_LAUNCH(16, true, SEG_BUILD_ARGS);
  else SEG_LAUNCH(64, true, SEG_BUILD_ARGS);
#undef SEG_BUILD_ARGS
  return hipGetLastError() == hipSuccess ? RGB_OK : RGB_E_HIP;
}
#undef SEG_LAUNCH

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
  for (uint32_t i = 0; i < n; ++i)
    if (!seg::slice_ok(entries[i].data_offset, entries[i].data_len, data_bytes)) return RGB_E_INVAL;
  if (hipSetDevice(rgb_ctx_device(ctx)) != hipSuccess) return RGB_E_HIP;
  std::lock_guard<std::recursive_mutex> lk(seg::g_mu);
  seg::stage &s = seg::g_stages[ctx];
  const size_t need_e = (size_t)n * sizeof(rgb_seg_entry);
  if (seg::grow(&s.d_entries, &s.cap_e, need_e) || seg::grow(&s.d_crcs, &s.cap_c, (size_t)n * 4u) ||
      seg::grow(&s.d_data, &s.cap_d, (size_t)data_bytes))
    return RGB_E_NOMEM;
  hipStream_t st = (hipStream_t)rgb_ctx_stream(ctx);
  if (hipMemcpyAsync(s.d_entries, entries, need_e, hipMemcpyHostToDevice, st) != hipSuccess) return RGB_E_HIP;
  if (data_bytes && hipMemcpyAsync(s.d_data, data, data_bytes, hipMemcpyHostToDevice, st) != hipSuccess) return RGB_E_HIP;
  int rc = rgb_crc32_device(ctx, s.d_entries, n, s.d_data, data_bytes, s.d_crcs, st);
  if (rc) return rc;
  if (hipMemcpyAsync(crcs, s.d_crcs, (size_t)n * 4u, hipMemcpyDeviceToHost, st) != hipSuccess) return RGB_E_HIP;
  return hipStreamSynchronize(st) == hipSuccess ? RGB_OK : RGB_E_HIP;
}

extern "C" int rgb_crc32_stream(rgb_ctx *ctx, const void *data, uint64_t n_bytes, uint32_t init, uint32_t *crc_out) {
  if (!ctx || !crc_out || (n_bytes && !data)) return RGB_E_INVAL;
  if (hipSetDevice(rgb_ctx_device(ctx)) != hipSuccess) return RGB_E_HIP;
  std::lock_guard<std::recursive_mutex> lk(seg::g_mu);
  seg::u32 *partials = seg::partials_of(ctx);
  if (!partials) return RGB_E_NOMEM;
  seg::stage &s = seg::g_stages[ctx];
  if (seg::grow(&s.d_data, &s.cap_d, (size_t)n_bytes)) return RGB_E_NOMEM;
  hipStream_t st = (hipStream_t)rgb_ctx_stream(ctx);
  if (n_bytes && hipMemcpyAsync(s.d_data, data, n_bytes, hipMemcpyHostToDevice, st) != hipSuccess) return RGB_E_HIP;
  seg::u32 *d_crc = partials + seg::STREAM_MAX_BLOCKS;
  int rc = rgb_crc32_stream_device(ctx, s.d_data, n_bytes, init, d_crc, st);
  if (rc) return rc;
  if (hipMemcpyAsync(crc_out, d_crc, 4u, hipMemcpyDeviceToHost, st) != hipSuccess) return RGB_E_HIP;
  return hipStreamSynchronize(st) == hipSuccess ? RGB_OK : RGB_E_HIP;
}

extern "C" int rgb_segment_build(rgb_ctx *ctx, const rgb_seg_entry *entries, uint32_t n, uint32_t max_count,
                                 const void *data, uint64_t data_bytes, void *out, uint64_t out_bytes, uint32_t flags) {
  if (!ctx || !out || (n && !entries) || (data_bytes && !data) || (flags & ~RGB_SEG_NO_CHECKSUMS)) return RGB_E_INVAL;
  if (n > max_count || max_count > 65535u) return RGB_E_INVAL;
  for (uint32_t i = 0; i < n; ++i)
    if (!seg::slice_ok(entries[i].data_offset, entries[i].data_len, data_bytes)) return RGB_E_INVAL;
  std::vector<uint64_t> offs(n ? n : 1);
  const uint64_t total = rgb_segment_layout(entries, n, max_count, offs.data());
  if (out_bytes < total) return RGB_E_INVAL;
  if (hipSetDevice(rgb_ctx_device(ctx)) != hipSuccess) return RGB_E_HIP;
  std::lock_guard<std::recursive_mutex> lk(seg::g_mu);
  seg::stage &s = seg::g_stages[ctx];
  const size_t need_e = (size_t)n * sizeof(rgb_seg_entry);
  if (seg::grow(&s.d_entries, &s.cap_e, need_e) || seg::grow(&s.d_offsets, &s.cap_o, (size_t)n * 8u) ||
      seg::grow(&s.d_data, &s.cap_d, (size_t)data_bytes) || seg::grow(&s.d_out, &s.cap_out, (size_t)total))
    return RGB_E_NOMEM;
  hipStream_t st = (hipStream_t)rgb_ctx_stream(ctx);
  if (n && hipMemcpyAsync(s.d_entries, entries, need_e, hipMemcpyHostToDevice, st) != hipSuccess) return RGB_E_HIP;
  if (n && hipMemcpyAsync(s.d_offsets, offs.data(), (size_t)n * 8u, hipMemcpyHostToDevice, st) != hipSuccess) return RGB_E_HIP;
  if (data_bytes && hipMemcpyAsync(s.d_data, data, data_bytes, hipMemcpyHostToDevice, st) != hipSuccess) return RGB_E_HIP;
  int rc = rgb_segment_build_device(ctx, s.d_entries, n, max_count, s.d_offsets, s.d_data, data_bytes, s.d_out, total,
                                    flags, st);
  if (rc) return rc;
  /* only the file's own bytes come back: `out` behind them is the caller's */
  if (hipMemcpyAsync(out, s.d_out, total, hipMemcpyDeviceToHost, st) != hipSuccess) return RGB_E_HIP;
  return hipStreamSynchronize(st) == hipSuccess ? RGB_OK : RGB_E_HIP;
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

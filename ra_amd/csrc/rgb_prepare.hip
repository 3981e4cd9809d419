/*
 * rgb_prepare.hip -- a batch of rgb_submit_raw / rgb_submit_commit put into device order BY THE DEVICE.
 *
 * rgb_submit does three passes over every message on the calling thread (validation + rounds + bucket key, the
 * bucket counts, the scatter into the pinned slot).  The raw form copies the records to the device as they were
 * submitted and runs the same three steps here, N-independent (the family order rgb_family(kind, flags) has no shard
 * bits):
 *
 *   rgb_prep_scan_kernel      every clause of validate_msg (rgb_api.hip) per record -> the batch's error word; per
 *                             server a counter and the list of its (at most max_rounds) messages, in arrival order of
 *                             the atomics (NOT submission order: the next kernel sorts that out)
 *   rgb_prep_rounds_kernel    a message's round = the entries of its server's list below its own index (exact, in
 *                             submission order); key = round x 32 + family; the (round, family) counts through a
 *                             256-counter LDS histogram per workgroup, one global add per non-empty counter
 *   rgb_prep_scatter_kernel   the bucket bases from the counts (every workgroup scans the 256 totals itself: no
 *                             fourth launch, no waiting between workgroups), a range per (workgroup, bucket) from the
 *                             bucket's cursor, then record -> its position, pos[i], a NOP's empty decision; the
 *                             per-server counters of the batch's servers go back to zero here
 *
 * The layout has host-known bases: round r holds at most floor(n / (r + 1)) messages (every server in it has sent at
 * least r + 1), so round r owns the positions [base_r, base_r + floor(n / (r + 1))), base_r = the bounds in front of
 * it -- rgb_raw_round_base.  Inside its region a round is in family order from the region's first position, which is
 * what rgb_tick_classes_kernel derives from the round's 32 family totals (the counts this file leaves in d_prep).
 * In-bucket order is the order the workgroups reached the cursor: a round holds at most one message per server, so
 * the decisions do not depend on it, and rgb_results_kernel hands everything out by submission index.
 *
 * A refused batch (a record validate_msg refuses, a written event with RGB_MF_SEQX, more than max_rounds messages
 * for one server) applies nothing: the counts stay zero (the round launches find no class), pos[i] = i stays in range
 * for the results kernels, and the code goes to the slot's pinned header.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "rgb_internal.h"

namespace {
namespace prep {

constexpr u32 THREADS = 256u;
static_assert(RGB_PREP_MAX_ROUNDS * RGB_N_FAMILIES == THREADS, "one lane per (round, family) counter");
constexpr u32 KEY_NOP = 30u;                      /* round 0, family 2 x 15: behind every class of round 0 */

struct Rec { u32 server, kind, from, flags; };
__device__ __forceinline__ Rec rec_of(u64 w0) {
  Rec r;
  r.server = (u32)(w0 & 0xFFFFFFFFull); r.kind = (u32)((w0 >> 32) & 0xFFull);
  r.from = (u32)((w0 >> 40) & 0xFFull); r.flags = (u32)((w0 >> 48) & 0xFFull);
  return r;
}
/* the record names a server row: it counts in the per-server scratch (and gives its counter back in the scatter) */
__device__ __forceinline__ bool has_server(const Rec &r, u32 n_servers) {
  return r.kind != RGB_MSG_NOP && r.kind <= RGB_MSG_KIND_MAX && r.server < n_servers;
}

__global__ __launch_bounds__(256) void rgb_prep_scan_kernel(const ulonglong2 *__restrict__ raw, u32 n, u32 n_servers,
                                                            u32 max_rounds, u32 *__restrict__ srv_cnt,
                                                            u32 *__restrict__ srv_list, u32 *__restrict__ prep) {
  const u32 i = blockIdx.x * THREADS + threadIdx.x;
  if (i >= n) return;
  const ulonglong2 m0 = raw[(size_t)i * 4u], m1 = raw[(size_t)i * 4u + 1u], m2 = raw[(size_t)i * 4u + 2u],
                   m3 = raw[(size_t)i * 4u + 3u];
  const Rec r = rec_of(m0.x);
  const u64 a = m1.x, b = m1.y, run0 = m3.x, run1 = m3.y;
  const u32 n_entries = (u32)(m2.y & 0xFFFFFFFFull), n_run0 = (u32)(m2.y >> 32);
  bool bad = r.kind > RGB_MSG_KIND_MAX;
  if (!bad && r.kind != RGB_MSG_NOP) {
    bad = r.server >= n_servers || (r.from != RGB_NONE && r.from >= RGB_MAX_MEMBERS) ||
          (r.kind == RGB_MSG_AER && n_run0 > n_entries);
    if (r.kind == RGB_MSG_WRITTEN) {
      bad = bad || a > b ||
            ((r.flags & RGB_MF_SEQ2) && !(run0 <= run1 && run1 != RGB_UNDEF && run1 + 1ull < a)) ||
            (r.flags & RGB_MF_SEQX);                /* (with or without SEQ2: the raw form carries no range list) */
    }
  }
  if (bad) atomicOr(prep + RGB_PREP_ERR, (u32)RGB_PREP_ERR_INVAL);
  if (has_server(r, n_servers)) {
    const u32 k = atomicAdd(srv_cnt + r.server, 1u);
    if (k < max_rounds) srv_list[(size_t)r.server * RGB_PREP_MAX_ROUNDS + k] = i;
    else atomicOr(prep + RGB_PREP_ERR, (u32)RGB_PREP_ERR_ROUNDS);
  }
}

__global__ __launch_bounds__(256) void rgb_prep_rounds_kernel(const u64 *__restrict__ raw, u32 n, u32 n_servers,
                                                              const u32 *__restrict__ srv_cnt,
                                                              const uint4 *__restrict__ srv_list, u32 *__restrict__ prep,
                                                              unsigned char *__restrict__ key) {
  __shared__ u32 hist[THREADS];
  const u32 tid = threadIdx.x, i = blockIdx.x * THREADS + tid;
  if (prep[RGB_PREP_ERR] != 0u) return;          /* refused (the whole grid sees the same word): the counts stay zero */
  hist[tid] = 0u;
  __syncthreads();
  if (i < n) {
    const Rec r = rec_of(raw[(size_t)i * 8u]);
    u32 k = KEY_NOP;
    if (r.kind != RGB_MSG_NOP) {
      const u32 c = srv_cnt[r.server];             /* <= max_rounds: the batch was not refused */
      const uint4 lo = srv_list[(size_t)r.server * 2u], hi = srv_list[(size_t)r.server * 2u + 1u];
      const u32 l[RGB_PREP_MAX_ROUNDS] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
      u32 round = 0;
#pragma unroll
      for (u32 q = 0; q < RGB_PREP_MAX_ROUNDS; ++q) round += (q < c && l[q] < i) ? 1u : 0u;
      k = round * RGB_N_FAMILIES + rgb_family(r.kind, r.flags);
    }
    key[i] = (unsigned char)k;
    atomicAdd(&hist[k], 1u);
  }
  __syncthreads();
  const u32 h = hist[tid];
  if (h) atomicAdd(prep + RGB_PREP_COUNTS + tid, h);
}

__global__ __launch_bounds__(256) void rgb_prep_scatter_kernel(const ulonglong2 *__restrict__ raw, u32 n, u32 n_servers,
                                                               u32 *__restrict__ srv_cnt, u32 *__restrict__ prep,
                                                               const unsigned char *__restrict__ key,
                                                               ulonglong2 *__restrict__ msgs, ulonglong2 *__restrict__ dec,
                                                               u32 *__restrict__ pos, u32 *__restrict__ code_out) {
  __shared__ u32 cnt[THREADS], base[THREADS], tot[THREADS];
  const u32 tid = threadIdx.x, i = blockIdx.x * THREADS + tid;
  const u32 err = prep[RGB_PREP_ERR];
  ulonglong2 m0 = make_ulonglong2(0, 0), m1 = m0, m2 = m0, m3 = m0;
  Rec r = rec_of(0);
  if (i < n) {
    m0 = raw[(size_t)i * 4u]; m1 = raw[(size_t)i * 4u + 1u]; m2 = raw[(size_t)i * 4u + 2u]; m3 = raw[(size_t)i * 4u + 3u];
    r = rec_of(m0.x);
    if (has_server(r, n_servers)) srv_cnt[r.server] = 0u;       /* the scratch is all-zero behind every batch */
  }
  if (blockIdx.x == 0u && tid == 0u)
    *code_out = (err & RGB_PREP_ERR_INVAL) ? (u32)(-RGB_E_INVAL) : err ? (u32)(-RGB_E_UNSUPPORTED) : 0u;
  if (err != 0u) {                                 /* refused: nothing moves; positions stay in range */
    if (i < n) pos[i] = i;
    return;
  }
  tot[tid] = prep[RGB_PREP_COUNTS + tid];
  cnt[tid] = 0u;
  __syncthreads();
  u32 k = 0, rank = 0;
  if (i < n) { k = key[i]; rank = atomicAdd(&cnt[k], 1u); }
  __syncthreads();
  {
    /* bucket tid = (round, family): the round's region, the families in front of it, this workgroup's range */
    const u32 round = tid / RGB_N_FAMILIES, fam = tid % RGB_N_FAMILIES;
    u32 b = rgb_raw_round_base(n, round);
    for (u32 f = 0; f < fam; ++f) b += tot[round * RGB_N_FAMILIES + f];
    const u32 c = cnt[tid];
    if (c) b += atomicAdd(prep + RGB_PREP_CURSORS + tid, c);
    base[tid] = b;
  }
  __syncthreads();
  if (i < n) {
    const u32 p = base[k] + rank;
    pos[i] = p;
    if (r.kind == RGB_MSG_NOP) {
      /* the empty decision of a NOP slot, as the tick kernel's NOP path makes it: the record's server word, no role,
       * reply_to undefined, everything else zero */
      ulonglong2 *d = dec + (size_t)p * 4u;
      const ulonglong2 z = make_ulonglong2(0ull, 0ull);
      d[0] = make_ulonglong2((u64)r.server | ((u64)RGB_NONE << 40), 0ull);
      d[1] = z; d[2] = z; d[3] = z;
    } else {
      ulonglong2 *d = msgs + (size_t)p * 4u;
      d[0] = m0; d[1] = m1; d[2] = m2; d[3] = m3;
    }
  }
}

}  // namespace prep
}  // namespace

int rgb_launch_prepare(const rgb_dev &dev, const rgb_msg *d_raw, u32 n, u32 max_rounds, u32 *d_srv_cnt, u32 *d_srv_list,
                       u32 *d_prep, unsigned char *d_key, rgb_msg *d_msgs, rgb_decision *d_dec, u32 *d_pos,
                       u32 *code_out, void *stream) {
  (void)hipGetLastError();   /* a stale error of an earlier call in this thread is not this launch's */
  if (n == 0) return 0;
  if (max_rounds < 1u || max_rounds > RGB_PREP_MAX_ROUNDS) return -1;
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(d_prep, 0, RGB_PREP_WORDS * sizeof(u32), st);
  if (e != hipSuccess) return (int)e;
  dim3 grid((n + prep::THREADS - 1u) / prep::THREADS), block(prep::THREADS);
  hipLaunchKernelGGL(prep::rgb_prep_scan_kernel, grid, block, 0, st, reinterpret_cast<const ulonglong2 *>(d_raw), n,
                     dev.n_servers, max_rounds, d_srv_cnt, d_srv_list, d_prep);
  hipLaunchKernelGGL(prep::rgb_prep_rounds_kernel, grid, block, 0, st, reinterpret_cast<const u64 *>(d_raw), n,
                     dev.n_servers, d_srv_cnt, reinterpret_cast<const uint4 *>(d_srv_list), d_prep, d_key);
  hipLaunchKernelGGL(prep::rgb_prep_scatter_kernel, grid, block, 0, st, reinterpret_cast<const ulonglong2 *>(d_raw), n,
                     dev.n_servers, d_srv_cnt, d_prep, d_key, reinterpret_cast<ulonglong2 *>(d_msgs),
                     reinterpret_cast<ulonglong2 *>(d_dec), d_pos, code_out);
  return (int)hipGetLastError();
}

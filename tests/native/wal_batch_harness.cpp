/*
 * wal_batch_harness.cpp -- TEST INFRASTRUCTURE: the host helpers of the WAL batch (rgb_wal_batch_check,
 * rgb_wal_batch_bound in ra_amd/csrc/rgb_wal_host.cpp) in a stand-alone program, built with -fsanitize=address,undefined
 * by tests/test_wal_batch.py.  Random batches in exactly sized heap arrays: every read or write outside them, every
 * overflow and misaligned access stops the program.  The per-writer order is checked against a stable sort.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <numeric>
#include <vector>
#include "ra_gpu_wal.h"

extern "C" int rgb_wal_batch_check(const rgb_wal_cmd *cmds, uint32_t n, const rgb_wal_writer *writers, uint32_t n_writers,
                                   const rgb_wal_file *file, uint64_t data_bytes, uint32_t flags, uint32_t *order,
                                   uint32_t *wstart, uint64_t *payload_bytes, uint64_t *header_bytes, uint32_t *longest);

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
#define CHECK(c) do { if (!(c)) { printf("line %d: %s\n", __LINE__, #c); return 1; } } while (0)

int main() {
  const uint64_t data_bytes = 100000;
  for (int round = 0; round < 200; ++round) {
    const uint32_t n = (uint32_t)(rnd() % 700), W = 1u + (uint32_t)(rnd() % 40);
    /* new[] of the exact size: the sanitizer's red zones sit right behind the last element */
    rgb_wal_cmd *cmds = new rgb_wal_cmd[n ? n : 1]();
    rgb_wal_writer *writers = new rgb_wal_writer[W]();
    uint32_t *order = new uint32_t[n ? n : 1], *wstart = new uint32_t[W + 1u];
    rgb_wal_file file = {};
    file.next_id_ref = (uint32_t)(rnd() % 100);
    uint64_t pay = 0, hdr = 0;
    for (uint32_t w = 0; w < W; ++w) {
      writers[w].state = (uint32_t)(rnd() % 3);
      writers[w].id_ref = rnd() % 2 ? RGB_WAL_NO_ID_REF : (uint32_t)(rnd() % RGB_WAL_MAX_ID_REFS);
      writers[w].uid_len = (uint32_t)(rnd() % 300);
      writers[w].uid_offset = rnd() % (data_bytes - writers[w].uid_len + 1u);
      hdr += 2u + writers[w].uid_len;
    }
    for (uint32_t i = 0; i < n; ++i) {
      cmds[i].writer = (uint32_t)(rnd() % W);
      cmds[i].data_len = (uint32_t)(rnd() % 5000);
      cmds[i].data_offset = rnd() % (data_bytes - cmds[i].data_len + 1u);
      pay += cmds[i].data_len;
    }
    uint64_t got_pay = 0, got_hdr = 0, out_bound = 0;
    uint32_t longest = 0, ev = 0, rg = 0;
    CHECK(rgb_wal_batch_check(cmds, n, writers, W, &file, data_bytes, 0, order, wstart, &got_pay, &got_hdr, &longest) == RGB_OK);
    CHECK(got_pay == pay && got_hdr == hdr);
    std::vector<uint32_t> want(n);
    std::iota(want.begin(), want.end(), 0u);
    std::stable_sort(want.begin(), want.end(), [&](uint32_t a, uint32_t b) { return cmds[a].writer < cmds[b].writer; });
    uint32_t most = 0;
    CHECK(wstart[0] == 0 && wstart[W] == n);
    for (uint32_t w = 0; w < W; ++w) {
      CHECK(wstart[w] <= wstart[w + 1u]);
      most = std::max(most, wstart[w + 1u] - wstart[w]);
      for (uint32_t k = wstart[w]; k < wstart[w + 1u]; ++k) CHECK(order[k] == want[k] && cmds[order[k]].writer == w);
    }
    CHECK(most == longest);
    CHECK(rgb_wal_batch_bound(cmds, n, writers, W, &file, data_bytes, &out_bound, &ev, &rg) == RGB_OK);
    CHECK(out_bound == pay + 27ull * n + hdr && ev == n && rg == n);
    /* every refusal, on a copy of a good batch; nothing may be written */
    if (n) {
      const uint32_t i = (uint32_t)(rnd() % n), w = (uint32_t)(rnd() % W);
      const rgb_wal_cmd c0 = cmds[i];
      const rgb_wal_writer w0 = writers[w];
      uint64_t keep = out_bound;
      cmds[i].writer = W;
      CHECK(rgb_wal_batch_bound(cmds, n, writers, W, &file, data_bytes, &out_bound, &ev, &rg) == RGB_E_INVAL);
      cmds[i] = c0; cmds[i].data_offset = UINT64_MAX - 3u; cmds[i].data_len = 8;      /* the sum wraps around */
      CHECK(rgb_wal_batch_bound(cmds, n, writers, W, &file, data_bytes, &out_bound, &ev, &rg) == RGB_E_INVAL);
      cmds[i] = c0; cmds[i].data_offset = data_bytes; cmds[i].data_len = 1;
      CHECK(rgb_wal_batch_bound(cmds, n, writers, W, &file, data_bytes, &out_bound, &ev, &rg) == RGB_E_INVAL);
      cmds[i] = c0; cmds[i].data_offset = data_bytes; cmds[i].data_len = 0;          /* an empty payload at the end */
      CHECK(rgb_wal_batch_bound(cmds, n, writers, W, &file, data_bytes, &out_bound, &ev, &rg) == RGB_OK);
      keep = out_bound;
      cmds[i] = c0;
      writers[w].uid_len = 65536; writers[w].uid_offset = 0;
      CHECK(rgb_wal_batch_bound(cmds, n, writers, W, &file, data_bytes, &out_bound, &ev, &rg) == RGB_E_INVAL);
      writers[w] = w0; writers[w].uid_offset = UINT64_MAX; writers[w].uid_len = 2;
      CHECK(rgb_wal_batch_bound(cmds, n, writers, W, &file, data_bytes, &out_bound, &ev, &rg) == RGB_E_INVAL);
      writers[w] = w0; writers[w].state = 3;
      CHECK(rgb_wal_batch_bound(cmds, n, writers, W, &file, data_bytes, &out_bound, &ev, &rg) == RGB_E_INVAL);
      writers[w] = w0; writers[w].id_ref = RGB_WAL_MAX_ID_REFS;
      CHECK(rgb_wal_batch_bound(cmds, n, writers, W, &file, data_bytes, &out_bound, &ev, &rg) == RGB_E_INVAL);
      writers[w] = w0; writers[w].id_ref = RGB_WAL_NO_ID_REF;
      rgb_wal_file full = file;
      full.next_id_ref = RGB_WAL_MAX_ID_REFS;                                         /* no IdRef left for that writer */
      CHECK(rgb_wal_batch_bound(cmds, n, writers, W, &full, data_bytes, &out_bound, &ev, &rg) == RGB_E_INVAL);
      writers[w] = w0;
      CHECK(rgb_wal_batch_check(cmds, n, writers, W, &file, data_bytes, 2u, order, wstart, nullptr, nullptr, nullptr) == RGB_E_INVAL);
      CHECK(rgb_wal_batch_check(cmds, n, writers, W, &file, data_bytes, 0u, order, nullptr, nullptr, nullptr, nullptr) == RGB_E_INVAL);
      CHECK(rgb_wal_batch_bound(nullptr, n, writers, W, &file, data_bytes, &out_bound, &ev, &rg) == RGB_E_INVAL);
      CHECK(rgb_wal_batch_bound(cmds, n, nullptr, W, &file, data_bytes, &out_bound, &ev, &rg) == RGB_E_INVAL);
      CHECK(rgb_wal_batch_bound(cmds, n, writers, W, nullptr, data_bytes, &out_bound, &ev, &rg) == RGB_E_INVAL);
      CHECK(rgb_wal_batch_bound(cmds, n, writers, W, &file, data_bytes, nullptr, &ev, &rg) == RGB_E_INVAL);
      CHECK(out_bound == keep);
    }
    delete[] cmds; delete[] writers; delete[] order; delete[] wstart;
  }
  /* n = 0 with and without writers */
  rgb_wal_file file = {};
  uint64_t ob = 1;
  uint32_t ev = 1, rg = 1, ws[1] = {7};
  if (rgb_wal_batch_bound(nullptr, 0, nullptr, 0, &file, 0, &ob, &ev, &rg) != RGB_OK || ob || ev || rg) return 1;
  if (rgb_wal_batch_check(nullptr, 0, nullptr, 0, &file, 0, 0, ws, ws, nullptr, nullptr, nullptr) != RGB_OK || ws[0]) return 1;
  printf("wal batch harness ok\n");
  return 0;
}

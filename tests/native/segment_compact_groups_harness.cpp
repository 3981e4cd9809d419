/* Harness for tests/test_segment_compact_groups.py::test_plan_helpers_under_sanitizers: runs the three pure host
 * helpers of the batched major compaction -- rgb_segment_compact_select, rgb_segment_compact_take_groups and
 * rgb_segment_compact_groups_bound, host-only code of ra_amd/csrc/rgb_segment_host.cpp -- over case files given on the
 * command line and prints what they answer.  A file starts with <<Kind:32/little, A:32, B:32, C:32, X:64, Y:64>>:
 *     kind 0  select       A members, B segrefs, C live pairs, X = live_out_cap, Y = 1: the sizing form
 *                          then A rgb_seg_member, B (first, last) pairs, C (first, last) pairs
 *     kind 1  take_groups  A members, B sources, X = max_count, Y = max_size
 *                          then A rgb_seg_take_member, B rgb_seg_info, B uint64 num_live
 *     kind 2  groups_bound A groups, B sources, C live pairs, X = files_bytes
 *                          then A rgb_seg_group, B rgb_seg_source, C (first, last) pairs
 * Every array, outputs included, is an exactly-sized heap block (no block at all for no elements), so that
 * AddressSanitizer reports any access past an end.  Built with g++ -fsanitize=address,undefined (no HIP needed). */
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <string.h>
#include "ra_gpu_wal.h"

static void *load(FILE *f, size_t bytes) {
  if (!bytes) return NULL;
  void *p = malloc(bytes);
  if (!p || fread(p, 1, bytes, f) != bytes) exit(4);
  return p;
}

int main(int argc, char **argv) {
  for (int a = 1; a < argc; ++a) {
    FILE *f = fopen(argv[a], "rb"); if (!f) return 2;
    uint32_t h[4]; uint64_t x[2];
    if (fread(h, 4, 4, f) != 4 || fread(x, 8, 2, f) != 2) return 3;
    if (h[0] == 0u) {
      rgb_seg_member *members = (rgb_seg_member *)load(f, (size_t)h[1] * sizeof(rgb_seg_member));
      uint64_t *segrefs = (uint64_t *)load(f, (size_t)h[2] * 16u), *live = (uint64_t *)load(f, (size_t)h[3] * 16u);
      const bool sizing = x[1] != 0u;
      rgb_seg_pick *picks = sizing || !h[2] ? NULL : (rgb_seg_pick *)malloc((size_t)h[2] * sizeof(rgb_seg_pick));
      uint64_t *out = sizing || !x[0] ? NULL : (uint64_t *)malloc((size_t)x[0] * 16u);
      if (picks) memset(picks, 0xEE, (size_t)h[2] * sizeof(rgb_seg_pick));
      uint32_t n_out = 0xEEEEEEEEu;
      const int rc = rgb_segment_compact_select(members, h[1], segrefs, h[2], live, h[3], picks, out, (uint32_t)x[0], &n_out);
      printf("%d %u", rc, rc ? 0u : n_out);
      if (!rc && !sizing) {
        /* (rows that no member names are not written: they still hold the fill) */
        for (uint32_t k = 0; k < h[2]; ++k)
          printf(" %llu %u %u %u", (unsigned long long)picks[k].num_live, picks[k].live_first, picks[k].live_n, picks[k].flags);
        for (uint32_t k = 0; k < 2u * n_out; ++k) printf(" %llu", (unsigned long long)out[k]);
      }
      printf("\n");
      free(members); free(segrefs); free(live); free(picks); free(out);
    } else if (h[0] == 1u) {
      rgb_seg_take_member *members = (rgb_seg_take_member *)load(f, (size_t)h[1] * sizeof(rgb_seg_take_member));
      rgb_seg_info *infos = (rgb_seg_info *)load(f, (size_t)h[2] * sizeof(rgb_seg_info));
      uint64_t *num_live = (uint64_t *)load(f, (size_t)h[2] * 8u);
      uint32_t *group_of = h[2] ? (uint32_t *)malloc((size_t)h[2] * 4u) : NULL;
      if (group_of) memset(group_of, 0xEE, (size_t)h[2] * 4u);
      const int rc = rgb_segment_compact_take_groups(members, h[1], infos, num_live, h[2], x[0], x[1], group_of);
      printf("%d", rc);
      if (!rc) {
        for (uint32_t m = 0; m < h[1]; ++m) printf(" %u %u", members[m].n_groups, members[m].status);
        for (uint32_t s = 0; s < h[2]; ++s) printf(" %u", group_of[s]);
      }
      printf("\n");
      free(members); free(infos); free(num_live); free(group_of);
    } else {
      rgb_seg_group *groups = (rgb_seg_group *)load(f, (size_t)h[1] * sizeof(rgb_seg_group));
      rgb_seg_source *sources = (rgb_seg_source *)load(f, (size_t)h[2] * sizeof(rgb_seg_source));
      uint64_t *live = (uint64_t *)load(f, (size_t)h[3] * 16u);
      uint32_t *counts = h[1] ? (uint32_t *)malloc((size_t)h[1] * 4u) : NULL;
      uint64_t total = 0;
      const int rc = rgb_segment_compact_groups_bound(groups, h[1], sources, h[2], live, h[3], x[0], &total, counts);
      printf("%d %llu", rc, (unsigned long long)(rc ? 0u : total));
      if (!rc)
        for (uint32_t g = 0; g < h[1]; ++g)
          printf(" %llu %llu %u", (unsigned long long)groups[g].out_offset, (unsigned long long)groups[g].out_bytes, counts[g]);
      printf("\n");
      free(groups); free(sources); free(live); free(counts);
    }
    fclose(f);
  }
  return 0;
}

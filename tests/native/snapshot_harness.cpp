/* Harness for tests/test_snapshot_files.py::test_snapshot_descriptors_under_sanitizers: runs the descriptor validation
 * every snapshot call does first (rgb_snapshot_spans_check, rgb_snapshot_build_check, rgb_snapshot_files_check) and
 * rgb_snapshot_layout -- host-only code of ra_amd/csrc/rgb_segment_host.cpp -- over descriptor files given on the command
 * line.  A file is
 *     <<Mode:32/little, N:32/little, BufferBytes:64/little, OutBytes:64/little, Base:64/little>>, N descriptors
 * with Mode 0 = rgb_crc_span, 1 = rgb_snap_item, 2 = rgb_snap_file; the array is loaded into an exactly-sized heap block
 * so that AddressSanitizer reports any read past its end.  Prints "rc sum_bytes" and, for Mode 1, the end rgb_snapshot_layout
 * returns from Base and a sum over the out_offsets it filled.  Built with g++ -fsanitize=address,undefined (no HIP needed). */
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <string.h>
#include "ra_gpu_wal.h"
extern "C" int rgb_snapshot_spans_check(const rgb_crc_span *spans, uint32_t n, uint64_t data_bytes, uint64_t *sum_bytes);
extern "C" int rgb_snapshot_build_check(const rgb_snap_item *items, uint32_t n, uint64_t data_bytes, uint64_t out_bytes,
                                        uint64_t *sum_bytes);
extern "C" int rgb_snapshot_files_check(const rgb_snap_file *files, uint32_t n, uint64_t files_bytes, uint64_t *sum_bytes);
int main(int argc, char **argv) {
  for (int a = 1; a < argc; ++a) {
    FILE *f = fopen(argv[a], "rb"); if (!f) return 2;
    uint32_t head[2]; uint64_t sizes[3];
    if (fread(head, 4, 2, f) != 2 || fread(sizes, 8, 3, f) != 3) return 3;
    const uint32_t mode = head[0], n = head[1];
    const size_t each = mode == 0 ? sizeof(rgb_crc_span) : mode == 1 ? sizeof(rgb_snap_item) : sizeof(rgb_snap_file);
    const size_t bytes = (size_t)n * each;
    void *desc = malloc(bytes ? bytes : 1);
    if (fread(desc, 1, bytes, f) != bytes) return 4;
    fclose(f);
    uint64_t sum = 0;
    int rc;
    if (mode == 0) rc = rgb_snapshot_spans_check(n ? (const rgb_crc_span *)desc : NULL, n, sizes[0], &sum);
    else if (mode == 1) rc = rgb_snapshot_build_check(n ? (const rgb_snap_item *)desc : NULL, n, sizes[0], sizes[1], &sum);
    else rc = rgb_snapshot_files_check(n ? (const rgb_snap_file *)desc : NULL, n, sizes[0], &sum);
    if (rc) sum = 0;
    printf("%d %llu", rc, (unsigned long long)sum);
    if (mode == 1) {
      rgb_snap_item *items = (rgb_snap_item *)desc;
      const uint64_t end = rgb_snapshot_layout(items, n, sizes[2]);
      uint64_t mix = 0;
      for (uint32_t i = 0; i < n; ++i) mix = mix * 31u + items[i].out_offset;
      printf(" %llu %llu", (unsigned long long)end, (unsigned long long)mix);
    }
    printf("\n");
    free(desc);
  }
  return 0;
}

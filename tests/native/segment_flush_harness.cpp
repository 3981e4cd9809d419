/* Harness for tests/test_segment_flush.py::test_flush_descriptors_under_sanitizers: runs rgb_segment_flush_bound
 * (the writer validation every flush call does first, host-only code of ra_amd/csrc/rgb_segment_host.cpp) over
 * descriptor files given on the command line.  A file is
 *     <<NWriters:32/little, NEntries:32/little, DataBytes:64/little>>, NWriters rgb_seg_writer;
 * the array is loaded into an exactly-sized heap block so that AddressSanitizer reports any read past its end.
 * Built with g++ -fsanitize=address,undefined (no HIP needed). */
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <string.h>
#include "ra_gpu_wal.h"
int main(int argc, char **argv) {
  for (int a = 1; a < argc; ++a) {
    FILE *f = fopen(argv[a], "rb"); if (!f) return 2;
    uint32_t head[2]; uint64_t data_bytes;
    if (fread(head, 4, 2, f) != 2 || fread(&data_bytes, 8, 1, f) != 1) return 3;
    const size_t w_bytes = (size_t)head[0] * sizeof(rgb_seg_writer);
    rgb_seg_writer *writers = (rgb_seg_writer *)malloc(w_bytes ? w_bytes : 1);
    if (fread(writers, 1, w_bytes, f) != w_bytes) return 4;
    fclose(f);
    uint64_t out_bound = 0; uint32_t pieces_bound = 0;
    int rc = rgb_segment_flush_bound(head[0] ? writers : NULL, head[0], head[1], data_bytes, &out_bound, &pieces_bound);
    if (rc) { out_bound = 0; pieces_bound = 0; }
    printf("%d %llu %u\n", rc, (unsigned long long)out_bound, pieces_bound);
    free(writers);
  }
  return 0;
}

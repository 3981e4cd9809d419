/* Harness for tests/test_segment_read.py::test_read_descriptors_under_sanitizers: runs rgb_seg_read_check (the source
 * validation every read call does first, host-only code of ra_amd/csrc/rgb_segment_host.cpp) over descriptor files given
 * on the command line.  A file is
 *     <<NSources:32/little, NReq:32/little, FilesBytes:64/little, Flags:32/little, 0:32>>, NSources rgb_seg_read_source;
 * the array is loaded into an exactly-sized heap block so that AddressSanitizer reports any read past its end.
 * Built with g++ -fsanitize=address,undefined (no HIP needed). */
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <string.h>
#include "ra_gpu_wal.h"
extern "C" int rgb_seg_read_check(const rgb_seg_read_source *sources, uint32_t n_sources, uint64_t files_bytes,
                                  uint32_t n_req, uint32_t flags, uint32_t *covered, uint64_t *sum_bytes,
                                  uint64_t *out_bound);
int main(int argc, char **argv) {
  for (int a = 1; a < argc; ++a) {
    FILE *f = fopen(argv[a], "rb"); if (!f) return 2;
    uint32_t head[2], tail[2]; uint64_t files_bytes;
    if (fread(head, 4, 2, f) != 2 || fread(&files_bytes, 8, 1, f) != 1 || fread(tail, 4, 2, f) != 2) return 3;
    const size_t s_bytes = (size_t)head[0] * sizeof(rgb_seg_read_source);
    rgb_seg_read_source *sources = (rgb_seg_read_source *)malloc(s_bytes ? s_bytes : 1);
    if (fread(sources, 1, s_bytes, f) != s_bytes) return 4;
    fclose(f);
    uint32_t covered = 0; uint64_t sum = 0, bound = 0;
    int rc = rgb_seg_read_check(head[0] ? sources : NULL, head[0], files_bytes, head[1], tail[0], &covered, &sum, &bound);
    if (rc) { covered = 0; sum = 0; bound = 0; }
    printf("%d %u %llu %llu\n", rc, covered, (unsigned long long)sum, (unsigned long long)bound);
    free(sources);
  }
  return 0;
}

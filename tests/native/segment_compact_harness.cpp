/* Harness for tests/test_segment_compact.py::test_compact_descriptors_under_sanitizers: runs
 * rgb_segment_compact_bound (the descriptor validation every compact call does first, host-only code of
 * ra_amd/csrc/rgb_segment_host.cpp) over descriptor files given on the command line.  A file is
 *     <<NSources:32/little, NLive:32/little, FilesBytes:64/little>>, NSources rgb_seg_source, NLive (first, last) pairs;
 * the two arrays are loaded into exactly-sized heap blocks so that AddressSanitizer reports any read past their end.
 * Built with g++ -fsanitize=address,undefined (no HIP needed). */
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <string.h>
#include "ra_gpu_wal.h"
int main(int argc, char **argv) {
  for (int a = 1; a < argc; ++a) {
    FILE *f = fopen(argv[a], "rb"); if (!f) return 2;
    uint32_t head[2]; uint64_t files_bytes;
    if (fread(head, 4, 2, f) != 2 || fread(&files_bytes, 8, 1, f) != 1) return 3;
    const size_t src_bytes = (size_t)head[0] * sizeof(rgb_seg_source), live_bytes = (size_t)head[1] * 16u;
    rgb_seg_source *sources = (rgb_seg_source *)malloc(src_bytes ? src_bytes : 1);
    uint64_t *live = (uint64_t *)malloc(live_bytes ? live_bytes : 1);
    if (fread(sources, 1, src_bytes, f) != src_bytes || fread(live, 1, live_bytes, f) != live_bytes) return 4;
    fclose(f);
    uint64_t bound = 0; uint32_t max_count = 0;
    int rc = rgb_segment_compact_bound(head[0] ? sources : NULL, head[0], head[1] ? live : NULL, head[1], files_bytes,
                                       &bound, &max_count);
    if (rc) { bound = 0; max_count = 0; }
    printf("%d %llu %u\n", rc, (unsigned long long)bound, max_count);
    free(sources); free(live);
  }
  return 0;
}

/* Harness for tests/test_segment.py::test_segment_scan_under_sanitizers: runs rgb_segment_scan (count mode, then
 * store mode) over files given on the command line, each loaded into an exactly-sized heap block so that
 * AddressSanitizer reports any read past the end.  Built with g++ -fsanitize=address,undefined together with
 * ra_amd/csrc/rgb_segment_host.cpp (no HIP needed). */
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include "ra_gpu_wal.h"
int main(int argc, char **argv) {
  for (int a = 1; a < argc; ++a) {
    FILE *f = fopen(argv[a], "rb"); if (!f) return 2;
    fseek(f, 0, SEEK_END); long n = ftell(f); fseek(f, 0, SEEK_SET);
    unsigned char *buf = (unsigned char *)malloc(n ? n : 1);      /* exactly sized: ASan sees any overrun */
    if (fread(buf, 1, n, f) != (size_t)n) return 3;
    fclose(f);
    uint32_t cnt = 0, n2 = 0, ver = 0, mc = 0, end = 0, end2 = 0;
    int rc = rgb_segment_scan(buf, n, NULL, 0, &cnt, &ver, &mc, &end);
    if (rc == 0) {
      rgb_seg_entry *recs = (rgb_seg_entry *)malloc(sizeof(rgb_seg_entry) * (cnt ? cnt : 1));
      rc = rgb_segment_scan(buf, n, recs, cnt, &n2, &ver, &mc, &end2);
      /* with room for exactly the counted records the store pass may stop at the cap where the count pass went on */
      if (rc || n2 != cnt || (end2 != end && end2 != RGB_SEG_END_CAP)) return 4;
      for (uint32_t i = 0; i < n2; ++i)
        if (recs[i].data_offset + recs[i].data_len > (uint64_t)n) return 5;
      free(recs);
    }
    printf("%d %u %u %u %u\n", rc, cnt, ver, mc, end);
    free(buf);
  }
  return 0;
}

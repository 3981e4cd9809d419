/* rgb_decision_expand (include/ra_gpu_batch.h) over a file of 64-byte records: argv[1] in, argv[2] out.  Every record
 * sits in its own exactly-sized heap block, so a decoder that reads or writes outside its record is a sanitizer report
 * (tests/test_compact_decisions.py builds this with -fsanitize=address,undefined). */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "ra_gpu_batch.h"

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
  if (!in || !out) return 2;
  unsigned char raw[sizeof(rgb_decision)];
  size_t n = 0;
  while (fread(raw, sizeof raw, 1, in) == 1) {
    rgb_decision *d = (rgb_decision *)malloc(sizeof *d);
    if (!d) return 3;
    memcpy(d, raw, sizeof *d);
    rgb_decision_expand(d);
    if (fwrite(d, sizeof *d, 1, out) != 1) return 3;
    free(d);
    n++;
  }
  fclose(in);
  if (fclose(out) != 0) return 3;
  printf("%zu\n", n);
  return 0;
}

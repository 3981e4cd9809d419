/* rgb_decision_expand (include/ra_gpu_batch.h) against abi.expand_decisions: argv[1] holds 64-byte slots of a decision
 * stream, argv[2] what the Python decoder made of them.  Every slot is expanded in its own exactly-sized heap block (a
 * decoder that reads or writes outside its record is a sanitizer report: tests/test_compact_forms.py builds this with
 * -fsanitize=address,undefined), then expanded a second time (a full record passes through untouched).  Prints the
 * number of records; the first record that differs is named on stderr and the exit status is 1. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "ra_gpu_batch.h"

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  FILE *in = fopen(argv[1], "rb"), *want = fopen(argv[2], "rb");
  if (!in || !want) return 2;
  unsigned char raw[sizeof(rgb_decision)], exp[sizeof(rgb_decision)];
  size_t n = 0;
  while (fread(raw, sizeof raw, 1, in) == 1) {
    if (fread(exp, sizeof exp, 1, want) != 1) { fprintf(stderr, "record %zu: nothing to compare with\n", n); return 1; }
    rgb_decision *d = (rgb_decision *)malloc(sizeof *d);
    if (!d) return 3;
    memcpy(d, raw, sizeof *d);
    rgb_decision_expand(d);
    if (memcmp(d, exp, sizeof *d) != 0) { fprintf(stderr, "record %zu: rgb_decision_expand differs\n", n); return 1; }
    rgb_decision_expand(d);
    if (memcmp(d, exp, sizeof *d) != 0) { fprintf(stderr, "record %zu: the second expansion changed it\n", n); return 1; }
    free(d);
    n++;
  }
  if (fread(exp, sizeof exp, 1, want) == 1) { fprintf(stderr, "more expected records than slots\n"); return 1; }
  fclose(in); fclose(want);
  printf("%zu\n", n);
  return 0;
}

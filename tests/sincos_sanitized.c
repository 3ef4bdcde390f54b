/* A program of its own around tests/sincos_restatement.h, for a run under the undefined-behaviour sanitizer
 * (tests/test_sincos_host.py builds it with -fsanitize=undefined,float-cast-overflow -fno-sanitize-recover=all and runs it as a
 * child process): sincos_restated for the binades first <= b < last (a binade is bits >> 23) at every stride-th mantissa.  Prints
 * the number of arguments and the xor of the result bits, so that nothing is optimised away. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "sincos_restatement.h"

int main(int argc, char **argv) {
  if (argc != 4) return 2;
  unsigned long first = strtoul(argv[1], NULL, 10), last = strtoul(argv[2], NULL, 10), stride = strtoul(argv[3], NULL, 10);
  if (first > last || last > 512 || stride == 0 || stride > (1u << 23)) return 2;
  uint32_t all = 0;
  unsigned long long n = 0;
  for (uint32_t b = (uint32_t)first; b < (uint32_t)last; b++)
    for (uint32_t m = 0; m < (1u << 23); m += (uint32_t)stride) {
      uint32_t bits = (b << 23) | m, sb, cb;
      float x, s, c;
      memcpy(&x, &bits, 4);
      sincos_restated(x, &s, &c);
      memcpy(&sb, &s, 4), memcpy(&cb, &c, 4);
      all ^= sb ^ (cb * 3u), n++;
    }
  printf("arguments %llu xor %08x\n", n, all);
  return 0;
}

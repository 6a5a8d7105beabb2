// Stand-alone host program around csrc/nerf_fixed_sum.h (plain C++, no HIP): tests/test_hashgrid_deterministic_cpu.py compiles it,
// feeds it operands and compares every answer with the Python restatement.  One request per input line:
//   q <bits> <emax> <K>      -> fx_quantize          (decimal int64)
//   f <acc> <emax> <K>       -> fx_finish            (the bits of the float, decimal uint32)
//   k <terms>                -> fx_guard_bits
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "../nerf_replication_amd/csrc/nerf_fixed_sum.h"

int main() {
  char op;
  long long a, b, c;
  while (scanf(" %c", &op) == 1) {
    if (op == 'k') {
      if (scanf("%lld", &a) != 1) return 2;
      printf("%d\n", fx_guard_bits((int64_t)a));
    } else {
      if (scanf("%lld %lld %lld", &a, &b, &c) != 3) return 2;
      if (op == 'q') {
        printf("%" PRId64 "\n", fx_quantize((uint32_t)a, (uint32_t)b, (int)c));
      } else if (op == 'f') {
        const float v = fx_finish((int64_t)a, (uint32_t)b, (int)c);
        uint32_t bits;
        memcpy(&bits, &v, sizeof bits);
        printf("%" PRIu32 "\n", bits);
      } else {
        return 2;
      }
    }
  }
  return 0;
}

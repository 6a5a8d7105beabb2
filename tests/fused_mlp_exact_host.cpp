// Stand-alone host program around csrc/nerf_fixed_sum.h (plain C++, no HIP) for the fused MLP's exact gradients (DESIGN.md section
// 2.13.1): tests/test_fused_mlp_exact_cpu.py compiles it, feeds it operands and compares every answer with the Python restatement.
// One request per input line, every operand the decimal bit pattern of a float:
//   p <a> <b>                              -> fx_product_exponent (a, b: sign-cleared)
//   e <K> <n> <dz_1> <in_1> ... <dz_n> <in_n>   -> one weight-gradient element summed from zero over n rows:
//                                             "<emax> <acc> <bits of the gradient>" (emax 0: untouched, bits 0; 255: the quiet NaN)
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../nerf_replication_amd/csrc/nerf_fixed_sum.h"

static float as_float(uint32_t bits) {
  float v;
  memcpy(&v, &bits, sizeof v);
  return v;
}

static uint32_t as_bits(float v) {
  uint32_t bits;
  memcpy(&bits, &v, sizeof bits);
  return bits;
}

int main() {
  char op;
  while (scanf(" %c", &op) == 1) {
    if (op == 'p') {
      unsigned long long a, b;
      if (scanf("%llu %llu", &a, &b) != 2) return 2;
      printf("%" PRIu32 "\n", fx_product_exponent((uint32_t)a, (uint32_t)b));
    } else if (op == 'e') {
      int K, n;
      if (scanf("%d %d", &K, &n) != 2 || n < 1) return 2;
      std::vector<uint32_t> dz(n), in(n);
      uint32_t A = 0, H = 0;
      for (int p = 0; p < n; ++p) {
        unsigned long long d, h;
        if (scanf("%llu %llu", &d, &h) != 2) return 2;
        dz[p] = (uint32_t)d; in[p] = (uint32_t)h;
        if ((dz[p] & 0x7fffffffu) > A) A = dz[p] & 0x7fffffffu;
        if ((in[p] & 0x7fffffffu) > H) H = in[p] & 0x7fffffffu;
      }
      const uint32_t emax = fx_product_exponent(A, H);
      int64_t acc = 0;
      if (emax != 0 && emax != kFxPoison)
        for (int p = 0; p < n; ++p) {
          const volatile float t = as_float(dz[p]) * as_float(in[p]);        // the term: one fp32 multiplication
          const uint32_t bits = as_bits(t), e = fx_exponent(bits);
          if (e != 0 && e != kFxPoison) acc += fx_quantize(bits, emax, K);
        }
      float grad = 0.0f;
      if (emax == kFxPoison) grad = as_float(0x7fc00000u);
      else if (emax != 0) grad = grad + fx_finish(acc, emax, K);
      printf("%" PRIu32 " %" PRId64 " %" PRIu32 "\n", emax, acc, as_bits(grad));
    } else {
      return 2;
    }
  }
  return 0;
}

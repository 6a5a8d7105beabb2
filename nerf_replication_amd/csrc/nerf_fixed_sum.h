// Exact fixed-point summation of fp32 terms: the arithmetic of the order-independent scatter-add (DESIGN.md section 2.12.1,
// include/nerf_mi355x_hashgrid.h).  A destination element owns an exponent emax (the largest biased exponent among its terms) and
// a signed 64-bit accumulator in units of 2^(emax - 150 - K), K guard bits.  A term joins as the integer fx_quantize() makes of it;
// integer addition is associative, so the sum is a function of the multiset of terms.  fx_finish() turns the accumulator back into
// one fp32 value, rounded once.  Nothing here knows about hash grids: any scatter-add of fp32 terms can run the same three passes
// (exponent max, quantised add, finish).  The fused MLP's exact weight gradients (section 2.13.1, include/nerf_mi355x_nn_exact.h) do,
// with an emax that bounds the terms' exponents from the column maxima of their two factors (fx_product_exponent) instead of being
// their maximum.  Plain C++ when compiled without HIP, so a host program can call every function.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define NERF_FX_INLINE __host__ __device__ __forceinline__
#else
#define NERF_FX_INLINE inline
#endif

constexpr int kFxMaxGuardBits = 30;
constexpr uint32_t kFxPoison = 255u;           // the exponent field of Inf and NaN

// the biased exponent field of a term: 0 = zero or subnormal (a null term), 255 = Inf or NaN (a poison term)
NERF_FX_INLINE uint32_t fx_exponent(uint32_t bits) { return (bits >> 23) & 0xffu; }

// The biased exponent field of fmul(|a|, |b|), a and b given as bit patterns with the sign cleared: the emax of a sum whose every
// term is a product fmul(u, v) with |u| <= |a| and |v| <= |b| (the fused MLP's weight gradient, DESIGN.md section 2.13.1, where a
// and b are column maxima).  Rounding is monotonic, so no term's exponent exceeds it.  255 when either is a NaN, when the product
// overflows, and for Inf * 0; 0 when the product is zero or subnormal (then every term is a null term).
NERF_FX_INLINE uint32_t fx_product_exponent(uint32_t a_bits, uint32_t b_bits) {
  float a, b;
  __builtin_memcpy(&a, &a_bits, sizeof a);
  __builtin_memcpy(&b, &b_bits, sizeof b);
  const float p = a * b;                                      // one fp32 multiplication, nothing to contract it into
  uint32_t bits;
  __builtin_memcpy(&bits, &p, sizeof bits);
  return fx_exponent(bits);
}

// Guard bits for at most `terms` (>= 1, <= 2^35) terms per element: K = min(30, 39 - ceil(log2(terms))).  Every |q| is at most
// (2^24 - 1) * 2^K, so |sum q| < 2^24 * 2^K * 2^ceil(log2(terms)) <= 2^63: the accumulator cannot overflow.
NERF_FX_INLINE int fx_guard_bits(int64_t terms) {
  int n = 0;
  while (((int64_t)1 << n) < terms) ++n;
  const int k = 39 - n;
  return k < kFxMaxGuardBits ? k : kFxMaxGuardBits;
}

// A live term (1 <= exponent <= 254) of an element whose emax (>= the term's exponent, <= 254) is known -> its integer q:
// the 24-bit significand (hidden bit set) shifted so that one unit is 2^(emax - 150 - K).  Terms more than K binades under emax
// lose their low bits by truncation of the magnitude; 24 or more binades beyond K give 0.
NERF_FX_INLINE int64_t fx_quantize(uint32_t bits, uint32_t emax, int K) {
  const uint64_t m = (uint64_t)((bits & 0x7fffffu) | 0x800000u);
  const int s = (int)emax - (int)fx_exponent(bits);           // >= 0
  const uint64_t mag = s <= K ? m << (K - s) : (s - K >= 24 ? (uint64_t)0 : m >> (s - K));
  return (bits >> 31) ? -(int64_t)mag : (int64_t)mag;
}

// the accumulator of an element with 1 <= emax <= 254 -> its value: one rounding to fp32 (to nearest even), then an exact scaling
// (a result in the subnormal range is rounded a second time by the scaling)
NERF_FX_INLINE float fx_finish(int64_t acc, uint32_t emax, int K) {
#if defined(__HIP_DEVICE_COMPILE__)
  const float a = __ll2float_rn(acc);
#else
  const float a = (float)acc;
#endif
  return ldexpf(a, (int)emax - 150 - K);
}

// The structured pick of a 62-wide score row: top-5 of the 50 main outputs | top-2 of the 12 stars, as a
// 64-bit mask in the layout of em_rows_to_masks (bit n-1 = main number n, bit 49+s = star s).  Shared by
// csrc/metrics.hip (the arg-max pick of draw_metrics_kernel) and csrc/tickets.hip (sampled tickets), so the
// stable order -- the earlier index wins a tie, as metrics.draw_metrics' stable argsort -- cannot diverge.
#pragma once
#include "common.h"

namespace {

constexpr uint64_t MAIN_BITS = (1ull << 50) - 1;
constexpr uint64_t STAR_BITS = ((1ull << 12) - 1) << 50;

template <int K>
EM_DEVICE uint64_t topk_mask(const float* z, int lo, int hi) {
  float bv[K];
  int bi[K];
#pragma unroll
  for (int k = 0; k < K; ++k) { bv[k] = -3.0e38f; bi[k] = lo; }
  for (int o = lo; o < hi; ++o) {
    float v = z[o];
    int id = o;
    // insertion (stable: earlier index wins ties).  Once v has taken slot k the displaced entries shift down
    // unconditionally: the list is sorted, and a displaced entry that EQUALS the one below it is the earlier
    // index of the two, so a strict compare there would drop it and keep the later one.
    bool sw = false;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      sw = sw || v > bv[k];
      const float tv = bv[k];
      const int ti = bi[k];
      bv[k] = sw ? v : tv;
      bi[k] = sw ? id : ti;
      v = sw ? tv : v;
      id = sw ? ti : id;
    }
  }
  uint64_t m = 0;
#pragma unroll
  for (int k = 0; k < K; ++k) m |= 1ull << bi[k];
  return m;
}

}  // namespace

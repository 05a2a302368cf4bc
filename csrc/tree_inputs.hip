// K15: draw masks -> the tree models' inputs, on the device.
//
// The forest and the GBDT read binary draw features in their own layouts: the forest packed bit rows
// (models/forest.pack_bits) and target masks, the GBDT one uint8 bin and one float32 target per
// (row, column).  Both used to be built with numpy on the host from draw rows and uploaded; these three
// kernels build them from the 8-byte feature masks (em_rows_to_masks, em_gen_masks) that are already
// in HBM, so GPU-generated draws reach the tree models without a host copy.
//   em_rf_lag_rows       masks -> packed lag-window rows X [S][W] + target masks Y [S]
//   em_mask_bit_counts   masks[a, b) -> per-bit set counts (the GBDT's cut rule needs 0 < count < rows)
//   em_gbdt_draw_inputs  masks -> bins uint8 [S][62] + targets float32 [S][62]
// Every entry point checks its arguments (the window against the n masks the caller holds included) and
// returns EM_ERR_ARG before any launch.
#include "common.h"
#include "draw_topk.h"  // MAIN_BITS, STAR_BITS

namespace {

constexpr uint64_t DRAW_BITS = MAIN_BITS | STAR_BITS;  // bits 0..61
constexpr int NF = 62;                                 // features / targets per draw

// ---------------------------------------------------------------- forest lag rows
// One sample per lane.  Feature k*62 + j = bit j of draw first+s+k (k = 0 the oldest), so the row is the
// concatenation of `LAGS` 62-bit fields: field k starts at bit 62k = word (62k >> 6), shift (62k & 63)
// and spills its top bits into the next word when the shift exceeds 2.  Every word is put together in
// registers (at most three masks touch one word) and stored once; W = ceil(62 LAGS / 64) = LAGS here.
template <int LAGS>
__global__ void __launch_bounds__(256)
rf_lag_rows_kernel(const uint64_t* __restrict__ masks, int64_t first, int64_t S, uint64_t* __restrict__ X,
                   uint64_t* __restrict__ Y) {
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (s >= S) return;
  const uint64_t* m = masks + first + s;
  uint64_t x[LAGS + 1];  // (one spare word: the spill of the last field is compiled for every k)
#pragma unroll
  for (int w = 0; w <= LAGS; ++w) x[w] = 0;
#pragma unroll
  for (int k = 0; k < LAGS; ++k) {
    const uint64_t v = m[k] & DRAW_BITS;
    const int pos = NF * k, w = pos >> 6, sh = pos & 63;
    x[w] |= v << sh;
    if (sh > 2) x[w + 1] |= v >> (64 - sh);  // (sh > 2 only for k >= 1, and then w + 1 < LAGS)
  }
  uint64_t* xr = X + s * LAGS;
  if constexpr (LAGS == 2) {  // 16-byte rows: one store
    *reinterpret_cast<u32x4*>(xr) = u32x4{(uint32_t)x[0], (uint32_t)(x[0] >> 32), (uint32_t)x[1], (uint32_t)(x[1] >> 32)};
  } else if constexpr (LAGS == 4) {  // 32-byte rows: two 16-byte stores
    *reinterpret_cast<u32x4*>(xr) = u32x4{(uint32_t)x[0], (uint32_t)(x[0] >> 32), (uint32_t)x[1], (uint32_t)(x[1] >> 32)};
    *reinterpret_cast<u32x4*>(xr + 2) =
        u32x4{(uint32_t)x[2], (uint32_t)(x[2] >> 32), (uint32_t)x[3], (uint32_t)(x[3] >> 32)};
  } else {  // 8- and 24-byte rows (24-byte rows are only 8-byte aligned)
#pragma unroll
    for (int w = 0; w < LAGS; ++w) xr[w] = x[w];
  }
  Y[s] = m[LAGS] & DRAW_BITS;
}

// ---------------------------------------------------------------- per-bit counts
// Each lane strides over the masks with eight 64-bit accumulators of eight byte counters: byte i of acc[c]
// counts bit 8i + c ((m >> c) & 0x0101...01 puts that bit in the byte's lowest position).  A byte holds
// 255 increments, so the lane empties the accumulators into 64 32-bit counters every 255 masks.  Then a
// wave sum per counter, the four waves through LDS, and one int64 row of 64 per block; the second kernel
// adds the rows in block order.  All integers: exact, and the same in every run.
constexpr int COUNT_MAX_BLOCKS = 2048;
constexpr int COUNT_PER_LANE = 64;  // masks per lane before the grid stops growing

__global__ void __launch_bounds__(256)
mask_bit_counts_kernel(const uint64_t* __restrict__ masks, int64_t a, int64_t b, int64_t* __restrict__ partials) {
  __shared__ uint32_t red[4][64];
  constexpr uint64_t LOW = 0x0101010101010101ull;
  uint32_t cnt[64];
#pragma unroll
  for (int j = 0; j < 64; ++j) cnt[j] = 0;
  uint64_t acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  int held = 0;
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = a + (int64_t)blockIdx.x * 256 + threadIdx.x; i < b; i += stride) {
    const uint64_t m = masks[i];
#pragma unroll
    for (int c = 0; c < 8; ++c) acc[c] += (m >> c) & LOW;
    if (++held == 255) {
#pragma unroll
      for (int c = 0; c < 8; ++c) {
#pragma unroll
        for (int q = 0; q < 8; ++q) cnt[8 * q + c] += (uint32_t)(acc[c] >> (8 * q)) & 0xFFu;
        acc[c] = 0;
      }
      held = 0;
    }
  }
#pragma unroll
  for (int c = 0; c < 8; ++c)
#pragma unroll
    for (int q = 0; q < 8; ++q) cnt[8 * q + c] += (uint32_t)(acc[c] >> (8 * q)) & 0xFFu;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < 64; ++j) {
    uint32_t v = cnt[j];  // (a wave's share of one launch stays far below 2^32: see em_mask_bit_counts)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if (lane == 0) red[w][j] = v;
  }
  __syncthreads();
  if (threadIdx.x < 64) {
    const int j = threadIdx.x;
    partials[(int64_t)blockIdx.x * 64 + j] = ((int64_t)red[0][j] + red[1][j]) + ((int64_t)red[2][j] + red[3][j]);
  }
}

__global__ void __launch_bounds__(64)
mask_bit_counts_final(const int64_t* __restrict__ partials, int nblocks, int64_t* __restrict__ counts) {
  int64_t v = 0;
  for (int k = 0; k < nblocks; ++k) v += partials[(int64_t)k * 64 + threadIdx.x];
  counts[threadIdx.x] = v;
}

int count_blocks(int64_t n) {
  const int64_t per_block = 256 * (int64_t)COUNT_PER_LANE;
  const int64_t nb = (n + per_block - 1) / per_block;
  return (int)(nb < 1 ? 1 : nb > COUNT_MAX_BLOCKS ? COUNT_MAX_BLOCKS : nb);
}

// ---------------------------------------------------------------- GBDT bins and targets
// Both outputs are row-major with 62 columns, so a row (62 and 248 bytes) is no multiple of a wide store.
// The kernel therefore walks the FLAT outputs: one lane per 16-byte piece of Y (4 targets) and one lane
// per 16-byte piece of bins (16 bins), whatever rows the piece lies in, then one lane per element of
// what is left past the last whole piece (at most 2 targets, at most 15 bins).  A piece starts in row
// e / 62 at column e % 62 and runs into at most the next row, so its bits are the low bits of
// (row >> column) | (next row << (62 - column)); lanes of a wave read the same one or two masks.
EM_DEVICE uint64_t flat_bits(const uint64_t* __restrict__ m, int64_t row, int col, int64_t rows, uint64_t keep) {
  uint64_t v = (m[row] & keep) >> col;
  if (col > 0 && row + 1 < rows) v |= (m[row + 1] & keep) << (NF - col);  // (col > 0: NF - col <= 61)
  return v;
}

// 4 bits -> 4 bytes of 0 / 1, byte k = bit k: the product lays bit i at i + 7k for k = 0..3 (sixteen
// distinct positions: no carries) and bit 8k of it is bit k
EM_DEVICE uint32_t bits4_to_bytes(uint32_t b) { return ((b & 0xFu) * 0x00204081u) & 0x01010101u; }

__global__ void __launch_bounds__(256)
gbdt_draw_inputs_kernel(const uint64_t* __restrict__ masks, int64_t first, int64_t S, uint64_t varied,
                        uint8_t* __restrict__ bins, float* __restrict__ Y, int64_t y_pieces, int64_t bin_pieces,
                        int y_tail, int bin_tail) {
  int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const uint64_t* in = masks + first;      // inputs: draw first + s
  const uint64_t* tg = masks + first + 1;  // targets: draw first + s + 1
  if (t < y_pieces) {
    const int64_t e = t * 4, row = e / NF;
    const uint32_t b = (uint32_t)flat_bits(tg, row, (int)(e - row * NF), S, DRAW_BITS);
    *reinterpret_cast<f32x4*>(Y + e) =
        f32x4{(float)(b & 1u), (float)((b >> 1) & 1u), (float)((b >> 2) & 1u), (float)((b >> 3) & 1u)};
    return;
  }
  t -= y_pieces;
  if (t < bin_pieces) {
    const int64_t e = t * 16, row = e / NF;
    const uint32_t b = (uint32_t)flat_bits(in, row, (int)(e - row * NF), S, varied & DRAW_BITS);
    *reinterpret_cast<u32x4*>(bins + e) =
        u32x4{bits4_to_bytes(b), bits4_to_bytes(b >> 4), bits4_to_bytes(b >> 8), bits4_to_bytes(b >> 12)};
    return;
  }
  t -= bin_pieces;
  if (t < y_tail) {
    const int64_t e = y_pieces * 4 + t, row = e / NF;
    Y[e] = (float)((tg[row] >> (int)(e - row * NF)) & 1ull);
    return;
  }
  t -= y_tail;
  if (t < bin_tail) {
    const int64_t e = bin_pieces * 16 + t, row = e / NF;
    bins[e] = (uint8_t)(((in[row] & varied) >> (int)(e - row * NF)) & 1ull);
  }
}

}  // namespace

// X [S][W] packed lag-window rows and Y [S] target masks of samples first .. first+S-1 of the n masks:
// sample s reads draws first+s .. first+s+lags-1 and its target is draw first+s+lags.  lags in 1..4
// (the forest's F <= 256), W = ceil(62 lags / 64).
EM_API int em_rf_lag_rows(const uint64_t* masks, int64_t n, int64_t first, int64_t S, int lags, uint64_t* X, int W,
                          uint64_t* Y, hipStream_t stream) {
  if (!masks || !X || !Y || lags < 1 || lags > 4 || W != (NF * lags + 63) / 64 || first < 0 || S < 1 || n < 0 ||
      first > n || S > n - first || lags > n - first - S)
    return EM_ERR_ARG;
  const int64_t nb = (S + 255) / 256;
  if (nb > 0x7FFFFFFFll) return EM_ERR_ARG;
  const dim3 grid((unsigned)nb), block(256);
  switch (lags) {
    case 1: hipLaunchKernelGGL(rf_lag_rows_kernel<1>, grid, block, 0, stream, masks, first, S, X, Y); break;
    case 2: hipLaunchKernelGGL(rf_lag_rows_kernel<2>, grid, block, 0, stream, masks, first, S, X, Y); break;
    case 3: hipLaunchKernelGGL(rf_lag_rows_kernel<3>, grid, block, 0, stream, masks, first, S, X, Y); break;
    default: hipLaunchKernelGGL(rf_lag_rows_kernel<4>, grid, block, 0, stream, masks, first, S, X, Y); break;
  }
  EM_CHECK_LAUNCH();
  return 0;
}

// rows of the partials buffer em_mask_bit_counts needs for b - a = count masks (int64 [rows][64])
EM_API int em_mask_bit_count_blocks(int64_t count) { return count > 0 ? count_blocks(count) : 0; }

// counts[j] = number of masks in [a, b) of the n masks with bit j set, int64 [64].  partials: int64
// [em_mask_bit_count_blocks(b - a)][64] scratch.  An empty range gives zeros.
EM_API int em_mask_bit_counts(const uint64_t* masks, int64_t n, int64_t a, int64_t b, int64_t* partials,
                              int64_t* counts, hipStream_t stream) {
  // (2^40 masks = 8 TiB: with at least 64 masks per lane up to 2048 blocks, a wave counts at most 2^27)
  if (!masks || !counts || n < 0 || a < 0 || b < a || b > n || b - a > (1ll << 40) || (b > a && !partials))
    return EM_ERR_ARG;
  const int nb = b > a ? count_blocks(b - a) : 0;
  if (nb > 0) {
    hipLaunchKernelGGL(mask_bit_counts_kernel, dim3(nb), dim3(256), 0, stream, masks, a, b, partials);
    EM_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(mask_bit_counts_final, dim3(1), dim3(64), 0, stream, partials, nb, counts);
  EM_CHECK_LAUNCH();
  return 0;
}

// bins uint8 [S][62]: bit f of draw first+s where bit f of `varied` is set, else 0.  Y float32 [S][62]:
// bit t of draw first+s+1, or Y = null for the bins alone (prediction: draw first+S need not exist then).
// Both must be 16-byte aligned (whole allocations are).
EM_API int em_gbdt_draw_inputs(const uint64_t* masks, int64_t n, int64_t first, int64_t S, uint64_t varied,
                               uint8_t* bins, float* Y, hipStream_t stream) {
  if (!masks || !bins || first < 0 || S < 1 || n < 0 || first > n || S > n - first ||
      (Y && n - first - S < 1) || S > (1ll << 40) || ((uintptr_t)bins & 15) || ((uintptr_t)Y & 15))
    return EM_ERR_ARG;
  const int64_t total = S * NF;
  const int64_t y_pieces = Y ? total / 4 : 0, bin_pieces = total / 16;
  const int y_tail = Y ? (int)(total - y_pieces * 4) : 0, bin_tail = (int)(total - bin_pieces * 16);
  const int64_t lanes = y_pieces + bin_pieces + y_tail + bin_tail;
  const int64_t nb = (lanes + 255) / 256;
  if (nb > 0x7FFFFFFFll) return EM_ERR_ARG;
  hipLaunchKernelGGL(gbdt_draw_inputs_kernel, dim3((unsigned)nb), dim3(256), 0, stream, masks, first, S, varied, bins,
                     Y, y_pieces, bin_pieces, y_tail, bin_tail);
  EM_CHECK_LAUNCH();
  return 0;
}

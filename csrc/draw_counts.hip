// K16: the transition-count baseline on draw masks.
//
// The planted generator lets each sorted position of draw t vote for a number of draw t + 1, so the table
// "bit a in this draw -> bit b in a later draw" is the sufficient statistic of the whole planted signal.
// Two kernels fit and score that table where the masks are (models/count_table.py is the specification):
//   em_pair_counts    masks -> C[a][b] = #{t in [first, first+count): bit a of masks[t] and bit b of
//                     masks[t+lag]}, int64 [64][64]; integers only, exact and the same in every run
//   em_count_logits   masks + float32 table [lags][64][64] + prior [64] -> logits [B][64], the additions in
//                     the fixed order of count_table.logits_np (bit for bit)
// Both entry points check their arguments (the window against the n masks the caller holds included) and
// return EM_ERR_ARG before anything is launched or written.
#include "common.h"
#include "draw_topk.h"  // MAIN_BITS, STAR_BITS

namespace {

constexpr uint64_t DRAW_BITS = MAIN_BITS | STAR_BITS;  // bits 0..61
constexpr int NF = 62;

// ---------------------------------------------------------------- pair counts
// A wave takes 64 samples at a time, one per lane: src = masks[t], tgt = masks[t + lag].  The 64 target
// words are transposed as a 64 x 64 bit matrix across the lanes (six exchange steps), after which lane b
// holds TB_b, whose bit s is bit b of sample s's target.  For every source bit a the ballot A_a (bit s =
// bit a of sample s's source) is wave-uniform, and popcount(A_a & TB_b) is the number of the 64 samples
// with source bit a and target bit b: lane b adds it to its private counter cnt[a].  No atomics and no
// LDS in the loop, and the cost does not depend on the data (any number of set bits, hot cells or not).
//
// Counters are 32-bit.  They cannot wrap: a launch takes at most 2^40 samples (em_pair_counts refuses
// more), a batch adds at most 64 to a counter, a wave sees at most count / 64 / waves + 1 batches, and
// the grid only stops growing at PAIR_MAX_BLOCKS = 2048 blocks of 4 waves; so a wave's counter stays
// below 2^40 / 2^13 + 64 < 2^28 and a block's LDS sum of four of them below 2^30.
constexpr int PAIR_MAX_BLOCKS = 2048;
constexpr int PAIR_BATCHES_PER_WAVE = 64;  // batches a wave takes before the grid stops growing
constexpr int64_t PAIR_MAX_COUNT = 1ll << 40;

// 64 x 64 bit transpose across a wave: in, lane s holds row s; out, lane b holds column b (bit s = bit b
// of row s).  Step j swaps the off-diagonal j x j blocks of every 2j x 2j block between lanes l and l ^ j.
EM_DEVICE uint64_t wave_bit_transpose(uint64_t x, int lane) {
#pragma unroll
  for (int j = 32; j > 0; j >>= 1) {
    // bits whose index has bit j clear: 0x00000000FFFFFFFF, 0x0000FFFF0000FFFF, ... 0x5555555555555555
    const uint64_t lo = ~0ull / ((1ull << j) + 1);
    const uint32_t ylo = __shfl_xor((uint32_t)x, j), yhi = __shfl_xor((uint32_t)(x >> 32), j);
    const uint64_t y = ((uint64_t)yhi << 32) | ylo;
    x = (lane & j) ? (x & (lo << j)) | ((y >> j) & lo) : (x & lo) | ((y & lo) << j);
  }
  return x;
}

__global__ void __launch_bounds__(256)
pair_counts_kernel(const uint64_t* __restrict__ masks, int64_t first, int64_t count, int lag,
                   unsigned long long* __restrict__ counts) {
  __shared__ uint32_t tab[NF * 64];
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (int i = threadIdx.x; i < NF * 64; i += 256) tab[i] = 0;
  uint32_t cnt[NF];
#pragma unroll
  for (int a = 0; a < NF; ++a) cnt[a] = 0;
  const int64_t batches = (count + 63) >> 6;
  const int64_t waves = (int64_t)gridDim.x * 4;
  const uint64_t* src = masks + first;
  const uint64_t* tgt = masks + first + lag;
  for (int64_t k = (int64_t)blockIdx.x * 4 + w; k < batches; k += waves) {
    const int64_t s = (k << 6) + lane;
    uint64_t ms = 0, mt = 0;  // (a lane past the window counts nothing)
    if (s < count) {
      ms = src[s] & DRAW_BITS;
      mt = tgt[s] & DRAW_BITS;
    }
    const uint64_t tb = wave_bit_transpose(mt, lane);
#pragma unroll
    for (int a = 0; a < NF; ++a) {
      const uint64_t A = __ballot((ms >> a) & 1ull);
      cnt[a] += __popcll(A & tb);
    }
  }
  __syncthreads();  // tab is zero
#pragma unroll
  for (int a = 0; a < NF; ++a) atomicAdd(&tab[a * 64 + lane], cnt[a]);  // (lane -> bank: conflict-free)
  __syncthreads();
  // one 64-bit integer atomic per non-zero cell and block: order-independent, so exact and reproducible
  for (int i = threadIdx.x; i < NF * 64; i += 256) {
    const uint32_t v = tab[i];
    if (v) atomicAdd(&counts[i], (unsigned long long)v);
  }
}

int pair_blocks(int64_t count) {
  const int64_t per_block = 4 * 64 * (int64_t)PAIR_BATCHES_PER_WAVE;
  const int64_t nb = (count + per_block - 1) / per_block;
  return (int)(nb < 1 ? 1 : nb > PAIR_MAX_BLOCKS ? PAIR_MAX_BLOCKS : nb);
}

// ---------------------------------------------------------------- logits
// A block stages the table in LDS (16 KB per lag) and its waves take chunks of 64 output rows: lane j
// loads the LAGS masks of row j (one coalesced load per lag; a gather under sidx), then the wave walks
// the rows.  The row's words are wave-uniform (readlane), lane b owns column b, and each set bit a in
// ascending order adds table[k][a][lane]: 64 consecutive floats, so conflict-free.  The additions stay in
// the specified order; the reads of a step are issued together.  A row is stored as one 256-byte run.
// Columns 62-63 are written as 0.
//
// Walking a mask's bits with scalar instructions costs about 6 of them per bit, and the CU's one scalar
// unit then bounds the kernel (measured: 67 scalar instructions per row, 41 % of the streaming rate).  So
// while every mask of a chunk has at most 8 set bits (draws have 7), each lane first packs its own masks
// into 8 bit indices of one byte each -- vector work shared by 64 rows -- and fills the unused slots with
// 63, the index of a table row that holds -0.0f in LDS (bits 62-63 are never walked, so rows 62-63 of the
// staged table are free): x + -0.0f == x for every x, signed zeros included, so a row is eight
// unconditional additions per lag.  A chunk with a denser mask takes the scalar walk.
constexpr int LOGIT_THREADS = 1024;  // 16 waves share one staged table: 2 blocks per CU at 64 KB
constexpr int LOGIT_ROWS = LOGIT_THREADS;  // rows per block and grid step (64 per wave)
constexpr int LOGIT_MAX_BLOCKS = 512;

constexpr int PAD_ROW = 63;  // row of the staged table that holds -0.0f

// the indices of the set bits of m (at most 8), ascending, one per byte; PAD_ROW in the unused bytes
EM_DEVICE uint64_t pack_bit_indices(uint64_t m) {
  uint64_t p = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint32_t a = m ? (uint32_t)__builtin_ctzll(m) : (uint32_t)PAD_ROW;
    p |= (uint64_t)a << (8 * i);
    m &= m - 1;
  }
  return p;
}

EM_DEVICE uint64_t readlane64(uint64_t v, int j) {
  const uint32_t lo = __builtin_amdgcn_readlane((uint32_t)v, j);
  const uint32_t hi = __builtin_amdgcn_readlane((uint32_t)(v >> 32), j);
  return ((uint64_t)hi << 32) | lo;
}

template <int LAGS>
__global__ void __launch_bounds__(LOGIT_THREADS)
count_logits_kernel(const uint64_t* __restrict__ masks, int64_t n, const int32_t* __restrict__ sidx, int64_t B,
                    int64_t offset, const float* __restrict__ table, const float* __restrict__ prior,
                    float* __restrict__ out, int64_t out_stride) {
  __shared__ __attribute__((aligned(16))) float tab[LAGS * 64 * 64];
  {
    const f32x4* g = reinterpret_cast<const f32x4*>(table);
    f32x4* t4 = reinterpret_cast<f32x4*>(tab);
    for (int i = threadIdx.x; i < LAGS * 1024; i += LOGIT_THREADS) t4[i] = g[i];
  }
  __syncthreads();
  if (threadIdx.x < LAGS * 64) tab[(threadIdx.x >> 6) * 4096 + PAD_ROW * 64 + (threadIdx.x & 63)] = -0.0f;
  __syncthreads();
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const float p = lane < NF ? prior[lane] : 0.0f;
  const float* col = tab + lane;
  for (int64_t base = (int64_t)blockIdx.x * LOGIT_ROWS + w * 64; base < B; base += (int64_t)gridDim.x * LOGIT_ROWS) {
    const int64_t left = B - base;
    const int rows = left < 64 ? (int)left : 64;
    uint64_t mk[LAGS];  // mk[k - 1] = the draw k steps before the target
#pragma unroll
    for (int k = 0; k < LAGS; ++k) mk[k] = 0;
    if (lane < rows) {
      const int64_t i = sidx ? (int64_t)sidx[base + lane] : offset + base + lane;
      if (i >= 0 && i <= n - LAGS) {  // (the callers check the range; a row outside it reads no mask)
#pragma unroll
        for (int k = 1; k <= LAGS; ++k) mk[k - 1] = masks[i + LAGS - k] & DRAW_BITS;
      }
    }
    bool dense = false;
#pragma unroll
    for (int k = 0; k < LAGS; ++k) dense = dense || __popcll(mk[k]) > 8;
    if (!__ballot(dense)) {  // wave-uniform: every mask of the chunk has at most 8 set bits
      uint64_t pk[LAGS];
#pragma unroll
      for (int k = 0; k < LAGS; ++k) pk[k] = pack_bit_indices(mk[k]);
      for (int j = 0; j < rows; ++j) {
        float acc = p;
#pragma unroll
        for (int k = 0; k < LAGS; ++k) {
          const uint64_t P = readlane64(pk[k], j);
          const float* t = col + k * 4096;
          float v[8];
#pragma unroll
          for (int i = 0; i < 8; ++i) v[i] = t[(int)((P >> (8 * i)) & 0xFF) * 64];
#pragma unroll
          for (int i = 0; i < 8; ++i) acc += v[i];
        }
        out[(base + j) * out_stride + lane] = lane < NF ? acc : 0.0f;
      }
      continue;
    }
    for (int j = 0; j < rows; ++j) {
      float acc = p;
#pragma unroll
      for (int k = 0; k < LAGS; ++k) {
        uint64_t m = readlane64(mk[k], j);
        const float* t = col + k * 4096;
        while (m) {  // wave-uniform: four set bits per step, their reads issued together
          const int cnt = __popcll(m);
          const int a0 = __builtin_ctzll(m);
          m &= m - 1;
          const int a1 = m ? __builtin_ctzll(m) : 0;
          m &= m - 1;
          const int a2 = m ? __builtin_ctzll(m) : 0;
          m &= m - 1;
          const int a3 = m ? __builtin_ctzll(m) : 0;
          m &= m - 1;
          const float v0 = t[a0 * 64], v1 = t[a1 * 64], v2 = t[a2 * 64], v3 = t[a3 * 64];
          acc += v0;
          if (cnt > 1) acc += v1;
          if (cnt > 2) acc += v2;
          if (cnt > 3) acc += v3;
        }
      }
      out[(base + j) * out_stride + lane] = lane < NF ? acc : 0.0f;
    }
  }
}

}  // namespace

// counts int64 [64][64]: counts[a][b] = number of t in [first, first + count) of the n masks with bit a of
// masks[t] and bit b of masks[t + lag] set (bits 62-63 ignored: their rows and columns are 0).  lag in
// 0..4; the window must end inside the masks (first + count + lag <= n); 1 <= count <= 2^40.
EM_API int em_pair_counts(const uint64_t* masks, int64_t n, int64_t first, int64_t count, int lag, int64_t* counts,
                          hipStream_t stream) {
  if (!masks || !counts || lag < 0 || lag > 4 || n < 0 || first < 0 || count < 1 || count > PAIR_MAX_COUNT ||
      first > n || count > n - first || lag > n - first - count)
    return EM_ERR_ARG;
  hipError_t e = hipMemsetAsync(counts, 0, 64 * 64 * sizeof(int64_t), stream);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(pair_counts_kernel, dim3(pair_blocks(count)), dim3(256), 0, stream, masks, first, count, lag,
                     reinterpret_cast<unsigned long long*>(counts));
  EM_CHECK_LAUNCH();
  return 0;
}

// out [B][out_stride] float32, columns 0..63 of each row written: out[s][b] = prior[b] plus, for k = 1..lags
// and each set bit a (ascending) of masks[i + lags - k], table[k - 1][a][b], added in that order in fp32;
// i = sidx[s], or offset + s when sidx is null.  Sample i must have its target inside the masks
// (i + lags < n); with sidx that is the caller's check (an index outside reads no mask).  table float32
// [lags][64][64] and out 16-byte aligned, out_stride >= 64 and a multiple of 4 floats.
EM_API int em_count_logits(const uint64_t* masks, int64_t n, const int32_t* sidx, int64_t B, int64_t offset, int lags,
                           const float* table, const float* prior, float* out, int64_t out_stride,
                           hipStream_t stream) {
  if (!masks || !table || !prior || !out || lags < 1 || lags > 4 || n < 0 || B < 1 || B > 0x7FFFFFFEll ||
      out_stride < 64 || (out_stride & 3) || ((uintptr_t)table & 15) || ((uintptr_t)out & 15) || lags >= n)
    return EM_ERR_ARG;
  if (!sidx && (offset < 0 || offset > n - lags - 1 || B > n - lags - offset)) return EM_ERR_ARG;
  const int64_t nb64 = (B + LOGIT_ROWS - 1) / LOGIT_ROWS;
  const dim3 grid((unsigned)(nb64 > LOGIT_MAX_BLOCKS ? LOGIT_MAX_BLOCKS : nb64)), block(LOGIT_THREADS);
#define EM_LOGITS(L)                                                                                              \
  hipLaunchKernelGGL(count_logits_kernel<L>, grid, block, 0, stream, masks, n, sidx, B, offset, table, prior, out, \
                     out_stride)
  switch (lags) {
    case 1: EM_LOGITS(1); break;
    case 2: EM_LOGITS(2); break;
    case 3: EM_LOGITS(3); break;
    default: EM_LOGITS(4); break;
  }
#undef EM_LOGITS
  EM_CHECK_LAUNCH();
  return 0;
}

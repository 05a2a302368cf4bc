// Ticket sampling + prize-tier back-test over logits that a model's logits() already produced.
//
// The reference predicts nothing a player could hand in: its output is checkPredicts' boolean
// (Main.java:143,150-162).  `euromillioner predict` prints the arg-max ticket; this kernel draws N distinct
// tickets per row from the Plackett-Luce distribution with weights exp(score / T) (Gumbel top-k) and, given
// the draws, scores every ticket against the next draw into the prize-tier table.
// The specification, including the RNG call order, is euromillioner_amd/tickets.py (sample_tickets_py,
// score_tickets_py); tests/test_tickets_gpu.py compares the two.
//
// Lane map: one lane per (row, ticket).  N is padded to NP = the next power of two, a 256-thread block owns
// 256 / NP whole rows, lane = row_in_block * NP + t, lanes t >= N idle.  A row's NP lanes sit inside one wave
// (64 % NP == 0), so the row's best rank is a butterfly minimum and no step crosses a block.  The NP lanes of
// a row read the same 256 B of logits (16 x 16-B loads, as draw_metrics_kernel): HBM sees each row once.
// Logits and keys live in registers (no scratch: check `_build.py --usage tickets.hip`).
//
// Per ticket: 1 + 31 mix64 (two 23-bit uniforms per 64-bit word), 124 logs, two insertion sorts: VALU-bound.
// Results depend only on (seed, row id, t, the row's logits, T): never on B, the chunking, the block shape
// or which optional outputs are requested.  Counts are uint32 per block (<= 256 per cell), summed by the
// host in int64.
#include "common.h"
#include "draw_topk.h"

namespace {

// splitmix64 finaliser and increment, as csrc/datagen.hip
constexpr uint64_t GOLDEN = 0x9E3779B97F4A7C15ull, TICKET_SALT = 0xD1B54A32D192ED03ull;

EM_DEVICE uint64_t mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// prize-tier rank of (m main hits, s star hits) at [m * 3 + s]; 14 = no prize (tickets.py TIER_RANK)
constexpr int NO_PRIZE = 14;
EM_DEVICE int tier_rank(int cell) {
  constexpr uint8_t LUT[18] = {14, 14, 14, 14, 14, 11, 13, 12, 8, 10, 9, 6, 7, 5, 4, 3, 2, 1};
  return LUT[cell];
}

// Gumbel noise of a 23-bit draw k: u = (2k + 1) 2^-24 is exact in fp32 and never 0 or 1.  The inner log is the
// accurate logf: the tail u -> 1 gives the largest G (up to 15.5) and decides picks, and there w = -log u is
// relative-accurate only with a log that is accurate near 1.  The outer log is the native v_log_f32 (w is in
// [6e-8, 16.7]: normal, and an absolute error of an ulp of G is all the key needs): 3056 instead of 3707 VALU
// per ticket, 1.29 -> 1.15 ms per 16.8 M tickets, the same key error against the fp64 keys (docs/DESIGN.md 6f).
EM_DEVICE float gumbel(uint32_t k) {
  const float u = (float)(2u * k + 1u) * 0x1p-24f;
  return -0.6931471806f * __builtin_amdgcn_logf(-logf(u));
}

constexpr int TK_T = 256;

__global__ void __launch_bounds__(TK_T)
draw_tickets_kernel(const float* __restrict__ logits, int ld, const uint64_t* __restrict__ masks,
                    const int32_t* __restrict__ sidx, int64_t B, int64_t offset, int64_t row_base, int n_tickets,
                    int np_log2, float temperature, uint64_t seed, uint64_t* __restrict__ tickets_out,
                    float* __restrict__ keys_out, int32_t* __restrict__ partials) {
  __shared__ uint32_t cnt[32];
  if (threadIdx.x < 32) cnt[threadIdx.x] = 0;
  __syncthreads();
  const int np = 1 << np_log2;
  const int t = threadIdx.x & (np - 1);
  const int64_t s = (((int64_t)blockIdx.x * TK_T) >> np_log2) + (threadIdx.x >> np_log2);
  const bool active = s < B && t < n_tickets;
  int rank = NO_PRIZE;
  if (active) {
    const int64_t idx = sidx ? (int64_t)sidx[s] : offset + s;
    float z[64];
    const f32x4* zr = reinterpret_cast<const f32x4*>(logits + s * ld);
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const f32x4 v = zr[k];
      z[4 * k] = v[0]; z[4 * k + 1] = v[1]; z[4 * k + 2] = v[2]; z[4 * k + 3] = v[3];
    }
    if (temperature != 0.f) {  // T == 0: greedy, key = score (no noise, no scaling)
      const float inv_t = 1.0f / temperature;
      const uint64_t r = (uint64_t)row_base + (uint64_t)idx;
      uint64_t st = mix64(seed ^ ((r * 64ull + (uint64_t)t + 1ull) * TICKET_SALT));
#pragma unroll
      for (int j = 0; j < 31; ++j) {
        st += GOLDEN;
        const uint64_t x = mix64(st);
        z[2 * j] = z[2 * j] * inv_t + gumbel((uint32_t)(x >> 41));
        z[2 * j + 1] = z[2 * j + 1] * inv_t + gumbel((uint32_t)(x >> 9) & 0x7FFFFFu);
      }
    }
    const uint64_t ticket = topk_mask<5>(z, 0, 50) | topk_mask<2>(z, 50, 62);
    const int64_t e = s * n_tickets + t;
    if (tickets_out) {
      *reinterpret_cast<u32x2*>(tickets_out + e) = u32x2{(uint32_t)ticket, (uint32_t)(ticket >> 32)};
    }
    if (keys_out) {
      f32x4* ko = reinterpret_cast<f32x4*>(keys_out + e * 64);
#pragma unroll
      for (int k = 0; k < 16; ++k)
        ko[k] = f32x4{z[4 * k], z[4 * k + 1], k < 15 ? z[4 * k + 2] : 0.f, k < 15 ? z[4 * k + 3] : 0.f};
    }
    if (masks) {
      const uint64_t hit = ticket & masks[idx + 1];
      const int cell = __builtin_popcountll(hit & MAIN_BITS) * 3 + __builtin_popcountll(hit & STAR_BITS);
      rank = tier_rank(cell);
      atomicAdd(&cnt[cell], 1u);  // LDS integer add: order-independent
    }
  }
  if (!masks) return;  // (uniform)
  // best (smallest) rank of the row's np lanes; idle lanes carry NO_PRIZE
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
    if (o < np) rank = min(rank, __shfl_xor(rank, o));
  if (active && t == 0) atomicAdd(&cnt[18 + rank - 1], 1u);
  __syncthreads();
  if (threadIdx.x < 32) partials[(int64_t)blockIdx.x * 32 + threadIdx.x] = (int32_t)cnt[threadIdx.x];
}

int np_log2_of(int n) {
  int l = 0;
  while ((1 << l) < n) ++l;
  return l;
}

}  // namespace

// rows of partials that em_draw_tickets writes: one per block of 256 / NP rows (NP = n_tickets rounded up to
// a power of two)
EM_API int em_ticket_blocks(int64_t B, int n_tickets) {
  if (B <= 0 || n_tickets < 1 || n_tickets > 64 || B > 0x7FFFFFFEll) return 0;
  const int64_t rows = TK_T >> np_log2_of(n_tickets);
  return (int)((B + rows - 1) / rows);
}

// N tickets per row from logits [B][ld] (fp32, 16-B aligned rows, ld >= 64 and a multiple of 4).
// RNG row id = row_base + (sidx ? sidx[s] : offset + s); target = masks[that index + 1] (as em_draw_metrics).
// B <= 2^31 - 2 (the limit of ops/fused_mlp._check_draws): the grid is then at most 2^29 blocks at N = 64,
// so no grid-stride loop is needed.
EM_API int em_draw_tickets(const float* logits, int ld, const uint64_t* masks, const int32_t* sidx, int64_t B,
                           int64_t offset, int64_t row_base, int n_tickets, float temperature, uint64_t seed,
                           uint64_t* tickets_out, float* keys_out, int32_t* partials, hipStream_t stream) {
  if (!logits || ld < 64 || (ld & 3) || ((uintptr_t)logits & 15) || B < 0 || B > 0x7FFFFFFEll) return EM_ERR_ARG;
  if (n_tickets < 1 || n_tickets > 64) return EM_ERR_ARG;
  if (!(temperature >= 0.f) || temperature > 3.0e38f) return EM_ERR_ARG;  // negative, NaN or inf
  if ((masks == nullptr) != (partials == nullptr)) return EM_ERR_ARG;
  if (((uintptr_t)masks & 7) || ((uintptr_t)sidx & 3) || ((uintptr_t)tickets_out & 7) ||
      ((uintptr_t)keys_out & 15) || ((uintptr_t)partials & 3))
    return EM_ERR_ARG;
  if (B == 0) return 0;
  const int l2 = np_log2_of(n_tickets);
  const int nb = em_ticket_blocks(B, n_tickets);
  hipLaunchKernelGGL(draw_tickets_kernel, dim3((unsigned)nb), dim3(TK_T), 0, stream, logits, ld, masks, sidx, B,
                     offset, row_base, n_tickets, l2, temperature, seed, tickets_out, keys_out, partials);
  EM_CHECK_LAUNCH();
  return 0;
}

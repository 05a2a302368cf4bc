// Calibration totals of 62-wide draw logits: per (group, bin) count / hits / sum of predicted values, and the Brier
// sum per group (specification: euromillioner_amd/calibration.py).
//
// Addressing as em_draw_metrics (csrc/metrics.hip): one row per lane, 16 loads of 16 bytes, row s scored against
// masks[idx + 1] with idx = sidx ? sidx[s] : offset + s.  Per element o < 62 (columns 62-63 are never used):
//   softmax  x = z - logsumexp(group), q = exp(x),     t = y / k (k = 5 main, 2 stars)
//   bce      x = z,                    q = sigmoid(z), t = y
//   bin = number of edges e (float32, x-space) with x >= e;  brier += (q - t)^2
//
// Cells.  256 rows x 62 elements land on 32 (group, bin) cells.  Every lane owns a private 8-byte slot
// {count | hits << 16, sum_q} per cell in LDS: cell c of wave w, lane l sits at dword w * WAVE_DW + c * CELL_DW + 2 l.
// A lane is the only writer of its slots, so the update is a plain ds_read_b64 / ds_write_b64 pair: no atomics of any
// kind, and a lane's float sum is formed in element order 0..61.  CELL_DW = 128 is 0 mod 64 banks, so the bank of
// a slot depends on the lane alone (2 l, 2 l + 1), not on the cell: the lanes of a group never conflict, whichever
// bins the data sends them to (a stride that is not 0 mod 64 would make lanes l and l' collide whenever their bins
// differ by (l' - l) / 2 strides).  The reduction then reads cells that all start on bank 0: lane l sums the 32 slots
// of parity l & 1 of cell c = l >> 1 starting at slot pair c and wrapping, so at step j it is on bank
// 4 ((j + c) & 15) + 2 (l & 1), distinct for the 32 lanes of a group.
//
// Order of every float sum (bit-reproducible run to run; it depends on nothing but the cell index): a lane's
// elements in order; a cell's even slots from slot pair c upwards, wrapping at 32, and its odd slots likewise,
// even + odd; the block's waves ((w0 + w1) + (w2 + w3)).  Brier: a lane's elements in order, the wave butterfly of
// wave_sum, the waves as above.  One row of partials per block, summed by the host in int64 / fp64.
#include <cmath>

#include "common.h"
#include "draw_topk.h"  // MAIN_BITS, STAR_BITS

namespace {

constexpr int CAL_BINS = 16, CAL_EDGES = 15, CAL_CELLS = 2 * CAL_BINS;
constexpr int CELL_DW = 128;                  // dwords between the cells of one wave: 64 slots of 2 dwords, 0 mod 64 banks
constexpr int WAVE_DW = CAL_CELLS * CELL_DW;  // 4096 dwords = 16 KiB per wave, 64 KiB per block

struct CalEdges {
  float e[CAL_EDGES];  // x-space, ascending; entries past n_edges are NaN (x >= NaN is false)
};

EM_DEVICE int bin_of(float x, const CalEdges& ed) {
  int b = 0;
#pragma unroll
  for (int k = 0; k < CAL_EDGES; ++k) b += x >= ed.e[k] ? 1 : 0;
  return b;
}

__global__ void __launch_bounds__(256)
draw_calibration_kernel(const float* __restrict__ logits, int ld, const uint64_t* __restrict__ masks,
                        const int32_t* __restrict__ sidx, int64_t B, int64_t offset, int loss_kind, CalEdges ed,
                        int32_t* __restrict__ counts, int32_t* __restrict__ hits, float* __restrict__ sum_q,
                        float* __restrict__ brier, uint8_t* __restrict__ bins) {
  __shared__ __attribute__((aligned(16))) uint32_t cells[4 * WAVE_DW];
  __shared__ uint32_t red_n[4][CAL_CELLS];
  __shared__ float red_q[4][CAL_CELLS];
  __shared__ float red_b[4][2];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint32_t* mine = cells + w * WAVE_DW + 2 * lane;  // this lane's slot of cell 0
#pragma unroll
  for (int c = 0; c < CAL_CELLS; ++c) *reinterpret_cast<u32x2*>(mine + c * CELL_DW) = u32x2{0u, 0u};

  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  float br_m = 0.f, br_s = 0.f;
  if (s < B) {
    const int64_t idx = sidx ? (int64_t)sidx[s] : offset + s;
    const uint64_t tm = masks[idx + 1] & (MAIN_BITS | STAR_BITS);
    float z[64];
    const f32x4* zr = reinterpret_cast<const f32x4*>(logits + s * ld);
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const f32x4 v = zr[k];
      z[4 * k] = v[0]; z[4 * k + 1] = v[1]; z[4 * k + 2] = v[2]; z[4 * k + 3] = v[3];
    }
    float lsm = 0.f, lss = 0.f;
    if (loss_kind == 0) {
      float mm = -3.0e38f, ms = -3.0e38f;
      for (int o = 0; o < 50; ++o) mm = fmaxf(mm, z[o]);
      for (int o = 50; o < 62; ++o) ms = fmaxf(ms, z[o]);
      float sm = 0.f, ss = 0.f;
      for (int o = 0; o < 50; ++o) sm += __expf(z[o] - mm);
      for (int o = 50; o < 62; ++o) ss += __expf(z[o] - ms);
      lsm = mm + __logf(sm);
      lss = ms + __logf(ss);
    }
    uint32_t packed[16];  // the row's bins, 4 per word (pads 0)
#pragma unroll
    for (int k = 0; k < 16; ++k) packed[k] = 0u;
#pragma unroll
    for (int o = 0; o < 62; ++o) {
      const bool main_o = o < 50;
      const uint32_t y = (uint32_t)(tm >> o) & 1u;
      float x, q, t;
      if (loss_kind == 0) {
        x = z[o] - (main_o ? lsm : lss);
        q = __expf(x);
        t = y ? (main_o ? 0.2f : 0.5f) : 0.f;
      } else {
        x = z[o];
        q = 1.f / (1.f + __expf(-x));
        t = (float)y;
      }
      const int b = bin_of(x, ed);
      packed[o >> 2] |= (uint32_t)b << (8 * (o & 3));
      u32x2* cell = reinterpret_cast<u32x2*>(mine + ((main_o ? 0 : CAL_BINS) + b) * CELL_DW);
      const u32x2 c = *cell;
      const uint32_t n0 = c[0], q0 = c[1];  // (scalars first: a bit cast straight from a vector element reads lane 0)
      *cell = u32x2{n0 + 1u + (y << 16), __float_as_uint(__uint_as_float(q0) + q)};
      const float d = q - t;
      if (main_o) br_m += d * d;
      else br_s += d * d;
    }
    if (bins) {
      u32x4* br = reinterpret_cast<u32x4*>(bins + s * 64);
#pragma unroll
      for (int k = 0; k < 4; ++k) br[k] = u32x4{packed[4 * k], packed[4 * k + 1], packed[4 * k + 2], packed[4 * k + 3]};
    }
  }
  br_m = wave_sum(br_m);
  br_s = wave_sum(br_s);
  if (lane == 0) {
    red_b[w][0] = br_m;
    red_b[w][1] = br_s;
  }
  __syncthreads();
  {  // the wave's 64 slots of cell c = lane >> 1: this lane takes the slots of parity lane & 1, from slot pair c on
    const int c0 = lane >> 1;
    const uint32_t* src = cells + w * WAVE_DW + c0 * CELL_DW + 2 * (lane & 1);
    uint32_t n = 0u;
    float q = 0.f;
#pragma unroll 8
    for (int j = 0; j < 32; ++j) {
      const u32x2 c = *reinterpret_cast<const u32x2*>(src + 4 * ((j + c0) & 31));
      const uint32_t n0 = c[0], q0 = c[1];
      n += n0;  // count <= 64 * 50 and hits <= 64 * 5 per wave: the 16-bit halves cannot carry
      q += __uint_as_float(q0);
    }
    n += __shfl_xor(n, 1);
    const float qo = __shfl_xor(q, 1);
    if ((lane & 1) == 0) {
      red_n[w][lane >> 1] = n;
      red_q[w][lane >> 1] = q + qo;  // even slots + odd slots
    }
  }
  __syncthreads();
  if (threadIdx.x < CAL_CELLS) {
    const int c = threadIdx.x;
    const uint32_t n = (red_n[0][c] + red_n[1][c]) + (red_n[2][c] + red_n[3][c]);  // <= 256 * 50: no carry
    const int64_t at = (int64_t)blockIdx.x * CAL_CELLS + c;
    counts[at] = (int32_t)(n & 0xFFFFu);
    hits[at] = (int32_t)(n >> 16);
    sum_q[at] = (red_q[0][c] + red_q[1][c]) + (red_q[2][c] + red_q[3][c]);
  } else if (threadIdx.x < CAL_CELLS + 2) {
    const int g = threadIdx.x - CAL_CELLS;
    brier[(int64_t)blockIdx.x * 2 + g] = (red_b[0][g] + red_b[1][g]) + (red_b[2][g] + red_b[3][g]);
  }
}

}  // namespace

// rows of counts / hits / sum_q / brier that em_draw_calibration writes: one per 256-row block
EM_API int em_calibration_blocks(int64_t B) { return B > 0 && B <= 2147483646ll ? (int)((B + 255) / 256) : 0; }

// counts, hits int32 [blocks][2][16], sum_q fp32 [blocks][2][16], brier fp32 [blocks][2]; bins (optional) uint8
// [B][64], pads 0.  `edges`: HOST pointer to n_edges float32 x-space edges (passed on as a kernel argument); their
// order is the caller's to check.  Any refusal returns EM_ERR_ARG before a launch: the outputs are untouched.
EM_API int em_draw_calibration(const float* logits, int ld, const uint64_t* masks, const int32_t* sidx, int64_t B,
                               int64_t offset, int loss_kind, const float* edges, int n_edges, int32_t* counts,
                               int32_t* hits, float* sum_q, float* brier, uint8_t* bins, hipStream_t stream) {
  if (!logits || !masks || !counts || !hits || !sum_q || !brier) return EM_ERR_ARG;
  if (n_edges < 0 || n_edges > CAL_EDGES || (n_edges > 0 && !edges)) return EM_ERR_ARG;
  if (ld < 64 || (ld & 3) || B < 1 || B > 2147483646ll || offset < 0) return EM_ERR_ARG;
  if (loss_kind < 0 || loss_kind > 1) return EM_ERR_ARG;
  if (((uintptr_t)logits & 15) || ((uintptr_t)bins & 15)) return EM_ERR_ARG;
  CalEdges ed;
  for (int k = 0; k < CAL_EDGES; ++k) ed.e[k] = k < n_edges ? edges[k] : NAN;
  const int64_t nb = (B + 255) / 256;
  hipLaunchKernelGGL(draw_calibration_kernel, dim3((unsigned)nb), dim3(256), 0, stream, logits, ld, masks, sidx, B,
                     offset, loss_kind, ed, counts, hits, sum_q, brier, bins);
  EM_CHECK_LAUNCH();
  return 0;
}

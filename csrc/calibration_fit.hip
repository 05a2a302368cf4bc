// Per-group scaling of 62-wide draw logits (specification: euromillioner_amd/scaling.py): the loss, gradient and
// Hessian sums a Newton fit of the scale a[g] (and, under the sigmoid head, the shift b[g]) needs, and the apply pass.
//
// Groups: g = 0 is outputs 0-49, g = 1 is outputs 50-61; columns 62-63 are loaded with their 16 bytes and never used.
// The calibrated logit is u = fl32(fl32(a[g] * z) + b[g]): two separately rounded operations (scaled() below),
// never an fma, so numpy float32 arithmetic gives the same bits.
//
// Addressing as em_draw_calibration (csrc/calibration.hip): one row per lane, 16 loads of 16 bytes, row s scored
// against masks[idx + 1] with idx = sidx ? sidx[s] : offset + s.  With y the target bits of the group and
// n = max(popcount(y), 1), a row adds to the six statistics of its group (order L, g_a, g_b, h_aa, h_ab, h_bb):
//   softmax  m = max u, S = sum exp(u - m), q = exp(u - m) / S, E = sum q z, zy = sum y z / n
//            L = (m + log S) - a zy      g_a = E - zy      h_aa = sum q (z - E)^2 (a second pass, once E is known;
//            exp(u - m) is recomputed there from the z still in registers)      g_b = h_ab = h_bb = 0
//   bce      e = exp(-|u|), r = 1 / (1 + e), sigma = u >= 0 ? r : e r, w = e r r
//            L = sum max(u, 0) + log(1 + e) - y u      g_a = sum (sigma - y) z      g_b = sum (sigma - y)
//            h_aa = sum w z z      h_ab = sum w z      h_bb = sum w
// Every exponent is <= 0 and every logarithm's argument is in [1, 50], so the sums stay finite for |u| up to 1000 and
// beyond.  exp and log are __expf / __logf; tests/_scaling_ref.py derives the error budget from these formulas.
//
// Order of every float sum (bit-reproducible; it depends on nothing but the row's place in its block): a lane's
// elements in order 0..61 (each group its own accumulator), the wave butterfly of wave_sum, the block's waves as
// (w0 + w1) + (w2 + w3).  Rows at or past B are not read and add 0.  No atomics: one [2][6] row of partials per block,
// summed by the host in fp64.
#include <cmath>

#include "common.h"
#include "draw_topk.h"  // MAIN_BITS, STAR_BITS

namespace {

constexpr int SC_STATS = 6;

struct ScaleAB {
  float a[2], b[2];
};

EM_DEVICE void load_row(const float* __restrict__ row, float (&z)[64]) {
  const f32x4* zr = reinterpret_cast<const f32x4*>(row);
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const f32x4 v = zr[k];
    z[4 * k] = v[0]; z[4 * k + 1] = v[1]; z[4 * k + 2] = v[2]; z[4 * k + 3] = v[3];
  }
}

// fl32(a * z) and fl32(fl32(a * z) + b).  The HIP headers define __fmul_rn / __fadd_rn as the plain operators inside
// their own scope, where the compiler's default contraction still fuses them with a neighbouring sum (the first
// build of this file came out as v_pk_fma_f32 and was one ulp off numpy).  So the operators are written out here with
// contraction switched off: each operation rounds on its own whatever the expression is inlined into.
EM_DEVICE float scale_rn(float a, float z) {
#pragma clang fp contract(off)
  const float p = a * z;
  return p;
}

EM_DEVICE float scaled(float a, float b, float z) {
#pragma clang fp contract(off)
  const float p = a * z;
  const float u = p + b;
  return u;
}

// exp(u - m): the difference rounds on its own (never an fma of a, z and -m)
EM_DEVICE float exp_below(float u, float m) {
#pragma clang fp contract(off)
  const float d = u - m;
  return __expf(d);
}

template <int LO, int HI>
EM_DEVICE void softmax_group(const float (&z)[64], uint64_t tm, float a, float* __restrict__ st) {
  float m = -3.0e38f;
#pragma unroll
  for (int o = LO; o < HI; ++o) m = fmaxf(m, scale_rn(a, z[o]));
  float S = 0.f, T = 0.f, ys = 0.f;
#pragma unroll
  for (int o = LO; o < HI; ++o) {
    const float e = exp_below(scale_rn(a, z[o]), m);
    S += e;
    T += e * z[o];
    ys += ((tm >> o) & 1ull) ? z[o] : 0.f;
  }
  const int n = __popcll(tm & (((1ull << (HI - LO)) - 1ull) << LO));
  const float zy = ys / (float)(n > 1 ? n : 1);
  const float r = __builtin_amdgcn_rcpf(S);
  const float E = T * r;
  float V = 0.f;
#pragma unroll
  for (int o = LO; o < HI; ++o) {
    const float e = exp_below(scale_rn(a, z[o]), m);
    const float d = z[o] - E;
    V += e * (d * d);
  }
  st[0] = (m + __logf(S)) - a * zy;
  st[1] = E - zy;
  st[2] = 0.f;
  st[3] = V * r;
  st[4] = 0.f;
  st[5] = 0.f;
}

template <int LO, int HI>
EM_DEVICE void bce_group(const float (&z)[64], uint64_t tm, float a, float b, float* __restrict__ st) {
  float L = 0.f, ga = 0.f, gb = 0.f, haa = 0.f, hab = 0.f, hbb = 0.f;
#pragma unroll
  for (int o = LO; o < HI; ++o) {
    const bool y = (tm >> o) & 1ull;
    const float u = scaled(a, b, z[o]);
    const float e = __expf(-fabsf(u));
    const float r = __builtin_amdgcn_rcpf(1.f + e);
    const float er = e * r;
    const float sg = u >= 0.f ? r : er;
    const float w = er * r;
    L += (fmaxf(u, 0.f) + __logf(1.f + e)) - (y ? u : 0.f);
    const float d = sg - (y ? 1.f : 0.f);
    ga += d * z[o];
    gb += d;
    const float wz = w * z[o];
    haa += wz * z[o];
    hab += wz;
    hbb += w;
  }
  st[0] = L; st[1] = ga; st[2] = gb; st[3] = haa; st[4] = hab; st[5] = hbb;
}

__global__ void __launch_bounds__(256)
scaling_stats_kernel(const float* __restrict__ logits, int ld, const uint64_t* __restrict__ masks,
                     const int32_t* __restrict__ sidx, int64_t B, int64_t offset, int loss_kind, ScaleAB p,
                     float* __restrict__ stats) {
  __shared__ float red[4][2 * SC_STATS];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  float st[2 * SC_STATS];
#pragma unroll
  for (int k = 0; k < 2 * SC_STATS; ++k) st[k] = 0.f;
  if (s < B) {
    const int64_t idx = sidx ? (int64_t)sidx[s] : offset + s;
    const uint64_t tm = masks[idx + 1] & (MAIN_BITS | STAR_BITS);
    float z[64];
    load_row(logits + s * ld, z);
    if (loss_kind == 0) {
      softmax_group<0, 50>(z, tm, p.a[0], st);
      softmax_group<50, 62>(z, tm, p.a[1], st + SC_STATS);
    } else {
      bce_group<0, 50>(z, tm, p.a[0], p.b[0], st);
      bce_group<50, 62>(z, tm, p.a[1], p.b[1], st + SC_STATS);
    }
  }
#pragma unroll
  for (int k = 0; k < 2 * SC_STATS; ++k) {
    const float v = wave_sum(st[k]);
    if (lane == 0) red[w][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < 2 * SC_STATS) {
    const int k = threadIdx.x;
    stats[(int64_t)blockIdx.x * (2 * SC_STATS) + k] = (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
  }
}

__global__ void __launch_bounds__(256)
scaling_apply_kernel(const float* logits, int ld, int64_t B, ScaleAB p, float* out, int ldo) {
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (s >= B) return;
  float z[64];
  load_row(logits + s * ld, z);  // the whole row is in registers before the first store: out may be logits
#pragma unroll
  for (int o = 0; o < 62; ++o) z[o] = scaled(p.a[o < 50 ? 0 : 1], p.b[o < 50 ? 0 : 1], z[o]);
  z[62] = 0.f;
  z[63] = 0.f;
  f32x4* dst = reinterpret_cast<f32x4*>(out + s * ldo);
#pragma unroll
  for (int k = 0; k < 16; ++k) dst[k] = f32x4{z[4 * k], z[4 * k + 1], z[4 * k + 2], z[4 * k + 3]};
}

// a finite and > 0, b finite (and 0 under the softmax head, where the shift cancels)
bool scale_ok(const float* a, const float* b, int loss_kind, ScaleAB* p) {
  if (!a || !b) return false;
  for (int g = 0; g < 2; ++g) {
    if (!std::isfinite(a[g]) || !(a[g] > 0.f) || !std::isfinite(b[g])) return false;
    if (loss_kind == 0 && b[g] != 0.f) return false;
    p->a[g] = a[g];
    p->b[g] = b[g];
  }
  return true;
}

}  // namespace

// rows of stats that em_scaling_stats writes: one per 256-row block
EM_API int em_scaling_blocks(int64_t B) { return B > 0 && B <= 2147483646ll ? (int)((B + 255) / 256) : 0; }

// stats fp32 [blocks][2][6].  `a`, `b`: HOST pointers to two floats each (passed on as a kernel argument).  Any
// refusal returns EM_ERR_ARG before a launch: stats is untouched.
EM_API int em_scaling_stats(const float* logits, int ld, const uint64_t* masks, const int32_t* sidx, int64_t B,
                            int64_t offset, int loss_kind, const float* a, const float* b, float* stats,
                            hipStream_t stream) {
  if (!logits || !masks || !stats) return EM_ERR_ARG;
  if (ld < 64 || (ld & 3) || B < 1 || B > 2147483646ll || offset < 0) return EM_ERR_ARG;
  if (loss_kind < 0 || loss_kind > 1) return EM_ERR_ARG;
  if ((uintptr_t)logits & 15) return EM_ERR_ARG;
  ScaleAB p;
  if (!scale_ok(a, b, loss_kind, &p)) return EM_ERR_ARG;
  const int64_t nb = (B + 255) / 256;
  hipLaunchKernelGGL(scaling_stats_kernel, dim3((unsigned)nb), dim3(256), 0, stream, logits, ld, masks, sidx, B,
                     offset, loss_kind, p, stats);
  EM_CHECK_LAUNCH();
  return 0;
}

// out[s][o] = u for o < 62 and 0 for o = 62, 63, rows of ldo floats; out may be logits itself (then ldo == ld).
EM_API int em_scaling_apply(const float* logits, int ld, int64_t B, const float* a, const float* b, float* out,
                            int ldo, hipStream_t stream) {
  if (!logits || !out) return EM_ERR_ARG;
  if (ld < 64 || (ld & 3) || ldo < 64 || (ldo & 3) || B < 1 || B > 2147483646ll) return EM_ERR_ARG;
  if (((uintptr_t)logits & 15) || ((uintptr_t)out & 15)) return EM_ERR_ARG;
  if (out == logits && ldo != ld) return EM_ERR_ARG;
  ScaleAB p;
  if (!scale_ok(a, b, 1, &p)) return EM_ERR_ARG;
  const int64_t nb = (B + 255) / 256;
  hipLaunchKernelGGL(scaling_apply_kernel, dim3((unsigned)nb), dim3(256), 0, stream, logits, ld, B, p, out, ldo);
  EM_CHECK_LAUNCH();
  return 0;
}

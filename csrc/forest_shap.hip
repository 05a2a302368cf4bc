// Random-forest explanations on the device: path-dependent TreeSHAP contributions of predict_proba and leaf
// indices.  The specification is euromillioner_amd/models/forest_explain.py.
//
// A forest leaf holds a 62-vector and the Shapley weight of a (row, leaf, path feature) does not depend on the
// output, so the decomposition differs from gbdt_shap (one lane per row): here a wave owns a ROW and lane o owns
// OUTPUT o.  The weight is computed once and applied to the leaf's whole 64-wide value row.
//
//   rf_shap_paths   one thread per (tree, heap slot) that the host marked as a leaf (slot[e] = its index in the
//                   compacted table, trees ascending then heap slots ascending): d path features (one byte
//                   each, F <= 256), the side taken at each as a bit, z_j = cover[child] / cover[parent] in
//                   float32, the leaf's value row, and the bias terms value[o] * prod z in fp64
//   rf_shap_bias    lane o: the bias terms of output o in fp64, 16 waves over contiguous segments of the table
//                   and their partial sums in wave order (a fixed order for a given table), times 1/T
//   rf_shap<MAXD>   a wave takes one row at a time (a block is RS_WAVES waves that share nothing; one wave
//                   measured as fast as four and faster than two, docs/DESIGN.md 6i).  The row's accumulators
//                   live in LDS as [F][65] floats, lane o at f * 65 + o: conflict-free in the leaf loop (a
//                   wave-uniform f, consecutive lanes) and in the transposing store of the epilogue.
//                   Phase A: the wave takes 64 leaves of the table, one per lane; a lane forms o_j from the
//                   row's bits and evaluates its leaf's weights (o_i - z_i) * sum_s w_s c_s once.  Leaves with
//                   d < MAXD are padded with null players (z = 1, o = 1), which leaves the other features'
//                   Shapley values unchanged, so every lane runs the same unrolled code without divergence.
//                   Phase B: the wave walks those leaves in table order; leaf k's d, features and weights are
//                   read from lane k (v_readlane, k wave-uniform), the value row is one coalesced 256-byte
//                   load (prefetched 4 leaves ahead), and every lane does acc[f][lane] += w * value[lane].
//                   A path's features are distinct (the host validates), so a leaf's d accumulators are read
//                   together and written together: one LDS round trip per leaf.
//                   Trees ascending, heap slots ascending, features in path order, no atomics: a row's result
//                   depends on nothing but the row.
//   rf_leaf_index   the predict walk, storing the node index (any W, any depth)
#include "common.h"

namespace {

constexpr int RS_AS = 65;                  // accumulator row stride in floats (odd)
constexpr int RS_MAX_DEPTH = 8;
constexpr int RS_MAX_F = 256;              // the forest's own limit; path features are stored as bytes
constexpr int RS_LDS_MAX = 160 * 1024;
constexpr int RS_OUT = 62;
constexpr int RS_MAX_WAVES = 4;
#ifndef RS_WAVES
#define RS_WAVES 1  // rows (= waves) per block, as far as the LDS holds them; an A/B knob: a side library with
                    // -DRS_WAVES=n comes from tools/build_variant.sh, timed by tools/rf_shap_bench.py --kernel-only
#endif

inline int rs_lds_bytes(int F) { return F * RS_AS * 4; }

__global__ void rf_shap_paths(int T, int NN, int S, int F, const int32_t* __restrict__ slot,
                              const int16_t* __restrict__ feat, const float* __restrict__ value,
                              const float* __restrict__ cover, int32_t* __restrict__ pd, uint8_t* __restrict__ pf,
                              float* __restrict__ pz, float* __restrict__ pval, double* __restrict__ pbias) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (int64_t)T * NN) return;
  const int64_t s = slot[e];
  if (s < 0) return;
  const int i = (int)(e % NN);
  const int64_t o = e - i;  // the tree's first node
  int depth = 31 - __clz(i + 1);
  if (depth > S) depth = S;  // (the host sizes S = max_depth: never taken)
  int side = 0;
  double zb = 1.0;
  for (int lvl = 0; lvl < 8; ++lvl) pf[s * 8 + lvl] = 0;
  for (int lvl = 0; lvl < S; ++lvl) pz[s * S + lvl] = 1.f;
  for (int lvl = 0; lvl < depth; ++lvl) {
    const int p = ((i + 1) >> (depth - lvl)) - 1, c = ((i + 1) >> (depth - lvl - 1)) - 1;
    int f = feat[o + p];
    if (f < 0 || f >= F) f = 0;  // (the host validates; never index by a bad feat)
    const float cp = cover[o + p], cc = cover[o + c];
    pf[s * 8 + lvl] = (uint8_t)f;
    side |= (c - (2 * p + 1)) << lvl;
    pz[s * S + lvl] = cc / cp;
    zb *= (double)cc / (double)cp;
  }
  pd[s] = depth | (side << 8);
  for (int q = 0; q < 64; ++q) {
    const float v = value[e * 64 + q];
    pval[s * 64 + q] = v;
    pbias[s * 64 + q] = (double)v * zb;
  }
}

// Two levels in a fixed order: wave w sums the leaves of its contiguous segment in table order, wave 0 then adds
// the RS_BIAS_WAVES partial sums in wave order.  The result depends on L only.
constexpr int RS_BIAS_WAVES = 16;
__global__ __launch_bounds__(64 * RS_BIAS_WAVES) void rf_shap_bias(const double* __restrict__ pbias, int L, int T,
                                                                   float* __restrict__ out) {
  __shared__ double part[RS_BIAS_WAVES][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int seg = (L + RS_BIAS_WAVES - 1) / RS_BIAS_WAVES;
  const int e1 = min(L, (wave + 1) * seg);
  double s = 0.0;
  for (int e = wave * seg; e < e1; ++e) s += pbias[(int64_t)e * 64 + lane];
  part[wave][lane] = s;
  __syncthreads();
  if (wave == 0) {
    double tot = 0.0;
    for (int w = 0; w < RS_BIAS_WAVES; ++w) tot += part[w][lane];
    out[lane] = lane < RS_OUT ? (float)(tot / (double)T) : 0.f;
  }
}

// s! (d-1-s)! / d!
constexpr double rs_fact(int k) {
  double r = 1.0;
  for (int i = 2; i <= k; ++i) r *= i;
  return r;
}
template <int d>
struct RsWeights {  // a compile-time table: the unrolled loops below read constants
  float w[d];
  constexpr RsWeights() : w{} {
    for (int s = 0; s < d; ++s) w[s] = (float)(rs_fact(s) * rs_fact(d - 1 - s) / rs_fact(d));
  }
};

EM_DEVICE float rs_lane_f(float v, int k) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), k));
}

// Leaf k of the wave's 64 (d path features) into every lane's accumulator column.
template <int d, int MAXD>
EM_DEVICE void rs_apply(const float (&t)[MAXD], uint32_t flo, uint32_t fhi, int k, float v, float* acc_lane) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)flo, k);
  const uint32_t hi = d > 4 ? (uint32_t)__builtin_amdgcn_readlane((int)fhi, k) : 0u;
  int f[d];
  float a[d], w[d];
#pragma unroll
  for (int j = 0; j < d; ++j) {
    f[j] = (int)(((j < 4 ? lo : hi) >> (8 * (j & 3))) & 255u) * RS_AS;
    w[j] = rs_lane_f(t[j], k);
    a[j] = acc_lane[f[j]];
  }
#pragma unroll
  for (int j = 0; j < d; ++j) a[j] = fmaf(w[j], v, a[j]);
#pragma unroll
  for (int j = 0; j < d; ++j) acc_lane[f[j]] = a[j];
}

template <int MAXD>
__global__ __launch_bounds__(64 * RS_MAX_WAVES) void rf_shap(const uint64_t* __restrict__ X, int W, int n, int F, int L,
                                                             const int32_t* __restrict__ pd,
                                                             const uint32_t* __restrict__ pf,
                                                             const float* __restrict__ pz,
                                                             const float* __restrict__ pval,
                                                             const float* __restrict__ bias, float n_trees,
                                                             float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), waves = blockDim.x >> 6;
  float* acc = reinterpret_cast<float*>(smem) + wave * F * RS_AS;  // this wave's [F][RS_AS]; waves share nothing
  float* acc_lane = acc + lane;
  constexpr RsWeights<MAXD> WT{};
  const int OW = F + 1;
  for (int r = blockIdx.x * waves + wave; r < n; r += gridDim.x * waves) {
    // the row's bits: wave-uniform (scalar loads)
    const uint64_t* xr = X + (int64_t)r * W;
    const uint64_t x0 = xr[0], x1 = W > 1 ? xr[1] : 0ull, x2 = W > 2 ? xr[2] : 0ull, x3 = W > 3 ? xr[3] : 0ull;
    for (int f = 0; f < F; ++f) acc_lane[f * RS_AS] = 0.f;
    for (int base = 0; base < L; base += 64) {
      const int cnt = min(64, L - base);
      // ---- phase A: lane = leaf base + lane
      float t[MAXD];
      uint32_t flo = 0u, fhi = 0u;
      int dreg = 0;
      {
        const int e = base + lane;
        float z[MAXD], o[MAXD];
        int side = 0;
        if (e < L) {
          const int m = pd[e];
          dreg = m & 255, side = m >> 8;
          flo = pf[2 * (int64_t)e];
          if (MAXD > 4) fhi = pf[2 * (int64_t)e + 1];
#pragma unroll
          for (int j = 0; j < MAXD; ++j) z[j] = pz[(int64_t)e * MAXD + j];
        } else {
#pragma unroll
          for (int j = 0; j < MAXD; ++j) z[j] = 1.f;
        }
#pragma unroll
        for (int j = 0; j < MAXD; ++j) {
          const uint32_t f = ((j < 4 ? flo : fhi) >> (8 * (j & 3))) & 255u;
          const uint32_t ws = f >> 6;
          const uint64_t xw = ws == 0 ? x0 : ws == 1 ? x1 : ws == 2 ? x2 : x3;
          const int bit = (int)((xw >> (f & 63u)) & 1ull);
          o[j] = ((j >= dreg) | (bit == ((side >> j) & 1))) ? 1.f : 0.f;  // (padding: a null player, z = 1, o = 1)
        }
#pragma unroll
        for (int i = 0; i < MAXD; ++i) {
          float c[MAXD];  // coefficients of prod_{j != i} (z_j + o_j x)
          c[0] = 1.f;
#pragma unroll
          for (int s = 1; s < MAXD; ++s) c[s] = 0.f;
          int deg = 0;
#pragma unroll
          for (int j = 0; j < MAXD; ++j) {
            if (j == i) continue;
#pragma unroll
            for (int s = deg + 1; s >= 1; --s) c[s] = fmaf(c[s - 1], o[j], c[s] * z[j]);
            c[0] *= z[j];
            ++deg;
          }
          float w = 0.f;
#pragma unroll
          for (int s = 0; s < MAXD; ++s) w = fmaf(WT.w[s], c[s], w);
          t[i] = (o[i] - z[i]) * w;
        }
      }
      // ---- phase B: the 64 leaves in table order, every lane its own output
      const float* vb = pval + (int64_t)base * 64 + lane;
      float vq[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) vq[u] = u < cnt ? vb[u * 64] : 0.f;
      for (int k0 = 0; k0 < cnt; k0 += 4) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int k = k0 + u;
          if (k >= cnt) break;
          const float v = vq[u];
          vq[u] = k + 4 < cnt ? vb[(k + 4) * 64] : 0.f;
          const int dk = __builtin_amdgcn_readlane(dreg, k);
          switch (dk) {
            case 1: rs_apply<1, MAXD>(t, flo, fhi, k, v, acc_lane); break;
            case 2: if constexpr (MAXD >= 2) rs_apply<2, MAXD>(t, flo, fhi, k, v, acc_lane); break;
            case 3: if constexpr (MAXD >= 3) rs_apply<3, MAXD>(t, flo, fhi, k, v, acc_lane); break;
            case 4: if constexpr (MAXD >= 4) rs_apply<4, MAXD>(t, flo, fhi, k, v, acc_lane); break;
            case 5: if constexpr (MAXD >= 5) rs_apply<5, MAXD>(t, flo, fhi, k, v, acc_lane); break;
            case 6: if constexpr (MAXD >= 6) rs_apply<6, MAXD>(t, flo, fhi, k, v, acc_lane); break;
            case 7: if constexpr (MAXD >= 7) rs_apply<7, MAXD>(t, flo, fhi, k, v, acc_lane); break;
            case 8: if constexpr (MAXD >= 8) rs_apply<8, MAXD>(t, flo, fhi, k, v, acc_lane); break;
            default: break;  // a root leaf: bias only
          }
        }
      }
    }
    wave_lds_sync();
    // transpose out: out[r][o][0 .. F], the row's 62 x (F + 1) floats are one contiguous run
    float* dst = out + (int64_t)r * RS_OUT * OW;
    int o = 0, c = lane;
    while (c >= OW) c -= OW, ++o;
    for (int e = lane; e < RS_OUT * OW; e += 64) {
      dst[e] = c < F ? acc[c * RS_AS + o] / n_trees : bias[o];  // (one correctly rounded division for the 1/T)
      c += 64;
      while (c >= OW) c -= OW, ++o;
    }
    wave_lds_sync();
  }
}

__global__ void rf_leaf_index(const uint64_t* __restrict__ X, int W, int64_t n, const int16_t* __restrict__ feat,
                              int T, int NN, int max_depth, int32_t* __restrict__ out) {
  const int64_t total = n * T;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = e / T;
    const int16_t* ft = feat + (e - r * T) * NN;
    const uint64_t* xr = X + r * W;
    int nd = 0;
    for (int lvl = 0; lvl < max_depth; ++lvl) {  // (bounded: a split never sits at the last level)
      const int f = ft[nd];
      if (f < 0) break;
      nd = 2 * nd + 1 + (int)((xr[f >> 6] >> (f & 63)) & 1ull);
    }
    out[e] = nd;
  }
}

template <int MAXD>
int launch_rf_shap(int grid, int waves, int lds, hipStream_t stream, const uint64_t* X, int W, int n, int F, int L, const int32_t* pd,
                   const uint32_t* pf, const float* pz, const float* pval, const float* bias, float n_trees, float* out) {
  if (lds > 64 * 1024) {  // beyond the default limit (F > 252): per device and per call, no state kept here
    hipError_t e = hipFuncSetAttribute((const void*)rf_shap<MAXD>, hipFuncAttributeMaxDynamicSharedMemorySize, RS_LDS_MAX);
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(rf_shap<MAXD>, dim3(grid), dim3(64 * waves), lds, stream, X, W, n, F, L, pd, pf, pz, pval, bias, n_trees, out);
  EM_CHECK_LAUNCH();
  return 0;
}

}  // namespace

// LDS bytes of the contribution kernel's row tile at F features, or -1 when the plan does not cover the shape
EM_API int em_rf_shap_lds_bytes(int F, int max_depth) {
  if (F < 1 || F > RS_MAX_F || max_depth < 0 || max_depth > RS_MAX_DEPTH) return -1;
  return rs_lds_bytes(F);
}

// The leaf-path table of a forest of T trees with L leaves (slot[T * nodes]: the leaf's table index, or -1) and
// the bias row bias_out[64].  Tables: pd[L], pf[L * 8] bytes, pz[L * max(1, max_depth)], pval[L * 64], pbias[L * 64].
EM_API int em_rf_shap_paths(int T, int max_depth, int F, int L, const int32_t* slot, const int16_t* feat,
                            const float* value, const float* cover, int32_t* pd, uint8_t* pf, float* pz, float* pval,
                            double* pbias, float* bias_out, hipStream_t stream) {
  if (!slot || !feat || !value || !cover || !pd || !pf || !pz || !pval || !pbias || !bias_out || T < 1 || L < 1 ||
      em_rf_shap_lds_bytes(F, max_depth) < 0)
    return EM_ERR_ARG;
  const int NN = (1 << (max_depth + 1)) - 1;
  if ((int64_t)L > (int64_t)T * NN || (int64_t)L * 64 >= (1ll << 31)) return EM_ERR_ARG;
  const int S = max_depth > 1 ? max_depth : 1;
  const int64_t total = (int64_t)T * NN;
  hipLaunchKernelGGL(rf_shap_paths, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, T, NN, S, F, slot, feat,
                     value, cover, pd, pf, pz, pval, pbias);
  EM_CHECK_LAUNCH();
  hipLaunchKernelGGL(rf_shap_bias, dim3(1), dim3(64 * RS_BIAS_WAVES), 0, stream, pbias, L, T, bias_out);
  EM_CHECK_LAUNCH();
  return 0;
}

// out[n][62][F+1] = contributions of the forest's predict_proba on n packed rows X[n][W]; bias[64] from
// em_rf_shap_paths.
EM_API int em_rf_shap(const uint64_t* X, int W, int n, int F, int max_depth, int T, int L, const int32_t* pd,
                      const uint8_t* pf, const float* pz, const float* pval, const float* bias, float* out,
                      hipStream_t stream) {
  if (!X || !pd || !pf || !pz || !pval || !bias || !out || n < 0 || T < 1 || L < 1 || W < 1 || W > 4 || F > 64 * W ||
      em_rf_shap_lds_bytes(F, max_depth) < 0 || (((uintptr_t)pf) & 7))
    return EM_ERR_ARG;
  if (n == 0) return 0;
  int waves = RS_WAVES < RS_MAX_WAVES ? RS_WAVES : RS_MAX_WAVES;
  while (waves > 1 && waves * rs_lds_bytes(F) > RS_LDS_MAX) --waves;
  const int blocks = (n + waves - 1) / waves;
  const int grid = blocks < (1 << 20) ? blocks : (1 << 20);
  const int lds = waves * rs_lds_bytes(F);
  const uint32_t* pf4 = reinterpret_cast<const uint32_t*>(pf);
#define RS_LAUNCH(D) return launch_rf_shap<D>(grid, waves, lds, stream, X, W, n, F, L, pd, pf4, pz, pval, bias, (float)T, out)
  switch (max_depth) {
    case 0: case 1: RS_LAUNCH(1);
    case 2: RS_LAUNCH(2);
    case 3: RS_LAUNCH(3);
    case 4: RS_LAUNCH(4);
    case 5: RS_LAUNCH(5);
    case 6: RS_LAUNCH(6);
    case 7: RS_LAUNCH(7);
    default: RS_LAUNCH(8);
  }
#undef RS_LAUNCH
}

// out[n][T] = heap index of the node where row r stops in tree t
EM_API int em_rf_leaf_index(const uint64_t* X, int W, int64_t n, int F, const int16_t* feat, int T, int max_depth,
                            int32_t* out, hipStream_t stream) {
  if (!X || !feat || !out || n < 0 || T < 0 || W < 1 || F < 1 || F > 64 * W || max_depth < 0 || max_depth > 14)
    return EM_ERR_ARG;
  if (n == 0 || T == 0) return 0;
  const int NN = (1 << (max_depth + 1)) - 1;
  const int64_t total = n * T;
  const int grid = (int)(total + 255 < 256ll * 65536 ? (total + 255) / 256 : 65536);
  hipLaunchKernelGGL(rf_leaf_index, dim3(grid), dim3(256), 0, stream, X, W, n, feat, T, NN, max_depth, out);
  EM_CHECK_LAUNCH();
  return 0;
}

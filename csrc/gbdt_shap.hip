// GBDT explanations on the device: path-dependent TreeSHAP contributions and leaf indices.
//
// The specification is euromillioner_amd/models/gbdt_explain.py (division-free TreeSHAP over a leaf-path table).
//
//   gbdt_shap_paths   one thread per (tree, heap slot): the leaf's path as d distinct features with a bin
//                     interval (lo, hi], a zero fraction z = prod cover[child] / cover[parent] (float32) and the
//                     leaf's bias term leaf * prod z (fp64)
//   gbdt_shap_bias    one wave per task: the bias terms of the task's trees in [k0, k1) summed in fp64 in a
//                     fixed order, plus base_margin
//   gbdt_shap<MAXD>   a block is one wave: 64 rows of one task.  The tile's bins are staged transposed in LDS
//                     ([F][64] bytes), the F accumulators of a row live in LDS as [F][65] floats: lane r owns
//                     column r, so every access of the tree loop is conflict-free and needs no barrier.  Tree
//                     and path data depend on the block and the loop counters only: scalar loads.  Trees
//                     ascending, heap slots ascending, features in path order: a row's result depends on
//                     nothing but the row.  No atomics, no cross-block communication.  The output is written
//                     as [T][n][F+1]: the block's 64 x (F+1) floats are one contiguous run.
//                     The tile is 324 F bytes of LDS, which bounds the waves a CU holds (7 at F = 66).  The
//                     loop is a chain of scalar loads, LDS round trips and short VALU runs, so waves per SIMD
//                     is what hides its latency: 256-row blocks (4 waves, 85 KB, one block per CU) ran the
//                     183k-row benchmark 1.58x slower than 64-row blocks.
//   gbdt_leaf_index   gbdt_predict's walk, storing the node index
#include "common.h"

namespace {

constexpr int SHAP_ROWS = 64;             // rows per block == threads per block (one wave)
constexpr int SHAP_AS = SHAP_ROWS + 1;    // accumulator row stride in floats (odd: the transposing epilogue is conflict-free)
constexpr int SHAP_MAX_DEPTH = 8;         // == the fused engine's SPLIT_FINAL_MAX_DEPTH
constexpr int SHAP_LDS_MAX = 160 * 1024;  // LDS of one CU

inline int shap_lds_bytes(int F) { return F * SHAP_AS * 4 + F * SHAP_ROWS; }

inline int grid_1d(int64_t total) { return (int)((total + 255) / 256); }

__global__ void gbdt_shap_paths(int K, int NN, int S, int F, const int8_t* __restrict__ status,
                                const int16_t* __restrict__ feat, const uint8_t* __restrict__ sbin,
                                const float* __restrict__ leaf, const float* __restrict__ cover, int* __restrict__ pd,
                                float* __restrict__ pleaf, int* __restrict__ pf, int* __restrict__ plo,
                                int* __restrict__ phi, float* __restrict__ pz, double* __restrict__ pbias) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (int64_t)K * NN) return;
  const int i = (int)(e % NN);
  const int64_t o = e - i;  // the tree's first node
  int d = -1;
  double bias = 0.0;
  if (status[e] == 2) {
    const int depth = 31 - __clz(i + 1);
    const int64_t q = e * S;  // this entry's S path slots
    bool ok = depth <= S;
    double zb = 1.0;
    d = 0;
    for (int lvl = 0; ok && lvl < depth; ++lvl) {
      const int p = ((i + 1) >> (depth - lvl)) - 1, c = ((i + 1) >> (depth - lvl - 1)) - 1;
      const int f = feat[o + p], b = sbin[o + p];
      const float cp = cover[o + p], cc = cover[o + c];
      if (status[o + p] != 1 || f < 0 || f >= F || !(cp > 0.f)) {  // (the host validates; never index by a bad feat)
        ok = false;
        break;
      }
      int j = 0;
      while (j < d && pf[q + j] != f) ++j;
      if (j == d) {
        pf[q + j] = f, plo[q + j] = -1, phi[q + j] = 0x7fffffff, pz[q + j] = 1.f;
        ++d;
      }
      if (c == 2 * p + 2) plo[q + j] = max(plo[q + j], b);
      else phi[q + j] = min(phi[q + j], b);
      pz[q + j] *= cc / cp;
      zb *= (double)cc / (double)cp;
    }
    if (ok) bias = (double)leaf[e] * zb;
    else d = -1;
  }
  pd[e] = d;
  pleaf[e] = d >= 0 ? leaf[e] : 0.f;
  pbias[e] = bias;
}

__global__ __launch_bounds__(64) void gbdt_shap_bias(const double* __restrict__ pbias, const int* __restrict__ pd, int NN,
                                                     int T, int k0, int k1, double base, float* __restrict__ out) {
  const int t = blockIdx.x, lane = threadIdx.x;
  const int first = k0 + ((t - k0 % T) % T + T) % T;
  const int64_t trees = first < k1 ? (k1 - first + T - 1) / T : 0;
  double s = 0.0;
  for (int64_t m = lane; m < trees * NN; m += 64) {
    const int64_t e = (first + (m / NN) * T) * NN + m % NN;
    if (pd[e] >= 0) s += pbias[e];
  }
  s = wave_sum_d(s);
  if (lane == 0) out[t] = (float)(base + s);
}

// s! (d-1-s)! / d!
constexpr double shap_fact(int k) {
  double r = 1.0;
  for (int i = 2; i <= k; ++i) r *= i;
  return r;
}
template <int d>
struct ShapWeights {  // a compile-time table: the unrolled loops below read constants
  float w[d];
  constexpr ShapWeights() : w{} {
    for (int s = 0; s < d; ++s) w[s] = (float)(shap_fact(s) * shap_fact(d - 1 - s) / shap_fact(d));
  }
};

// One leaf with d distinct path features into this lane's accumulator column.
template <int d>
EM_DEVICE void shap_leaf(const int* __restrict__ pf, const int* __restrict__ plo, const int* __restrict__ phi,
                         const float* __restrict__ pz, float leafv, const uint8_t* sb_lane, float* acc_lane) {
  constexpr ShapWeights<d> W{};
  float z[d], o[d], a[d];
  int f[d];
  // the path's features are distinct, so are the d accumulators: read them all with the bins (one LDS round
  // trip per leaf), write them all at the end
#pragma unroll
  for (int j = 0; j < d; ++j) {
    f[j] = pf[j];
    z[j] = pz[j];
    a[j] = acc_lane[f[j] * SHAP_AS];
  }
#pragma unroll
  for (int j = 0; j < d; ++j) {
    const int b = sb_lane[f[j] * SHAP_ROWS];
    o[j] = ((b > plo[j]) & (b <= phi[j])) ? 1.f : 0.f;  // (& not &&: a select, no branch)
  }
#pragma unroll
  for (int i = 0; i < d; ++i) {
    float c[d];  // coefficients of prod_{j != i} (z_j + o_j x)
    c[0] = 1.f;
#pragma unroll
    for (int s = 1; s < d; ++s) c[s] = 0.f;
    int deg = 0;
#pragma unroll
    for (int j = 0; j < d; ++j) {
      if (j == i) continue;
#pragma unroll
      for (int s = deg + 1; s >= 1; --s) c[s] = fmaf(c[s - 1], o[j], c[s] * z[j]);
      c[0] *= z[j];
      ++deg;
    }
    float w = 0.f;
#pragma unroll
    for (int s = 0; s < d; ++s) w = fmaf(W.w[s], c[s], w);
    a[i] += leafv * (o[i] - z[i]) * w;
  }
#pragma unroll
  for (int i = 0; i < d; ++i) acc_lane[f[i] * SHAP_AS] = a[i];
}

template <int MAXD>
__global__ __launch_bounds__(SHAP_ROWS) void gbdt_shap(const uint8_t* __restrict__ bins, int n, int F, int T, int NN,
                                                       int S, int k0, int k1, const int* __restrict__ pd,
                                                       const float* __restrict__ pleaf, const int* __restrict__ pf,
                                                       const int* __restrict__ plo, const int* __restrict__ phi,
                                                       const float* __restrict__ pz, const float* __restrict__ bias,
                                                       float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* acc = reinterpret_cast<float*>(smem);                         // [F][SHAP_AS]
  uint8_t* sb = reinterpret_cast<uint8_t*>(smem) + F * SHAP_AS * 4;  // [F][SHAP_ROWS]
  const int tid = threadIdx.x, t = blockIdx.y;
  const int r0 = blockIdx.x * SHAP_ROWS;
  const int rows = min(SHAP_ROWS, n - r0);
  for (int e = tid; e < F * SHAP_AS; e += SHAP_ROWS) acc[e] = 0.f;
  // the tile's rows are contiguous (rows * F bytes from a 4-byte aligned address): coalesced dword reads
  const uint8_t* tile = bins + (int64_t)r0 * F;
  const uint32_t* tile4 = reinterpret_cast<const uint32_t*>(tile);
  const int nb = rows * F;
#pragma unroll 4
  for (int q = tid; q < SHAP_ROWS / 4 * F; q += SHAP_ROWS) {
    const int e = 4 * q;
    uint32_t v = 0u;
    if (e + 3 < nb) {
      v = tile4[q];
    } else {
      for (int b = 0; b < 4; ++b)
        if (e + b < nb) v |= (uint32_t)tile[e + b] << (8 * b);
    }
    int row = e / F, f = e - row * F;
    for (int b = 0; b < 4; ++b) {
      while (f >= F) f -= F, ++row;
      sb[f * SHAP_ROWS + row] = (uint8_t)(v >> (8 * b));  // (bytes past the tile's rows are 0)
      ++f;
    }
  }
  __syncthreads();
  const uint8_t* sb_lane = sb + tid;
  float* acc_lane = acc + tid;
  for (int k = k0 + ((t - k0 % T) % T + T) % T; k < k1; k += T) {
    for (int i = 0; i < NN; ++i) {
      const int64_t e = (int64_t)k * NN + i;
      const int d = pd[e];
      if (d <= 0) continue;  // not a leaf, or a root leaf (bias only)
      const float leafv = pleaf[e];
      const int64_t q = e * S;
      switch (d) {
        case 1: shap_leaf<1>(pf + q, plo + q, phi + q, pz + q, leafv, sb_lane, acc_lane); break;
        case 2: if constexpr (MAXD >= 2) shap_leaf<2>(pf + q, plo + q, phi + q, pz + q, leafv, sb_lane, acc_lane); break;
        case 3: if constexpr (MAXD >= 3) shap_leaf<3>(pf + q, plo + q, phi + q, pz + q, leafv, sb_lane, acc_lane); break;
        case 4: if constexpr (MAXD >= 4) shap_leaf<4>(pf + q, plo + q, phi + q, pz + q, leafv, sb_lane, acc_lane); break;
        case 5: if constexpr (MAXD >= 5) shap_leaf<5>(pf + q, plo + q, phi + q, pz + q, leafv, sb_lane, acc_lane); break;
        case 6: if constexpr (MAXD >= 6) shap_leaf<6>(pf + q, plo + q, phi + q, pz + q, leafv, sb_lane, acc_lane); break;
        case 7: if constexpr (MAXD >= 7) shap_leaf<7>(pf + q, plo + q, phi + q, pz + q, leafv, sb_lane, acc_lane); break;
        case 8: if constexpr (MAXD >= 8) shap_leaf<8>(pf + q, plo + q, phi + q, pz + q, leafv, sb_lane, acc_lane); break;
        default: break;
      }
    }
  }
  __syncthreads();
  // transpose out: the block's rows x (F+1) floats are contiguous in out[T][n][F+1]
  const int W = F + 1;
  const float b = bias[t];
  float* dst = out + ((int64_t)t * n + r0) * W;
  for (int e = tid; e < rows * W; e += SHAP_ROWS) {
    const int row = e / W, c = e - row * W;
    dst[e] = c < F ? acc[c * SHAP_AS + row] : b;
  }
}

__global__ void gbdt_leaf_index(const uint8_t* __restrict__ bins, int* __restrict__ out, int n, int F, int NN, int K,
                                int max_depth, const int8_t* __restrict__ status, const int16_t* __restrict__ feat,
                                const uint8_t* __restrict__ sbin) {
  const int64_t total = (int64_t)n * K;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = e / K;
    const int64_t o = (e - r * K) * NN;
    const uint8_t* row = bins + r * F;
    int nd = 0;
    for (int lvl = 0; lvl < max_depth && status[o + nd] == 1; ++lvl)  // (bounded: a split never sits at the last level)
      nd = 2 * nd + 1 + (row[feat[o + nd]] > sbin[o + nd] ? 1 : 0);
    out[e] = nd;
  }
}

template <int MAXD>
int launch_shap(dim3 grid, int lds, hipStream_t stream, const uint8_t* bins, int n, int F, int T, int NN, int S, int k0,
                int k1, const int* pd, const float* pleaf, const int* pf, const int* plo, const int* phi, const float* pz,
                const float* bias, float* out) {
  static bool attr = false;
  if (!attr) {
    hipError_t e = hipFuncSetAttribute((const void*)gbdt_shap<MAXD>, hipFuncAttributeMaxDynamicSharedMemorySize, SHAP_LDS_MAX);
    if (e != hipSuccess) return (int)e;
    attr = true;
  }
  hipLaunchKernelGGL(gbdt_shap<MAXD>, grid, dim3(SHAP_ROWS), lds, stream, bins, n, F, T, NN, S, k0, k1, pd, pleaf, pf, plo,
                     phi, pz, bias, out);
  EM_CHECK_LAUNCH();
  return 0;
}

}  // namespace

// LDS bytes of the contribution kernel's tile at F features, or -1 when the plan does not cover the shape
EM_API int em_gbdt_shap_lds_bytes(int F, int max_depth) {
  if (F < 1 || max_depth < 1 || max_depth > SHAP_MAX_DEPTH) return -1;
  if ((int64_t)F * (SHAP_AS * 4 + SHAP_ROWS) > SHAP_LDS_MAX) return -1;
  return shap_lds_bytes(F);
}

// The path table of trees [0, K) (tables sized K*NN and K*NN*max_depth) from the device trees.
EM_API int em_gbdt_shap_paths(int K, int max_depth, int F, const int8_t* status, const int16_t* feat, const uint8_t* sbin,
                              const float* leaf, const float* cover, int* pd, float* pleaf, int* pf, int* plo, int* phi,
                              float* pz, double* pbias, hipStream_t stream) {
  if (!status || !feat || !sbin || !leaf || !cover || !pd || !pleaf || !pf || !plo || !phi || !pz || !pbias || K < 0 ||
      F < 1 || max_depth < 1 || max_depth > SHAP_MAX_DEPTH)
    return EM_ERR_ARG;
  if (K == 0) return 0;
  const int NN = (1 << (max_depth + 1)) - 1;
  if ((int64_t)K * NN * max_depth >= (1ll << 31)) return EM_ERR_ARG;
  hipLaunchKernelGGL(gbdt_shap_paths, dim3(grid_1d((int64_t)K * NN)), dim3(256), 0, stream, K, NN, max_depth, F, status,
                     feat, sbin, leaf, cover, pd, pleaf, pf, plo, phi, pz, pbias);
  EM_CHECK_LAUNCH();
  return 0;
}

// out[T][n][F+1] = contributions of trees [k0, k1) (tree k -> task k % T) on n binned rows; bias_out[T] is scratch.
EM_API int em_gbdt_shap(const uint8_t* bins, int n, int F, int T, int max_depth, int K, int k0, int k1, double base_margin,
                        const int* pd, const float* pleaf, const int* pf, const int* plo, const int* phi, const float* pz,
                        const double* pbias, float* bias_out, float* out, hipStream_t stream) {
  if (!bins || !pd || !pleaf || !pf || !plo || !phi || !pz || !pbias || !bias_out || !out || n < 0 || T < 1 || T > 65535 ||
      k0 < 0 || k1 < k0 || k1 > K || em_gbdt_shap_lds_bytes(F, max_depth) < 0 || (((uintptr_t)bins) & 3))
    return EM_ERR_ARG;
  if (n == 0) return 0;
  if ((int64_t)n * F >= (1ll << 31)) return EM_ERR_ARG;  // 32-bit tile offsets: the caller chunks the rows
  const int NN = (1 << (max_depth + 1)) - 1;
  hipLaunchKernelGGL(gbdt_shap_bias, dim3(T), dim3(64), 0, stream, pbias, pd, NN, T, k0, k1, base_margin, bias_out);
  EM_CHECK_LAUNCH();
  const dim3 grid((n + SHAP_ROWS - 1) / SHAP_ROWS, T);
  const int lds = shap_lds_bytes(F);
  if (max_depth <= 3)
    return launch_shap<3>(grid, lds, stream, bins, n, F, T, NN, max_depth, k0, k1, pd, pleaf, pf, plo, phi, pz, bias_out, out);
  if (max_depth <= 5)
    return launch_shap<5>(grid, lds, stream, bins, n, F, T, NN, max_depth, k0, k1, pd, pleaf, pf, plo, phi, pz, bias_out, out);
  return launch_shap<8>(grid, lds, stream, bins, n, F, T, NN, max_depth, k0, k1, pd, pleaf, pf, plo, phi, pz, bias_out, out);
}

// out[n][K] = heap index of the node where row r stops in tree k
EM_API int em_gbdt_leaf_index(const uint8_t* bins, int* out, int n, int F, int max_depth, int K, const int8_t* status,
                              const int16_t* feat, const uint8_t* sbin, hipStream_t stream) {
  if (!bins || !out || !status || !feat || !sbin || n < 0 || K < 0 || F < 1 || max_depth < 1 || max_depth > 12)
    return EM_ERR_ARG;
  if (n == 0 || K == 0) return 0;
  const int NN = (1 << (max_depth + 1)) - 1;
  const int64_t total = (int64_t)n * K;
  const int grid = (int)(total + 255 < 256ll * 65536 ? (total + 255) / 256 : 65536);
  hipLaunchKernelGGL(gbdt_leaf_index, dim3(grid), dim3(256), 0, stream, bins, out, n, F, NN, K, max_depth, status, feat, sbin);
  EM_CHECK_LAUNCH();
  return 0;
}

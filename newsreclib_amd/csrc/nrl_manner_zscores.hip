// nrl_manner_zscores: MANNeR's ensemble scorer (nrl_manner.hip: nrl_manner_scores) with the combination left out.  out (T, N), row t =
// table t's z-scores of every candidate, flat and ragged in cand_offsets order -- the bits mn_scores_kernel gives table t alone under
// weight 1 (1.0f * z is exact).  What a weight grid (nrl_grid_metrics) combines: computed once per batch, whatever the number of
// weight rows.
//
// A unit of its own, and a sibling kernel rather than a template parameter of mn_scores_kernel: that kernel is pinned by bits, and
// both sharing its text and merely compiling a second kernel beside it moved its instructions (profiles/grid_metrics_resources.txt);
// nrl_manner.hip stays byte for byte what it was (tkr_scores_kernel in nrl_topk.hip is the precedent for the sibling).  The user
// vector, the dot products and the two block sums below are mn_scores_kernel's statements in its order; tests/test_gpu_grid_metrics.py
// holds the two kernels to the same bits.  The same quirks, no epsilon anywhere: one candidate, zero variance or an empty history
// give a non-finite row; indices outside [0, V) are clamped.  A candidate beyond max_cand or outside [0, N) is not written.
#include <math.h>

#include "nrl_common.h"

namespace nrl {

// the limits of nrl_manner_scores (include/newsreclib_amd.h states them for both entries)
constexpr int MZ_THREADS = 256;
constexpr int MZ_WAVES = MZ_THREADS / 64;
constexpr int MZ_MAX_D = 1024;
constexpr int MZ_MAX_CAND = 2048;
constexpr int MZ_MAX_TABLES = 3;

struct MzTables {
  const float* table[MZ_MAX_TABLES];
  int k;
};

__global__ __launch_bounds__(MZ_THREADS) void mn_zscores_kernel(MzTables T, int64_t V, const int64_t* __restrict__ hist_idx,
                                                                const int64_t* __restrict__ hist_off,
                                                                const int64_t* __restrict__ cand_idx,
                                                                const int64_t* __restrict__ cand_off, int max_cand, int D, int64_t N,
                                                                float* __restrict__ out) {
  extern __shared__ float4 mz_smem4[];
  float* u = reinterpret_cast<float*>(mz_smem4);          // [D] user vector of the current sub-model
  float* sc = u + D;                                      // [max_cand] its raw scores
  __shared__ float red[MZ_WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, D4 = D >> 2;
  const int64_t b = blockIdx.x;
  const int64_t h0 = hist_off[b], c0 = cand_off[b];
  const int nh = (int)(hist_off[b + 1] - h0);
  int nc = (int)(cand_off[b + 1] - c0);
  if (nc > max_cand) nc = max_cand;
  for (int t = 0; t < T.k; ++t) {
    const float* tab = T.table[t];
    __syncthreads();                                      // the previous sub-model's u / sc are no longer read
    // user vector: thread d4 owns four columns, rows added in history order
    for (int d4 = threadIdx.x; d4 < D4; d4 += MZ_THREADS) {
      float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int h = 0; h < nh; ++h) {
        int64_t id = hist_idx[h0 + h];
        id = id < 0 ? 0 : (id >= V ? V - 1 : id);
        const float4 x = ld4(tab + id * D + 4 * d4);
        a.x += x.x; a.y += x.y; a.z += x.z; a.w += x.w;
      }
      const float n = (float)nh;
      *reinterpret_cast<float4*>(u + 4 * d4) = make_float4(a.x / n, a.y / n, a.z / n, a.w / n);
    }
    __syncthreads();
    // one wave per candidate
    for (int c = wave; c < nc; c += MZ_WAVES) {
      int64_t id = cand_idx[c0 + c];
      id = id < 0 ? 0 : (id >= V ? V - 1 : id);
      const float* x = tab + id * D;
      float dot = 0.f;
      for (int d4 = lane; d4 < D4; d4 += 64) {
        const float4 a = ld4(u + 4 * d4), v = ld4(x + 4 * d4);
        dot += a.x * v.x + a.y * v.y + a.z * v.z + a.w * v.w;
      }
      dot = wave_sum(dot);
      if (lane == 0) sc[c] = dot;
    }
    __syncthreads();
    // mean, unbiased std over the impression's own candidates (two passes), z-score
    float part = 0.f;
    for (int c = threadIdx.x; c < nc; c += MZ_THREADS) part += sc[c];
    const float mean = block_sum<MZ_WAVES>(part, red) / (float)nc;
    part = 0.f;
    for (int c = threadIdx.x; c < nc; c += MZ_THREADS) {
      const float d = sc[c] - mean;
      part += d * d;
    }
    const float sd = sqrtf(block_sum<MZ_WAVES>(part, red) / (float)(nc - 1));        // nc == 1: 0 / 0 = NaN, as torch.std
    float* row = out + (int64_t)t * N;
    for (int c = threadIdx.x; c < nc; c += MZ_THREADS)
      if (c0 >= 0 && c0 + c < N) row[c0 + c] = (sc[c] - mean) / sd;
  }
}

}  // namespace nrl

using namespace nrl;

extern "C" {

int nrl_manner_zscores(const float* const* tables, int32_t k, int64_t V, const int64_t* hist_idx, const int64_t* hist_offsets,
                       const int64_t* cand_idx, const int64_t* cand_offsets, int64_t N, int64_t B, int32_t max_cand, int32_t D,
                       float* out, void* stream) {
  NRL_REQUIRE(tables && hist_offsets && cand_offsets, "manner_zscores: null argument");
  NRL_REQUIRE(k >= 1 && k <= MZ_MAX_TABLES, "manner_zscores: 1 <= k <= %d news-vector tables (got %d)", MZ_MAX_TABLES, k);
  NRL_REQUIRE(V >= 1 && B >= 0 && N >= 0, "manner_zscores: bad sizes");
  NRL_REQUIRE(D >= 4 && D <= MZ_MAX_D && D % 4 == 0, "manner_zscores: D a multiple of 4 up to %d (got %d)", MZ_MAX_D, D);
  NRL_REQUIRE(max_cand >= 1 && max_cand <= MZ_MAX_CAND, "manner_zscores: 1 <= max_cand <= %d (got %d)", MZ_MAX_CAND, max_cand);
  MzTables T;
  T.k = k;
  for (int t = 0; t < MZ_MAX_TABLES; ++t) {
    T.table[t] = t < k ? tables[t] : nullptr;
    NRL_REQUIRE(t >= k || (T.table[t] != nullptr && ((uintptr_t)T.table[t] & 15) == 0), "manner_zscores: table %d null or not 16-byte aligned", t);
  }
  if (B == 0 || N == 0) return NRL_OK;
  NRL_REQUIRE(hist_idx && cand_idx && out, "manner_zscores: null argument");
  const size_t smem = (size_t)(D + ((max_cand + 3) & ~3)) * sizeof(float);
  mn_zscores_kernel<<<(unsigned)B, MZ_THREADS, smem, (hipStream_t)stream>>>(T, V, hist_idx, hist_offsets, cand_idx, cand_offsets,
                                                                            max_cand, D, N, out);
  NRL_LAUNCH_CHECK();
  return NRL_OK;
}

}  // extern "C"

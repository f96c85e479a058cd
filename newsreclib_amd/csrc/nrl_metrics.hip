// Streaming evaluation metrics (nrms_module.py:182-195,456-493; metrics/functional.py:8-127; metrics/base.py:137-182): the
// per-impression reciprocal rank, nDCG@k, aspect diversity@k and personalization@k of one batch of ragged impressions, and their
// column sums added into an epoch accumulator.  No sort, no dense (impressions, longest impression) tensor, no per-class table in
// global memory.
//
//   mt_impressions_kernel   256 threads, four consecutive impressions per workgroup.
//       * an impression of up to MT_WAVE_C = 128 candidates is done by ONE wave (MIND's mean is ~37 candidates: a workgroup per
//         impression would idle most lanes); a longer one (up to 4096) by the whole workgroup, after the waves' short ones;
//       * exact stable rank by COUNTING: every lane owns OWN candidates in registers and counts, over LDS-staged tiles of the
//         impression, how many candidates precede each of them (higher score, or the same score at a lower position).  Scores are
//         compared as order-preserving 32-bit keys (NaN first, -0 == +0: torch's comparison).  The same loop counts the targets
//         for the ideal ranking, so the ideal DCG needs no second pass;
//       * rr / DCG / ideal DCG are accumulated from (rank, target) of the owned candidates and finished by wave (or workgroup)
//         reductions in a fixed order;
//       * per aspect: one LDS histogram of the history, then per k one LDS histogram of the candidates ranked below k (integer LDS
//         atomics: exact, order-free); entropy and generalised Jaccard are reductions over the classes;
//       * offsets and aspect ids are validated BEFORE they index anything; a bad impression ORs a flag into the status word, writes
//         a zero row and -1 ranks (where its range is known to be inside the buffers) and counts as absent.
//   mt_reduce_parts_kernel / mt_reduce_final_kernel   column sums of the rows in float64: a tree inside fixed parts of 4096 rows,
//       a tree over the parts, then one plain add per column into the accumulator.  Nothing depends on scheduling.
//   mt_grid_kernel          mt_impressions_kernel for G score vectors that are weighted sums of T component vectors (a grid of
//       ensemble weights): grid (impressions / 4, ranges of configs), every workgroup loops over a contiguous range of configs.
//       Per impression, ONCE: the offsets and aspect ids, the targets' ideal DCG (the ct counts), the history histogram of every
//       aspect, and -- wave form -- the owned candidates' T components and targets in registers.  Per config: the owned scores
//       (the first non-zero weight a product, every later one an fma, as mn_scores_kernel rounds them; zero weights skipped), their
//       keys staged in the LDS tile, the cs counts, rr / DCG, the ranks in an LDS array of 16-bit words (never in global memory),
//       the top-k class histograms.  Every statement that produces a row value is mt_impression's, in its order: row (g, b) has
//       the bits mt_impressions_kernel writes when it is fed config g's scores.  The workgroup form (C > 128) recomputes the scores
//       it stages from the components in global memory (L2): its tiles are not its owned candidates.
//   mt_grid_reduce_*        the two reductions with a config index on a grid dimension, bodies of their own (the two kernels above
//       keep their text): the same trees, the same bits.
#include <math.h>

#include "nrl_common.h"

namespace nrl {

constexpr int MT_THREADS = 256;
constexpr int MT_WAVES = MT_THREADS / 64;
constexpr int MT_WAVE_C = 128;                 // longest impression one wave takes: 2 owned candidates per lane, one tile
constexpr int MT_BLOCK_TILE = MT_WAVES * MT_WAVE_C;      // the workgroup path stages tiles in the four waves' regions together
constexpr int MT_MAX_C = NRL_METRICS_MAX_CAND;
constexpr int MT_MAX_K = NRL_METRICS_MAX_NK;
constexpr int MT_PART_ROWS = 4096;             // rows of one part of the column reduction

struct MtArgs {
  const float* preds;
  const float* targets;
  const int64_t* cand_off;
  const int64_t* hist_off;
  const int64_t* cand_asp[2];
  const int64_t* hist_asp[2];
  int32_t num_classes[2];
  int32_t n_aspects;
  int32_t k[MT_MAX_K];
  int32_t n_k;
  int32_t n_cols;
  int32_t nc_pad;            // LDS ints per histogram
  int64_t N, n_hist, B;
  int32_t* rank;             // N (the caller's, or workspace)
  float* rows;               // (B, n_cols) (the caller's, or workspace)
  int32_t* valid;            // B
  int32_t* status;
};

template <bool BLOCK>
__device__ __forceinline__ void mt_sync() {
  if (BLOCK)
    __syncthreads();
  else
    wave_lds_sync();
}

__device__ __forceinline__ int mt_wave_sum_i(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
__device__ __forceinline__ int mt_wave_min_i(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off, 64));
  return v;
}
__device__ __forceinline__ int mt_wave_or_i(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v |= __shfl_xor(v, off, 64);
  return v;
}

// group-wide reductions, identical in every thread of the group; the workgroup form adds the waves in wave order
// (not block_sum: no leading +0, so four waves of -0 give -0 here)
template <bool BLOCK>
__device__ __forceinline__ float mt_sum_f(float v, float* red) {
  v = wave_sum(v);
  if (!BLOCK) return v;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}
template <bool BLOCK>
__device__ __forceinline__ int mt_sum_i(int v, float* red) {
  v = mt_wave_sum_i(v);
  if (!BLOCK) return v;
  int* r = reinterpret_cast<int*>(red);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) r[threadIdx.x >> 6] = v;
  __syncthreads();
  return r[0] + r[1] + r[2] + r[3];
}
template <bool BLOCK>
__device__ __forceinline__ int mt_min_i(int v, float* red) {
  v = mt_wave_min_i(v);
  if (!BLOCK) return v;
  int* r = reinterpret_cast<int*>(red);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) r[threadIdx.x >> 6] = v;
  __syncthreads();
  return min(min(r[0], r[1]), min(r[2], r[3]));
}
template <bool BLOCK>
__device__ __forceinline__ int mt_or_i(int v, float* red) {
  v = mt_wave_or_i(v);
  if (!BLOCK) return v;
  int* r = reinterpret_cast<int*>(red);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) r[threadIdx.x >> 6] = v;
  __syncthreads();
  return r[0] | r[1] | r[2] | r[3];
}

// what the offsets say about impression b: 0 = fine, otherwise the flag to raise
__device__ __forceinline__ int mt_read_offsets(const MtArgs& A, int64_t b, int64_t& c0, int64_t& C, int64_t& h0, int64_t& H) {
  c0 = A.cand_off[b];
  const int64_t c1 = A.cand_off[b + 1];
  C = c1 - c0;
  h0 = 0;
  H = 0;
  if (c0 < 0 || c1 < c0 || c1 > A.N) return NRL_METRICS_E_OFFSETS;
  if (A.n_aspects > 0) {
    h0 = A.hist_off[b];
    const int64_t h1 = A.hist_off[b + 1];
    H = h1 - h0;
    if (h0 < 0 || h1 < h0 || h1 > A.n_hist) return NRL_METRICS_E_OFFSETS;
  }
  return 0;
}

// a flagged impression: zero row, absent from the sums, -1 ranks when its candidate range is inside the buffers
template <int G>
__device__ __forceinline__ void mt_reject(const MtArgs& A, int64_t b, int t, int flag, bool range_ok, int64_t c0, int64_t C) {
  for (int c = t; c < A.n_cols; c += G) A.rows[b * A.n_cols + c] = 0.f;
  if (range_ok)
    for (int64_t i = t; i < C; i += G) A.rank[c0 + i] = -1;
  if (t == 0) {
    A.valid[b] = 0;
    atomicOr(A.status, flag);
  }
}

// One impression by a group of G threads (a wave, or the workgroup); t = this thread's index in the group.  skey / tkey: TILE keys
// each, hc / hh: nc_pad ints each, red: 4 words (workgroup form only).  The caller has read the offsets (flag == 0) and chose the
// group by C.
template <int G, int OWN, int TILE, bool BLOCK>
__device__ __forceinline__ void mt_impression(const MtArgs& A, int64_t b, int t, int64_t c0, int C, int64_t h0, int64_t H,
                                              uint32_t* skey, uint32_t* tkey, int* hc, int* hh, float* red) {
  // ---- aspect ids are validated before anything is written
  int nonzero[2] = {0, 0};
  if (A.n_aspects > 0) {
    int bad = 0;
    for (int a = 0; a < A.n_aspects; ++a) {
      const int64_t nc = A.num_classes[a];
      int nz = 0;
      for (int i = t; i < C; i += G) {
        const int64_t id = A.cand_asp[a][c0 + i];
        bad |= (id < 0 || id >= nc);
        nz |= (id != 0);
      }
      for (int64_t i = t; i < H; i += G) {
        const int64_t id = A.hist_asp[a][h0 + i];
        bad |= (id < 0 || id >= nc);
      }
      nonzero[a] = nz;
    }
    const int word = mt_or_i<BLOCK>(bad | (nonzero[0] << 1) | (nonzero[1] << 2), red);
    if (word & 1) {
      mt_reject<G>(A, b, t, NRL_METRICS_E_ASPECT, true, c0, C);
      return;
    }
    nonzero[0] = (word >> 1) & 1;
    nonzero[1] = (word >> 2) & 1;
  }

  // ---- ranks by counting; rr / DCG / ideal DCG from the owned candidates
  float dcg[MT_MAX_K], idcg[MT_MAX_K];
#pragma unroll
  for (int q = 0; q < MT_MAX_K; ++q) dcg[q] = idcg[q] = 0.f;
  int kmax = 0;
#pragma unroll
  for (int q = 0; q < MT_MAX_K; ++q)
    if (q < A.n_k) kmax = max(kmax, A.k[q]);
  int best = 0x7FFFFFFF;
  for (int base = 0; base < C; base += G * OWN) {
    uint32_t ks[OWN], kt[OWN];
    float tv[OWN];
    int cs[OWN], ct[OWN];
#pragma unroll
    for (int o = 0; o < OWN; ++o) {
      const int i = base + o * G + t;
      const bool act = i < C;
      tv[o] = act ? A.targets[c0 + i] : 0.f;
      ks[o] = act ? score_key(A.preds[c0 + i]) : 0u;
      kt[o] = score_key(tv[o]);
      cs[o] = ct[o] = 0;
    }
    for (int tb = 0; tb < C; tb += TILE) {
      const int n = min(TILE, C - tb);
      mt_sync<BLOCK>();                   // the previous tile is no longer read
      for (int j = t; j < n; j += G) {
        skey[j] = score_key(A.preds[c0 + tb + j]);
        tkey[j] = score_key(A.targets[c0 + tb + j]);
      }
      mt_sync<BLOCK>();
      for (int j = 0; j < n; ++j) {
        const uint32_t sj = skey[j], tj = tkey[j];          // LDS broadcast reads
        const int jj = tb + j;
#pragma unroll
        for (int o = 0; o < OWN; ++o) {
          const int i = base + o * G + t;
          cs[o] += (sj > ks[o]) | ((sj == ks[o]) & (jj < i));
          ct[o] += (tj > kt[o]) | ((tj == kt[o]) & (jj < i));
        }
      }
    }
#pragma unroll
    for (int o = 0; o < OWN; ++o) {
      const int i = base + o * G + t;
      if (i < C) {
        A.rank[c0 + i] = cs[o];
        if (tv[o] > 0.f) best = min(best, cs[o]);
        if (cs[o] < kmax) {
          const float g = tv[o] / log2f((float)(cs[o] + 2));
#pragma unroll
          for (int q = 0; q < MT_MAX_K; ++q)
            if (q < A.n_k && cs[o] < A.k[q]) dcg[q] += g;
        }
        if (ct[o] < kmax) {
          const float g = tv[o] / log2f((float)(ct[o] + 2));
#pragma unroll
          for (int q = 0; q < MT_MAX_K; ++q)
            if (q < A.n_k && ct[o] < A.k[q]) idcg[q] += g;
        }
      }
    }
  }
  float* row = A.rows + b * A.n_cols;
  best = mt_min_i<BLOCK>(best, red);
  if (t == 0) {
    row[0] = best == 0x7FFFFFFF ? 0.f : 1.f / (float)(best + 1);
    A.valid[b] = 1;
  }
#pragma unroll
  for (int q = 0; q < MT_MAX_K; ++q) {
    if (q < A.n_k) {
      const float d = mt_sum_f<BLOCK>(dcg[q], red), id = mt_sum_f<BLOCK>(idcg[q], red);
      if (t == 0) row[1 + q] = id > 0.f ? d / id : 0.f;
    }
  }

  // ---- aspects: history histogram once, top-k histogram per k
  for (int a = 0; a < A.n_aspects; ++a) {
    const int nc = A.num_classes[a];
    const int64_t* ca = A.cand_asp[a] + c0;
    const int64_t* ha = A.hist_asp[a] + h0;
    float* arow = row + 1 + A.n_k + 2 * A.n_k * a;
    mt_sync<BLOCK>();
    for (int c = t; c < nc; c += G) hh[c] = 0;
    mt_sync<BLOCK>();
    for (int64_t i = t; i < H; i += G) atomicAdd(&hh[(int)ha[i]], 1);
    const float inv_log_nc = 1.f / logf((float)nc);
    for (int q = 0; q < A.n_k; ++q) {
      const int k = A.k[q];
      mt_sync<BLOCK>();                   // the previous k's histogram is no longer read
      for (int c = t; c < nc; c += G) hc[c] = 0;
      mt_sync<BLOCK>();
      for (int i = t; i < C; i += G)
        if (A.rank[c0 + i] < k) atomicAdd(&hc[(int)ca[i]], 1);      // (this thread wrote rank[c0 + i] above: i % G == t)
      mt_sync<BLOCK>();
      const float inv_top = 1.f / (float)min(k, C);
      float ent = 0.f;
      int smin = 0, smax = 0;
      for (int c = t; c < nc; c += G) {
        const int x = hc[c], y = hh[c];
        if (x > 0) {
          const float p = (float)x * inv_top;
          ent -= p * logf(p);
        }
        smin += min(x, y);
        smax += max(x, y);
      }
      ent = mt_sum_f<BLOCK>(ent, red);
      smin = mt_sum_i<BLOCK>(smin, red);
      smax = mt_sum_i<BLOCK>(smax, red);
      if (t == 0) {
        arow[q] = nonzero[a] ? ent * inv_log_nc : 0.f;
        arow[A.n_k + q] = (nonzero[a] && smax > 0) ? (float)smin / (float)smax : 0.f;
      }
    }
  }
}

__global__ __launch_bounds__(MT_THREADS) void mt_impressions_kernel(MtArgs A) {
  extern __shared__ uint32_t mt_smem[];
  __shared__ float red[MT_WAVES];
  uint32_t* skey = mt_smem;                                  // [MT_WAVES][MT_WAVE_C]
  uint32_t* tkey = skey + MT_BLOCK_TILE;                     // [MT_WAVES][MT_WAVE_C]
  int* hc = reinterpret_cast<int*>(tkey + MT_BLOCK_TILE);    // [MT_WAVES][nc_pad]
  int* hh = hc + MT_WAVES * A.nc_pad;                        // [MT_WAVES][nc_pad]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t b_first = (int64_t)blockIdx.x * MT_WAVES;
  int64_t c0, C, h0, H;
  // short (or rejected) impressions: wave w takes impression b_first + w
  {
    const int64_t b = b_first + wave;
    if (b < A.B) {
      const int flag = mt_read_offsets(A, b, c0, C, h0, H);
      if (flag)
        mt_reject<64>(A, b, lane, flag, false, 0, 0);
      else if (C > MT_MAX_C)
        mt_reject<64>(A, b, lane, NRL_METRICS_E_TOO_LONG, true, c0, C);
      else if (C <= MT_WAVE_C)
        mt_impression<64, 2, MT_WAVE_C, false>(A, b, lane, c0, (int)C, h0, H, skey + wave * MT_WAVE_C, tkey + wave * MT_WAVE_C,
                                               hc + wave * A.nc_pad, hh + wave * A.nc_pad, red);
    }
  }
  // long impressions: the whole workgroup, one after the other (every thread reads the same offsets: the branch is uniform)
  for (int w = 0; w < MT_WAVES; ++w) {
    const int64_t b = b_first + w;
    if (b >= A.B) break;
    if (mt_read_offsets(A, b, c0, C, h0, H) != 0 || C <= MT_WAVE_C || C > MT_MAX_C) continue;
    __syncthreads();                      // the waves' own regions are free
    mt_impression<MT_THREADS, 4, MT_BLOCK_TILE, true>(A, b, (int)threadIdx.x, c0, (int)C, h0, H, skey, tkey, hc, hh, red);
  }
}

// ---- column sums: partial[part][c] = tree sum of the part's rows in float64 (column n_cols: the number of valid rows)
__global__ __launch_bounds__(MT_THREADS) void mt_reduce_parts_kernel(const float* __restrict__ rows, const int32_t* __restrict__ valid,
                                                                     int64_t B, int n_cols, double* __restrict__ partial) {
  __shared__ double acc[MT_THREADS];
  const int64_t r0 = (int64_t)blockIdx.x * MT_PART_ROWS;
  const int64_t r1 = r0 + MT_PART_ROWS < B ? r0 + MT_PART_ROWS : B;
  for (int c = 0; c <= n_cols; ++c) {
    double v = 0.0;
    for (int64_t r = r0 + threadIdx.x; r < r1; r += MT_THREADS)
      if (valid[r]) v += c < n_cols ? (double)rows[r * n_cols + c] : 1.0;
    acc[threadIdx.x] = v;
    __syncthreads();
    for (int s = MT_THREADS / 2; s > 0; s >>= 1) {
      if ((int)threadIdx.x < s) acc[threadIdx.x] += acc[threadIdx.x + s];
      __syncthreads();
    }
    if (threadIdx.x == 0) partial[(int64_t)blockIdx.x * (n_cols + 1) + c] = acc[0];
    __syncthreads();
  }
}

__global__ __launch_bounds__(MT_THREADS) void mt_reduce_final_kernel(const double* __restrict__ partial, int64_t parts, int n_cols,
                                                                     double* __restrict__ sums, int64_t* __restrict__ count) {
  __shared__ double acc[MT_THREADS];
  for (int c = 0; c <= n_cols; ++c) {
    double v = 0.0;
    for (int64_t p = threadIdx.x; p < parts; p += MT_THREADS) v += partial[p * (n_cols + 1) + c];
    acc[threadIdx.x] = v;
    __syncthreads();
    for (int s = MT_THREADS / 2; s > 0; s >>= 1) {
      if ((int)threadIdx.x < s) acc[threadIdx.x] += acc[threadIdx.x + s];
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      if (c < n_cols)
        sums[c] += acc[0];
      else
        count[0] += (int64_t)acc[0];
    }
    __syncthreads();
  }
}

// ---- a grid of weight rows ---------------------------------------------------------------------------------------------------------
constexpr int MG_MAX_T = NRL_GRID_MAX_COMPONENTS;
constexpr int MG_MAX_G = NRL_GRID_MAX_CONFIGS;
constexpr int MG_TARGET_BLOCKS = 2048;         // workgroups a launch aims at: 8 per CU of the 256

struct MgArgs {
  MtArgs M;                  // preds / rank unused; rows: (G, B, n_cols); valid: (B)
  const float* comp;         // (T, N)
  const float* weights;      // (G, T)
  float* preds;              // (G, N) or null
  int32_t T, G, g_per;       // configs per workgroup: blockIdx.y takes [y * g_per, min(G, (y + 1) * g_per))
};

// score of one candidate under one weight row: terms with weight 0 are skipped (w beyond T is 0), the first remaining one is the
// plain product, every later one a fused multiply-add -- mn_scores_kernel's `t == 0 ? wt * z : acc + wt * z` as its code object
// rounds it (v_mul_f32, then v_fma_f32).  No term: +0.
__device__ __forceinline__ float mg_combine(const float (&w)[MG_MAX_T], const float (&z)[MG_MAX_T]) {
  float acc = 0.f;
  bool first = true;
#pragma unroll
  for (int t = 0; t < MG_MAX_T; ++t) {
    if (w[t] != 0.f) {
      acc = first ? __fmul_rn(w[t], z[t]) : __fmaf_rn(w[t], z[t], acc);
      first = false;
    }
  }
  return acc;
}
__device__ __forceinline__ float mg_score(const MgArgs& A, const float (&w)[MG_MAX_T], int64_t idx) {
  float z[MG_MAX_T];
#pragma unroll
  for (int t = 0; t < MG_MAX_T; ++t) z[t] = t < A.T ? A.comp[(int64_t)t * A.M.N + idx] : 0.f;
  return mg_combine(w, z);
}

// a flagged impression: a zero row under every config of this workgroup's range; the flag and the valid word once
template <int GT>
__device__ __forceinline__ void mg_reject(const MgArgs& A, int64_t b, int t, int flag, int g_lo, int g_hi) {
  const MtArgs& M = A.M;
  for (int g = g_lo; g < g_hi; ++g)
    for (int c = t; c < M.n_cols; c += GT) M.rows[((int64_t)g * M.B + b) * M.n_cols + c] = 0.f;
  if (t == 0 && blockIdx.y == 0) {
    M.valid[b] = 0;
    atomicOr(M.status, flag);
  }
}

// mt_impression for the configs [g_lo, g_hi).  key: TILE keys, lrank: C 16-bit ranks (C <= 4096), hc: nc_pad ints, hh: 2 * nc_pad
// ints (one history histogram per aspect), red: 4 words (workgroup form only).
template <int GT, int OWN, int TILE, bool BLOCK>
__device__ __forceinline__ void mg_impression(const MgArgs& A, int64_t b, int t, int64_t c0, int C, int64_t h0, int64_t H, int g_lo,
                                              int g_hi, uint32_t* key, uint16_t* lrank, int* hc, int* hh, float* red) {
  const MtArgs& M = A.M;
  // ---- once: aspect ids are validated before anything is written
  int nonzero[2] = {0, 0};
  if (M.n_aspects > 0) {
    int bad = 0;
    for (int a = 0; a < M.n_aspects; ++a) {
      const int64_t nc = M.num_classes[a];
      int nz = 0;
      for (int i = t; i < C; i += GT) {
        const int64_t id = M.cand_asp[a][c0 + i];
        bad |= (id < 0 || id >= nc);
        nz |= (id != 0);
      }
      for (int64_t i = t; i < H; i += GT) {
        const int64_t id = M.hist_asp[a][h0 + i];
        bad |= (id < 0 || id >= nc);
      }
      nonzero[a] = nz;
    }
    const int word = mt_or_i<BLOCK>(bad | (nonzero[0] << 1) | (nonzero[1] << 2), red);
    if (word & 1) {
      mg_reject<GT>(A, b, t, NRL_METRICS_E_ASPECT, g_lo, g_hi);
      return;
    }
    nonzero[0] = (word >> 1) & 1;
    nonzero[1] = (word >> 2) & 1;
  }
  int kmax = 0;
#pragma unroll
  for (int q = 0; q < MT_MAX_K; ++q)
    if (q < M.n_k) kmax = max(kmax, M.k[q]);

  // ---- once: the ideal DCG from the targets' own ranking
  float ideal[MT_MAX_K];
  {
    float idcg[MT_MAX_K];
#pragma unroll
    for (int q = 0; q < MT_MAX_K; ++q) idcg[q] = 0.f;
    for (int base = 0; base < C; base += GT * OWN) {
      uint32_t kt[OWN];
      float tv[OWN];
      int ct[OWN];
#pragma unroll
      for (int o = 0; o < OWN; ++o) {
        const int i = base + o * GT + t;
        tv[o] = i < C ? M.targets[c0 + i] : 0.f;
        kt[o] = score_key(tv[o]);
        ct[o] = 0;
      }
      for (int tb = 0; tb < C; tb += TILE) {
        const int n = min(TILE, C - tb);
        mt_sync<BLOCK>();                   // the previous tile is no longer read
        for (int j = t; j < n; j += GT) key[j] = score_key(M.targets[c0 + tb + j]);
        mt_sync<BLOCK>();
        for (int j = 0; j < n; ++j) {
          const uint32_t tj = key[j];
          const int jj = tb + j;
#pragma unroll
          for (int o = 0; o < OWN; ++o) {
            const int i = base + o * GT + t;
            ct[o] += (tj > kt[o]) | ((tj == kt[o]) & (jj < i));
          }
        }
      }
#pragma unroll
      for (int o = 0; o < OWN; ++o) {
        const int i = base + o * GT + t;
        if (i < C && ct[o] < kmax) {
          const float g = tv[o] / log2f((float)(ct[o] + 2));
#pragma unroll
          for (int q = 0; q < MT_MAX_K; ++q)
            if (q < M.n_k && ct[o] < M.k[q]) idcg[q] += g;
        }
      }
    }
#pragma unroll
    for (int q = 0; q < MT_MAX_K; ++q) {
      ideal[q] = 0.f;
      if (q < M.n_k) ideal[q] = mt_sum_f<BLOCK>(idcg[q], red);
    }
  }

  // ---- once: the history histogram of every aspect
  for (int a = 0; a < M.n_aspects; ++a) {
    const int nc = M.num_classes[a];
    const int64_t* ha = M.hist_asp[a] + h0;
    int* h = hh + a * M.nc_pad;
    mt_sync<BLOCK>();
    for (int c = t; c < nc; c += GT) h[c] = 0;
    mt_sync<BLOCK>();
    for (int64_t i = t; i < H; i += GT) atomicAdd(&h[(int)ha[i]], 1);
  }

  // ---- once (wave form: one chunk, one tile): the owned candidates' components and targets stay in registers
  float cv[MG_MAX_T][OWN], tvr[OWN];
  if constexpr (!BLOCK) {
#pragma unroll
    for (int o = 0; o < OWN; ++o) {
      const int i = o * GT + t;
      const bool act = i < C;
      tvr[o] = act ? M.targets[c0 + i] : 0.f;
#pragma unroll
      for (int tt = 0; tt < MG_MAX_T; ++tt) cv[tt][o] = (act && tt < A.T) ? A.comp[(int64_t)tt * M.N + c0 + i] : 0.f;
    }
  }

  for (int g = g_lo; g < g_hi; ++g) {
    float w[MG_MAX_T];
#pragma unroll
    for (int tt = 0; tt < MG_MAX_T; ++tt) w[tt] = tt < A.T ? A.weights[(int64_t)g * A.T + tt] : 0.f;
    // ---- ranks by counting; rr / DCG from the owned candidates
    float dcg[MT_MAX_K];
#pragma unroll
    for (int q = 0; q < MT_MAX_K; ++q) dcg[q] = 0.f;
    int best = 0x7FFFFFFF;
    for (int base = 0; base < C; base += GT * OWN) {
      uint32_t ks[OWN];
      float tv[OWN];
      int cs[OWN];
#pragma unroll
      for (int o = 0; o < OWN; ++o) {
        const int i = base + o * GT + t;
        const bool act = i < C;
        float s;
        if constexpr (BLOCK) {
          tv[o] = act ? M.targets[c0 + i] : 0.f;
          s = act ? mg_score(A, w, c0 + i) : 0.f;
        } else {
          tv[o] = tvr[o];
          const float z[MG_MAX_T] = {cv[0][o], cv[1][o], cv[2][o], cv[3][o]};
          s = mg_combine(w, z);
        }
        ks[o] = act ? score_key(s) : 0u;
        cs[o] = 0;
        if (act && A.preds) A.preds[(int64_t)g * M.N + c0 + i] = s;
      }
      for (int tb = 0; tb < C; tb += TILE) {
        const int n = min(TILE, C - tb);
        mt_sync<BLOCK>();                   // the previous tile is no longer read
        if constexpr (BLOCK) {
          for (int j = t; j < n; j += GT) key[j] = score_key(mg_score(A, w, c0 + tb + j));
        } else {
#pragma unroll
          for (int o = 0; o < OWN; ++o)     // the one tile is the owned candidates
            if (o * GT + t < n) key[o * GT + t] = ks[o];
        }
        mt_sync<BLOCK>();
        for (int j = 0; j < n; ++j) {
          const uint32_t sj = key[j];       // LDS broadcast read
          const int jj = tb + j;
#pragma unroll
          for (int o = 0; o < OWN; ++o) {
            const int i = base + o * GT + t;
            cs[o] += (sj > ks[o]) | ((sj == ks[o]) & (jj < i));
          }
        }
      }
#pragma unroll
      for (int o = 0; o < OWN; ++o) {
        const int i = base + o * GT + t;
        if (i < C) {
          lrank[i] = (uint16_t)cs[o];
          if (tv[o] > 0.f) best = min(best, cs[o]);
          if (cs[o] < kmax) {
            const float gn = tv[o] / log2f((float)(cs[o] + 2));
#pragma unroll
            for (int q = 0; q < MT_MAX_K; ++q)
              if (q < M.n_k && cs[o] < M.k[q]) dcg[q] += gn;
          }
        }
      }
    }
    float* row = M.rows + ((int64_t)g * M.B + b) * M.n_cols;
    best = mt_min_i<BLOCK>(best, red);
    if (t == 0) row[0] = best == 0x7FFFFFFF ? 0.f : 1.f / (float)(best + 1);
#pragma unroll
    for (int q = 0; q < MT_MAX_K; ++q) {
      if (q < M.n_k) {
        const float d = mt_sum_f<BLOCK>(dcg[q], red), id = ideal[q];
        if (t == 0) row[1 + q] = id > 0.f ? d / id : 0.f;
      }
    }

    // ---- aspects: top-k histogram per k against the hoisted history histogram
    for (int a = 0; a < M.n_aspects; ++a) {
      const int nc = M.num_classes[a];
      const int64_t* ca = M.cand_asp[a] + c0;
      const int* h = hh + a * M.nc_pad;
      float* arow = row + 1 + M.n_k + 2 * M.n_k * a;
      const float inv_log_nc = 1.f / logf((float)nc);
      for (int q = 0; q < M.n_k; ++q) {
        const int k = M.k[q];
        mt_sync<BLOCK>();                   // the previous histogram is no longer read
        for (int c = t; c < nc; c += GT) hc[c] = 0;
        mt_sync<BLOCK>();
        for (int i = t; i < C; i += GT)
          if ((int)lrank[i] < k) atomicAdd(&hc[(int)ca[i]], 1);      // (this thread wrote lrank[i] above: i % GT == t)
        mt_sync<BLOCK>();
        const float inv_top = 1.f / (float)min(k, C);
        float ent = 0.f;
        int smin = 0, smax = 0;
        for (int c = t; c < nc; c += GT) {
          const int x = hc[c], y = h[c];
          if (x > 0) {
            const float p = (float)x * inv_top;
            ent -= p * logf(p);
          }
          smin += min(x, y);
          smax += max(x, y);
        }
        ent = mt_sum_f<BLOCK>(ent, red);
        smin = mt_sum_i<BLOCK>(smin, red);
        smax = mt_sum_i<BLOCK>(smax, red);
        if (t == 0) {
          arow[q] = nonzero[a] ? ent * inv_log_nc : 0.f;
          arow[M.n_k + q] = (nonzero[a] && smax > 0) ? (float)smin / (float)smax : 0.f;
        }
      }
    }
  }
  if (t == 0 && blockIdx.y == 0) M.valid[b] = 1;
}

__global__ __launch_bounds__(MT_THREADS) void mt_grid_kernel(MgArgs A) {
  extern __shared__ uint32_t mg_smem[];
  __shared__ float red[MT_WAVES];
  const MtArgs& M = A.M;
  uint32_t* key = mg_smem;                                             // [MT_WAVES][MT_WAVE_C]
  int* hc = reinterpret_cast<int*>(key + MT_BLOCK_TILE);               // [MT_WAVES][nc_pad]
  int* hh = hc + MT_WAVES * M.nc_pad;                                  // [MT_WAVES][2][nc_pad]
  uint16_t* lrank = reinterpret_cast<uint16_t*>(hh + 2 * MT_WAVES * M.nc_pad);      // [MT_MAX_C] (a wave: its MT_WAVE_C)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t b_first = (int64_t)blockIdx.x * MT_WAVES;
  const int g_lo = (int)blockIdx.y * A.g_per, g_hi = min(A.G, g_lo + A.g_per);
  int64_t c0, C, h0, H;
  // short (or rejected) impressions: wave w takes impression b_first + w
  {
    const int64_t b = b_first + wave;
    if (b < M.B) {
      const int flag = mt_read_offsets(M, b, c0, C, h0, H);
      if (flag)
        mg_reject<64>(A, b, lane, flag, g_lo, g_hi);
      else if (C > MT_MAX_C)
        mg_reject<64>(A, b, lane, NRL_METRICS_E_TOO_LONG, g_lo, g_hi);
      else if (C <= MT_WAVE_C)
        mg_impression<64, 2, MT_WAVE_C, false>(A, b, lane, c0, (int)C, h0, H, g_lo, g_hi, key + wave * MT_WAVE_C,
                                               lrank + wave * MT_WAVE_C, hc + wave * M.nc_pad, hh + wave * 2 * M.nc_pad, red);
    }
  }
  // long impressions: the whole workgroup, one after the other (every thread reads the same offsets: the branch is uniform)
  for (int w = 0; w < MT_WAVES; ++w) {
    const int64_t b = b_first + w;
    if (b >= M.B) break;
    if (mt_read_offsets(M, b, c0, C, h0, H) != 0 || C <= MT_WAVE_C || C > MT_MAX_C) continue;
    __syncthreads();                      // the waves' own regions are free
    mg_impression<MT_THREADS, 4, MT_BLOCK_TILE, true>(A, b, (int)threadIdx.x, c0, (int)C, h0, H, g_lo, g_hi, key, lrank, hc, hh, red);
  }
}

// the two reductions for G accumulator rows: mt_reduce_parts_kernel / mt_reduce_final_kernel (whose text stays as it is) with the
// config on a grid dimension -- blockIdx.y (parts) / blockIdx.x (final).  The same statements in the same order: the same trees.
// count is added once, by config 0 (the valid rows do not depend on the config).
__global__ __launch_bounds__(MT_THREADS) void mt_grid_reduce_parts_kernel(const float* __restrict__ rows, const int32_t* __restrict__ valid,
                                                                          int64_t B, int n_cols, int64_t parts,
                                                                          double* __restrict__ partial) {
  __shared__ double acc[MT_THREADS];
  rows += (int64_t)blockIdx.y * B * n_cols;
  partial += (int64_t)blockIdx.y * parts * (n_cols + 1);
  const int64_t r0 = (int64_t)blockIdx.x * MT_PART_ROWS;
  const int64_t r1 = r0 + MT_PART_ROWS < B ? r0 + MT_PART_ROWS : B;
  for (int c = 0; c <= n_cols; ++c) {
    double v = 0.0;
    for (int64_t r = r0 + threadIdx.x; r < r1; r += MT_THREADS)
      if (valid[r]) v += c < n_cols ? (double)rows[r * n_cols + c] : 1.0;
    acc[threadIdx.x] = v;
    __syncthreads();
    for (int s = MT_THREADS / 2; s > 0; s >>= 1) {
      if ((int)threadIdx.x < s) acc[threadIdx.x] += acc[threadIdx.x + s];
      __syncthreads();
    }
    if (threadIdx.x == 0) partial[(int64_t)blockIdx.x * (n_cols + 1) + c] = acc[0];
    __syncthreads();
  }
}

__global__ __launch_bounds__(MT_THREADS) void mt_grid_reduce_final_kernel(const double* __restrict__ partial, int64_t parts, int n_cols,
                                                                          double* __restrict__ sums, int64_t* __restrict__ count) {
  __shared__ double acc[MT_THREADS];
  partial += (int64_t)blockIdx.x * parts * (n_cols + 1);
  sums += (int64_t)blockIdx.x * n_cols;
  for (int c = 0; c <= n_cols; ++c) {
    double v = 0.0;
    for (int64_t p = threadIdx.x; p < parts; p += MT_THREADS) v += partial[p * (n_cols + 1) + c];
    acc[threadIdx.x] = v;
    __syncthreads();
    for (int s = MT_THREADS / 2; s > 0; s >>= 1) {
      if ((int)threadIdx.x < s) acc[threadIdx.x] += acc[threadIdx.x + s];
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      if (c < n_cols)
        sums[c] += acc[0];
      else if (blockIdx.x == 0)
        count[0] += (int64_t)acc[0];
    }
    __syncthreads();
  }
}

static int mt_cols(int n_aspects, int n_k) { return 1 + n_k + 2 * n_k * n_aspects; }

}  // namespace nrl

using namespace nrl;

extern "C" {

// ranks and rows when the caller keeps none | the per-impression valid flags | the reduction's per-part sums (+ count)
struct MtWs {
  int32_t *rank, *valid;
  float* rows;
  double* partial;
};
static void mt_layout(Arena& a, int64_t N, int64_t B, int n_aspects, int n_k, MtWs* w) {
  const int cols = mt_cols(n_aspects, n_k);
  w->rank = a.take<int32_t>((size_t)(N > 0 ? N : 1));
  w->rows = a.take<float>((size_t)B * cols);
  w->valid = a.take<int32_t>((size_t)B);
  w->partial = a.take<double>((size_t)ceil_div(B, MT_PART_ROWS) * (cols + 1));
}

size_t nrl_impression_metrics_workspace_bytes(int64_t N, int64_t B, int32_t n_aspects, int32_t n_k) {
  if (N < 0 || B <= 0 || n_aspects < 0 || n_aspects > 2 || n_k < 0 || n_k > MT_MAX_K) return 256;
  return measure_workspace<MtWs>([&](Arena& a, auto* w) { mt_layout(a, N, B, n_aspects, n_k, w); });
}

int nrl_impression_metrics(const float* preds, const float* targets, const int64_t* cand_offsets, int64_t N, int64_t B,
                           int32_t n_aspects, const int64_t* cand_aspects0, const int64_t* hist_aspects0, int32_t num_classes0,
                           const int64_t* cand_aspects1, const int64_t* hist_aspects1, int32_t num_classes1,
                           const int64_t* hist_offsets, int64_t n_hist, const int32_t* top_k, int32_t n_k, int32_t* rank,
                           float* rows, double* sums, int64_t* count, int32_t* status, void* ws, size_t ws_bytes, void* stream) {
  NRL_REQUIRE(N >= 0 && B >= 0 && n_hist >= 0, "impression_metrics: negative size");
  NRL_REQUIRE(B < ((int64_t)1 << 31), "impression_metrics: at most 2^31 - 1 impressions per call (got %lld)", (long long)B);
  NRL_REQUIRE(n_aspects >= 0 && n_aspects <= 2, "impression_metrics: n_aspects in {0, 1, 2} (got %d)", n_aspects);
  NRL_REQUIRE(n_k >= 0 && n_k <= MT_MAX_K && (n_k == 0 || top_k), "impression_metrics: at most %d top_k values (got %d)", MT_MAX_K,
              n_k);
  for (int q = 0; q < n_k; ++q)
    NRL_REQUIRE(top_k[q] >= 1 && top_k[q] <= NRL_METRICS_MAX_K, "impression_metrics: every k in [1, %d] (got %d)",
                NRL_METRICS_MAX_K, top_k[q]);
  NRL_REQUIRE((sums == nullptr) == (count == nullptr), "impression_metrics: sums and count go together");
  NRL_REQUIRE(status, "impression_metrics: the status word is required");
  if (B == 0) return NRL_OK;
  NRL_REQUIRE(cand_offsets && (N == 0 || (preds && targets)), "impression_metrics: null argument");
  const int64_t* ca[2] = {cand_aspects0, cand_aspects1};
  const int64_t* ha[2] = {hist_aspects0, hist_aspects1};
  const int32_t ncs[2] = {num_classes0, num_classes1};
  int nc_max = 0;
  for (int a = 0; a < n_aspects; ++a) {
    NRL_REQUIRE(ncs[a] >= 2 && ncs[a] <= NRL_METRICS_MAX_CLASSES, "impression_metrics: num_classes in [2, %d] (aspect %d: %d)",
                NRL_METRICS_MAX_CLASSES, a, ncs[a]);
    NRL_REQUIRE((N == 0 || ca[a]) && (n_hist == 0 || ha[a]) && hist_offsets, "impression_metrics: aspect %d: null argument", a);
    nc_max = ncs[a] > nc_max ? ncs[a] : nc_max;
  }
  MtWs w;
  NRL_TRY(carve_workspace(ws, ws_bytes, [&](Arena& ar) { mt_layout(ar, N, B, n_aspects, n_k, &w); }));
  const int cols = mt_cols(n_aspects, n_k);
  const int64_t parts = ceil_div(B, MT_PART_ROWS);
  int32_t *const rank_ws = w.rank, *const valid = w.valid;
  float* const rows_ws = w.rows;
  double* const partial = w.partial;

  MtArgs A;
  A.preds = preds;
  A.targets = targets;
  A.cand_off = cand_offsets;
  A.hist_off = hist_offsets;
  for (int a = 0; a < 2; ++a) {
    A.cand_asp[a] = a < n_aspects ? ca[a] : nullptr;
    A.hist_asp[a] = a < n_aspects ? ha[a] : nullptr;
    A.num_classes[a] = a < n_aspects ? ncs[a] : 0;
  }
  A.n_aspects = n_aspects;
  for (int q = 0; q < MT_MAX_K; ++q) A.k[q] = q < n_k ? top_k[q] : 0;
  A.n_k = n_k;
  A.n_cols = cols;
  A.nc_pad = (nc_max + 63) & ~63;
  A.N = N;
  A.n_hist = n_hist;
  A.B = B;
  A.rank = rank ? rank : rank_ws;
  A.rows = rows ? rows : rows_ws;
  A.valid = valid;
  A.status = status;
  hipStream_t st = (hipStream_t)stream;
  const size_t smem = (size_t)(2 * MT_BLOCK_TILE + 2 * MT_WAVES * A.nc_pad) * sizeof(uint32_t);      // 4 KB + 32 B per class: <= 36 KB
  mt_impressions_kernel<<<(unsigned)ceil_div(B, MT_WAVES), MT_THREADS, smem, st>>>(A);
  NRL_LAUNCH_CHECK();
  if (sums) {
    mt_reduce_parts_kernel<<<(unsigned)parts, MT_THREADS, 0, st>>>(A.rows, valid, B, cols, partial);
    NRL_LAUNCH_CHECK();
    mt_reduce_final_kernel<<<1, MT_THREADS, 0, st>>>(partial, parts, cols, sums, count);
    NRL_LAUNCH_CHECK();
  }
  return NRL_OK;
}

// ---- a grid of weight rows
// the rows, only when the caller keeps none | the per-impression valid flags | the reductions' per-config, per-part sums (+ count)
struct MgWs {
  float* rows;
  int32_t* valid;
  double* partial;
};
static void mg_layout(Arena& a, int64_t B, int32_t G, int n_aspects, int n_k, bool own_rows, MgWs* w) {
  const int cols = mt_cols(n_aspects, n_k);
  w->rows = own_rows ? a.take<float>((size_t)G * B * cols) : nullptr;
  w->valid = a.take<int32_t>((size_t)B);
  w->partial = a.take<double>((size_t)G * ceil_div(B, MT_PART_ROWS) * (cols + 1));
}

int32_t nrl_grid_metrics_configs_per_block(int64_t B, int32_t G) {
  if (B <= 0 || G <= 0) return 1;
  const int64_t blocks = ceil_div(B, MT_WAVES);
  int64_t ranges = ceil_div(MG_TARGET_BLOCKS, blocks);
  ranges = ranges < 1 ? 1 : (ranges > G ? G : ranges);
  return (int32_t)ceil_div(G, ranges);
}

size_t nrl_grid_metrics_workspace_size(int64_t B, int32_t G, int32_t n_aspects, int32_t n_k, int32_t caller_rows) {
  if (B <= 0 || B >= ((int64_t)1 << 31) || G < 1 || G > MG_MAX_G || n_aspects < 0 || n_aspects > 2 || n_k < 0 || n_k > MT_MAX_K)
    return 256;
  return measure_workspace<MgWs>([&](Arena& a, auto* w) { mg_layout(a, B, G, n_aspects, n_k, caller_rows == 0, w); });
}

int nrl_grid_metrics(const float* comp, int32_t T, const float* weights, int32_t G, const float* targets, const int64_t* cand_offsets,
                     int64_t N, int64_t B, int32_t n_aspects, const int64_t* cand_aspects0, const int64_t* hist_aspects0,
                     int32_t num_classes0, const int64_t* cand_aspects1, const int64_t* hist_aspects1, int32_t num_classes1,
                     const int64_t* hist_offsets, int64_t n_hist, const int32_t* top_k, int32_t n_k, int32_t configs_per_block,
                     float* rows, float* preds, double* sums, int64_t* count, int32_t* status, void* ws, size_t ws_bytes,
                     void* stream) {
  NRL_REQUIRE(N >= 0 && B >= 0 && n_hist >= 0, "grid_metrics: negative size");
  NRL_REQUIRE(B < ((int64_t)1 << 31), "grid_metrics: at most 2^31 - 1 impressions per call (got %lld)", (long long)B);
  NRL_REQUIRE(T >= 1 && T <= MG_MAX_T, "grid_metrics: 1 <= T <= %d components (got %d)", MG_MAX_T, T);
  NRL_REQUIRE(G >= 1 && G <= MG_MAX_G, "grid_metrics: 1 <= G <= %d weight rows (got %d)", MG_MAX_G, G);
  NRL_REQUIRE(configs_per_block >= 0, "grid_metrics: configs_per_block >= 0, 0 = the plan (got %d)", configs_per_block);
  NRL_REQUIRE(n_aspects >= 0 && n_aspects <= 2, "grid_metrics: n_aspects in {0, 1, 2} (got %d)", n_aspects);
  NRL_REQUIRE(n_k >= 0 && n_k <= MT_MAX_K && (n_k == 0 || top_k), "grid_metrics: at most %d top_k values (got %d)", MT_MAX_K, n_k);
  for (int q = 0; q < n_k; ++q)
    NRL_REQUIRE(top_k[q] >= 1 && top_k[q] <= NRL_METRICS_MAX_K, "grid_metrics: every k in [1, %d] (got %d)", NRL_METRICS_MAX_K,
                top_k[q]);
  NRL_REQUIRE((sums == nullptr) == (count == nullptr), "grid_metrics: sums and count go together");
  NRL_REQUIRE(status, "grid_metrics: the status word is required");
  NRL_REQUIRE(weights, "grid_metrics: null weights");
  if (B == 0) return NRL_OK;
  NRL_REQUIRE(cand_offsets && (N == 0 || (comp && targets)), "grid_metrics: null argument");
  const int64_t* ca[2] = {cand_aspects0, cand_aspects1};
  const int64_t* ha[2] = {hist_aspects0, hist_aspects1};
  const int32_t ncs[2] = {num_classes0, num_classes1};
  int nc_max = 0;
  for (int a = 0; a < n_aspects; ++a) {
    NRL_REQUIRE(ncs[a] >= 2 && ncs[a] <= NRL_METRICS_MAX_CLASSES, "grid_metrics: num_classes in [2, %d] (aspect %d: %d)",
                NRL_METRICS_MAX_CLASSES, a, ncs[a]);
    NRL_REQUIRE((N == 0 || ca[a]) && (n_hist == 0 || ha[a]) && hist_offsets, "grid_metrics: aspect %d: null argument", a);
    nc_max = ncs[a] > nc_max ? ncs[a] : nc_max;
  }
  MgWs w;
  NRL_TRY(carve_workspace(ws, ws_bytes, [&](Arena& ar) { mg_layout(ar, B, G, n_aspects, n_k, rows == nullptr, &w); }));
  const int cols = mt_cols(n_aspects, n_k);
  const int64_t parts = ceil_div(B, MT_PART_ROWS);

  MgArgs A;
  MtArgs& M = A.M;
  M.preds = nullptr;
  M.targets = targets;
  M.cand_off = cand_offsets;
  M.hist_off = hist_offsets;
  for (int a = 0; a < 2; ++a) {
    M.cand_asp[a] = a < n_aspects ? ca[a] : nullptr;
    M.hist_asp[a] = a < n_aspects ? ha[a] : nullptr;
    M.num_classes[a] = a < n_aspects ? ncs[a] : 0;
  }
  M.n_aspects = n_aspects;
  for (int q = 0; q < MT_MAX_K; ++q) M.k[q] = q < n_k ? top_k[q] : 0;
  M.n_k = n_k;
  M.n_cols = cols;
  M.nc_pad = (nc_max + 63) & ~63;
  M.N = N;
  M.n_hist = n_hist;
  M.B = B;
  M.rank = nullptr;
  M.rows = rows ? rows : w.rows;
  M.valid = w.valid;
  M.status = status;
  A.comp = comp;
  A.weights = weights;
  A.preds = preds;
  A.T = T;
  A.G = G;
  A.g_per = configs_per_block > 0 ? (configs_per_block < G ? configs_per_block : G) : nrl_grid_metrics_configs_per_block(B, G);
  hipStream_t st = (hipStream_t)stream;
  // keys 2 KB + three histograms per wave (12 B a class a wave) + 16-bit ranks 8 KB: <= 58 KB
  const size_t smem = (size_t)(MT_BLOCK_TILE + 3 * MT_WAVES * M.nc_pad) * sizeof(uint32_t) + (size_t)MT_MAX_C * sizeof(uint16_t);
  const dim3 grid((unsigned)ceil_div(B, MT_WAVES), (unsigned)ceil_div(G, A.g_per));
  mt_grid_kernel<<<grid, MT_THREADS, smem, st>>>(A);
  NRL_LAUNCH_CHECK();
  if (sums) {
    mt_grid_reduce_parts_kernel<<<dim3((unsigned)parts, (unsigned)G), MT_THREADS, 0, st>>>(M.rows, w.valid, B, cols, parts, w.partial);
    NRL_LAUNCH_CHECK();
    mt_grid_reduce_final_kernel<<<(unsigned)G, MT_THREADS, 0, st>>>(w.partial, parts, cols, sums, count);
    NRL_LAUNCH_CHECK();
  }
  return NRL_OK;
}

}  // extern "C"

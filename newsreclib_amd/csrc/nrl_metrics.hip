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

}  // extern "C"

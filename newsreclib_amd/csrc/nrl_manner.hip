// MANNeR (fair_rec/manner_a_module.py:151-176, manner_module.py:152-204): the two computations of the family that had no kernel.
//
//   nrl_supcon_embed_fwd_bwd   the A-Module loss: pytorch-metric-learning's SupConLoss over DotProductSimilarity of a batch of news
//                              embeddings E (N, D) with integer labels, loss and dE in one call.
//       1. S = E E^T on the library's exact-fp32 MFMA GEMM (nrl_linear_fwd) into an (N, Np) workspace -- under BOTH engine settings:
//          the scores go through exp(), the two products are a few MFLOP, and the (hi, lo) bf16 split's ~1e-5 relative error
//          measured up to 7x over the bound the loss is held to (tests/test_gpu_manner.py); the call runs under EngineScope(1).
//          Np = N rounded up to 4 (the activation-gradient GEMM reads it as its k-contiguous operand); E is copied to Np zero-padded
//          rows when N % 4 != 0;
//       2. mn_row_stats_kernel: one wave per anchor row -- max, log-sum-exp over the off-diagonal, number of positives, row loss;
//       3. mn_pair_grad_kernel: every wave first adds the N row losses in the SAME fixed order (n_kept, the loss, the three "exactly
//          zero" cases), then writes its row of G = dS + dS^T.  G_ij needs row j's statistics and S_ji; S_ji is read as S_ij (equal
//          up to the rounding of the symmetric product).  G is stored in column chunks of MA_KCHUNK = 128: chunk c is an
//          (N, width_c) row-major matrix;
//       4. dE = G E (nrl_linear_bwd, activation gradient only), ONE GEMM PER COLUMN CHUNK, the chunks' partial products added in
//          chunk order by mn_chunk_sum_kernel.  The exact GEMM keeps one running fp32 accumulator along its reduction; over the
//          1024 anchors of the largest batch that running sum alone put the gradient 1.9e-10 from float64 where the same loss in
//          torch ops is at 4e-11 (an fp32 emulation of both orders on the CPU attributes 1.0e-10 to it and 2.6e-11 to the
//          two-level order).  N <= 128 is one chunk written straight into dE: no extra launch at the configured batch of 85.
//       No atomics, no host synchronisation: run-to-run bit-identical.
//
//   nrl_manner_scores          the ensemble scorer: one workgroup per impression, straight from up to three cached news-vector tables.
//       per sub-model: mean of the history rows (registers -> LDS), one wave per candidate dot product, mean and UNBIASED standard
//       deviation over the impression's own candidates (two passes over the scores in LDS), z-score, weighted sum in registers.
//       Reference quirks kept (manner_module.py:175-186), no epsilon anywhere:
//         * one candidate   -> torch.std of one value is NaN -> the row is NaN;
//         * zero variance   -> (s - mean) / 0 = NaN (or +-inf when rounding leaves a residue);
//         * empty history   -> 0 / 0 user vector -> NaN row.
//       Padded slots of `out` are written 0.  News indices outside [0, V) are clamped: the kernel never reads outside a table.
#include <math.h>

#include "nrl_api_internal.h"          // EngineScope: the per-call engine of this thread

namespace nrl {

// This unit's own names carry MA_ / ma_ (MN_ / mn_ is nrl_miner.hip's).  The kernels and the MnTables of their signature keep the
// mn_ spelling: it is the symbol the code object and every profile of it carry.
constexpr int MA_THREADS = 256;
constexpr int MA_WAVES = MA_THREADS / 64;
constexpr int MA_MAX_N = 1024;       // anchors of one SupCon batch
constexpr int MA_MAX_D = 1024;
constexpr int MA_CAND_REGS = 8;      // candidates per thread held in registers: max_cand <= MA_THREADS * MA_CAND_REGS
constexpr int MA_MAX_TABLES = 3;
constexpr int MA_KCHUNK = 128;       // anchors per partial product of dE = G E

// ---- embedding SupCon ------------------------------------------------------------------------------------------------------
// dst (Np, D) = [E; 0]
__global__ void mn_pad_rows_kernel(const float* __restrict__ E, int64_t N, int64_t Np, int D, float* __restrict__ dst) {
  const int64_t total = Np * (int64_t)(D >> 2);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / (D >> 2);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r < N) v = ld4(E + 4 * i);
    *reinterpret_cast<float4*>(dst + 4 * i) = v;
  }
}

// stats: lse (N) | row loss (N) | number of positives (N)
__global__ __launch_bounds__(MA_THREADS) void mn_row_stats_kernel(const float* __restrict__ S, const int64_t* __restrict__ labels,
                                                                  int N, int ld, float inv_t, float* __restrict__ stats) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = blockIdx.x * MA_WAVES + wave;
  if (i >= N) return;
  const float* row = S + (int64_t)i * ld;
  const int64_t li = labels[i];
  float mx = -INFINITY;
  for (int j = lane; j < N; j += 64)
    if (j != i) mx = fmaxf(mx, row[j] * inv_t);
  mx = wave_max(mx);
  float se = 0.f, sp = 0.f, np = 0.f;
  for (int j = lane; j < N; j += 64) {
    if (j == i) continue;
    const float v = row[j] * inv_t;
    se += expf(v - mx);
    if (labels[j] == li) {
      sp += v;
      np += 1.f;
    }
  }
  se = wave_sum(se);
  sp = wave_sum(sp);
  np = wave_sum(np);
  if (lane == 0) {
    const float lse = N > 1 ? mx + logf(se) : 0.f;          // (nothing kept: the library's masked logsumexp gives 0)
    stats[i] = lse;
    stats[N + i] = np > 0.f ? lse - sp / np : 0.f;          // -mean over positives of (s - lse); no positive: 0, dropped by the reducer
    stats[2 * N + i] = np;
  }
}

// G: column chunk c (columns [c * MA_KCHUNK, min(ld, (c + 1) * MA_KCHUNK))) is an (N, width_c) row-major matrix at G + N * c * MA_KCHUNK
__global__ __launch_bounds__(MA_THREADS) void mn_pair_grad_kernel(const float* __restrict__ S, float* __restrict__ G,
                                                                  const int64_t* __restrict__ labels, int N, int ld, float inv_t,
                                                                  float grad_scale, const float* __restrict__ stats,
                                                                  float* __restrict__ loss) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = blockIdx.x * MA_WAVES + wave;
  if (i >= N) return;
  const float* lse = stats;
  const float* rl = stats + N;
  const float* npos = stats + 2 * N;
  // the reducer, identically in every wave: lane l adds rows l, l + 64, ... in order, then the butterfly
  float kept = 0.f, lsum = 0.f, tot_pos = 0.f, some_neg = 0.f;
  for (int r = lane; r < N; r += 64) {
    const float l = rl[r];
    if (l > 0.f) {
      kept += 1.f;
      lsum += l;
    }
    tot_pos += npos[r];
    if (npos[r] < (float)(N - 1)) some_neg = 1.f;
  }
  kept = wave_sum(kept);
  lsum = wave_sum(lsum);
  tot_pos = wave_sum(tot_pos);
  some_neg = wave_max(some_neg);
  const bool live = tot_pos > 0.f && some_neg > 0.f && kept > 0.f;
  if (i == 0 && lane == 0) *loss = live ? lsum / kept : 0.f;
  const float coef = live ? grad_scale * inv_t / kept : 0.f;
  const int64_t li = labels[i];
  const float lse_i = lse[i], np_i = npos[i];
  const bool keep_i = rl[i] > 0.f;
  const float* row = S + (int64_t)i * ld;
  for (int j = lane; j < ld; j += 64) {
    float g = 0.f;
    if (j < N && j != i && coef != 0.f) {
      const float v = row[j] * inv_t;
      const bool same = labels[j] == li;
      if (keep_i) g += expf(v - lse_i) - (same ? 1.f / np_i : 0.f);
      if (rl[j] > 0.f) g += expf(v - lse[j]) - (same ? 1.f / npos[j] : 0.f);
      g *= coef;
    }
    const int c0 = (j / MA_KCHUNK) * MA_KCHUNK;
    const int wc = ld - c0 < MA_KCHUNK ? ld - c0 : MA_KCHUNK;
    G[(int64_t)N * c0 + (int64_t)i * wc + (j - c0)] = g;
  }
}

// out (n4 float4) = part[0] + part[1] + ... + part[chunks - 1], in that order
__global__ void mn_chunk_sum_kernel(const float* __restrict__ part, int chunks, int64_t n4, float* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    float4 a = ld4(part + 4 * i);
    for (int c = 1; c < chunks; ++c) {
      const float4 b = ld4(part + ((int64_t)c * n4 + i) * 4);
      a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
    }
    *reinterpret_cast<float4*>(out + 4 * i) = a;
  }
}

// ---- ensemble scorer -----------------------------------------------------------------------------------------------------------
struct MnTables {
  const float* table[MA_MAX_TABLES];
  float weight[MA_MAX_TABLES];
  int k;
};

__global__ __launch_bounds__(MA_THREADS) void mn_scores_kernel(MnTables T, int64_t V, const int64_t* __restrict__ hist_idx,
                                                               const int64_t* __restrict__ hist_off,
                                                               const int64_t* __restrict__ cand_idx,
                                                               const int64_t* __restrict__ cand_off, int max_cand, int D,
                                                               float* __restrict__ out) {
  extern __shared__ float4 ma_smem4[];
  float* u = reinterpret_cast<float*>(ma_smem4);          // [D] user vector of the current sub-model
  float* sc = u + D;                                      // [max_cand] its raw scores
  __shared__ float red[MA_WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, D4 = D >> 2;
  const int64_t b = blockIdx.x;
  const int64_t h0 = hist_off[b], c0 = cand_off[b];
  const int nh = (int)(hist_off[b + 1] - h0);
  int nc = (int)(cand_off[b + 1] - c0);
  if (nc > max_cand) nc = max_cand;                       // (validated on the host: never write outside the row)
  float acc[MA_CAND_REGS];
#pragma unroll
  for (int r = 0; r < MA_CAND_REGS; ++r) acc[r] = 0.f;
  for (int t = 0; t < T.k; ++t) {
    const float* tab = T.table[t];
    __syncthreads();                                      // the previous sub-model's u / sc are no longer read
    // user vector: thread d4 owns four columns, rows added in history order
    for (int d4 = threadIdx.x; d4 < D4; d4 += MA_THREADS) {
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
    for (int c = wave; c < nc; c += MA_WAVES) {
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
    for (int c = threadIdx.x; c < nc; c += MA_THREADS) part += sc[c];
    const float mean = block_sum<MA_WAVES>(part, red) / (float)nc;
    part = 0.f;
    for (int c = threadIdx.x; c < nc; c += MA_THREADS) {
      const float d = sc[c] - mean;
      part += d * d;
    }
    const float sd = sqrtf(block_sum<MA_WAVES>(part, red) / (float)(nc - 1));        // nc == 1: 0 / 0 = NaN, as torch.std
    const float wt = T.weight[t];
#pragma unroll
    for (int r = 0; r < MA_CAND_REGS; ++r) {
      const int c = threadIdx.x + r * MA_THREADS;
      if (c < nc) {
        const float z = (sc[c] - mean) / sd;
        acc[r] = t == 0 ? wt * z : acc[r] + wt * z;
      }
    }
  }
#pragma unroll
  for (int r = 0; r < MA_CAND_REGS; ++r) {
    const int c = threadIdx.x + r * MA_THREADS;
    if (c < max_cand) out[b * max_cand + c] = c < nc ? acc[r] : 0.f;
  }
}

}  // namespace nrl

using namespace nrl;

extern "C" {

// workspace of the two nrl_linear_* calls | E padded to Np rows | S | G | row stats | per-chunk dE (more than one column chunk only)
struct SupconWs {
  unsigned char* gemm;
  size_t gemm_bytes;
  float *Epad, *S, *G, *stats, *part;
};
static void supcon_layout(Arena& a, int64_t N, int32_t D, SupconWs* w) {
  const int64_t Np = (N + 3) & ~(int64_t)3;
  const int64_t chunks = ceil_div(Np, MA_KCHUNK);
  w->gemm_bytes = Arena::round_up(nrl_linear_workspace_bytes((int32_t)Np, D), 256);
  w->gemm = a.take<unsigned char>(w->gemm_bytes);
  w->Epad = a.take<float>((size_t)Np * D);
  w->S = a.take<float>((size_t)N * Np);
  w->G = a.take<float>((size_t)N * Np);
  w->stats = a.take<float>((size_t)3 * N);
  w->part = chunks > 1 ? a.take<float>((size_t)chunks * N * D) : nullptr;
}

size_t nrl_supcon_embed_workspace_bytes(int64_t N, int32_t D) {
  if (N <= 0 || D <= 0) return 256;
  return measure_workspace<SupconWs>([&](Arena& a, auto* w) { supcon_layout(a, N, D, w); });
}

int nrl_supcon_embed_fwd_bwd(const float* E, const int64_t* labels, int64_t N, int32_t D, float temperature, float grad_scale,
                             float* loss, float* dE, void* ws, size_t ws_bytes, void* stream) {
  NRL_REQUIRE(E && labels && loss && dE, "supcon_embed: null argument");
  NRL_REQUIRE(N >= 1 && N <= MA_MAX_N, "supcon_embed: 1 <= N <= %d anchors (got %lld)", MA_MAX_N, (long long)N);
  NRL_REQUIRE(D >= 4 && D <= MA_MAX_D && D % 4 == 0, "supcon_embed: D a multiple of 4 up to %d (got %d)", MA_MAX_D, D);
  NRL_REQUIRE(temperature > 0.f, "supcon_embed: temperature must be positive");
  NRL_REQUIRE((((uintptr_t)E | (uintptr_t)dE) & 15) == 0, "supcon_embed: E / dE must be 16-byte aligned");
  SupconWs w;
  NRL_TRY(carve_workspace(ws, ws_bytes, [&](Arena& a) { supcon_layout(a, N, D, &w); }));
  hipStream_t st = (hipStream_t)stream;
  const EngineScope exact(1);          // 1 = exact fp32 for the two nrl_linear_* calls below, whatever the process default
  const int64_t Np = (N + 3) & ~(int64_t)3;
  void* const gemm_ws = w.gemm;
  float *const Epad = w.Epad, *const S = w.S, *const G = w.G, *const stats = w.stats, *const part = w.part;
  const int chunks = (int)ceil_div(Np, MA_KCHUNK);
  const float* Ew = E;
  if (Np != N) {
    const int64_t total = Np * (int64_t)(D / 4);
    mn_pad_rows_kernel<<<(unsigned)ceil_div(total, 256), 256, 0, st>>>(E, N, Np, D, Epad);
    NRL_LAUNCH_CHECK();
    Ew = Epad;
  }
  const float inv_t = 1.0f / temperature;
  const unsigned blocks = (unsigned)ceil_div(N, MA_WAVES);
  NRL_TRY(nrl_linear_fwd(E, Ew, nullptr, N, (int32_t)Np, D, S, gemm_ws, w.gemm_bytes, stream));      // S (N, Np) = E [E; 0]^T
  mn_row_stats_kernel<<<blocks, MA_THREADS, 0, st>>>(S, labels, (int)N, (int)Np, inv_t, stats);
  NRL_LAUNCH_CHECK();
  mn_pair_grad_kernel<<<blocks, MA_THREADS, 0, st>>>(S, G, labels, (int)N, (int)Np, inv_t, grad_scale, stats, loss);
  NRL_LAUNCH_CHECK();
  // dE (N, D) = sum over the column chunks of G_c (N, width_c) [E; 0][chunk rows]
  for (int c = 0; c < chunks; ++c) {
    const int64_t c0 = (int64_t)c * MA_KCHUNK;
    const int32_t wc = (int32_t)(Np - c0 < MA_KCHUNK ? Np - c0 : MA_KCHUNK);
    float* dst = chunks == 1 ? dE : part + (int64_t)c * N * D;
    NRL_TRY(nrl_linear_bwd(nullptr, Ew + c0 * D, G + N * c0, N, wc, D, dst, nullptr, nullptr, gemm_ws, w.gemm_bytes, stream));
  }
  if (chunks > 1) {
    const int64_t n4 = N * (int64_t)(D / 4);
    mn_chunk_sum_kernel<<<(unsigned)ceil_div(n4, 256), 256, 0, st>>>(part, chunks, n4, dE);
    NRL_LAUNCH_CHECK();
  }
  return NRL_OK;
}

int nrl_manner_scores(const float* const* tables, const float* weights, int32_t k, int64_t V, const int64_t* hist_idx,
                      const int64_t* hist_offsets, const int64_t* cand_idx, const int64_t* cand_offsets, int64_t B,
                      int32_t max_cand, int32_t D, float* out, void* stream) {
  NRL_REQUIRE(tables && weights && hist_idx && hist_offsets && cand_idx && cand_offsets && out, "manner_scores: null argument");
  NRL_REQUIRE(k >= 1 && k <= MA_MAX_TABLES, "manner_scores: 1 <= k <= %d news-vector tables (got %d)", MA_MAX_TABLES, k);
  NRL_REQUIRE(V >= 1 && B >= 0, "manner_scores: bad sizes");
  NRL_REQUIRE(D >= 4 && D <= MA_MAX_D && D % 4 == 0, "manner_scores: D a multiple of 4 up to %d (got %d)", MA_MAX_D, D);
  NRL_REQUIRE(max_cand >= 1 && max_cand <= MA_THREADS * MA_CAND_REGS, "manner_scores: 1 <= max_cand <= %d (got %d)",
              MA_THREADS * MA_CAND_REGS, max_cand);
  MnTables T;
  T.k = k;
  for (int t = 0; t < MA_MAX_TABLES; ++t) {
    T.table[t] = t < k ? tables[t] : nullptr;
    T.weight[t] = t < k ? weights[t] : 0.f;
    NRL_REQUIRE(t >= k || (T.table[t] != nullptr && ((uintptr_t)T.table[t] & 15) == 0), "manner_scores: table %d null or not 16-byte aligned", t);
  }
  if (B == 0) return NRL_OK;
  const size_t smem = (size_t)(D + ((max_cand + 3) & ~3)) * sizeof(float);
  mn_scores_kernel<<<(unsigned)B, MA_THREADS, smem, (hipStream_t)stream>>>(T, V, hist_idx, hist_offsets, cand_idx, cand_offsets,
                                                                           max_cand, D, out);
  NRL_LAUNCH_CHECK();
  return NRL_OK;
}

}  // extern "C"

// SentiDebias (fair_rec/senti_debias_module.py:164-263,406-411,475-530): the head around the NRMS encoders.  Plain fp32 vector code
// under both engines.  The organising fact: with S = num_sent_classes + 1 classes every sentiment vector is a row of the (S, D) table
// T = tanh(E W^T + b) (aspect.py SentimentEncoder), so no (N, 256) embedding, (N, D) sentiment vector or N x 256 x 300 GEMM exists:
//   nrl_sd_rowcos_*     cos(news_r, T[id_r]) per flat news row (one wave per row), both side sums (history | candidates) in one launch;
//                       backward: d_news rows and the gradient of T binned by class
//   nrl_sd_hist_*       the dense (B, H, D) sentiment history straight from ids and T, ZERO at padded slots (a real row of id 0 is
//                       T[0] = tanh(bias), not zero); backward bins into T
//   nrl_sd_late_*       late fusion: u_aware = (class counts / n_b) T, no dense tensor
//   nrl_sd_scores_*     bias-aware scores u_aware T^T gathered by candidate class (0 at padded slots) added onto the bias-free scores
//   nrl_sd_disc_tail_*  (N, Hd) hidden rows -> linear2 (O outputs) -> log-softmax -> cross entropy against the wrapped target
//                       (:409: column id - 1, id 0 wraps to the LAST column) -> both side sums; backward: d_pre = d_hidden (1 - h^2)
//                       and the gradients of linear2
//   nrl_sd_bt_matmul    out (S, D) = W^T X for W (B, S), X (B, D), users added in order
// No float atomics: what is reduced over rows (the side sums, the gradients of T / linear2) goes through per-wave LDS bins, per-block
// slabs and a fixed-order sum (nrl_sd_pair_sum here, nrl_miner_slab_sum for the slabs): bit-reproducible run to run.
#include <math.h>

#include "nrl_kernels.h"

namespace nrl {

constexpr int SD_THREADS = 256;
constexpr int SD_WAVES = SD_THREADS / 64;
constexpr int SD_ROWS = 64;          // rows (or slots) per workgroup = per slab
constexpr int SD_MAXC = 8;           // classes (sentiment table rows, discriminator outputs) held in registers
constexpr float SD_EPS = 1e-8f;      // senti_debias_module.py:212,223,235

// floats of one discriminator slab: O * Hd (d_W2) | O (d_b2), padded to 4 so that every wave's bins stay 16-byte aligned
__host__ __device__ __forceinline__ int sd_disc_width(int Hd, int O) { return (O * Hd + O + 3) & ~3; }

// the per-wave bins of a workgroup added in wave order into its slab
__device__ __forceinline__ void sd_bins_to_slab(const float* bins, int n, float* __restrict__ slab) {
  __syncthreads();
  for (int j = threadIdx.x; j < n; j += SD_THREADS) {
    float acc = 0.f;
#pragma unroll
    for (int w = 0; w < SD_WAVES; ++w) acc += bins[w * n + j];
    slab[j] = acc;
  }
}

// the two side sums of a workgroup (lane-uniform per wave) added in wave order
__device__ __forceinline__ void sd_pair_to_partial(float a, float b, float* __restrict__ partial) {
  __shared__ float red[SD_WAVES][2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    red[wave][0] = a;
    red[wave][1] = b;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    float acc = 0.f;
#pragma unroll
    for (int w = 0; w < SD_WAVES; ++w) acc += red[w][threadIdx.x];
    partial[threadIdx.x] = acc;
  }
}

// out[j] = scale_j * sum over the workgroups (in order) of partial[2 g + j], j in {0, 1}
__global__ void sd_pair_sum_kernel(const float* __restrict__ partial, int64_t groups, float s0, float s1, float* __restrict__ out) {
  if (threadIdx.x < 2) {
    float acc = 0.f;
    for (int64_t g = 0; g < groups; ++g) acc += partial[2 * g + threadIdx.x];
    out[threadIdx.x] = acc * (threadIdx.x == 0 ? s0 : s1);
  }
}

// ---- row cosines -----------------------------------------------------------------------------------------------------------
struct SdCos {
  float dot, aa, bb;
};
__device__ __forceinline__ SdCos sd_cos_terms(const float* __restrict__ a, const float* __restrict__ b, int D4, int lane) {
  SdCos c = {0.f, 0.f, 0.f};
  for (int d4 = lane; d4 < D4; d4 += 64) {
    const float4 x = ld4(a + 4 * d4), y = ld4(b + 4 * d4);
    c.dot += dot4(x, y);
    c.aa += dot4(x, x);
    c.bb += dot4(y, y);
  }
  c.dot = wave_sum(c.dot);
  c.aa = wave_sum(c.aa);
  c.bb = wave_sum(c.bb);
  return c;
}

__global__ __launch_bounds__(SD_THREADS) void sd_rowcos_fwd_kernel(const float* __restrict__ news, const int64_t* __restrict__ ids,
                                                                   const float* __restrict__ T, int64_t N, int64_t n_hist, int D,
                                                                   int S, float* __restrict__ partial) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, D4 = D >> 2;
  const int64_t r0 = (int64_t)blockIdx.x * SD_ROWS;
  const int64_t r1 = r0 + SD_ROWS < N ? r0 + SD_ROWS : N;
  float acc_h = 0.f, acc_c = 0.f;
  for (int64_t r = r0 + wave; r < r1; r += SD_WAVES) {
    const int64_t id = ids[r];
    if (id < 0 || id >= S) continue;          // (validated on the host; never read outside T)
    const SdCos c = sd_cos_terms(news + r * D, T + id * D, D4, lane);
    const float cosv = c.dot / (SD_EPS + sqrtf(c.aa) * sqrtf(c.bb));
    if (r < n_hist) acc_h += cosv; else acc_c += cosv;
  }
  sd_pair_to_partial(acc_h, acc_c, partial + 2 * (int64_t)blockIdx.x);
}

// d_out: (2) gradients of the two side MEANS; d_news (N, D) overwritten (may be null); slab (S * D) per workgroup (may be null)
__global__ __launch_bounds__(SD_THREADS) void sd_rowcos_bwd_kernel(const float* __restrict__ news, const int64_t* __restrict__ ids,
                                                                   const float* __restrict__ T, const float* __restrict__ d_out,
                                                                   int64_t N, int64_t n_hist, int D, int S, float inv_h, float inv_c,
                                                                   float* __restrict__ d_news, float* __restrict__ slab) {
  extern __shared__ float4 sd_smem4[];
  float* bins = reinterpret_cast<float*>(sd_smem4);            // [SD_WAVES][S * D]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, D4 = D >> 2, SDn = S * D;
  if (slab != nullptr) {
    for (int j = threadIdx.x; j < SD_WAVES * SDn; j += SD_THREADS) bins[j] = 0.f;
    __syncthreads();
  }
  const float g_h = d_out[0] * inv_h, g_c = d_out[1] * inv_c;
  const int64_t r0 = (int64_t)blockIdx.x * SD_ROWS;
  const int64_t r1 = r0 + SD_ROWS < N ? r0 + SD_ROWS : N;
  for (int64_t r = r0 + wave; r < r1; r += SD_WAVES) {
    const int64_t id = ids[r];
    const bool ok = id >= 0 && id < S;
    const float* a = news + r * D;
    const float* b = T + (ok ? id : 0) * D;
    const SdCos c = sd_cos_terms(a, b, D4, lane);
    const float na = sqrtf(c.aa), nb = sqrtf(c.bb), den = SD_EPS + na * nb;
    const float g = ok ? (r < n_hist ? g_h : g_c) : 0.f;
    const float lin = g / den;                                                  // coefficient of the other operand
    const float qa = na > 0.f ? g * c.dot * nb / (na * den * den) : 0.f;        // of a itself (norm subgradient 0 at 0)
    const float qb = nb > 0.f ? g * c.dot * na / (nb * den * den) : 0.f;
    float* wb = bins + wave * SDn + (ok ? id : 0) * D;
    for (int d4 = lane; d4 < D4; d4 += 64) {
      const float4 x = ld4(a + 4 * d4), y = ld4(b + 4 * d4);
      if (d_news != nullptr)
        st4(d_news + r * D + 4 * d4,
               make_float4(lin * y.x - qa * x.x, lin * y.y - qa * x.y, lin * y.z - qa * x.z, lin * y.w - qa * x.w));
      if (slab != nullptr && ok) {
        float4 t = ld4(wb + 4 * d4);
        t.x += lin * x.x - qb * y.x;
        t.y += lin * x.y - qb * y.y;
        t.z += lin * x.z - qb * y.z;
        t.w += lin * x.w - qb * y.w;
        st4(wb + 4 * d4, t);
      }
    }
  }
  if (slab != nullptr) sd_bins_to_slab(bins, SDn, slab + (int64_t)blockIdx.x * SDn);
}

// ---- dense sentiment history -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SD_THREADS) void sd_hist_fwd_kernel(const int64_t* __restrict__ ids, const int64_t* __restrict__ off,
                                                                 const float* __restrict__ T, int64_t B, int H, int D, int S,
                                                                 int64_t n_ids, float* __restrict__ out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, D4 = D >> 2;
  const int64_t slots = B * H;
  const int64_t s0 = (int64_t)blockIdx.x * SD_ROWS;
  const int64_t s1 = s0 + SD_ROWS < slots ? s0 + SD_ROWS : slots;
  for (int64_t s = s0 + wave; s < s1; s += SD_WAVES) {
    const int64_t b = s / H, h = s % H, o = off[b], n = off[b + 1] - o;
    int64_t id = -1;
    if (h < n && o + h < n_ids) id = ids[o + h];
    const bool ok = id >= 0 && id < S;
    for (int d4 = lane; d4 < D4; d4 += 64)
      st4(out + s * D + 4 * d4, ok ? ld4(T + id * D + 4 * d4) : make_float4(0.f, 0.f, 0.f, 0.f));
  }
}

__global__ __launch_bounds__(SD_THREADS) void sd_hist_bwd_kernel(const float* __restrict__ d_out, const int64_t* __restrict__ ids,
                                                                 const int64_t* __restrict__ off, int64_t B, int H, int D, int S,
                                                                 int64_t n_ids, float* __restrict__ slab) {
  extern __shared__ float4 sd_smem4[];
  float* bins = reinterpret_cast<float*>(sd_smem4);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, D4 = D >> 2, SDn = S * D;
  for (int j = threadIdx.x; j < SD_WAVES * SDn; j += SD_THREADS) bins[j] = 0.f;
  __syncthreads();
  const int64_t slots = B * H;
  const int64_t s0 = (int64_t)blockIdx.x * SD_ROWS;
  const int64_t s1 = s0 + SD_ROWS < slots ? s0 + SD_ROWS : slots;
  for (int64_t s = s0 + wave; s < s1; s += SD_WAVES) {
    const int64_t b = s / H, h = s % H, o = off[b], n = off[b + 1] - o;
    int64_t id = -1;
    if (h < n && o + h < n_ids) id = ids[o + h];
    if (id < 0 || id >= S) continue;
    float* wb = bins + wave * SDn + id * D;
    for (int d4 = lane; d4 < D4; d4 += 64) {
      const float4 g = ld4(d_out + s * D + 4 * d4);
      float4 t = ld4(wb + 4 * d4);
      t.x += g.x;
      t.y += g.y;
      t.z += g.z;
      t.w += g.w;
      st4(wb + 4 * d4, t);
    }
  }
  sd_bins_to_slab(bins, SDn, slab + (int64_t)blockIdx.x * SDn);
}

// ---- late fusion: class fractions and u_aware = frac T (one wave per user) -------------------------------------------------------
__global__ __launch_bounds__(SD_THREADS) void sd_late_fwd_kernel(const int64_t* __restrict__ ids, const int64_t* __restrict__ off,
                                                                 const float* __restrict__ T, int64_t B, int D, int S, int64_t n_ids,
                                                                 float* __restrict__ frac, float* __restrict__ u) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, D4 = D >> 2;
  const int64_t b = (int64_t)blockIdx.x * SD_WAVES + wave;
  if (b >= B) return;
  const int64_t o = off[b], n = off[b + 1] - o;
  float cnt[SD_MAXC];
#pragma unroll
  for (int c = 0; c < SD_MAXC; ++c) cnt[c] = 0.f;
  for (int64_t h = lane; h < n && o + h < n_ids; h += 64) {
    const int64_t id = ids[o + h];
#pragma unroll
    for (int c = 0; c < SD_MAXC; ++c) cnt[c] += id == c ? 1.f : 0.f;
  }
  const float nf = (float)n;                       // (:203-205: the sum over the history divided by the history size)
#pragma unroll
  for (int c = 0; c < SD_MAXC; ++c) {
    cnt[c] = wave_sum(cnt[c]) / nf;
    if (lane == 0 && c < S) frac[b * S + c] = cnt[c];
  }
  for (int d4 = lane; d4 < D4; d4 += 64) {
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int c = 0; c < SD_MAXC; ++c)
      if (c < S) {
        const float4 t = ld4(T + c * D + 4 * d4);
        acc.x += cnt[c] * t.x;
        acc.y += cnt[c] * t.y;
        acc.z += cnt[c] * t.z;
        acc.w += cnt[c] * t.w;
      }
    st4(u + b * D + 4 * d4, acc);
  }
}

// out (S, D) = W^T X, W (B, S), X (B, D); the users are added in order
__global__ void sd_bt_matmul_kernel(const float* __restrict__ W, const float* __restrict__ X, int64_t B, int S, int D,
                                    float* __restrict__ out) {
  const int D4 = D >> 2;
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= S * D4) return;
  const int s = idx / D4, d4 = idx % D4;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int64_t b = 0; b < B; ++b) {
    const float w = W[b * S + s];
    const float4 x = ld4(X + b * D + 4 * d4);
    acc.x += w * x.x;
    acc.y += w * x.y;
    acc.z += w * x.z;
    acc.w += w * x.w;
  }
  st4(out + (int64_t)s * D + 4 * d4, acc);
}

// ---- bias-aware scores (one wave per user) -----------------------------------------------------------------------------------
__global__ __launch_bounds__(SD_THREADS) void sd_scores_fwd_kernel(const float* __restrict__ u, const float* __restrict__ T,
                                                                   const int64_t* __restrict__ ids, const int64_t* __restrict__ off,
                                                                   const float* __restrict__ free_scores, int64_t B, int C, int D,
                                                                   int S, int64_t n_ids, float* __restrict__ P,
                                                                   float* __restrict__ out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, D4 = D >> 2;
  const int64_t b = (int64_t)blockIdx.x * SD_WAVES + wave;
  if (b >= B) return;                       // (no workgroup barrier below)
  float p[SD_MAXC];                         // u_aware . T[c], lane-uniform
#pragma unroll
  for (int c = 0; c < SD_MAXC; ++c) {
    float acc = 0.f;
    if (c < S)
      for (int d4 = lane; d4 < D4; d4 += 64) acc += dot4(ld4(u + b * D + 4 * d4), ld4(T + c * D + 4 * d4));
    p[c] = wave_sum(acc);
    if (lane == 0 && c < S && P != nullptr) P[b * S + c] = p[c];
  }
  const int64_t o = off[b], n = off[b + 1] - o;
  for (int c = lane; c < C; c += 64) {
    float aware = 0.f;
    if (c < n && o + c < n_ids) {
      const int64_t id = ids[o + c];
#pragma unroll
      for (int k = 0; k < SD_MAXC; ++k) aware += (k < S && id == k) ? p[k] : 0.f;
    }
    out[b * C + c] = free_scores[b * C + c] + aware;
  }
}

// d_out (B, C) -> dP (B, S), d_u (B, D) = dP T
__global__ __launch_bounds__(SD_THREADS) void sd_scores_bwd_kernel(const float* __restrict__ d_out, const float* __restrict__ T,
                                                                   const int64_t* __restrict__ ids, const int64_t* __restrict__ off,
                                                                   int64_t B, int C, int D, int S, int64_t n_ids,
                                                                   float* __restrict__ dP, float* __restrict__ d_u) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, D4 = D >> 2;
  const int64_t b = (int64_t)blockIdx.x * SD_WAVES + wave;
  if (b >= B) return;
  const int64_t o = off[b], n = off[b + 1] - o;
  float acc[SD_MAXC];
#pragma unroll
  for (int c = 0; c < SD_MAXC; ++c) acc[c] = 0.f;
  for (int c = lane; c < C && c < n && o + c < n_ids; c += 64) {
    const int64_t id = ids[o + c];
    const float g = d_out[b * C + c];
#pragma unroll
    for (int k = 0; k < SD_MAXC; ++k) acc[k] += id == k ? g : 0.f;
  }
#pragma unroll
  for (int c = 0; c < SD_MAXC; ++c) {
    acc[c] = wave_sum(acc[c]);
    if (lane == 0 && c < S) dP[b * S + c] = acc[c];
  }
  for (int d4 = lane; d4 < D4; d4 += 64) {
    float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int c = 0; c < SD_MAXC; ++c)
      if (c < S) {
        const float4 t = ld4(T + c * D + 4 * d4);
        g.x += acc[c] * t.x;
        g.y += acc[c] * t.y;
        g.z += acc[c] * t.z;
        g.w += acc[c] * t.w;
      }
    st4(d_u + b * D + 4 * d4, g);
  }
}

// ---- discriminator tail ------------------------------------------------------------------------------------------------------
// logits of one hidden row (lane-uniform), their log-sum-exp, and the wrapped target column: senti_debias_module.py:409 writes the
// one-hot at column `targets[i] - 1`, so id 0 (unknown sentiment) indexes column -1 = the LAST column; ids above O raise on the host
struct SdLogits {
  float l[SD_MAXC];
  float lse;
  int target;       // -1: id out of range (no loss, no gradient)
};
__device__ __forceinline__ SdLogits sd_logits(const float* __restrict__ h, const float* __restrict__ W2, const float* __restrict__ b2,
                                              int64_t id, int Hd4, int Hd, int O, int lane) {
  SdLogits r;
  float mx = -INFINITY;
#pragma unroll
  for (int o = 0; o < SD_MAXC; ++o) {
    float acc = 0.f;
    if (o < O)
      for (int d4 = lane; d4 < Hd4; d4 += 64) acc += dot4(ld4(h + 4 * d4), ld4(W2 + o * Hd + 4 * d4));
    acc = wave_sum(acc);
    r.l[o] = o < O ? acc + b2[o] : -INFINITY;
    mx = fmaxf(mx, r.l[o]);
  }
  float se = 0.f;
#pragma unroll
  for (int o = 0; o < SD_MAXC; ++o) se += o < O ? expf(r.l[o] - mx) : 0.f;
  r.lse = mx + logf(se);
  r.target = (id < 0 || id > O) ? -1 : (id == 0 ? O - 1 : (int)id - 1);
  return r;
}

__global__ __launch_bounds__(SD_THREADS) void sd_disc_tail_fwd_kernel(const float* __restrict__ Hh, const float* __restrict__ W2,
                                                                      const float* __restrict__ b2, const int64_t* __restrict__ ids,
                                                                      int64_t N, int64_t n_hist, int Hd, int O,
                                                                      float* __restrict__ partial) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, Hd4 = Hd >> 2;
  const int64_t r0 = (int64_t)blockIdx.x * SD_ROWS;
  const int64_t r1 = r0 + SD_ROWS < N ? r0 + SD_ROWS : N;
  float acc_h = 0.f, acc_c = 0.f;
  for (int64_t r = r0 + wave; r < r1; r += SD_WAVES) {
    const SdLogits g = sd_logits(Hh + r * Hd, W2, b2, ids[r], Hd4, Hd, O, lane);
    float lt = 0.f;
#pragma unroll
    for (int o = 0; o < SD_MAXC; ++o) lt += o == g.target ? g.l[o] : 0.f;
    const float loss = g.target >= 0 ? g.lse - lt : 0.f;
    if (r < n_hist) acc_h += loss; else acc_c += loss;
  }
  sd_pair_to_partial(acc_h, acc_c, partial + 2 * (int64_t)blockIdx.x);
}

// d_pre (N, Hd) = (sum_o dl_o W2[o]) (1 - h^2), dl_o = g (softmax_o - [o == target]); slab per workgroup: O * Hd (d_W2) | O (d_b2)
__global__ __launch_bounds__(SD_THREADS) void sd_disc_tail_bwd_kernel(const float* __restrict__ Hh, const float* __restrict__ W2,
                                                                      const float* __restrict__ b2, const int64_t* __restrict__ ids,
                                                                      const float* __restrict__ d_out, int64_t N, int64_t n_hist,
                                                                      int Hd, int O, float inv_h, float inv_c,
                                                                      float* __restrict__ d_pre, float* __restrict__ slab) {
  extern __shared__ float4 sd_smem4[];
  float* bins = reinterpret_cast<float*>(sd_smem4);            // [SD_WAVES][sd_disc_width]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, Hd4 = Hd >> 2, W = sd_disc_width(Hd, O);
  if (slab != nullptr) {
    for (int j = threadIdx.x; j < SD_WAVES * W; j += SD_THREADS) bins[j] = 0.f;
    __syncthreads();
  }
  const float g_h = d_out[0] * inv_h, g_c = d_out[1] * inv_c;
  const int64_t r0 = (int64_t)blockIdx.x * SD_ROWS;
  const int64_t r1 = r0 + SD_ROWS < N ? r0 + SD_ROWS : N;
  float* wb = bins + wave * W;
  for (int64_t r = r0 + wave; r < r1; r += SD_WAVES) {
    const float* h = Hh + r * Hd;
    const SdLogits g = sd_logits(h, W2, b2, ids[r], Hd4, Hd, O, lane);
    const float gr = g.target >= 0 ? (r < n_hist ? g_h : g_c) : 0.f;
    float dl[SD_MAXC];
#pragma unroll
    for (int o = 0; o < SD_MAXC; ++o) dl[o] = o < O ? gr * (expf(g.l[o] - g.lse) - (o == g.target ? 1.f : 0.f)) : 0.f;
    for (int d4 = lane; d4 < Hd4; d4 += 64) {
      const float4 x = ld4(h + 4 * d4);
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int o = 0; o < SD_MAXC; ++o)
        if (o < O) {
          const float4 w = ld4(W2 + o * Hd + 4 * d4);
          acc.x += dl[o] * w.x;
          acc.y += dl[o] * w.y;
          acc.z += dl[o] * w.z;
          acc.w += dl[o] * w.w;
          if (slab != nullptr) {
            float4 t = ld4(wb + o * Hd + 4 * d4);
            t.x += dl[o] * x.x;
            t.y += dl[o] * x.y;
            t.z += dl[o] * x.z;
            t.w += dl[o] * x.w;
            st4(wb + o * Hd + 4 * d4, t);
          }
        }
      st4(d_pre + r * Hd + 4 * d4, make_float4(acc.x * (1.f - x.x * x.x), acc.y * (1.f - x.y * x.y),
                                                  acc.z * (1.f - x.z * x.z), acc.w * (1.f - x.w * x.w)));
    }
    if (slab != nullptr && lane == 0) {
#pragma unroll
      for (int o = 0; o < SD_MAXC; ++o)
        if (o < O) wb[O * Hd + o] += dl[o];
    }
  }
  if (slab != nullptr) sd_bins_to_slab(bins, W, slab + (int64_t)blockIdx.x * W);
}

static int sd_pair_sum(const float* partial, int64_t groups, float s0, float s1, float* out, hipStream_t st) {
  sd_pair_sum_kernel<<<1, 64, 0, st>>>(partial, groups, s0, s1, out);
  NRL_LAUNCH_CHECK();
  return NRL_OK;
}

static inline unsigned sd_blocks(int64_t rows) { return (unsigned)ceil_div(rows, SD_ROWS); }
static inline float sd_inv(int64_t n) { return n > 0 ? 1.f / (float)n : 0.f; }
constexpr size_t SD_LDS_STATIC_MAX = 48 * 1024;      // bins: SD_WAVES * width floats, kept under the default dynamic-LDS limit

}  // namespace nrl

using namespace nrl;

extern "C" {

int64_t nrl_sd_num_slabs(int64_t rows) { return rows > 0 ? ceil_div(rows, SD_ROWS) : 0; }
int32_t nrl_sd_disc_slab_width(int32_t Hd, int32_t O) { return sd_disc_width(Hd, O); }

int nrl_sd_rowcos_fwd(const float* news, const int64_t* ids, const float* T, int64_t N, int64_t n_hist, int32_t D, int32_t S,
                      float* partial, float* out2, void* stream) {
  NRL_REQUIRE(news && ids && T && partial && out2 && N > 0 && n_hist >= 0 && n_hist <= N && D > 0 && D % 4 == 0 && S > 0 &&
                  S <= SD_MAXC, "nrl_sd_rowcos_fwd: bad arguments (D %% 4 == 0, S <= %d)", SD_MAXC);
  hipStream_t st = (hipStream_t)stream;
  sd_rowcos_fwd_kernel<<<sd_blocks(N), SD_THREADS, 0, st>>>(news, ids, T, N, n_hist, D, S, partial);
  NRL_LAUNCH_CHECK();
  return sd_pair_sum(partial, nrl_sd_num_slabs(N), sd_inv(n_hist), sd_inv(N - n_hist), out2, st);
}

int nrl_sd_rowcos_bwd(const float* news, const int64_t* ids, const float* T, const float* d_out2, int64_t N, int64_t n_hist,
                      int32_t D, int32_t S, float* d_news, float* slabs, void* stream) {
  NRL_REQUIRE(news && ids && T && d_out2 && N > 0 && n_hist >= 0 && n_hist <= N && D > 0 && D % 4 == 0 && S > 0 && S <= SD_MAXC &&
                  (d_news || slabs), "nrl_sd_rowcos_bwd: bad arguments");
  const size_t lds = slabs ? (size_t)SD_WAVES * S * D * sizeof(float) : 0;
  NRL_REQUIRE(lds <= SD_LDS_STATIC_MAX, "nrl_sd_rowcos_bwd: S * D = %d exceeds the LDS bins", S * D);
  sd_rowcos_bwd_kernel<<<sd_blocks(N), SD_THREADS, lds, (hipStream_t)stream>>>(news, ids, T, d_out2, N, n_hist, D, S, sd_inv(n_hist),
                                                                              sd_inv(N - n_hist), d_news, slabs);
  NRL_LAUNCH_CHECK();
  return NRL_OK;
}

int nrl_sd_hist_fwd(const int64_t* ids, const int64_t* hist_off, const float* T, int64_t B, int32_t H, int32_t D, int32_t S,
                    int64_t n_ids, float* out, void* stream) {
  NRL_REQUIRE(ids && hist_off && T && out && B > 0 && H > 0 && D > 0 && D % 4 == 0 && S > 0 && S <= SD_MAXC && n_ids >= 0,
              "nrl_sd_hist_fwd: bad arguments");
  sd_hist_fwd_kernel<<<sd_blocks(B * H), SD_THREADS, 0, (hipStream_t)stream>>>(ids, hist_off, T, B, H, D, S, n_ids, out);
  NRL_LAUNCH_CHECK();
  return NRL_OK;
}

int nrl_sd_hist_bwd(const float* d_out, const int64_t* ids, const int64_t* hist_off, int64_t B, int32_t H, int32_t D, int32_t S,
                    int64_t n_ids, float* slabs, void* stream) {
  NRL_REQUIRE(d_out && ids && hist_off && slabs && B > 0 && H > 0 && D > 0 && D % 4 == 0 && S > 0 && S <= SD_MAXC && n_ids >= 0,
              "nrl_sd_hist_bwd: bad arguments");
  const size_t lds = (size_t)SD_WAVES * S * D * sizeof(float);
  NRL_REQUIRE(lds <= SD_LDS_STATIC_MAX, "nrl_sd_hist_bwd: S * D = %d exceeds the LDS bins", S * D);
  sd_hist_bwd_kernel<<<sd_blocks(B * H), SD_THREADS, lds, (hipStream_t)stream>>>(d_out, ids, hist_off, B, H, D, S, n_ids, slabs);
  NRL_LAUNCH_CHECK();
  return NRL_OK;
}

int nrl_sd_late_fwd(const int64_t* ids, const int64_t* hist_off, const float* T, int64_t B, int32_t D, int32_t S, int64_t n_ids,
                    float* frac, float* u, void* stream) {
  NRL_REQUIRE(ids && hist_off && T && frac && u && B > 0 && D > 0 && D % 4 == 0 && S > 0 && S <= SD_MAXC && n_ids >= 0,
              "nrl_sd_late_fwd: bad arguments");
  sd_late_fwd_kernel<<<(unsigned)ceil_div(B, SD_WAVES), SD_THREADS, 0, (hipStream_t)stream>>>(ids, hist_off, T, B, D, S, n_ids, frac, u);
  NRL_LAUNCH_CHECK();
  return NRL_OK;
}

int nrl_sd_bt_matmul(const float* W, const float* X, int64_t B, int32_t S, int32_t D, float* out, void* stream) {
  NRL_REQUIRE(W && X && out && B > 0 && S > 0 && D > 0 && D % 4 == 0, "nrl_sd_bt_matmul: bad arguments");
  const int n = S * (D / 4);
  sd_bt_matmul_kernel<<<(unsigned)ceil_div(n, SD_THREADS), SD_THREADS, 0, (hipStream_t)stream>>>(W, X, B, S, D, out);
  NRL_LAUNCH_CHECK();
  return NRL_OK;
}

int nrl_sd_scores_fwd(const float* u, const float* T, const int64_t* ids, const int64_t* cand_off, const float* free_scores,
                      int64_t B, int32_t C, int32_t D, int32_t S, int64_t n_ids, float* P, float* out, void* stream) {
  NRL_REQUIRE(u && T && ids && cand_off && free_scores && out && B > 0 && C > 0 && D > 0 && D % 4 == 0 && S > 0 && S <= SD_MAXC &&
                  n_ids >= 0, "nrl_sd_scores_fwd: bad arguments");
  sd_scores_fwd_kernel<<<(unsigned)ceil_div(B, SD_WAVES), SD_THREADS, 0, (hipStream_t)stream>>>(u, T, ids, cand_off, free_scores, B, C,
                                                                                               D, S, n_ids, P, out);
  NRL_LAUNCH_CHECK();
  return NRL_OK;
}

int nrl_sd_scores_bwd(const float* d_out, const float* T, const int64_t* ids, const int64_t* cand_off, int64_t B, int32_t C,
                      int32_t D, int32_t S, int64_t n_ids, float* dP, float* d_u, void* stream) {
  NRL_REQUIRE(d_out && T && ids && cand_off && dP && d_u && B > 0 && C > 0 && D > 0 && D % 4 == 0 && S > 0 && S <= SD_MAXC &&
                  n_ids >= 0, "nrl_sd_scores_bwd: bad arguments");
  sd_scores_bwd_kernel<<<(unsigned)ceil_div(B, SD_WAVES), SD_THREADS, 0, (hipStream_t)stream>>>(d_out, T, ids, cand_off, B, C, D, S,
                                                                                               n_ids, dP, d_u);
  NRL_LAUNCH_CHECK();
  return NRL_OK;
}

int nrl_sd_disc_tail_fwd(const float* hidden, const float* w2, const float* b2, const int64_t* ids, int64_t N, int64_t n_hist,
                         int32_t Hd, int32_t O, float* partial, float* out2, void* stream) {
  NRL_REQUIRE(hidden && w2 && b2 && ids && partial && out2 && N > 0 && n_hist >= 0 && n_hist <= N && Hd > 0 && Hd % 4 == 0 &&
                  O > 0 && O <= SD_MAXC, "nrl_sd_disc_tail_fwd: bad arguments (hidden %% 4 == 0, outputs <= %d)", SD_MAXC);
  hipStream_t st = (hipStream_t)stream;
  sd_disc_tail_fwd_kernel<<<sd_blocks(N), SD_THREADS, 0, st>>>(hidden, w2, b2, ids, N, n_hist, Hd, O, partial);
  NRL_LAUNCH_CHECK();
  return sd_pair_sum(partial, nrl_sd_num_slabs(N), sd_inv(n_hist), sd_inv(N - n_hist), out2, st);
}

int nrl_sd_disc_tail_bwd(const float* hidden, const float* w2, const float* b2, const int64_t* ids, const float* d_out2, int64_t N,
                         int64_t n_hist, int32_t Hd, int32_t O, float* d_pre, float* slabs, void* stream) {
  NRL_REQUIRE(hidden && w2 && b2 && ids && d_out2 && d_pre && N > 0 && n_hist >= 0 && n_hist <= N && Hd > 0 && Hd % 4 == 0 &&
                  O > 0 && O <= SD_MAXC, "nrl_sd_disc_tail_bwd: bad arguments");
  const size_t lds = slabs ? (size_t)SD_WAVES * sd_disc_width(Hd, O) * sizeof(float) : 0;
  NRL_REQUIRE(lds <= SD_LDS_STATIC_MAX, "nrl_sd_disc_tail_bwd: outputs * hidden = %d exceeds the LDS bins", O * Hd);
  sd_disc_tail_bwd_kernel<<<sd_blocks(N), SD_THREADS, lds, (hipStream_t)stream>>>(hidden, w2, b2, ids, d_out2, N, n_hist, Hd, O,
                                                                                 sd_inv(n_hist), sd_inv(N - n_hist), d_pre, slabs);
  NRL_LAUNCH_CHECK();
  return NRL_OK;
}

}  // extern "C"

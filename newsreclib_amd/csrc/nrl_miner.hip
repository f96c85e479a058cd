// MINER (miner_module.py:258-323,398-406; layers/attention.py:93-166; components/utils.py): the non-GEMM stages of the
// poly-attention user encoder, its category bias, the three score aggregations and the disagreement loss.  Plain fp32 vector
// code under both engines; the two bias-free projections (E W^T, user_vector Wt^T) run on the GEMM engines through
// ops_blocks.LinearActFn / LinearFn.  History and candidate rows stay FLAT (ragged, offsets): a padded history row of the
// reference has a zero embedding and logit 1e-30, so it only adds exp(1e-30 - max) to a softmax denominator -- a closed-form
// term here (max_hist - n_i of them for user i), never a row.
//   nrl_miner_categ_bias_*   unit-normalised category rows, per-user and total candidate sums, bias per flat history row
//   nrl_miner_poly_*         one workgroup per user: logits P codes^T (+ bias), the 1e-30 fill, softmax over max_hist, A E
//   nrl_miner_score_*        one workgroup per user: S = cand user_vector^T, then max / mean / target-aware weighted sum;
//                            candidates are walked in tiles (LDS does not grow with the candidate count)
//   nrl_miner_cos_*          sum of the off-diagonal cosines of the rows of each group (the disagreement loss), its gradient
//   nrl_miner_wgrad          d_W = G^T X of a bias-free projection: slabs of 64 rows, then the slabs in order (the engines'
//                            weight gradient adds split partial sums atomically); nrl_miner_tanh_grad feeds it
//   nrl_miner_slab_sum       out[j] = scale * sum over slabs s (in order) of slabs[s][j]
// No float atomics: reductions over users write per-user slabs that nrl_miner_slab_sum adds in a fixed order.
#include <math.h>

#include "nrl_kernels.h"

namespace nrl {

constexpr int MN_THREADS = 256;
constexpr int MN_WAVES = MN_THREADS / 64;
constexpr size_t MN_LDS_MAX = 160 * 1024;      // LDS of one gfx950 workgroup
constexpr int MN_CT = 32;                      // candidates per tile of the score backward
constexpr float MN_FILL = 1e-30f;              // attention.py:117: masked_fill_(~mask, 1e-30), NOT -inf

__device__ __forceinline__ float4 mn_sub4(float4 a, float4 b) { return make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w); }
__device__ __forceinline__ void mn_fma4(float4& acc, float s, float4 v) {
  acc.x += s * v.x;
  acc.y += s * v.y;
  acc.z += s * v.z;
  acc.w += s * v.w;
}
__device__ __forceinline__ float mn_gelu(float z) { return 0.5f * z * (1.f + erff(z * 0.70710678118654752f)); }
__device__ __forceinline__ float mn_gelu_grad(float z) {
  return 0.5f * (1.f + erff(z * 0.70710678118654752f)) + z * 0.39894228040143268f * expf(-0.5f * z * z);
}

// every kernel here may take up to the whole LDS of a workgroup: the attribute is raised once per kernel, not per launch
static int mn_set_lds(const void* fn, size_t bytes, const char* what, bool* raised) {
  NRL_REQUIRE(bytes <= MN_LDS_MAX, "%s: needs %zu bytes of LDS (limit %zu)", what, bytes, MN_LDS_MAX);
  if (bytes > 64 * 1024 && !*raised) {
    NRL_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)MN_LDS_MAX));
    *raised = true;
  }
  return NRL_OK;
}

// ---- bit-reproducible weight gradient of a bias-free projection ------------------------------------------------------------
// d_pre = d_c * (1 - c^2): the tanh derivative from the saved output
__global__ void miner_tanh_grad_kernel(const float4* __restrict__ d_c, const float4* __restrict__ c, int64_t n4,
                                       float4* __restrict__ out) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const float4 g = d_c[i], y = c[i];
    out[i] = make_float4(g.x * (1.f - y.x * y.x), g.y * (1.f - y.y * y.y), g.z * (1.f - y.z * y.z), g.w * (1.f - y.w * y.w));
  }
}

constexpr int MN_WG_ROWS = 64;       // rows per slab
constexpr int MN_WG_TN = 16;         // weight rows per workgroup
// slab[chunk][n][k] = sum over the rows r of the chunk (in order) of G[r][n] X[r][k], for G (R, N), X (R, K)
__global__ __launch_bounds__(MN_THREADS) void miner_wgrad_kernel(const float* __restrict__ G, const float* __restrict__ X,
                                                                 int64_t R, int N, int K, float* __restrict__ slab) {
  const int64_t r0 = (int64_t)blockIdx.x * MN_WG_ROWS;
  const int64_t r1 = r0 + MN_WG_ROWS < R ? r0 + MN_WG_ROWS : R;
  const int n0 = blockIdx.y * MN_WG_TN, K4 = K >> 2;
  for (int idx = threadIdx.x; idx < MN_WG_TN * K4; idx += MN_THREADS) {
    const int n = n0 + idx / K4, k4 = idx % K4;
    if (n >= N) break;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 8
    for (int64_t r = r0; r < r1; ++r) mn_fma4(acc, G[r * N + n], ld4(X + r * K + 4 * k4));
    st4(slab + ((int64_t)blockIdx.x * N + n) * K + 4 * k4, acc);
  }
}

// ---- fixed-order slab sum ------------------------------------------------------------------------------------------------
__global__ void miner_slab_sum_kernel(const float* __restrict__ slabs, int64_t S, int64_t n, float scale,
                                      float* __restrict__ out) {
  for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < n; j += (int64_t)gridDim.x * blockDim.x) {
    float acc = 0.f;
    for (int64_t s = 0; s < S; ++s) acc += slabs[s * n + j];
    out[j] = acc * scale;
  }
}

static int mn_slab_sum(const float* slabs, int64_t S, int64_t n, float scale, float* out, hipStream_t st) {
  const int64_t g = ceil_div(n, MN_THREADS);
  miner_slab_sum_kernel<<<(unsigned)(g < 1 ? 1 : (g > 4096 ? 4096 : g)), MN_THREADS, 0, st>>>(slabs, S, n, scale, out);
  NRL_LAUNCH_CHECK();
  return NRL_OK;
}

// ---- cosine disagreement ---------------------------------------------------------------------------------------------------
// group g holds R rows of D features; xh_k = x_k / (|x_k| + eps).  The sum over k != l of xh_k . xh_l is |sum_k xh_k|^2 -
// sum_k |xh_k|^2: no R x R matrix.  LDS: sS[D] (the row sum), sR[R] (1 / (|x_k| + eps)).
__device__ __forceinline__ void mn_cos_rowsum(const float* __restrict__ x, int R, int D, float eps, float* sS, float* sR,
                                              float& sumsq) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, D4 = D >> 2;
  sumsq = 0.f;
  for (int k = wave; k < R; k += MN_WAVES) {
    float acc = 0.f;
    for (int d4 = lane; d4 < D4; d4 += 64) {
      const float4 v = ld4(x + (int64_t)k * D + 4 * d4);
      acc += dot4(v, v);
    }
    acc = wave_sum(acc);
    const float r = 1.f / (sqrtf(acc) + eps);
    if (lane == 0) {
      sR[k] = r;
      sumsq += acc * r * r;
    }
  }
  __syncthreads();
  for (int d4 = threadIdx.x; d4 < D4; d4 += MN_THREADS) {
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int k = 0; k < R; ++k) mn_fma4(acc, sR[k], ld4(x + (int64_t)k * D + 4 * d4));
    st4(sS + 4 * d4, acc);
  }
  __syncthreads();
}

__global__ __launch_bounds__(MN_THREADS) void miner_cos_fwd_kernel(const float* __restrict__ X, int R, int D, float eps,
                                                                   float* __restrict__ partial) {
  extern __shared__ float4 mn_smem4[];
  float* sS = reinterpret_cast<float*>(mn_smem4);
  float* sR = sS + D;
  __shared__ float red[MN_WAVES];
  const float* x = X + (int64_t)blockIdx.x * R * D;
  float sumsq;
  mn_cos_rowsum(x, R, D, eps, sS, sR, sumsq);
  float ss = 0.f;
  for (int d = threadIdx.x; d < D; d += MN_THREADS) ss += sS[d] * sS[d];
  const float total = block_sum<MN_WAVES>(ss, red);
  const float diag = block_sum<MN_WAVES>(sumsq, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = total - diag;
}

// d_x of loss = coef * sum_g partial[g], coef = d_loss[0] * scale
__global__ __launch_bounds__(MN_THREADS) void miner_cos_bwd_kernel(const float* __restrict__ X, int R, int D, float eps,
                                                                   const float* __restrict__ d_loss, float scale,
                                                                   float* __restrict__ d_X) {
  extern __shared__ float4 mn_smem4[];
  float* sS = reinterpret_cast<float*>(mn_smem4);
  float* sR = sS + D;
  const float* x = X + (int64_t)blockIdx.x * R * D;
  float* dx = d_X + (int64_t)blockIdx.x * R * D;
  float unused;
  mn_cos_rowsum(x, R, D, eps, sS, sR, unused);
  const float c = d_loss[0] * scale;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, D4 = D >> 2;
  for (int k = wave; k < R; k += MN_WAVES) {
    float sx = 0.f, xx = 0.f;
    for (int d4 = lane; d4 < D4; d4 += 64) {
      const float4 v = ld4(x + (int64_t)k * D + 4 * d4);
      sx += dot4(v, ld4(sS + 4 * d4));
      xx += dot4(v, v);
    }
    sx = wave_sum(sx);
    xx = wave_sum(xx);
    const float r = sR[k];
    const float nrm = sqrtf(xx);
    const float vx = 2.f * (sx - r * xx);                       // v_k . x_k, v_k = 2 (S - xh_k)
    const float coef = nrm > 0.f ? vx * r * r / nrm : 0.f;      // (the norm's subgradient at 0 is 0, as in autograd)
    for (int d4 = lane; d4 < D4; d4 += 64) {
      const float4 v = ld4(x + (int64_t)k * D + 4 * d4), s = ld4(sS + 4 * d4);
      float4 o;
      o.x = c * (2.f * (s.x - v.x * r) * r - v.x * coef);
      o.y = c * (2.f * (s.y - v.y * r) * r - v.y * coef);
      o.z = c * (2.f * (s.z - v.z * r) * r - v.z * coef);
      o.w = c * (2.f * (s.w - v.w * r) * r - v.w * coef);
      st4(dx + (int64_t)k * D + 4 * d4, o);
    }
  }
}

// ---- category bias -------------------------------------------------------------------------------------------------------
// workspace (floats): rn_h[nh4] | rn_c[nc4] | s_own[B * Dc] | s_all[Dc] | q_own[B * Dc] | q_all[Dc]   (nh4, nc4: padded to 4)
struct CbWs {
  float *rn_h, *rn_c, *s_own, *s_all, *q_own, *q_all;
};
static void cb_layout(Arena& a, int64_t B, int64_t n_hist, int64_t n_cand, int32_t Dc, CbWs* w) {
  w->rn_h = a.take<float>((size_t)n_hist, 4 * sizeof(float));
  w->rn_c = a.take<float>((size_t)n_cand, 4 * sizeof(float));
  w->s_own = a.take<float>((size_t)B * Dc, sizeof(float));
  w->s_all = a.take<float>((size_t)Dc, sizeof(float));
  w->q_own = a.take<float>((size_t)B * Dc, sizeof(float));
  w->q_all = a.take<float>((size_t)Dc, sizeof(float));
}
// the slab workspaces: per-chunk partial weight gradients (wgrad) / per-user code gradients (poly backward), summed by mn_slab_sum
static void mn_slabs_layout(Arena& a, int64_t num_slabs, int64_t n, float** slabs) {
  *slabs = a.take<float>((size_t)num_slabs * (size_t)n, sizeof(float));
}

// one workgroup per user: 1 / |c| of its candidate rows, then s_own[b] = sum of its unit rows (row order)
__global__ __launch_bounds__(MN_THREADS) void miner_cb_cand_kernel(const float* __restrict__ cc,
                                                                   const int64_t* __restrict__ cand_off, int Dc,
                                                                   float* rn_c, float* __restrict__ s_own) {
  const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, D4 = Dc >> 2;
  const int64_t c0 = cand_off[b], c1 = cand_off[b + 1];
  for (int64_t c = c0 + wave; c < c1; c += MN_WAVES) {
    float acc = 0.f;
    for (int d4 = lane; d4 < D4; d4 += 64) {
      const float4 v = ld4(cc + c * Dc + 4 * d4);
      acc += dot4(v, v);
    }
    acc = wave_sum(acc);
    if (lane == 0) rn_c[c] = 1.f / sqrtf(acc);           // no epsilon (torchmetrics' cosine): a zero row gives NaN there too
  }
  __syncthreads();
  for (int d4 = threadIdx.x; d4 < D4; d4 += MN_THREADS) {
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int64_t c = c0; c < c1; ++c) mn_fma4(acc, rn_c[c], ld4(cc + c * Dc + 4 * d4));
    st4(s_own + (int64_t)b * Dc + 4 * d4, acc);
  }
}

// one wave per history row: bias[t] = hh_t . (s_all - s_own[user(t)]) / n_cand
__global__ __launch_bounds__(MN_THREADS) void miner_cb_hist_kernel(const float* __restrict__ hc,
                                                                   const int64_t* __restrict__ batch_hist, int64_t n_hist,
                                                                   int Dc, float inv_n, const float* __restrict__ s_own,
                                                                   const float* __restrict__ s_all,
                                                                   float* __restrict__ rn_h, float* __restrict__ bias) {
  const int lane = threadIdx.x & 63, D4 = Dc >> 2;
  const int64_t t = blockIdx.x * (int64_t)MN_WAVES + (threadIdx.x >> 6);
  if (t >= n_hist) return;
  const float* so = s_own + batch_hist[t] * Dc;
  float ss = 0.f, dv = 0.f;
  for (int d4 = lane; d4 < D4; d4 += 64) {
    const float4 h = ld4(hc + t * Dc + 4 * d4);
    ss += dot4(h, h);
    dv += dot4(h, mn_sub4(ld4(s_all + 4 * d4), ld4(so + 4 * d4)));
  }
  ss = wave_sum(ss);
  dv = wave_sum(dv);
  if (lane == 0) {
    const float rn = 1.f / sqrtf(ss);
    rn_h[t] = rn;
    bias[t] = dv * rn * inv_n;
  }
}

// one workgroup per user: d_hc of its history rows and q_own[b] = sum_t (d_bias[t] / n_cand) hh_t (row order)
__global__ __launch_bounds__(MN_THREADS) void miner_cb_bwd_hist_kernel(
    const float* __restrict__ d_bias, const float* __restrict__ hc, const int64_t* __restrict__ hist_off, int Dc, float inv_n,
    const float* __restrict__ bias, const float* __restrict__ rn_h, const float* __restrict__ s_own,
    const float* __restrict__ s_all, float* __restrict__ q_own, float* __restrict__ d_hc) {
  const int b = blockIdx.x, D4 = Dc >> 2;
  const int64_t t0 = hist_off[b], t1 = hist_off[b + 1];
  for (int d4 = threadIdx.x; d4 < D4; d4 += MN_THREADS) {
    const float4 V = mn_sub4(ld4(s_all + 4 * d4), ld4(s_own + (int64_t)b * Dc + 4 * d4));
    float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int64_t t = t0; t < t1; ++t) {
      const float4 h = ld4(hc + t * Dc + 4 * d4);
      const float rn = rn_h[t], g = d_bias[t] * inv_n, hd = d_bias[t] * bias[t] * rn;      // hd: (hh . d_hh) / |h|
      mn_fma4(q, g * rn, h);
      float4 dh;
      dh.x = rn * (g * V.x - h.x * hd);
      dh.y = rn * (g * V.y - h.y * hd);
      dh.z = rn * (g * V.z - h.z * hd);
      dh.w = rn * (g * V.w - h.w * hd);
      st4(d_hc + t * Dc + 4 * d4, dh);
    }
    st4(q_own + (int64_t)b * Dc + 4 * d4, q);
  }
}

// one wave per candidate row: d_ch = q_all - q_own[user(c)], through the normalisation
__global__ __launch_bounds__(MN_THREADS) void miner_cb_bwd_cand_kernel(const float* __restrict__ cc,
                                                                       const int64_t* __restrict__ batch_cand, int64_t n_cand,
                                                                       int Dc, const float* __restrict__ rn_c,
                                                                       const float* __restrict__ q_own,
                                                                       const float* __restrict__ q_all,
                                                                       float* __restrict__ d_cc) {
  const int lane = threadIdx.x & 63, D4 = Dc >> 2;
  const int64_t c = blockIdx.x * (int64_t)MN_WAVES + (threadIdx.x >> 6);
  if (c >= n_cand) return;
  const float* qo = q_own + batch_cand[c] * Dc;
  const float rn = rn_c[c];
  float cd = 0.f;
  for (int d4 = lane; d4 < D4; d4 += 64)
    cd += dot4(ld4(cc + c * Dc + 4 * d4), mn_sub4(ld4(q_all + 4 * d4), ld4(qo + 4 * d4)));
  cd = wave_sum(cd) * rn * rn;                                                            // (ch . d_ch) / |c|
  for (int d4 = lane; d4 < D4; d4 += 64) {
    const float4 v = ld4(cc + c * Dc + 4 * d4), q = mn_sub4(ld4(q_all + 4 * d4), ld4(qo + 4 * d4));
    float4 d;
    d.x = rn * (q.x - v.x * cd);
    d.y = rn * (q.y - v.y * cd);
    d.z = rn * (q.z - v.z * cd);
    d.w = rn * (q.w - v.w * cd);
    st4(d_cc + c * Dc + 4 * d4, d);
  }
}

// ---- poly attention ------------------------------------------------------------------------------------------------------
// One workgroup per user b with n = its history length (rows r0 .. r0 + n of the flat E / P / bias).  LDS: the user's n x D
// tile of E when it fits (else it is read through the caches), then sA[K * Hs] (logits, then weights; Hs = max_hist).
// A (B, K, max_hist) keeps the weights of the n real rows (the rest of a row is not written).
__global__ __launch_bounds__(MN_THREADS) void miner_poly_fwd_kernel(
    const float* __restrict__ E, const float* __restrict__ P, const float* __restrict__ codes, const float* __restrict__ bias,
    const int64_t* __restrict__ hist_off, int Hs, int D, int Cd, int K, int tile_in_lds, float* __restrict__ uv,
    float* __restrict__ A) {
  extern __shared__ float4 mn_smem4[];
  float* sE = reinterpret_cast<float*>(mn_smem4);
  float* sA = sE + (tile_in_lds ? (size_t)Hs * D : 0);
  const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, D4 = D >> 2, C4 = Cd >> 2;
  const int64_t r0 = hist_off[b];
  const int n = min((int)(hist_off[b + 1] - r0), Hs);
  const float* Eb = E + r0 * D;
  if (tile_in_lds)
    for (int i = threadIdx.x; i < n * D4; i += MN_THREADS) st4(sE + 4 * i, ld4(Eb + 4 * (int64_t)i));
  // logits[k][t] = P[t] . codes[k] + bias[t]
  for (int idx = threadIdx.x; idx < K * n; idx += MN_THREADS) {
    const int k = idx / n, t = idx - k * n;
    const float* p = P + (r0 + t) * Cd;
    const float* q = codes + (int64_t)k * Cd;
    float acc = 0.f;
    for (int c4 = 0; c4 < C4; ++c4) acc += dot4(ld4(p + 4 * c4), ld4(q + 4 * c4));
    sA[k * Hs + t] = acc + (bias ? bias[r0 + t] : 0.f);
  }
  __syncthreads();
  // softmax over the max_hist positions: n logits and (Hs - n) times the fill value
  const int pad = Hs - n;
  for (int k = wave; k < K; k += MN_WAVES) {
    float m = pad > 0 ? MN_FILL : -INFINITY;
    for (int t = lane; t < n; t += 64) m = fmaxf(m, sA[k * Hs + t]);
    m = wave_max(m);
    float s = 0.f;
    for (int t = lane; t < n; t += 64) s += expf(sA[k * Hs + t] - m);
    s = wave_sum(s) + (float)pad * expf(MN_FILL - m);
    const float inv = 1.f / s;
    for (int t = lane; t < n; t += 64) {
      const float a = expf(sA[k * Hs + t] - m) * inv;
      sA[k * Hs + t] = a;
      A[((int64_t)b * K + k) * Hs + t] = a;
    }
  }
  __syncthreads();
  // user_vector[k] = sum_t A[k][t] E[t]   (padded rows have zero embeddings)
  const float* Et = tile_in_lds ? sE : Eb;
  for (int idx = threadIdx.x; idx < K * D4; idx += MN_THREADS) {
    const int k = idx / D4, d4 = idx - k * D4;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int t = 0; t < n; ++t) mn_fma4(acc, sA[k * Hs + t], ld4(Et + (int64_t)t * D + 4 * d4));
    st4(uv + ((int64_t)b * K + k) * D + 4 * d4, acc);
  }
}

// LDS: sA[K * Hs] weights, sL[K * Hs] d_A then d_logits.  slab (B, K, Cd): this user's part of d_codes.
__global__ __launch_bounds__(MN_THREADS) void miner_poly_bwd_kernel(
    const float* __restrict__ d_uv, const float* __restrict__ E, const float* __restrict__ P, const float* __restrict__ codes,
    const float* __restrict__ A, const int64_t* __restrict__ hist_off, int Hs, int D, int Cd, int K, float* __restrict__ d_E,
    float* __restrict__ d_P, float* __restrict__ d_bias, float* __restrict__ slab) {
  extern __shared__ float4 mn_smem4[];
  float* sA = reinterpret_cast<float*>(mn_smem4);
  float* sL = sA + (size_t)K * Hs;
  const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, D4 = D >> 2, C4 = Cd >> 2;
  const int64_t r0 = hist_off[b];
  const int n = min((int)(hist_off[b + 1] - r0), Hs);
  const float* du = d_uv + (int64_t)b * K * D;
  for (int idx = threadIdx.x; idx < K * n; idx += MN_THREADS) {
    const int k = idx / n, t = idx - k * n;
    sA[k * Hs + t] = A[((int64_t)b * K + k) * Hs + t];
    const float* e = E + (r0 + t) * D;
    const float* g = du + (int64_t)k * D;
    float acc = 0.f;
    for (int d4 = 0; d4 < D4; ++d4) acc += dot4(ld4(e + 4 * d4), ld4(g + 4 * d4));
    sL[k * Hs + t] = acc;                                          // d_A[k][t]; 0 at the padded rows (zero embeddings)
  }
  __syncthreads();
  for (int k = wave; k < K; k += MN_WAVES) {
    float dot = 0.f;
    for (int t = lane; t < n; t += 64) dot += sA[k * Hs + t] * sL[k * Hs + t];
    dot = wave_sum(dot);
    for (int t = lane; t < n; t += 64) sL[k * Hs + t] = sA[k * Hs + t] * (sL[k * Hs + t] - dot);
  }
  __syncthreads();
  if (d_bias)
    for (int t = threadIdx.x; t < n; t += MN_THREADS) {
      float acc = 0.f;
      for (int k = 0; k < K; ++k) acc += sL[k * Hs + t];
      d_bias[r0 + t] = acc;
    }
  for (int idx = threadIdx.x; idx < n * D4; idx += MN_THREADS) {
    const int t = idx / D4, d4 = idx - t * D4;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int k = 0; k < K; ++k) mn_fma4(acc, sA[k * Hs + t], ld4(du + (int64_t)k * D + 4 * d4));
    st4(d_E + (r0 + t) * D + 4 * d4, acc);
  }
  for (int idx = threadIdx.x; idx < n * C4; idx += MN_THREADS) {
    const int t = idx / C4, c4 = idx - t * C4;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int k = 0; k < K; ++k) mn_fma4(acc, sL[k * Hs + t], ld4(codes + (int64_t)k * Cd + 4 * c4));
    st4(d_P + (r0 + t) * Cd + 4 * c4, acc);
  }
  for (int idx = threadIdx.x; idx < K * C4; idx += MN_THREADS) {
    const int k = idx / C4, c4 = idx - k * C4;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int t = 0; t < n; ++t) mn_fma4(acc, sL[k * Hs + t], ld4(P + (r0 + t) * Cd + 4 * c4));
    st4(slab + ((int64_t)b * K + k) * Cd + 4 * c4, acc);
  }
}

// ---- scores ----------------------------------------------------------------------------------------------------------------
// mode 0 max, 1 mean, 2 weighted.  One workgroup per user; LDS: sC[waves][D] one candidate row per wave, sU[K][D + 1] the
// user's interest vectors, sG[K][D + 1] gelu(Z) (weighted only).  Lane k (and k + 64, ...: K <= 255) owns context code k.
// Saved per flat candidate row for the backward: Ssave (n_cand, K) matching scores, Wsave (n_cand, K) softmax weights
// (weighted), arg (n_cand) the index of the maximum (max).  scores (B, Cmax): 0 at the padded slots.
__global__ __launch_bounds__(MN_THREADS) void miner_score_fwd_kernel(
    const float* __restrict__ cand, const float* __restrict__ uv, const float* __restrict__ Z,
    const int64_t* __restrict__ cand_off, int Cmax, int D, int K, int mode, float* __restrict__ scores,
    float* __restrict__ Gsave, float* __restrict__ Ssave, float* __restrict__ Wsave, uint8_t* __restrict__ arg) {
  extern __shared__ float4 mn_smem4[];
  const int Ds = D + 1;
  float* sC = reinterpret_cast<float*>(mn_smem4);
  float* sU = sC + MN_WAVES * D;
  float* sG = sU + (size_t)K * Ds;
  const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, D4 = D >> 2;
  const int64_t c0 = cand_off[b];
  const int nc = min((int)(cand_off[b + 1] - c0), Cmax);
  for (int idx = threadIdx.x; idx < K * D; idx += MN_THREADS) {
    const int k = idx / D, d = idx - k * D;
    sU[k * Ds + d] = uv[(int64_t)b * K * D + idx];
    if (mode == 2) {
      const float g = mn_gelu(Z[(int64_t)b * K * D + idx]);
      sG[k * Ds + d] = g;
      if (Gsave) Gsave[(int64_t)b * K * D + idx] = g;
    }
  }
  for (int j = nc + threadIdx.x; j < Cmax; j += MN_THREADS) scores[(int64_t)b * Cmax + j] = 0.f;
  float* myC = sC + wave * D;
  for (int j0 = 0; j0 < nc; j0 += MN_WAVES) {                       // (uniform trip count: the barriers are safe)
    const int j = j0 + wave;
    __syncthreads();
    if (j < nc)
      for (int d4 = lane; d4 < D4; d4 += 64) st4(myC + 4 * d4, ld4(cand + (c0 + j) * D + 4 * d4));
    __syncthreads();
    if (j >= nc) continue;
    float s[4] = {0.f, 0.f, 0.f, 0.f}, t[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int k = lane + 64 * i;
      if (k < K) {
        float as = 0.f, at = 0.f;
        for (int d = 0; d < D; ++d) {
          const float c = myC[d];
          as += c * sU[k * Ds + d];
          if (mode == 2) at += c * sG[k * Ds + d];
        }
        s[i] = as;
        t[i] = at;
        if (Ssave && mode == 2) Ssave[(c0 + j) * K + k] = as;
      }
    }
    float out;
    if (mode == 2) {
      float m = -INFINITY;
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (lane + 64 * i < K) m = fmaxf(m, t[i]);
      m = wave_max(m);
      float e[4], den = 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        e[i] = lane + 64 * i < K ? expf(t[i] - m) : 0.f;
        den += e[i];
      }
      den = wave_sum(den);
      float acc = 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (lane + 64 * i < K) {
          const float w = e[i] / den;
          acc += w * s[i];
          if (Wsave) Wsave[(c0 + j) * K + lane + 64 * i] = w;
        }
      out = wave_sum(acc);
    } else if (mode == 1) {
      float acc = 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (lane + 64 * i < K) acc += s[i];
      out = wave_sum(acc) / (float)K;
    } else {
      float best = -INFINITY;
      int bi = 0x7fffffff;
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (lane + 64 * i < K && s[i] > best) {                    // ascending k, strict: the lowest index of a tie
          best = s[i];
          bi = lane + 64 * i;
        }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_xor(best, off, 64);
        const int oi = __shfl_xor(bi, off, 64);
        if (ov > best || (ov == best && oi < bi)) {
          best = ov;
          bi = oi;
        }
      }
      out = best;
      if (arg && lane == 0) arg[c0 + j] = (uint8_t)bi;
    }
    if (lane == 0) scores[(int64_t)b * Cmax + j] = out;
  }
}

// LDS: sdS[CT][K], sdT[CT][K] of one tile of candidates.  d_uv / d_Z (B, K, D): every element has ONE owner thread, which
// adds the tiles in order (first tile: from 0) and, for d_Z, applies gelu'(Z) after the last.
__global__ __launch_bounds__(MN_THREADS) void miner_score_bwd_kernel(
    const float* __restrict__ d_scores, const float* __restrict__ scores, const float* __restrict__ cand,
    const float* __restrict__ uv, const float* __restrict__ Z, const float* __restrict__ G, const float* __restrict__ Ssave,
    const float* __restrict__ Wsave, const uint8_t* __restrict__ arg, const int64_t* __restrict__ cand_off, int Cmax, int D,
    int K, int mode, float* __restrict__ d_cand, float* d_uv, float* d_Z) {
  extern __shared__ float4 mn_smem4[];
  float* sdS = reinterpret_cast<float*>(mn_smem4);
  float* sdT = sdS + MN_CT * K;
  const int b = blockIdx.x, D4 = D >> 2;
  const int64_t c0 = cand_off[b];
  const int nc = min((int)(cand_off[b + 1] - c0), Cmax);
  const float* ub = uv + (int64_t)b * K * D;
  const float* gb = mode == 2 ? G + (int64_t)b * K * D : nullptr;
  float* dub = d_uv + (int64_t)b * K * D;
  float* dzb = mode == 2 ? d_Z + (int64_t)b * K * D : nullptr;
  const int tiles = nc > 0 ? (nc + MN_CT - 1) / MN_CT : 1;
  for (int tile = 0; tile < tiles; ++tile) {
    const int j0 = tile * MN_CT;
    const int ct = max(min(MN_CT, nc - j0), 0);
    __syncthreads();
    for (int idx = threadIdx.x; idx < ct * K; idx += MN_THREADS) {
      const int j = idx / K, k = idx - j * K;
      const int64_t c = c0 + j0 + j;
      const float ds = d_scores[(int64_t)b * Cmax + j0 + j];
      float dS, dT = 0.f;
      if (mode == 2) {
        const float w = Wsave[c * K + k];
        dS = ds * w;
        dT = w * ds * (Ssave[c * K + k] - scores[(int64_t)b * Cmax + j0 + j]);
      } else if (mode == 1) {
        dS = ds / (float)K;
      } else {
        dS = k == (int)arg[c] ? ds : 0.f;
      }
      sdS[idx] = dS;
      sdT[idx] = dT;
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < ct * D4; idx += MN_THREADS) {
      const int j = idx / D4, d4 = idx - j * D4;
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int k = 0; k < K; ++k) {
        mn_fma4(acc, sdS[j * K + k], ld4(ub + (int64_t)k * D + 4 * d4));
        if (mode == 2) mn_fma4(acc, sdT[j * K + k], ld4(gb + (int64_t)k * D + 4 * d4));
      }
      st4(d_cand + (c0 + j0 + j) * D + 4 * d4, acc);
    }
    const bool last = tile == tiles - 1;
    for (int idx = threadIdx.x; idx < K * D4; idx += MN_THREADS) {
      const int k = idx / D4, d4 = idx - k * D4;
      float4 au = make_float4(0.f, 0.f, 0.f, 0.f), az = au;
      if (tile > 0) {
        au = ld4(dub + (int64_t)k * D + 4 * d4);
        if (mode == 2) az = ld4(dzb + (int64_t)k * D + 4 * d4);
      }
      for (int j = 0; j < ct; ++j) {
        const float4 c = ld4(cand + (c0 + j0 + j) * D + 4 * d4);
        mn_fma4(au, sdS[j * K + k], c);
        if (mode == 2) mn_fma4(az, sdT[j * K + k], c);
      }
      st4(dub + (int64_t)k * D + 4 * d4, au);
      if (mode == 2) {
        if (last) {
          const float4 z = ld4(Z + ((int64_t)b * K + k) * D + 4 * d4);
          az.x *= mn_gelu_grad(z.x);
          az.y *= mn_gelu_grad(z.y);
          az.z *= mn_gelu_grad(z.z);
          az.w *= mn_gelu_grad(z.w);
        }
        st4(dzb + (int64_t)k * D + 4 * d4, az);
      }
    }
  }
}

}  // namespace nrl

using namespace nrl;

extern "C" {

int nrl_miner_slab_sum(const float* slabs, int64_t num_slabs, int64_t n, float scale, float* out, void* stream) {
  NRL_REQUIRE(slabs && out && num_slabs >= 0 && n > 0, "nrl_miner_slab_sum: bad arguments");
  return mn_slab_sum(slabs, num_slabs, n, scale, out, (hipStream_t)stream);
}

int nrl_miner_cos_fwd(const float* x, int64_t groups, int32_t R, int32_t D, float eps, float* partial, void* stream) {
  NRL_REQUIRE(x && partial && groups > 0 && R > 0 && D > 0 && D % 4 == 0, "nrl_miner_cos_fwd: bad shape (D %% 4 == 0)");
  const size_t lds = (size_t)(D + R) * sizeof(float);
  static bool raised = false;
  NRL_TRY(mn_set_lds(reinterpret_cast<const void*>(&miner_cos_fwd_kernel), lds, "nrl_miner_cos_fwd", &raised));
  miner_cos_fwd_kernel<<<(unsigned)groups, MN_THREADS, lds, (hipStream_t)stream>>>(x, R, D, eps, partial);
  NRL_LAUNCH_CHECK();
  return NRL_OK;
}

int nrl_miner_cos_bwd(const float* x, int64_t groups, int32_t R, int32_t D, float eps, const float* d_loss, float scale,
                      float* d_x, void* stream) {
  NRL_REQUIRE(x && d_loss && d_x && groups > 0 && R > 0 && D > 0 && D % 4 == 0, "nrl_miner_cos_bwd: bad shape");
  const size_t lds = (size_t)(D + R) * sizeof(float);
  static bool raised = false;
  NRL_TRY(mn_set_lds(reinterpret_cast<const void*>(&miner_cos_bwd_kernel), lds, "nrl_miner_cos_bwd", &raised));
  miner_cos_bwd_kernel<<<(unsigned)groups, MN_THREADS, lds, (hipStream_t)stream>>>(x, R, D, eps, d_loss, scale, d_x);
  NRL_LAUNCH_CHECK();
  return NRL_OK;
}

int nrl_miner_tanh_grad(const float* d_c, const float* c, int64_t n, float* d_pre, void* stream) {
  NRL_REQUIRE(d_c && c && d_pre && n > 0 && n % 4 == 0, "nrl_miner_tanh_grad: bad arguments (n %% 4 == 0)");
  const int64_t n4 = n / 4, g = ceil_div(n4, MN_THREADS);
  miner_tanh_grad_kernel<<<(unsigned)(g > 4096 ? 4096 : g), MN_THREADS, 0, (hipStream_t)stream>>>(
      (const float4*)d_c, (const float4*)c, n4, (float4*)d_pre);
  NRL_LAUNCH_CHECK();
  return NRL_OK;
}

size_t nrl_miner_wgrad_workspace_bytes(int64_t R, int32_t N, int32_t K) {
  const int64_t chunks = ceil_div(R > 0 ? R : 1, MN_WG_ROWS);
  return measure_workspace<float*>([&](Arena& a, auto* w) { mn_slabs_layout(a, chunks, (int64_t)N * K, w); });
}

int nrl_miner_wgrad(const float* G, const float* X, int64_t R, int32_t N, int32_t K, float* d_w, void* ws, size_t ws_bytes,
                    void* stream) {
  NRL_REQUIRE(G && X && d_w && R > 0 && N > 0 && K > 0 && K % 4 == 0, "nrl_miner_wgrad: bad arguments (K %% 4 == 0)");
  const int64_t chunks = ceil_div(R, MN_WG_ROWS);
  float* slabs;
  NRL_TRY(carve_workspace(ws, ws_bytes, [&](Arena& a) { mn_slabs_layout(a, chunks, (int64_t)N * K, &slabs); }));
  hipStream_t st = (hipStream_t)stream;
  miner_wgrad_kernel<<<dim3((unsigned)chunks, (unsigned)ceil_div(N, MN_WG_TN)), MN_THREADS, 0, st>>>(G, X, R, N, K, slabs);
  NRL_LAUNCH_CHECK();
  return mn_slab_sum(slabs, chunks, (int64_t)N * K, 1.f, d_w, st);
}

size_t nrl_miner_categ_bias_workspace_bytes(int64_t B, int64_t n_hist, int64_t n_cand, int32_t Dc) {
  return measure_workspace<CbWs>([&](Arena& a, auto* w) { cb_layout(a, B, n_hist, n_cand, Dc, w); });
}

int nrl_miner_categ_bias_fwd(const float* hc, const float* cc, const int64_t* batch_hist, const int64_t* cand_off, int64_t B,
                             int64_t n_hist, int64_t n_cand, int32_t Dc, float* bias, void* ws, size_t ws_bytes,
                             void* stream) {
  NRL_REQUIRE(hc && cc && batch_hist && cand_off && bias, "nrl_miner_categ_bias_fwd: null argument");
  NRL_REQUIRE(B > 0 && n_hist > 0 && n_cand > 0 && Dc > 0 && Dc % 4 == 0, "nrl_miner_categ_bias_fwd: bad shape (Dc %% 4 == 0)");
  CbWs w;
  NRL_TRY(carve_workspace(ws, ws_bytes, [&](Arena& a) { cb_layout(a, B, n_hist, n_cand, Dc, &w); }));
  hipStream_t st = (hipStream_t)stream;
  miner_cb_cand_kernel<<<(unsigned)B, MN_THREADS, 0, st>>>(cc, cand_off, Dc, w.rn_c, w.s_own);
  NRL_LAUNCH_CHECK();
  NRL_TRY(mn_slab_sum(w.s_own, B, Dc, 1.f, w.s_all, st));
  miner_cb_hist_kernel<<<(unsigned)ceil_div(n_hist, MN_WAVES), MN_THREADS, 0, st>>>(hc, batch_hist, n_hist, Dc,
                                                                                    1.f / (float)n_cand, w.s_own, w.s_all,
                                                                                    w.rn_h, bias);
  NRL_LAUNCH_CHECK();
  return NRL_OK;
}

int nrl_miner_categ_bias_bwd(const float* d_bias, const float* hc, const float* cc, const int64_t* hist_off,
                             const int64_t* batch_cand, const float* bias, int64_t B, int64_t n_hist, int64_t n_cand,
                             int32_t Dc, float* d_hc, float* d_cc, void* ws, size_t ws_bytes, void* stream) {
  NRL_REQUIRE(d_bias && hc && cc && hist_off && batch_cand && bias && d_hc && d_cc, "nrl_miner_categ_bias_bwd: null argument");
  NRL_REQUIRE(B > 0 && n_hist > 0 && n_cand > 0 && Dc > 0 && Dc % 4 == 0, "nrl_miner_categ_bias_bwd: bad shape");
  CbWs w;
  NRL_TRY(carve_workspace(ws, ws_bytes, [&](Arena& a) { cb_layout(a, B, n_hist, n_cand, Dc, &w); }));
  hipStream_t st = (hipStream_t)stream;
  miner_cb_bwd_hist_kernel<<<(unsigned)B, MN_THREADS, 0, st>>>(d_bias, hc, hist_off, Dc, 1.f / (float)n_cand, bias, w.rn_h,
                                                              w.s_own, w.s_all, w.q_own, d_hc);
  NRL_LAUNCH_CHECK();
  NRL_TRY(mn_slab_sum(w.q_own, B, Dc, 1.f, w.q_all, st));
  miner_cb_bwd_cand_kernel<<<(unsigned)ceil_div(n_cand, MN_WAVES), MN_THREADS, 0, st>>>(cc, batch_cand, n_cand, Dc, w.rn_c,
                                                                                        w.q_own, w.q_all, d_cc);
  NRL_LAUNCH_CHECK();
  return NRL_OK;
}

size_t nrl_miner_poly_workspace_bytes(int64_t B, int32_t K, int32_t Cd) {
  return measure_workspace<float*>([&](Arena& a, auto* w) { mn_slabs_layout(a, B, (int64_t)K * Cd, w); });
}

int nrl_miner_poly_fwd(const float* E, const float* P, const float* codes, const float* bias, const int64_t* hist_off,
                       int64_t B, int32_t max_hist, int32_t D, int32_t Cd, int32_t K, float* user_vector, float* A,
                       void* stream) {
  NRL_REQUIRE(E && P && codes && hist_off && user_vector && A, "nrl_miner_poly_fwd: null argument");
  NRL_REQUIRE(B > 0 && max_hist > 0 && K > 0 && D > 0 && Cd > 0 && D % 4 == 0 && Cd % 4 == 0,
              "nrl_miner_poly_fwd: bad shape (D, context_code_dim: multiples of 4)");
  const size_t lds_a = (size_t)K * max_hist * sizeof(float), lds_e = (size_t)max_hist * D * sizeof(float);
  const int tile = lds_a + lds_e <= MN_LDS_MAX ? 1 : 0;            // else the tile is read through the caches
  const size_t lds = lds_a + (tile ? lds_e : 0);
  static bool raised = false;
  NRL_TRY(mn_set_lds(reinterpret_cast<const void*>(&miner_poly_fwd_kernel), lds, "nrl_miner_poly_fwd", &raised));
  miner_poly_fwd_kernel<<<(unsigned)B, MN_THREADS, lds, (hipStream_t)stream>>>(E, P, codes, bias, hist_off, max_hist, D, Cd, K,
                                                                             tile, user_vector, A);
  NRL_LAUNCH_CHECK();
  return NRL_OK;
}

int nrl_miner_poly_bwd(const float* d_user_vector, const float* E, const float* P, const float* codes, const float* A,
                       const int64_t* hist_off, int64_t B, int32_t max_hist, int32_t D, int32_t Cd, int32_t K, float* d_E,
                       float* d_P, float* d_codes, float* d_bias, void* ws, size_t ws_bytes, void* stream) {
  NRL_REQUIRE(d_user_vector && E && P && codes && A && hist_off && d_E && d_P && d_codes,
              "nrl_miner_poly_bwd: null argument");
  NRL_REQUIRE(B > 0 && max_hist > 0 && K > 0 && D > 0 && Cd > 0 && D % 4 == 0 && Cd % 4 == 0, "nrl_miner_poly_bwd: bad shape");
  float* slabs;
  NRL_TRY(carve_workspace(ws, ws_bytes, [&](Arena& a) { mn_slabs_layout(a, B, (int64_t)K * Cd, &slabs); }));
  const size_t lds = 2 * (size_t)K * max_hist * sizeof(float);
  static bool raised = false;
  NRL_TRY(mn_set_lds(reinterpret_cast<const void*>(&miner_poly_bwd_kernel), lds, "nrl_miner_poly_bwd", &raised));
  hipStream_t st = (hipStream_t)stream;
  miner_poly_bwd_kernel<<<(unsigned)B, MN_THREADS, lds, st>>>(d_user_vector, E, P, codes, A, hist_off, max_hist, D, Cd, K, d_E,
                                                            d_P, d_bias, slabs);
  NRL_LAUNCH_CHECK();
  return mn_slab_sum(slabs, B, (int64_t)K * Cd, 1.f, d_codes, st);
}

int nrl_miner_score_fwd(const float* cand, const float* user_vector, const float* Z, const int64_t* cand_off, int64_t B,
                        int32_t max_cand, int32_t D, int32_t K, int32_t mode, float* scores, float* G, float* S, float* W,
                        uint8_t* argmax, void* stream) {
  NRL_REQUIRE(cand && user_vector && cand_off && scores, "nrl_miner_score_fwd: null argument");
  NRL_REQUIRE(mode >= 0 && mode <= 2 && (mode != 2 || Z), "nrl_miner_score_fwd: mode 0 max / 1 mean / 2 weighted (needs Z)");
  NRL_REQUIRE(B > 0 && max_cand > 0 && D > 0 && D % 4 == 0 && K > 0 && K <= 255,
              "nrl_miner_score_fwd: bad shape (D %% 4 == 0, at most 255 context codes)");
  const size_t lds = ((size_t)(mode == 2 ? 2 : 1) * K * (D + 1) + (size_t)MN_WAVES * D) * sizeof(float);
  static bool raised = false;
  NRL_TRY(mn_set_lds(reinterpret_cast<const void*>(&miner_score_fwd_kernel), lds, "nrl_miner_score_fwd", &raised));
  miner_score_fwd_kernel<<<(unsigned)B, MN_THREADS, lds, (hipStream_t)stream>>>(cand, user_vector, Z, cand_off, max_cand, D, K,
                                                                              mode, scores, G, S, W, argmax);
  NRL_LAUNCH_CHECK();
  return NRL_OK;
}

int nrl_miner_score_bwd(const float* d_scores, const float* scores, const float* cand, const float* user_vector,
                        const float* Z, const float* G, const float* S, const float* W, const uint8_t* argmax,
                        const int64_t* cand_off, int64_t B, int32_t max_cand, int32_t D, int32_t K, int32_t mode,
                        float* d_cand, float* d_user_vector, float* d_Z, void* stream) {
  NRL_REQUIRE(d_scores && scores && cand && user_vector && cand_off && d_cand && d_user_vector,
              "nrl_miner_score_bwd: null argument");
  NRL_REQUIRE(mode >= 0 && mode <= 2, "nrl_miner_score_bwd: bad mode");
  NRL_REQUIRE(mode != 2 || (Z && G && S && W && d_Z), "nrl_miner_score_bwd: the weighted mode needs Z, G, S, W, d_Z");
  NRL_REQUIRE(mode != 0 || argmax, "nrl_miner_score_bwd: the max mode needs the saved argmax");
  NRL_REQUIRE(B > 0 && max_cand > 0 && D > 0 && D % 4 == 0 && K > 0 && K <= 255, "nrl_miner_score_bwd: bad shape");
  const size_t lds = 2 * (size_t)MN_CT * K * sizeof(float);
  static bool raised = false;
  NRL_TRY(mn_set_lds(reinterpret_cast<const void*>(&miner_score_bwd_kernel), lds, "nrl_miner_score_bwd", &raised));
  miner_score_bwd_kernel<<<(unsigned)B, MN_THREADS, lds, (hipStream_t)stream>>>(d_scores, scores, cand, user_vector, Z, G, S, W,
                                                                              argmax, cand_off, max_cand, D, K, mode, d_cand,
                                                                              d_user_vector, d_Z);
  NRL_LAUNCH_CHECK();
  return NRL_OK;
}

}  // extern "C"

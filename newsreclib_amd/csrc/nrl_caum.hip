// CAUM (caum_module.py:326-360, user/caum.py:81-125): the candidate-aware user encoder's non-GEMM stages, every candidate
// slot in one pass, plus the head-padded self-attention of the news encoder.  Plain fp32 vector code under both engines;
// the projections run on the GEMM engines through ops_blocks.LinearFn / LinearActFn.
//   nrl_caum_attn_*            attention over a packed q|k|v buffer at any built head dim, seq-first or batch-first
//   nrl_caum_dropout           y = x * mask (the library's counter-based mask; the backward is the same call)
//   nrl_caum_expand_*          per-slot dropout1 / dropout2 of the candidate and of the dense history
//   nrl_caum_combine_*         candi-CNN (circular neighbours) and linear2 from their history / candidate / bias parts
//   nrl_caum_concat_dropout_*  dropout3([cnn, self])
//   nrl_caum_group_tanh_*      tanh(history part + candidate part) of DenseAttention's first layer
//   nrl_caum_score_*           DenseAttention's last layer, softmax over max_hist, weighted sum, score, padded-slot zero
// Dropout streams of slot i (relative to stream_base): 3i -> dropout1 over (B, D), 3i + 1 -> dropout2 over (B, H, D),
// 3i + 2 -> dropout3 over (B, H, F + U); flat row-major indices over those shapes (tests/caum_oracle.py restates them).
// No float atomics: every reduction runs in a fixed order.
#include <math.h>

#include "nrl_kernels.h"

namespace nrl {

constexpr int CAUM_THREADS = 256;

struct SlotDrop {
  uint64_t seed;
  uint32_t stream_base;
  uint32_t thresh;
  float scale;
  __device__ __forceinline__ uint32_t key(uint32_t stream) const { return dropout_key(seed, stream); }
  __device__ __forceinline__ float mult(uint32_t k, uint32_t flat_idx) const {
    return lowbias32(flat_idx * 0x9E3779B1u + k) >= thresh ? scale : 0.0f;
  }
};

static SlotDrop make_slot_drop(double p, uint64_t seed, uint32_t stream_base) {
  const Dropout d = make_dropout(p, seed, 0);
  SlotDrop s;
  s.seed = seed;
  s.stream_base = stream_base;
  s.thresh = d.thresh;
  s.scale = d.scale;
  return s;
}

static unsigned grid_for(int64_t n) {
  const int64_t g = ceil_div(n, CAUM_THREADS);
  return (unsigned)(g < 65536 ? (g > 0 ? g : 1) : 65536);
}

// ---- y = x * mask ------------------------------------------------------------------------------------------------------
__global__ void caum_dropout_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t n, Dropout d) {
  for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x)
    y[k] = x[k] * d.mult((uint32_t)k);
}

// ---- per-slot dropout of the candidate (dropout1) and of the history (dropout2) ---------------------------------------
// hd (B, C, H, D) = h (B, H, D) * mask(3i + 1); cd (B, C, D) = c (B, C, D) * mask(3i)
__global__ void caum_expand_fwd_kernel(const float* __restrict__ h, const float* __restrict__ c, int B, int C, int H, int D,
                                       SlotDrop sd, float* __restrict__ hd, float* __restrict__ cd) {
  const int64_t nh = (int64_t)B * C * H * D, nc = (int64_t)B * C * D;
  for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < nh + nc; k += (int64_t)gridDim.x * blockDim.x) {
    if (k < nh) {
      const int d = (int)(k % D);
      const int64_t r = k / D;
      const int t = (int)(r % H);
      const int i = (int)((r / H) % C);
      const int64_t b = r / ((int64_t)H * C);
      const int64_t src = (b * H + t) * D + d;
      hd[k] = h[src] * sd.mult(sd.key(sd.stream_base + 3u * i + 1u), (uint32_t)src);
    } else {
      const int64_t q = k - nh;
      const int d = (int)(q % D);
      const int i = (int)((q / D) % C);
      const int64_t b = q / ((int64_t)D * C);
      cd[q] = c[q] * sd.mult(sd.key(sd.stream_base + 3u * i), (uint32_t)(b * D + d));
    }
  }
}

// d_h[b, t] = sum over slots i (in order) of d_hd[b, i, t] * mask_i; d_c = d_cd * mask
__global__ void caum_expand_bwd_kernel(const float* __restrict__ d_hd, const float* __restrict__ d_cd, int B, int C, int H,
                                       int D, SlotDrop sd, float* __restrict__ d_h, float* __restrict__ d_c) {
  const int64_t nh = (int64_t)B * H * D, nc = (int64_t)B * C * D;
  for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < nh + nc; k += (int64_t)gridDim.x * blockDim.x) {
    if (k < nh) {
      const int d = (int)(k % D);
      const int t = (int)((k / D) % H);
      const int64_t b = k / ((int64_t)D * H);
      float acc = 0.f;
      for (int i = 0; i < C; ++i)
        acc += d_hd[((b * C + i) * H + t) * D + d] * sd.mult(sd.key(sd.stream_base + 3u * i + 1u), (uint32_t)k);
      d_h[k] = acc;
    } else {
      const int64_t q = k - nh;
      const int d = (int)(q % D);
      const int i = (int)((q / D) % C);
      const int64_t b = q / ((int64_t)D * C);
      d_c[q] = d_cd[q] * sd.mult(sd.key(sd.stream_base + 3u * i), (uint32_t)(b * D + d));
    }
  }
}

// ---- candi-CNN + linear2 from their parts --------------------------------------------------------------------------------
// P rows (b, i', t), width 3F + U: [W1a h | W1b h | W1c h | W2b h] (+ b1 in the first block, b2 in the last); i' = i when the
// history is per slot (hs == C), 0 when it is shared (hs == 1, evaluation).  Q rows (b, i), width F + U: [W1d c | W2a c].
//   cnn[b, i, t] = P[b, i', t-1 (circular), 0:F] + P[b, i', t, F:2F] + P[b, i', t+1 (circular), 2F:3F] + Q[b, i, 0:F]
//   s  [b, i, t] = P[b, i', t, 3F:]                                                                      + Q[b, i, F:]
__global__ void caum_combine_fwd_kernel(const float* __restrict__ P, const float* __restrict__ Q, int B, int C, int H,
                                        int F, int U, int hs, float* __restrict__ cnn, float* __restrict__ s) {
  const int W = 3 * F + U;
  const int64_t R = (int64_t)B * C * H;
  const int64_t n = R * (F + U);
  for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x) {
    const int j = (int)(k % (F + U));
    const int64_t r = k / (F + U);
    const int t = (int)(r % H);
    const int i = (int)((r / H) % C);
    const int64_t b = r / ((int64_t)H * C);
    const int64_t prow = (b * hs + (hs == 1 ? 0 : i)) * H;
    const float* q = Q + (b * C + i) * (int64_t)(F + U);
    if (j < F) {
      const int tl = t == 0 ? H - 1 : t - 1, tr = t == H - 1 ? 0 : t + 1;
      cnn[r * F + j] = P[(prow + tl) * W + j] + P[(prow + t) * W + F + j] + P[(prow + tr) * W + 2 * F + j] + q[j];
    } else {
      const int u = j - F;
      s[r * U + u] = P[(prow + t) * W + 3 * F + u] + q[F + u];
    }
  }
}

// d_P (B * hs * H, 3F + U) written; every slot mapped onto a P row adds in slot order
__global__ void caum_combine_bwd_p_kernel(const float* __restrict__ d_cnn, const float* __restrict__ d_s, int B, int C, int H,
                                          int F, int U, int hs, float* __restrict__ d_P) {
  const int W = 3 * F + U;
  const int64_t n = (int64_t)B * hs * H * W;
  for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x) {
    const int j = (int)(k % W);
    const int64_t pr = k / W;
    const int t = (int)(pr % H);
    const int ip = (int)((pr / H) % hs);
    const int64_t b = pr / ((int64_t)H * hs);
    const int i0 = hs == 1 ? 0 : ip, i1 = hs == 1 ? C : ip + 1;
    float acc = 0.f;
    for (int i = i0; i < i1; ++i) {
      const int64_t base = (b * C + i) * H;
      if (j < F) {                                       // left-neighbour block: feeds the row to its right
        const int tt = t == H - 1 ? 0 : t + 1;
        acc += d_cnn[(base + tt) * F + j];
      } else if (j < 2 * F) {
        acc += d_cnn[(base + t) * F + (j - F)];
      } else if (j < 3 * F) {                            // right-neighbour block: feeds the row to its left
        const int tt = t == 0 ? H - 1 : t - 1;
        acc += d_cnn[(base + tt) * F + (j - 2 * F)];
      } else {
        acc += d_s[(base + t) * U + (j - 3 * F)];
      }
    }
    d_P[k] = acc;
  }
}

// d_Q (B * C, F + U) written: sums over t in order
__global__ void caum_combine_bwd_q_kernel(const float* __restrict__ d_cnn, const float* __restrict__ d_s, int B, int C, int H,
                                          int F, int U, float* __restrict__ d_Q) {
  const int64_t n = (int64_t)B * C * (F + U);
  for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x) {
    const int j = (int)(k % (F + U));
    const int64_t g = k / (F + U);
    float acc = 0.f;
    if (j < F) {
      for (int t = 0; t < H; ++t) acc += d_cnn[(g * H + t) * F + j];
    } else {
      for (int t = 0; t < H; ++t) acc += d_s[(g * H + t) * U + (j - F)];
    }
    d_Q[k] = acc;
  }
}

// ---- dropout3([cnn, self]) -----------------------------------------------------------------------------------------------
// rows r = (b, i, t); element j of the (F + U)-wide concatenation takes mask(3i + 2) at ((b * H + t) * (F + U) + j).
// Forward: z = mask * [x0, x1].  Backward (the same mask): [y0, y1] = mask * z.
__global__ void caum_concat_dropout_kernel(const float* __restrict__ x0, const float* __restrict__ x1, int B, int C, int H,
                                           int F, int U, SlotDrop sd, int backward, float* __restrict__ y0,
                                           float* __restrict__ y1, float* __restrict__ z) {
  const int W = F + U;
  const int64_t n = (int64_t)B * C * H * W;
  for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x) {
    const int j = (int)(k % W);
    const int64_t r = k / W;
    const int t = (int)(r % H);
    const int i = (int)((r / H) % C);
    const int64_t b = r / ((int64_t)H * C);
    const float m = sd.mult(sd.key(sd.stream_base + 3u * i + 2u), (uint32_t)((b * H + t) * W + j));
    if (!backward) {
      z[k] = (j < F ? x0[r * F + j] : x1[r * U + (j - F)]) * m;
    } else if (j < F) {
      y0[r * F + j] = z[k] * m;
    } else {
      y1[r * U + (j - F)] = z[k] * m;
    }
  }
}

// ---- tanh(a1 + g[row / H]) -----------------------------------------------------------------------------------------------
__global__ void caum_group_tanh_fwd_kernel(const float* __restrict__ a, const float* __restrict__ g, int64_t R, int N, int H,
                                           float* __restrict__ z) {
  const int64_t n = R * N;
  for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x) {
    const int j = (int)(k % N);
    const int64_t r = k / N;
    z[k] = tanhf(a[k] + g[(r / H) * N + j]);
  }
}

__global__ void caum_group_tanh_bwd_kernel(const float* __restrict__ d_z, const float* __restrict__ z, int64_t G, int N, int H,
                                           float* __restrict__ d_a, float* __restrict__ d_g) {
  const int64_t n = G * N;
  for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x) {
    const int j = (int)(k % N);
    const int64_t g = k / N;
    float acc = 0.f;
    for (int t = 0; t < H; ++t) {
      const int64_t e = (g * H + t) * N + j;
      const float v = d_z[e] * (1.f - z[e] * z[e]);
      d_a[e] = v;
      acc += v;
    }
    d_g[k] = acc;
  }
}

// ---- DenseAttention layer 3 + softmax over max_hist + weighted sum + score, one workgroup per (b, i) ----------------------
// slot i of the call is candidate slot slot0 + i of the impression (evaluation runs the slots in chunks)
__global__ __launch_bounds__(CAUM_THREADS) void caum_score_fwd_kernel(
    const float* __restrict__ z2, const float* __restrict__ w3, const float* __restrict__ b3, const float* __restrict__ x,
    const float* __restrict__ cd, const int64_t* __restrict__ cand_offsets, int C, int slot0, int H, int N2, int U,
    float* __restrict__ scores, float* __restrict__ alpha, float* __restrict__ user) {
  extern __shared__ float sm[];           // logits, then weights [H] | red[4]
  float* lg = sm;
  float* red = sm + H;
  const int64_t g = blockIdx.x;
  const int64_t b = g / C;
  const int i = (int)(g % C);
  const bool valid = (int64_t)(slot0 + i) < cand_offsets[b + 1] - cand_offsets[b];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int t = wave; t < H; t += CAUM_THREADS / 64) {
    const float* row = z2 + (g * H + t) * (int64_t)N2;
    float part = 0.f;
    for (int j = lane; j < N2; j += 64) part += row[j] * w3[j];
    part = wave_sum(part);
    if (lane == 0) lg[t] = part + b3[0];
  }
  __syncthreads();
  float m = -INFINITY;
  for (int t = 0; t < H; ++t) m = fmaxf(m, lg[t]);
  float l = 0.f;
  for (int t = 0; t < H; ++t) l += __expf(lg[t] - m);
  const float inv = 1.f / l;
  __syncthreads();                        // every thread has read the logits before they are overwritten
  for (int t = threadIdx.x; t < H; t += CAUM_THREADS) {
    const float a = __expf(lg[t] - m) * inv;
    lg[t] = a;
    alpha[g * H + t] = a;
  }
  __syncthreads();
  float part = 0.f;
  for (int u = threadIdx.x; u < U; u += CAUM_THREADS) {
    float acc = 0.f;
    for (int t = 0; t < H; ++t) acc += lg[t] * x[(g * H + t) * (int64_t)U + u];
    user[g * U + u] = acc;
    part += acc * cd[g * U + u];
  }
  const float s = block_sum<CAUM_THREADS / 64>(part, red);
  if (threadIdx.x == 0) scores[g] = valid ? s : 0.f;
}

// d_z2 (R, N2), d_x (R, U), d_cd (G, U) and d_logit (R) written.  A padded slot takes no score gradient.
__global__ __launch_bounds__(CAUM_THREADS) void caum_score_bwd_kernel(
    const float* __restrict__ d_scores, const float* __restrict__ w3, const float* __restrict__ x,
    const float* __restrict__ cd, const float* __restrict__ alpha, const float* __restrict__ user,
    const int64_t* __restrict__ cand_offsets, int C, int slot0, int H, int N2, int U, float* __restrict__ d_z2,
    float* __restrict__ d_x, float* __restrict__ d_cd, float* __restrict__ d_logit) {
  extern __shared__ float sm[];           // d_alpha[H]
  float* da = sm;
  const int64_t g = blockIdx.x;
  const int64_t b = g / C;
  const int i = (int)(g % C);
  const bool valid = (int64_t)(slot0 + i) < cand_offsets[b + 1] - cand_offsets[b];
  const float ds = valid ? d_scores[g] : 0.f;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int u = threadIdx.x; u < U; u += CAUM_THREADS) d_cd[g * U + u] = ds * user[g * U + u];
  for (int t = wave; t < H; t += CAUM_THREADS / 64) {       // d_alpha_t = d_user . x_t,  d_user = ds * c
    const float* row = x + (g * H + t) * (int64_t)U;
    float part = 0.f;
    for (int u = lane; u < U; u += 64) part += row[u] * cd[g * U + u];
    part = wave_sum(part);
    if (lane == 0) da[t] = ds * part;
  }
  __syncthreads();
  float dot = 0.f;
  for (int t = 0; t < H; ++t) dot += alpha[g * H + t] * da[t];
  for (int t = wave; t < H; t += CAUM_THREADS / 64) {
    const float a = alpha[g * H + t];
    const float dl = a * (da[t] - dot);
    if (lane == 0) d_logit[g * H + t] = dl;
    float* zrow = d_z2 + (g * H + t) * (int64_t)N2;
    for (int j = lane; j < N2; j += 64) zrow[j] = dl * w3[j];
    float* xrow = d_x + (g * H + t) * (int64_t)U;
    for (int u = lane; u < U; u += 64) xrow[u] = a * ds * cd[g * U + u];
  }
}

// d_w3[j] += sum_r d_logit[r] z2[r, j], d_b3 += sum_r d_logit[r]: row chunks -> partials, then the chunks in order
constexpr int CAUM_RED_ROWS = 64;
__global__ void caum_colsum_partial_kernel(const float* __restrict__ z2, const float* __restrict__ d_logit, int64_t R, int N2,
                                           float* __restrict__ part) {
  const int64_t r0 = blockIdx.x * (int64_t)CAUM_RED_ROWS;
  const int64_t r1 = r0 + CAUM_RED_ROWS < R ? r0 + CAUM_RED_ROWS : R;
  for (int j = threadIdx.x; j <= N2; j += CAUM_THREADS) {
    float acc = 0.f;
    for (int64_t r = r0; r < r1; ++r) acc += d_logit[r] * (j < N2 ? z2[r * N2 + j] : 1.f);
    part[blockIdx.x * (int64_t)(N2 + 1) + j] = acc;
  }
}

__global__ void caum_colsum_final_kernel(const float* __restrict__ part, int64_t chunks, int N2, float* __restrict__ d_w3,
                                         float* __restrict__ d_b3) {
  for (int j = threadIdx.x; j <= N2; j += CAUM_THREADS) {
    float acc = 0.f;
    for (int64_t c = 0; c < chunks; ++c) acc += part[c * (N2 + 1) + j];
    if (j < N2) d_w3[j] += acc;
    else d_b3[0] += acc;
  }
}

// ---- factored evaluation: x[(jj, t)] = y[(jj, t)] + Xh[(user of pair j0 + jj, t)] + Xc[j0 + jj] over the compact rows ------
// (y may be x: every element is read and written by the same thread.)  A user index out of range: zeros, status |= 1.
__global__ void caum_eval_add_kernel(const float* y, const float* __restrict__ xh, const float* __restrict__ xc,
                                     const int64_t* __restrict__ pair_user, int64_t j0, int64_t pairs, int B, int H, int U4,
                                     float* x, int32_t* __restrict__ status) {
  const int64_t n = pairs * H * U4;
  for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x) {
    const int u = (int)(k % U4);
    const int64_t r = k / U4;
    const int t = (int)(r % H);
    const int64_t jj = r / H;
    const int64_t b = pair_user[j0 + jj];
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (b >= 0 && b < B) {
      const float4 a = reinterpret_cast<const float4*>(y)[k];
      const float4 h = reinterpret_cast<const float4*>(xh)[(b * H + t) * U4 + u];
      const float4 c = reinterpret_cast<const float4*>(xc)[(j0 + jj) * U4 + u];
      v = make_float4(a.x + h.x + c.x, a.y + h.y + c.y, a.z + h.z + c.z, a.w + h.w + c.w);
    } else if (u == 0 && t == 0) {
      atomicOr(status, 1);
    }
    reinterpret_cast<float4*>(x)[k] = v;
  }
}

static AttnGeom caum_geom(int64_t outer, int64_t seq, int heads, int dh, int seq_first, float scale) {
  AttnGeom g;
  const int D = heads * dh;
  if (seq_first) {                        // rows s * outer + n (nn.MultiheadAttention, batch_first=False)
    g.q_outer = 3 * D; g.q_seq = outer * 3 * D;
    g.o_outer = D; g.o_seq = outer * D;
  } else {                                // rows n * seq + s (the news encoder's tokens)
    g.q_outer = seq * 3 * D; g.q_seq = 3 * D;
    g.o_outer = seq * D; g.o_seq = D;
  }
  g.groups = outer * heads; g.heads = heads; g.S = (int)seq; g.D = D; g.dh = dh;
  g.scale = scale > 0.f ? scale : 1.0f / sqrtf((float)dh);
  return g;
}

static int caum_attn_check(int64_t outer, int64_t seq, int heads, int dh) {
  NRL_REQUIRE(outer > 0 && seq > 0 && seq < (1LL << 31) && heads > 0, "caum_attn: bad shape");
  NRL_REQUIRE(attn_head_dim_supported(dh), "caum_attn: head dim %d unsupported (16, 20, 32, 48, 64)", dh);
  return NRL_OK;
}

static int caum_dims_ok(int64_t B, int32_t C, int32_t H, int64_t width) {
  NRL_REQUIRE(B > 0 && C > 0 && H > 0 && width > 0, "caum: bad dimensions");
  NRL_REQUIRE(B * H * width < (1LL << 32), "caum: a dropout mask would exceed 2^32 elements");
  return NRL_OK;
}

}  // namespace nrl

using namespace nrl;

extern "C" {

int nrl_caum_attn_fwd(const float* qkv, float* o, float* lse, int64_t outer, int64_t seq, int32_t heads, int32_t head_dim,
                      int32_t seq_first, float scale, void* stream) {
  NRL_TRY(caum_attn_check(outer, seq, heads, head_dim));
  NRL_REQUIRE(qkv && o && (((uintptr_t)qkv | (uintptr_t)o) & 15) == 0, "caum_attn_fwd: bad arguments");
  return attn_fwd(qkv, o, lse, caum_geom(outer, seq, heads, head_dim, seq_first, scale), (hipStream_t)stream);
}

int nrl_caum_attn_bwd(const float* qkv, const float* o, const float* d_o, const float* lse, float* dqkv, int64_t outer,
                      int64_t seq, int32_t heads, int32_t head_dim, int32_t seq_first, float scale, void* stream) {
  NRL_TRY(caum_attn_check(outer, seq, heads, head_dim));
  NRL_REQUIRE(qkv && o && d_o && lse && dqkv &&
                  (((uintptr_t)qkv | (uintptr_t)o | (uintptr_t)d_o | (uintptr_t)dqkv) & 15) == 0,
              "caum_attn_bwd: bad arguments");
  return attn_bwd(qkv, o, d_o, lse, dqkv, caum_geom(outer, seq, heads, head_dim, seq_first, scale), (hipStream_t)stream);
}

int nrl_caum_dropout(const float* x, float* y, int64_t n, double p, uint64_t seed, uint32_t stream_id, void* stream) {
  NRL_REQUIRE(x && y && n >= 0 && n < (1LL << 32) && p >= 0.0 && p < 1.0, "caum_dropout: bad arguments");
  if (n == 0) return NRL_OK;
  hipLaunchKernelGGL(caum_dropout_kernel, dim3(grid_for(n)), dim3(CAUM_THREADS), 0, (hipStream_t)stream, x, y, n,
                     make_dropout(p, seed, stream_id));
  NRL_LAUNCH_CHECK();
  return NRL_OK;
}

int nrl_caum_expand_fwd(const float* h, const float* c, int64_t B, int32_t C, int32_t H, int32_t D, double p, uint64_t seed,
                        uint32_t stream_base, float* hd, float* cd, void* stream) {
  NRL_TRY(caum_dims_ok(B, C, H, D));
  NRL_REQUIRE(h && c && hd && cd && p >= 0.0 && p < 1.0, "caum_expand_fwd: bad arguments");
  const int64_t n = B * C * ((int64_t)H + 1) * D;
  hipLaunchKernelGGL(caum_expand_fwd_kernel, dim3(grid_for(n)), dim3(CAUM_THREADS), 0, (hipStream_t)stream, h, c, (int)B, C,
                     H, D, make_slot_drop(p, seed, stream_base), hd, cd);
  NRL_LAUNCH_CHECK();
  return NRL_OK;
}

int nrl_caum_expand_bwd(const float* d_hd, const float* d_cd, int64_t B, int32_t C, int32_t H, int32_t D, double p,
                        uint64_t seed, uint32_t stream_base, float* d_h, float* d_c, void* stream) {
  NRL_TRY(caum_dims_ok(B, C, H, D));
  NRL_REQUIRE(d_hd && d_cd && d_h && d_c && p >= 0.0 && p < 1.0, "caum_expand_bwd: bad arguments");
  const int64_t n = B * ((int64_t)H + C) * D;
  hipLaunchKernelGGL(caum_expand_bwd_kernel, dim3(grid_for(n)), dim3(CAUM_THREADS), 0, (hipStream_t)stream, d_hd, d_cd,
                     (int)B, C, H, D, make_slot_drop(p, seed, stream_base), d_h, d_c);
  NRL_LAUNCH_CHECK();
  return NRL_OK;
}

int nrl_caum_combine_fwd(const float* P, const float* Q, int64_t B, int32_t C, int32_t H, int32_t F, int32_t U,
                         int32_t hist_slots, float* cnn, float* s, void* stream) {
  NRL_TRY(caum_dims_ok(B, C, H, 3 * (int64_t)F + U));
  NRL_REQUIRE(P && Q && cnn && s && F > 0 && U > 0 && (hist_slots == 1 || hist_slots == C),
              "caum_combine_fwd: bad arguments");
  const int64_t n = B * C * (int64_t)H * (F + U);
  hipLaunchKernelGGL(caum_combine_fwd_kernel, dim3(grid_for(n)), dim3(CAUM_THREADS), 0, (hipStream_t)stream, P, Q, (int)B, C,
                     H, F, U, hist_slots, cnn, s);
  NRL_LAUNCH_CHECK();
  return NRL_OK;
}

int nrl_caum_combine_bwd(const float* d_cnn, const float* d_s, int64_t B, int32_t C, int32_t H, int32_t F, int32_t U,
                         int32_t hist_slots, float* d_P, float* d_Q, void* stream) {
  NRL_TRY(caum_dims_ok(B, C, H, 3 * (int64_t)F + U));
  NRL_REQUIRE(d_cnn && d_s && d_P && d_Q && F > 0 && U > 0 && (hist_slots == 1 || hist_slots == C),
              "caum_combine_bwd: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  const int64_t np = B * hist_slots * (int64_t)H * (3 * F + U), nq = B * C * (int64_t)(F + U);
  hipLaunchKernelGGL(caum_combine_bwd_p_kernel, dim3(grid_for(np)), dim3(CAUM_THREADS), 0, st, d_cnn, d_s, (int)B, C, H, F, U,
                     hist_slots, d_P);
  NRL_LAUNCH_CHECK();
  hipLaunchKernelGGL(caum_combine_bwd_q_kernel, dim3(grid_for(nq)), dim3(CAUM_THREADS), 0, st, d_cnn, d_s, (int)B, C, H, F, U,
                     d_Q);
  NRL_LAUNCH_CHECK();
  return NRL_OK;
}

int nrl_caum_concat_dropout_fwd(const float* cnn, const float* a, int64_t B, int32_t C, int32_t H, int32_t F, int32_t U,
                                double p, uint64_t seed, uint32_t stream_base, float* z, void* stream) {
  NRL_TRY(caum_dims_ok(B, C, H, (int64_t)F + U));
  NRL_REQUIRE(cnn && a && z && p >= 0.0 && p < 1.0, "caum_concat_dropout_fwd: bad arguments");
  const int64_t n = B * C * (int64_t)H * (F + U);
  hipLaunchKernelGGL(caum_concat_dropout_kernel, dim3(grid_for(n)), dim3(CAUM_THREADS), 0, (hipStream_t)stream, cnn, a,
                     (int)B, C, H, F, U, make_slot_drop(p, seed, stream_base), 0, nullptr, nullptr, z);
  NRL_LAUNCH_CHECK();
  return NRL_OK;
}

int nrl_caum_concat_dropout_bwd(const float* d_z, int64_t B, int32_t C, int32_t H, int32_t F, int32_t U, double p,
                                uint64_t seed, uint32_t stream_base, float* d_cnn, float* d_a, void* stream) {
  NRL_TRY(caum_dims_ok(B, C, H, (int64_t)F + U));
  NRL_REQUIRE(d_z && d_cnn && d_a && p >= 0.0 && p < 1.0, "caum_concat_dropout_bwd: bad arguments");
  const int64_t n = B * C * (int64_t)H * (F + U);
  hipLaunchKernelGGL(caum_concat_dropout_kernel, dim3(grid_for(n)), dim3(CAUM_THREADS), 0, (hipStream_t)stream, nullptr,
                     nullptr, (int)B, C, H, F, U, make_slot_drop(p, seed, stream_base), 1, d_cnn, d_a,
                     const_cast<float*>(d_z));
  NRL_LAUNCH_CHECK();
  return NRL_OK;
}

int nrl_caum_group_tanh_fwd(const float* a, const float* g, int64_t groups, int32_t rows_per_group, int32_t N, float* z,
                            void* stream) {
  NRL_REQUIRE(a && g && z && groups > 0 && rows_per_group > 0 && N > 0, "caum_group_tanh_fwd: bad arguments");
  const int64_t R = groups * rows_per_group;
  hipLaunchKernelGGL(caum_group_tanh_fwd_kernel, dim3(grid_for(R * N)), dim3(CAUM_THREADS), 0, (hipStream_t)stream, a, g, R,
                     N, rows_per_group, z);
  NRL_LAUNCH_CHECK();
  return NRL_OK;
}

int nrl_caum_group_tanh_bwd(const float* d_z, const float* z, int64_t groups, int32_t rows_per_group, int32_t N, float* d_a,
                            float* d_g, void* stream) {
  NRL_REQUIRE(d_z && z && d_a && d_g && groups > 0 && rows_per_group > 0 && N > 0, "caum_group_tanh_bwd: bad arguments");
  hipLaunchKernelGGL(caum_group_tanh_bwd_kernel, dim3(grid_for(groups * N)), dim3(CAUM_THREADS), 0, (hipStream_t)stream, d_z,
                     z, groups, N, rows_per_group, d_a, d_g);
  NRL_LAUNCH_CHECK();
  return NRL_OK;
}

int nrl_caum_score_fwd(const float* z2, const float* w3, const float* b3, const float* x, const float* cd,
                       const int64_t* cand_offsets, int64_t B, int32_t C, int32_t slot0, int32_t H, int32_t N2, int32_t U,
                       float* scores, float* alpha, float* user, void* stream) {
  NRL_REQUIRE(z2 && w3 && b3 && x && cd && cand_offsets && scores && alpha && user, "caum_score_fwd: null pointer");
  NRL_REQUIRE(B > 0 && C > 0 && slot0 >= 0 && H > 0 && H <= 8192 && N2 > 0 && U > 0,
              "caum_score_fwd: bad dimensions (max_hist <= 8192)");
  const size_t lds = (H + CAUM_THREADS / 64) * sizeof(float);
  hipLaunchKernelGGL(caum_score_fwd_kernel, dim3((unsigned)(B * C)), dim3(CAUM_THREADS), lds, (hipStream_t)stream, z2, w3,
                     b3, x, cd, cand_offsets, C, slot0, H, N2, U, scores, alpha, user);
  NRL_LAUNCH_CHECK();
  return NRL_OK;
}

// score backward: d_logit per (impression, slot, history row) | the column-sum partials of every row chunk, packed floats
struct CaumScoreWs {
  float *d_logit, *part;
};
static void caum_score_layout(Arena& a, int64_t B, int C, int H, int N2, CaumScoreWs* w) {
  const int64_t R = B * C * H;
  w->d_logit = a.take<float>((size_t)R, sizeof(float));
  w->part = a.take<float>((size_t)(ceil_div(R, CAUM_RED_ROWS) * (int64_t)(N2 + 1)), sizeof(float));
}

size_t nrl_caum_score_workspace_bytes(int64_t B, int32_t C, int32_t H, int32_t N2) {
  if (B <= 0 || C <= 0 || H <= 0 || N2 <= 0) return 0;
  return measure_workspace<CaumScoreWs>([&](Arena& a, auto* w) { caum_score_layout(a, B, C, H, N2, w); });
}

int nrl_caum_score_bwd(const float* d_scores, const float* z2, const float* w3, const float* x, const float* cd,
                       const float* alpha, const float* user, const int64_t* cand_offsets, int64_t B, int32_t C,
                       int32_t slot0, int32_t H, int32_t N2, int32_t U, float* d_z2, float* d_x, float* d_cd, float* d_w3,
                       float* d_b3, void* ws, size_t ws_bytes, void* stream) {
  NRL_REQUIRE(d_scores && z2 && w3 && x && cd && alpha && user && cand_offsets && d_z2 && d_x && d_cd && d_w3 && d_b3,
              "caum_score_bwd: null pointer");
  NRL_REQUIRE(B > 0 && C > 0 && slot0 >= 0 && H > 0 && H <= 8192 && N2 > 0 && U > 0,
              "caum_score_bwd: bad dimensions (max_hist <= 8192)");
  CaumScoreWs w;
  NRL_TRY(carve_workspace(ws, ws_bytes, [&](Arena& a) { caum_score_layout(a, B, C, H, N2, &w); }));
  hipStream_t st = (hipStream_t)stream;
  const int64_t R = B * C * H, chunks = ceil_div(R, CAUM_RED_ROWS);
  float *const d_logit = w.d_logit, *const part = w.part;
  const size_t lds = H * sizeof(float);
  hipLaunchKernelGGL(caum_score_bwd_kernel, dim3((unsigned)(B * C)), dim3(CAUM_THREADS), lds, st, d_scores, w3, x, cd, alpha,
                     user, cand_offsets, C, slot0, H, N2, U, d_z2, d_x, d_cd, d_logit);
  NRL_LAUNCH_CHECK();
  hipLaunchKernelGGL(caum_colsum_partial_kernel, dim3((unsigned)chunks), dim3(CAUM_THREADS), 0, st, z2, d_logit, R, N2, part);
  NRL_LAUNCH_CHECK();
  hipLaunchKernelGGL(caum_colsum_final_kernel, dim3(1), dim3(CAUM_THREADS), 0, st, part, chunks, N2, d_w3, d_b3);
  NRL_LAUNCH_CHECK();
  return NRL_OK;
}

int nrl_caum_eval_attn(const float* qkv_h, const float* qkv_c, const int64_t* cand_offsets, const int64_t* pair_row,
                       const int64_t* pair_user, const int32_t* slot_tab, int32_t entries, int64_t n_items, int64_t B, int32_t H,
                       int64_t n, int64_t j0, int64_t j1, int32_t heads, int32_t head_dim, float scale, float* o,
                       int32_t* status, void* stream) {
  NRL_REQUIRE(qkv_h && qkv_c && cand_offsets && pair_row && pair_user && slot_tab && o && status,
              "caum_eval_attn: null pointer");
  NRL_REQUIRE((((uintptr_t)qkv_h | (uintptr_t)qkv_c | (uintptr_t)o) & 15) == 0, "caum_eval_attn: rows must be 16-byte aligned");
  NRL_REQUIRE(B > 0 && B < (1LL << 31) && H > 0 && heads > 0 && n > 0 && entries > 0 && n_items >= 0 && scale > 0.f,
              "caum_eval_attn: bad dimensions");
  NRL_REQUIRE(0 <= j0 && j0 < j1 && j1 <= n, "caum_eval_attn: the pair range must lie inside the pair list");
  NRL_REQUIRE(attn_head_dim_supported(head_dim), "caum_eval_attn: head dim %d unsupported (16, 20, 32, 48, 64)", head_dim);
  CaumEvalArgs a;
  a.qkv_h = qkv_h; a.qkv_c = qkv_c; a.cand_offsets = cand_offsets; a.pair_row = pair_row; a.pair_user = pair_user;
  a.slot_tab = slot_tab; a.o = o; a.status = status;
  a.n = n; a.j0 = j0; a.j1 = j1; a.n_items = n_items;
  a.B = (int)B; a.H = H; a.heads = heads; a.D = heads * head_dim; a.dh = head_dim; a.entries = entries;
  a.scale = scale;
  return caum_eval_attn(a, (hipStream_t)stream);
}

int nrl_caum_eval_add(const float* y, const float* xh, const float* xc, const int64_t* pair_user, int64_t n, int64_t j0,
                      int64_t pairs, int64_t B, int32_t H, int32_t U, float* x, int32_t* status, void* stream) {
  NRL_REQUIRE(y && xh && xc && pair_user && x && status, "caum_eval_add: null pointer");
  NRL_REQUIRE(j0 >= 0 && pairs > 0 && pairs <= n - j0 && B > 0 && B < (1LL << 31) && H > 0 && U > 0 && U % 4 == 0,
              "caum_eval_add: bad dimensions (U a multiple of 4)");
  NRL_REQUIRE((((uintptr_t)y | (uintptr_t)xh | (uintptr_t)xc | (uintptr_t)x) & 15) == 0,
              "caum_eval_add: rows must be 16-byte aligned");
  hipLaunchKernelGGL(caum_eval_add_kernel, dim3(grid_for(pairs * H * (U / 4))), dim3(CAUM_THREADS), 0, (hipStream_t)stream, y,
                     xh, xc, pair_user, j0, pairs, (int)B, H, U / 4, x, status);
  NRL_LAUNCH_CHECK();
  return NRL_OK;
}

}  // extern "C"

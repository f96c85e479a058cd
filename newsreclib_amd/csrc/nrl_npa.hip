// NPA (npa_module.py:208-252): the personalized-attention kernels.  Plain fp32 vector code under both GEMM engines.
//   npa_pool_*            the text encoder's pooling (attention.py:244-259 over the conv features c, one query per user)
//   npa_query_grad        segmented sum of the per-row query gradients onto the users' query rows (no float atomics)
//   nrl_npa_user_queries  every per-user query: user embedding -> dropout -> (Linear -> ReLU -> dropout -> Linear -> tanh)
//   nrl_personalized_user_attention  the user encoder (user/npa.py) over the ragged history, zero-padded to max_hist
//   nrl_npa_cached_scores  eval-mode scores of whole impressions from the cached conv features (encode-once evaluation)
#include <math.h>

#include "nrl_kernels.h"

namespace nrl {

constexpr int NPA_WAVES = 4;
constexpr int NPA_THREADS = 64 * NPA_WAVES;
constexpr int NPA_MAX_CH = 4;        // float4 chunks per lane: F <= 4 * 4 * 64 = 1024

// ---- text encoder pooling, forward --------------------------------------------------------------------------------
// One workgroup per news row n, the L tokens dealt round-robin to its 4 waves, the F columns as float4 chunks over the
// lanes (CH per lane).  c is read ONCE: each wave keeps an online softmax (running max m, sum l, weighted sum acc) over its
// tokens; the four states are merged through LDS.  s_t goes to LDS so that w (N, L) can be written for the backward.
template <int CH>
__global__ __launch_bounds__(NPA_THREADS) void npa_pool_fwd_kernel(const float* __restrict__ c, const float* __restrict__ Qw,
                                                                  const int32_t* __restrict__ owner, int64_t n_queries,
                                                                  int L, int F, float* __restrict__ w,
                                                                  float* __restrict__ out) {
  extern __shared__ float sm[];                 // s[L] | m[4] | l[4] | acc[4][F]
  float* s_tok = sm;
  float* m_w = sm + L;
  float* l_w = m_w + NPA_WAVES;
  float* acc_w = l_w + NPA_WAVES;
  const int64_t n = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int F4 = F >> 2;
  const int o = owner[n];
  const bool valid = o >= 0 && (int64_t)o < n_queries;
  float4 q[CH], acc[CH];
#pragma unroll
  for (int k = 0; k < CH; ++k) {
    const int j = lane + 64 * k;
    q[k] = (valid && j < F4) ? reinterpret_cast<const float4*>(Qw + (int64_t)o * F)[j] : make_float4(0.f, 0.f, 0.f, 0.f);
    acc[k] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  float m = -INFINITY, l = 0.f;
  for (int t = wave; t < L; t += NPA_WAVES) {
    const float4* row = reinterpret_cast<const float4*>(c + (n * L + t) * (int64_t)F);
    float4 v[CH];
    float part = 0.f;
#pragma unroll
    for (int k = 0; k < CH; ++k) {
      const int j = lane + 64 * k;
      v[k] = j < F4 ? row[j] : make_float4(0.f, 0.f, 0.f, 0.f);
      part += q[k].x * v[k].x + q[k].y * v[k].y + q[k].z * v[k].z + q[k].w * v[k].w;
    }
    const float s = wave_sum(part);
    if (lane == 0) s_tok[t] = s;
    const float m_new = fmaxf(m, s);
    const float a = __expf(m - m_new), p = __expf(s - m_new);
    l = l * a + p;
#pragma unroll
    for (int k = 0; k < CH; ++k) {
      acc[k].x = acc[k].x * a + p * v[k].x;
      acc[k].y = acc[k].y * a + p * v[k].y;
      acc[k].z = acc[k].z * a + p * v[k].z;
      acc[k].w = acc[k].w * a + p * v[k].w;
    }
    m = m_new;
  }
  if (lane == 0) { m_w[wave] = m; l_w[wave] = l; }
#pragma unroll
  for (int k = 0; k < CH; ++k) {
    const int j = lane + 64 * k;
    if (j < F4) reinterpret_cast<float4*>(acc_w + wave * F)[j] = acc[k];
  }
  __syncthreads();
  float mx = m_w[0];
#pragma unroll
  for (int i = 1; i < NPA_WAVES; ++i) mx = fmaxf(mx, m_w[i]);
  float sc[NPA_WAVES], den = 0.f;
#pragma unroll
  for (int i = 0; i < NPA_WAVES; ++i) { sc[i] = l_w[i] > 0.f ? __expf(m_w[i] - mx) : 0.f; den += sc[i] * l_w[i]; }
  const float inv = 1.f / den;
  for (int f = threadIdx.x; f < F; f += NPA_THREADS) {
    float r = 0.f;
#pragma unroll
    for (int i = 0; i < NPA_WAVES; ++i) r += sc[i] * acc_w[i * F + f];
    out[n * F + f] = r * inv;
  }
  if (w != nullptr)
    for (int t = threadIdx.x; t < L; t += NPA_THREADS) w[n * L + t] = __expf(s_tok[t] - mx) * inv;
}

// ---- text encoder pooling, backward -------------------------------------------------------------------------------
//   g_t = d_out . c_t;  ds_t = w_t (g_t - sum_u w_u g_u)
//   dc[t] = (w_t d_out + ds_t q) * dropout2 * [c_t > 0]     (the gradient at the conv pre-activation)
//   dq[n] = sum_t ds_t c_t
// Two passes over the tokens of the row (the second read of c finds it in the cache).
template <int CH>
__global__ __launch_bounds__(NPA_THREADS) void npa_pool_bwd_kernel(const float* __restrict__ d_out, const float* __restrict__ c,
                                                                  const float* __restrict__ w, const float* __restrict__ Qw,
                                                                  const int32_t* __restrict__ owner, int64_t n_queries,
                                                                  int L, int F, Dropout drop2, float* __restrict__ dc,
                                                                  float* __restrict__ dq) {
  extern __shared__ float sm[];                 // g[L] | w[L] | ds[L] | dq[4][F] | wg[1]
  float* g_tok = sm;
  float* w_tok = sm + L;
  float* ds_tok = w_tok + L;
  float* dq_w = ds_tok + L;
  float* wg_sum = dq_w + NPA_WAVES * F;
  const int64_t n = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int F4 = F >> 2;
  const int o = owner[n];
  const bool valid = o >= 0 && (int64_t)o < n_queries;
  float4 q[CH], g[CH], acc[CH];
#pragma unroll
  for (int k = 0; k < CH; ++k) {
    const int j = lane + 64 * k;
    const bool in = j < F4;
    q[k] = (valid && in) ? reinterpret_cast<const float4*>(Qw + (int64_t)o * F)[j] : make_float4(0.f, 0.f, 0.f, 0.f);
    g[k] = in ? reinterpret_cast<const float4*>(d_out + n * F)[j] : make_float4(0.f, 0.f, 0.f, 0.f);
    acc[k] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  for (int t = threadIdx.x; t < L; t += NPA_THREADS) w_tok[t] = w[n * L + t];
  for (int t = wave; t < L; t += NPA_WAVES) {
    const float4* row = reinterpret_cast<const float4*>(c + (n * L + t) * (int64_t)F);
    float part = 0.f;
#pragma unroll
    for (int k = 0; k < CH; ++k) {
      const int j = lane + 64 * k;
      if (j < F4) {
        const float4 v = row[j];
        part += g[k].x * v.x + g[k].y * v.y + g[k].z * v.z + g[k].w * v.w;
      }
    }
    part = wave_sum(part);
    if (lane == 0) g_tok[t] = part;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float sgw = 0.f;
    for (int t = 0; t < L; ++t) sgw += w_tok[t] * g_tok[t];
    *wg_sum = sgw;
  }
  __syncthreads();
  const float sgw = *wg_sum;
  for (int t = threadIdx.x; t < L; t += NPA_THREADS) ds_tok[t] = w_tok[t] * (g_tok[t] - sgw);
  __syncthreads();
  for (int t = wave; t < L; t += NPA_WAVES) {
    const int64_t r = n * L + t;
    const float4* row = reinterpret_cast<const float4*>(c + r * (int64_t)F);
    float4* drow = reinterpret_cast<float4*>(dc + r * (int64_t)F);
    const float wt = w_tok[t], dst = ds_tok[t];
    const uint32_t base = (uint32_t)(r * F);
#pragma unroll
    for (int k = 0; k < CH; ++k) {
      const int j = lane + 64 * k;
      if (j < F4) {
        const float4 v = row[j];
        const uint32_t e = base + 4u * (uint32_t)j;
        float4 d;
        d.x = v.x > 0.f ? (wt * g[k].x + dst * q[k].x) * drop2.mult(e) : 0.f;
        d.y = v.y > 0.f ? (wt * g[k].y + dst * q[k].y) * drop2.mult(e + 1) : 0.f;
        d.z = v.z > 0.f ? (wt * g[k].z + dst * q[k].z) * drop2.mult(e + 2) : 0.f;
        d.w = v.w > 0.f ? (wt * g[k].w + dst * q[k].w) * drop2.mult(e + 3) : 0.f;
        drow[j] = d;
        acc[k].x += dst * v.x; acc[k].y += dst * v.y; acc[k].z += dst * v.z; acc[k].w += dst * v.w;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < CH; ++k) {
    const int j = lane + 64 * k;
    if (j < F4) reinterpret_cast<float4*>(dq_w + wave * F)[j] = acc[k];
  }
  __syncthreads();
  for (int f = threadIdx.x; f < F; f += NPA_THREADS) {
    float r = 0.f;
#pragma unroll
    for (int i = 0; i < NPA_WAVES; ++i) r += dq_w[i * F + f];
    dq[n * F + f] = r;
  }
}

// dQw[b] = sum over rows [seg[b], seg[b+1]) of dq, in row order
__global__ __launch_bounds__(256) void npa_query_grad_kernel(const float* __restrict__ dq, const int64_t* __restrict__ seg,
                                                            int F, float* __restrict__ dQw) {
  const int64_t b = blockIdx.x;
  const int64_t r0 = seg[b], r1 = seg[b + 1];
  for (int f = threadIdx.x; f < F; f += blockDim.x) {
    float s = 0.f;
    for (int64_t r = r0; r < r1; ++r) s += dq[r * F + f];
    dQw[b * F + f] = s;
  }
}

static int npa_ch(int F) { return (F / 4 + 63) / 64; }

int npa_pool_fwd(const float* c, const float* Qw, const int32_t* owner, int64_t n_queries, int64_t N, int L, int F,
                 float* w, float* out, hipStream_t st) {
  NRL_REQUIRE(F > 0 && F % 4 == 0 && npa_ch(F) <= NPA_MAX_CH, "npa pooling: num_filters must be a multiple of 4, <= 1024");
  if (N == 0) return NRL_OK;
  const size_t lds = (size_t)(L + 2 * NPA_WAVES + NPA_WAVES * F) * sizeof(float);
  NRL_REQUIRE(lds <= 64 * 1024, "npa pooling: too many tokens");
  const dim3 grid((unsigned)N), block(NPA_THREADS);
  switch (npa_ch(F)) {
    case 1: hipLaunchKernelGGL(npa_pool_fwd_kernel<1>, grid, block, lds, st, c, Qw, owner, n_queries, L, F, w, out); break;
    case 2: hipLaunchKernelGGL(npa_pool_fwd_kernel<2>, grid, block, lds, st, c, Qw, owner, n_queries, L, F, w, out); break;
    case 3: hipLaunchKernelGGL(npa_pool_fwd_kernel<3>, grid, block, lds, st, c, Qw, owner, n_queries, L, F, w, out); break;
    default: hipLaunchKernelGGL(npa_pool_fwd_kernel<4>, grid, block, lds, st, c, Qw, owner, n_queries, L, F, w, out); break;
  }
  NRL_LAUNCH_CHECK();
  return NRL_OK;
}

int npa_pool_bwd(const float* d_out, const float* c, const float* w, const float* Qw, const int32_t* owner,
                 int64_t n_queries, int64_t N, int L, int F, Dropout drop2, float* dc, float* dq, hipStream_t st) {
  NRL_REQUIRE(F > 0 && F % 4 == 0 && npa_ch(F) <= NPA_MAX_CH, "npa pooling: num_filters must be a multiple of 4, <= 1024");
  if (N == 0) return NRL_OK;
  const size_t lds = (size_t)(3 * L + NPA_WAVES * F + 1) * sizeof(float);
  NRL_REQUIRE(lds <= 64 * 1024, "npa pooling: too many tokens");
  const dim3 grid((unsigned)N), block(NPA_THREADS);
  switch (npa_ch(F)) {
    case 1: hipLaunchKernelGGL(npa_pool_bwd_kernel<1>, grid, block, lds, st, d_out, c, w, Qw, owner, n_queries, L, F, drop2, dc, dq); break;
    case 2: hipLaunchKernelGGL(npa_pool_bwd_kernel<2>, grid, block, lds, st, d_out, c, w, Qw, owner, n_queries, L, F, drop2, dc, dq); break;
    case 3: hipLaunchKernelGGL(npa_pool_bwd_kernel<3>, grid, block, lds, st, d_out, c, w, Qw, owner, n_queries, L, F, drop2, dc, dq); break;
    default: hipLaunchKernelGGL(npa_pool_bwd_kernel<4>, grid, block, lds, st, d_out, c, w, Qw, owner, n_queries, L, F, drop2, dc, dq); break;
  }
  NRL_LAUNCH_CHECK();
  return NRL_OK;
}

int npa_query_grad(const float* dq, const int64_t* seg, int64_t n_queries, int F, float* dQw, hipStream_t st) {
  if (n_queries == 0) return NRL_OK;
  hipLaunchKernelGGL(npa_query_grad_kernel, dim3((unsigned)n_queries), dim3(256), 0, st, dq, seg, F, dQw);
  NRL_LAUNCH_CHECK();
  return NRL_OK;
}

// ---- per-user queries ----------------------------------------------------------------------------------------------
// head 0: text query with the history's dropout draw, head 1: the candidates' draw, head 2: news query (user encoder).
struct NpaHead {
  const float *w_t, *b_t, *w_a, *b_a;   // Linear(U -> P), Linear(P -> F)
  int P;
};
struct NpaQueryArgs {
  const float* table;
  const int64_t* user_idx;
  int64_t B, num_users;
  int U, F;
  NpaHead head[3];
  Dropout du, dh[3];
};

__device__ __forceinline__ int64_t npa_user(const NpaQueryArgs& a, int64_t b) {
  const int64_t u = a.user_idx[b];
  return (u >= 0 && u < a.num_users) ? u : -1;
}

// u = dropout(E_u[user]) and h = dropout(relu(W_t u + b_t)) of (b, head) into LDS; pre-activations too when `pre` is given
__device__ void npa_head_front(const NpaQueryArgs& a, int64_t b, int head, float* u, float* h, float* pre) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t user = npa_user(a, b);
  for (int k = threadIdx.x; k < a.U; k += blockDim.x)
    u[k] = user >= 0 ? a.table[user * a.U + k] * a.du.mult((uint32_t)(b * a.U + k)) : 0.f;
  __syncthreads();
  const NpaHead& hd = a.head[head];
  for (int j = wave; j < hd.P; j += NPA_WAVES) {
    float part = 0.f;
    for (int k = lane; k < a.U; k += 64) part += hd.w_t[(int64_t)j * a.U + k] * u[k];
    part = wave_sum(part);
    if (lane == 0) {
      const float z = part + hd.b_t[j];
      if (pre != nullptr) pre[j] = z;
      h[j] = fmaxf(z, 0.f) * a.dh[head].mult((uint32_t)(b * hd.P + j));
    }
  }
  __syncthreads();
}

// q = tanh(W_a h + b_a) for row (b, head): one wave per output feature
__global__ __launch_bounds__(NPA_THREADS) void npa_user_queries_fwd_kernel(NpaQueryArgs a, float* __restrict__ text_q,
                                                                          float* __restrict__ news_q) {
  extern __shared__ float sm[];   // u[U] | h[P]
  const int64_t b = blockIdx.x;
  const int head = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float* u = sm;
  float* h = sm + a.U;
  npa_head_front(a, b, head, u, h, nullptr);
  const NpaHead& hd = a.head[head];
  float* out = head == 2 ? news_q + b * a.F : text_q + (head * a.B + b) * a.F;
  for (int f = wave; f < a.F; f += NPA_WAVES) {
    float part = 0.f;
    for (int j = lane; j < hd.P; j += 64) part += hd.w_a[(int64_t)f * hd.P + j] * h[j];
    part = wave_sum(part);
    if (lane == 0) out[f] = tanhf(part + hd.b_a[f]);
  }
}

// Per (b, head): ga = dq (1 - q^2); gt = (W_a^T ga) * dropout * [pre > 0]; du = W_t^T gt.  Saved for the reductions: ga, gt,
// h (after dropout), du, and u (after dropout, head 0 only).
struct NpaQueryWs {
  float *ga, *gt, *h, *du, *u;   // (3B, F) | (3B, Pmax) | (3B, Pmax) | (3B, U) | (B, U)
  int Pmax;
};

__global__ __launch_bounds__(NPA_THREADS) void npa_user_queries_bwd_rows_kernel(NpaQueryArgs a, const float* __restrict__ d_text_q,
                                                                               const float* __restrict__ d_news_q, NpaQueryWs ws) {
  extern __shared__ float sm[];   // u[U] | h[P] | pre[P] | ga[F] | gt[P]
  const int64_t b = blockIdx.x;
  const int head = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const NpaHead& hd = a.head[head];
  float* u = sm;
  float* h = u + a.U;
  float* pre = h + hd.P;
  float* ga = pre + hd.P;
  float* gt = ga + a.F;
  npa_head_front(a, b, head, u, h, pre);
  const int64_t row = head * a.B + b;
  const float* dq = head == 2 ? d_news_q + b * a.F : d_text_q + row * a.F;
  for (int f = wave; f < a.F; f += NPA_WAVES) {
    float part = 0.f;
    for (int j = lane; j < hd.P; j += 64) part += hd.w_a[(int64_t)f * hd.P + j] * h[j];
    part = wave_sum(part);
    if (lane == 0) {
      const float q = tanhf(part + hd.b_a[f]);
      const float g = dq[f] * (1.f - q * q);
      ga[f] = g;
      ws.ga[row * a.F + f] = g;
    }
  }
  __syncthreads();
  for (int j = threadIdx.x; j < hd.P; j += NPA_THREADS) {
    float s = 0.f;
    for (int f = 0; f < a.F; ++f) s += hd.w_a[(int64_t)f * hd.P + j] * ga[f];
    const float g = pre[j] > 0.f ? s * a.dh[head].mult((uint32_t)(b * hd.P + j)) : 0.f;
    gt[j] = g;
    ws.gt[row * ws.Pmax + j] = g;
    ws.h[row * ws.Pmax + j] = h[j];
  }
  __syncthreads();
  for (int k = threadIdx.x; k < a.U; k += NPA_THREADS) {
    float s = 0.f;
    for (int j = 0; j < hd.P; ++j) s += hd.w_t[(int64_t)j * a.U + k] * gt[j];
    ws.du[row * a.U + k] = s;
    if (head == 0) ws.u[b * a.U + k] = u[k];
  }
}

struct NpaGradTargets {
  float *w_t, *b_t, *w_a, *b_a;
};
struct NpaQueryGradArgs {
  NpaGradTargets g[2];       // text, news (null: late fusion)
  int P[2];
  int nheads[2];             // heads summed into each: text 2 (rows 0..2B), news 1 (rows 2B..3B)
  int64_t B;
  int U, F;
};

// Weight and bias gradients, one workgroup per output row: rows [0, F) of W_a, then [F, F + P) of W_t, per parameter set
// (blockIdx.y).  Every element is owned by one thread and summed over the batch in row order: no atomics.
__global__ __launch_bounds__(256) void npa_user_queries_wgrad_kernel(NpaQueryGradArgs a, NpaQueryWs ws) {
  const int set = blockIdx.y;
  const NpaGradTargets& g = a.g[set];
  if (g.w_t == nullptr) return;
  const int P = a.P[set];
  const int64_t r0 = set == 0 ? 0 : 2 * a.B, r1 = r0 + a.nheads[set] * a.B;
  const int row = blockIdx.x;
  if (row < a.F) {
    const int f = row;
    for (int j = threadIdx.x; j < P; j += blockDim.x) {
      float s = 0.f;
      for (int64_t r = r0; r < r1; ++r) s += ws.ga[r * a.F + f] * ws.h[r * ws.Pmax + j];
      g.w_a[(int64_t)f * P + j] += s;
    }
    if (threadIdx.x == 0) {
      float s = 0.f;
      for (int64_t r = r0; r < r1; ++r) s += ws.ga[r * a.F + f];
      g.b_a[f] += s;
    }
  } else if (row < a.F + P) {
    const int j = row - a.F;
    for (int k = threadIdx.x; k < a.U; k += blockDim.x) {
      float s = 0.f;
      for (int64_t r = r0; r < r1; ++r) s += ws.gt[r * ws.Pmax + j] * ws.u[(r % a.B) * a.U + k];
      g.w_t[(int64_t)j * a.U + k] += s;
    }
    if (threadIdx.x == 0) {
      float s = 0.f;
      for (int64_t r = r0; r < r1; ++r) s += ws.gt[r * ws.Pmax + j];
      g.b_t[j] += s;
    }
  }
}

// User-table rows: the first impression of each user sums the gradient of all its impressions (in batch order), so a user
// that appears twice in a batch gets one deterministic update.
__global__ __launch_bounds__(64) void npa_user_table_grad_kernel(NpaQueryArgs a, int nheads, NpaQueryWs ws,
                                                                float* __restrict__ d_table) {
  const int64_t b = blockIdx.x;
  const int64_t user = npa_user(a, b);
  if (user < 0) return;
  for (int64_t e = 0; e < b; ++e)
    if (a.user_idx[e] == user) return;
  for (int k = threadIdx.x; k < a.U; k += blockDim.x) {
    float s = 0.f;
    for (int64_t e = b; e < a.B; ++e) {
      if (a.user_idx[e] != user) continue;
      float d = 0.f;
      for (int hd = 0; hd < nheads; ++hd) d += ws.du[(hd * a.B + e) * a.U + k];
      s += d * a.du.mult((uint32_t)(e * a.U + k));
    }
    d_table[user * a.U + k] += s;
  }
}

// ---- user encoder: personalized attention over the zero-padded history -------------------------------------------
// Rows [off[b], off[b+1]) of hist plus (max_hist - n_b) virtual zero rows, which take part in the softmax with score 0.
__device__ void npa_user_weights(const float* hist, int64_t r0, int n, int max_hist, const float* q, int F, float* s,
                                 float* scal) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i = wave; i < n; i += NPA_WAVES) {
    float part = 0.f;
    for (int f = lane; f < F; f += 64) part += q[f] * hist[(r0 + i) * F + f];
    part = wave_sum(part);
    if (lane == 0) s[i] = part;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const int pad = max_hist - n;
    float m = pad > 0 ? 0.f : -INFINITY;
    for (int i = 0; i < n; ++i) m = fmaxf(m, s[i]);
    float den = pad > 0 ? pad * expf(-m) : 0.f;
    for (int i = 0; i < n; ++i) den += expf(s[i] - m);
    for (int i = 0; i < n; ++i) s[i] = expf(s[i] - m) / den;
    scal[0] = den;
  }
  __syncthreads();
}

__global__ __launch_bounds__(NPA_THREADS) void npa_user_att_fwd_kernel(const float* __restrict__ hist, const int64_t* __restrict__ off,
                                                                      int max_hist, int F, const float* __restrict__ q,
                                                                      float* __restrict__ out) {
  extern __shared__ float sm[];   // w[max_hist] | scal[1]
  const int64_t b = blockIdx.x;
  const int64_t r0 = off[b];
  const int64_t nr = off[b + 1] - r0;
  const int n = (int)(nr < max_hist ? nr : max_hist);
  npa_user_weights(hist, r0, n, max_hist, q + b * F, F, sm, sm + max_hist);
  for (int f = threadIdx.x; f < F; f += NPA_THREADS) {
    float r = 0.f;
    for (int i = 0; i < n; ++i) r += sm[i] * hist[(r0 + i) * F + f];
    out[b * F + f] = r;
  }
}

__global__ __launch_bounds__(NPA_THREADS) void npa_user_att_bwd_kernel(const float* __restrict__ hist, const int64_t* __restrict__ off,
                                                                      int max_hist, int F, const float* __restrict__ q,
                                                                      const float* __restrict__ d_out, float* __restrict__ d_hist,
                                                                      float* __restrict__ d_q) {
  extern __shared__ float sm[];   // w[max_hist] | ds[max_hist] | scal[2]
  float* w = sm;
  float* ds = sm + max_hist;
  float* scal = ds + max_hist;
  const int64_t b = blockIdx.x;
  const int64_t r0 = off[b];
  const int64_t nr = off[b + 1] - r0;
  const int n = (int)(nr < max_hist ? nr : max_hist);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* qb = q + b * F;
  const float* gb = d_out + b * F;
  npa_user_weights(hist, r0, n, max_hist, qb, F, w, scal);
  for (int i = wave; i < n; i += NPA_WAVES) {   // g_i = d_out . v_i (the virtual rows have g = 0)
    float part = 0.f;
    for (int f = lane; f < F; f += 64) part += gb[f] * hist[(r0 + i) * F + f];
    part = wave_sum(part);
    if (lane == 0) ds[i] = part;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float s = 0.f;
    for (int i = 0; i < n; ++i) s += w[i] * ds[i];
    scal[1] = s;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < n; i += NPA_THREADS) ds[i] = w[i] * (ds[i] - scal[1]);
  __syncthreads();
  for (int f = threadIdx.x; f < F; f += NPA_THREADS) {
    const float g = gb[f], qf = qb[f];
    float dqf = 0.f;
    for (int i = 0; i < n; ++i) {
      const int64_t r = (r0 + i) * F + f;
      dqf += ds[i] * hist[r];
      d_hist[r] = w[i] * g + ds[i] * qf;
    }
    d_q[b * F + f] = dqf;
  }
}

// ---- encode-once evaluation: scores from the cached conv features ----------------------------------------------------------
// table (num_news, L, F) holds c = relu(conv(E[ids]) + b) of every news (nrl_npa_conv_features).  A WAVE pools one news row at a
// time: the F columns as float4 chunks over its lanes (CH per lane), an online softmax over all L tokens with the next token's
// loads issued before the current one is used.  Each table row is read once; every sum has a fixed order (no atomics).
constexpr int NPA_USER_WAVES = 8;     // 50 history rows over 8 waves; 2 workgroups of <= 33 KB LDS per CU keep 16 waves loading

// feat: the (L, F) feature map of the news, or null (index outside the table: an all-zero map, which pools to zero)
template <int CH>
__device__ __forceinline__ void npa_cached_pool(const float* __restrict__ feat, const float4 (&q)[CH], int L, int F, int lane,
                                                float4 (&out)[CH]) {
  const int F4 = F >> 2;
#pragma unroll
  for (int k = 0; k < CH; ++k) out[k] = make_float4(0.f, 0.f, 0.f, 0.f);
  if (feat == nullptr) return;
  float4 cur[CH], nxt[CH];
#pragma unroll
  for (int k = 0; k < CH; ++k) {
    const int j = lane + 64 * k;
    cur[k] = j < F4 ? reinterpret_cast<const float4*>(feat)[j] : make_float4(0.f, 0.f, 0.f, 0.f);
    nxt[k] = cur[k];
  }
  float m = -INFINITY, l = 0.f;
  for (int t = 0; t < L; ++t) {
    if (t + 1 < L) {
      const float4* row = reinterpret_cast<const float4*>(feat + (int64_t)(t + 1) * F);
#pragma unroll
      for (int k = 0; k < CH; ++k) {
        const int j = lane + 64 * k;
        nxt[k] = j < F4 ? row[j] : make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
    float part = 0.f;
#pragma unroll
    for (int k = 0; k < CH; ++k) part += q[k].x * cur[k].x + q[k].y * cur[k].y + q[k].z * cur[k].z + q[k].w * cur[k].w;
    const float s = wave_sum(part);
    const float m_new = fmaxf(m, s);
    const float a = __expf(m - m_new), p = __expf(s - m_new);
    l = l * a + p;
#pragma unroll
    for (int k = 0; k < CH; ++k) {
      out[k].x = out[k].x * a + p * cur[k].x;
      out[k].y = out[k].y * a + p * cur[k].y;
      out[k].z = out[k].z * a + p * cur[k].z;
      out[k].w = out[k].w * a + p * cur[k].w;
      cur[k] = nxt[k];
    }
    m = m_new;
  }
  const float inv = 1.f / l;
#pragma unroll
  for (int k = 0; k < CH; ++k) { out[k].x *= inv; out[k].y *= inv; out[k].z *= inv; out[k].w *= inv; }
}

struct NpaCachedArgs {
  const float* table;
  int64_t num_news;
  const int64_t *hist_idx, *hist_off, *cand_idx, *cand_off;
  int64_t n_hist, n_cand, B;
  const float *q_hist, *q_cand, *q_news;   // q_news null: late fusion
  int L, F, max_hist, max_cand;
  float* user;     // (B, F)
  float* scores;   // (B, max_cand)
};

__device__ __forceinline__ int64_t npa_clamp(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

template <int CH>
__device__ __forceinline__ void npa_load_q(const float* __restrict__ q, int F, int lane, float4 (&out)[CH]) {
#pragma unroll
  for (int k = 0; k < CH; ++k) {
    const int j = lane + 64 * k;
    out[k] = j < (F >> 2) ? reinterpret_cast<const float4*>(q)[j] : make_float4(0.f, 0.f, 0.f, 0.f);
  }
}

// User vectors: one workgroup per impression b.  Wave w pools history rows w, w + 8, ... with q_hist[b] and folds each pooled
// row v_i into its own online state of the history attention (s_i = q_news[b] . v_i; running max, sum, weighted sum), or into a
// plain sum under late fusion.  The eight states meet in LDS; the softmax also counts max_hist - n_b virtual zero rows of
// score 0 (the to_dense_batch rows of the reference).  No (n_hist, F) intermediate leaves the chip.  The workgroup also clears
// the padded score slots of its impression.
template <int CH>
__global__ __launch_bounds__(64 * NPA_USER_WAVES) void npa_cached_user_kernel(NpaCachedArgs a) {
  extern __shared__ float sm[];                 // m[8] | l[8] | acc[8][F]
  float* m_w = sm;
  float* l_w = sm + NPA_USER_WAVES;
  float* acc_w = l_w + NPA_USER_WAVES;
  const int64_t b = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int F = a.F, F4 = F >> 2;
  const int64_t r0 = npa_clamp(a.hist_off[b], 0, a.n_hist);
  const int64_t nr = npa_clamp(a.hist_off[b + 1], r0, a.n_hist) - r0;
  const int n = (int)(nr < a.max_hist ? nr : a.max_hist);
  const bool early = a.q_news != nullptr;
  float4 q[CH], qn[CH], acc[CH], v[CH];
  npa_load_q<CH>(a.q_hist + b * F, F, lane, q);
  if (early) npa_load_q<CH>(a.q_news + b * F, F, lane, qn);
#pragma unroll
  for (int k = 0; k < CH; ++k) acc[k] = make_float4(0.f, 0.f, 0.f, 0.f);
  float m = -INFINITY, l = 0.f;
  for (int i = wave; i < n; i += NPA_USER_WAVES) {
    const int64_t idx = a.hist_idx[r0 + i];
    const float* feat = (idx >= 0 && idx < a.num_news) ? a.table + idx * (int64_t)a.L * F : nullptr;
    npa_cached_pool<CH>(feat, q, a.L, F, lane, v);
    float wgt = 1.f, keep = 1.f;
    if (early) {
      float part = 0.f;
#pragma unroll
      for (int k = 0; k < CH; ++k) part += qn[k].x * v[k].x + qn[k].y * v[k].y + qn[k].z * v[k].z + qn[k].w * v[k].w;
      const float s = wave_sum(part);
      const float m_new = fmaxf(m, s);
      keep = expf(m - m_new);
      wgt = expf(s - m_new);
      m = m_new;
    }
    l = l * keep + wgt;
#pragma unroll
    for (int k = 0; k < CH; ++k) {
      acc[k].x = acc[k].x * keep + wgt * v[k].x;
      acc[k].y = acc[k].y * keep + wgt * v[k].y;
      acc[k].z = acc[k].z * keep + wgt * v[k].z;
      acc[k].w = acc[k].w * keep + wgt * v[k].w;
    }
  }
  if (lane == 0) { m_w[wave] = m; l_w[wave] = l; }
#pragma unroll
  for (int k = 0; k < CH; ++k) {
    const int j = lane + 64 * k;
    if (j < F4) reinterpret_cast<float4*>(acc_w + wave * F)[j] = acc[k];
  }
  __syncthreads();
  float sc[NPA_USER_WAVES], den = 0.f;
  if (early) {
    const int pad = a.max_hist - n;
    float mx = pad > 0 ? 0.f : -INFINITY;
#pragma unroll
    for (int i = 0; i < NPA_USER_WAVES; ++i) mx = fmaxf(mx, m_w[i]);
#pragma unroll
    for (int i = 0; i < NPA_USER_WAVES; ++i) { sc[i] = l_w[i] > 0.f ? expf(m_w[i] - mx) : 0.f; den += sc[i] * l_w[i]; }
    if (pad > 0) den += pad * expf(-mx);
  } else {
#pragma unroll
    for (int i = 0; i < NPA_USER_WAVES; ++i) { sc[i] = l_w[i] > 0.f ? 1.f : 0.f; den += l_w[i]; }   // den = n_b: the mean
  }
  const float inv = den > 0.f ? 1.f / den : 0.f;
  for (int f = threadIdx.x; f < F; f += 64 * NPA_USER_WAVES) {
    float r = 0.f;
#pragma unroll
    for (int i = 0; i < NPA_USER_WAVES; ++i) r += sc[i] * acc_w[i * F + f];
    a.user[b * F + f] = r * inv;
  }
  const int64_t c0 = npa_clamp(a.cand_off[b], 0, a.n_cand);
  const int64_t nc = npa_clamp(a.cand_off[b + 1], c0, a.n_cand) - c0;
  for (int64_t j = nc + threadIdx.x; j < a.max_cand; j += 64 * NPA_USER_WAVES) a.scores[b * a.max_cand + j] = 0.f;
}

// Candidate scores: the waves of the grid spread flat over ALL candidate rows of the batch (a 300-candidate impression is 300
// waves, not one workgroup's tail).  Wave r finds its impression by bisection of cand_off, pools its row with q_cand[b] and dots
// it with user[b].
template <int CH>
__global__ __launch_bounds__(NPA_THREADS) void npa_cached_cand_kernel(NpaCachedArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * NPA_WAVES + (threadIdx.x >> 6);
  if (r >= a.n_cand) return;
  int64_t lo = 0, hi = a.B;                     // the last b with cand_off[b] <= r
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (a.cand_off[mid] <= r) lo = mid; else hi = mid;
  }
  const int64_t b = lo;
  const int64_t j = r - a.cand_off[b];
  if (j < 0 || j >= a.max_cand || r >= a.cand_off[b + 1]) return;
  const int F = a.F;
  float4 q[CH], u[CH], v[CH];
  npa_load_q<CH>(a.q_cand + b * F, F, lane, q);
  const int64_t idx = a.cand_idx[r];
  const float* feat = (idx >= 0 && idx < a.num_news) ? a.table + idx * (int64_t)a.L * F : nullptr;
  npa_cached_pool<CH>(feat, q, a.L, F, lane, v);
  npa_load_q<CH>(a.user + b * F, F, lane, u);
  float part = 0.f;
#pragma unroll
  for (int k = 0; k < CH; ++k) part += u[k].x * v[k].x + u[k].y * v[k].y + u[k].z * v[k].z + u[k].w * v[k].w;
  const float s = wave_sum(part);
  if (lane == 0) a.scores[b * a.max_cand + j] = s;
}

template <int CH>
static int npa_cached_launch(const NpaCachedArgs& a, hipStream_t st) {
  const size_t lds = (size_t)(2 * NPA_USER_WAVES + NPA_USER_WAVES * a.F) * sizeof(float);
  hipLaunchKernelGGL(npa_cached_user_kernel<CH>, dim3((unsigned)a.B), dim3(64 * NPA_USER_WAVES), lds, st, a);
  NRL_LAUNCH_CHECK();
  if (a.n_cand > 0) {
    hipLaunchKernelGGL(npa_cached_cand_kernel<CH>, dim3((unsigned)ceil_div(a.n_cand, NPA_WAVES)), dim3(NPA_THREADS), 0, st, a);
    NRL_LAUNCH_CHECK();
  }
  return NRL_OK;
}

static int npa_query_args(const NrlNpaQueryParams* p, const int64_t* user_idx, int64_t B, double p_drop, uint64_t seed,
                          uint32_t stream0, NpaQueryArgs* a, int* nheads) {
  NRL_REQUIRE(p != nullptr && p->user_table && p->text_proj_weight && p->text_proj_bias && p->text_att_weight &&
                  p->text_att_bias && user_idx, "npa user queries: null argument");
  NRL_REQUIRE(p->user_dim > 0 && p->text_query_dim > 0 && p->num_filters > 0 && p->num_users > 0 && B >= 0,
              "npa user queries: bad dimensions");
  NRL_REQUIRE(p_drop >= 0.0 && p_drop < 1.0, "p_drop must be in [0, 1)");
  const bool news = p->news_proj_weight != nullptr;
  NRL_REQUIRE(!news || (p->news_proj_bias && p->news_att_weight && p->news_att_bias && p->news_query_dim > 0),
              "npa user queries: incomplete news-query head");
  const int64_t widest = p->num_filters > p->text_query_dim ? p->num_filters : p->text_query_dim;
  NRL_REQUIRE(B * (int64_t)(widest > p->news_query_dim ? widest : p->news_query_dim) < (1LL << 32),
              "dropout index space is 32-bit");
  a->table = p->user_table; a->user_idx = user_idx; a->B = B; a->num_users = p->num_users;
  a->U = p->user_dim; a->F = p->num_filters;
  a->head[0] = a->head[1] = NpaHead{p->text_proj_weight, p->text_proj_bias, p->text_att_weight, p->text_att_bias,
                                    p->text_query_dim};
  a->head[2] = news ? NpaHead{p->news_proj_weight, p->news_proj_bias, p->news_att_weight, p->news_att_bias, p->news_query_dim}
                    : a->head[0];
  a->du = make_dropout(p_drop, seed, stream0);
  for (int h = 0; h < 3; ++h) a->dh[h] = make_dropout(p_drop, seed, stream0 + 1 + h);
  *nheads = news ? 3 : 2;
  return NRL_OK;
}

static int npa_pmax(const NrlNpaQueryParams* p) {
  return p->news_proj_weight != nullptr && p->news_query_dim > p->text_query_dim ? p->news_query_dim : p->text_query_dim;
}

static void npa_query_layout(Arena& a, int64_t B, int U, int Pmax, int F, NpaQueryWs* w) {
  w->Pmax = Pmax;
  w->ga = a.take<float>((size_t)3 * B * F);
  w->gt = a.take<float>((size_t)3 * B * Pmax);
  w->h = a.take<float>((size_t)3 * B * Pmax);
  w->du = a.take<float>((size_t)3 * B * U);
  w->u = a.take<float>((size_t)B * U);
}

}  // namespace nrl

using namespace nrl;

extern "C" {

size_t nrl_npa_user_queries_workspace_bytes(const NrlNpaQueryParams* p, int64_t batch) {
  if (p == nullptr) return 0;
  return measure_workspace<NpaQueryWs>(
      [&](Arena& a, auto* w) { npa_query_layout(a, batch, p->user_dim, npa_pmax(p), p->num_filters, w); });
}

int nrl_npa_user_queries_fwd(const NrlNpaQueryParams* p, const int64_t* user_idx, int64_t batch, double p_drop,
                             uint64_t seed, uint32_t stream0, float* text_queries, float* news_queries, void* stream) {
  NpaQueryArgs a;
  int nheads = 0;
  NRL_TRY(npa_query_args(p, user_idx, batch, p_drop, seed, stream0, &a, &nheads));
  NRL_REQUIRE(text_queries != nullptr && (nheads == 2 || news_queries != nullptr), "npa user queries: null output");
  if (batch == 0) return NRL_OK;
  const size_t lds = (size_t)(a.U + npa_pmax(p)) * sizeof(float);
  hipLaunchKernelGGL(npa_user_queries_fwd_kernel, dim3((unsigned)batch, nheads), dim3(NPA_THREADS), lds, (hipStream_t)stream,
                     a, text_queries, news_queries);
  NRL_LAUNCH_CHECK();
  return NRL_OK;
}

int nrl_npa_user_queries_bwd(const NrlNpaQueryParams* p, const NrlNpaQueryGrads* g, const int64_t* user_idx, int64_t batch,
                             double p_drop, uint64_t seed, uint32_t stream0, const float* d_text_queries,
                             const float* d_news_queries, void* ws, size_t ws_bytes, void* stream) {
  NpaQueryArgs a;
  int nheads = 0;
  NRL_TRY(npa_query_args(p, user_idx, batch, p_drop, seed, stream0, &a, &nheads));
  NRL_REQUIRE(g != nullptr && g->user_table && g->text_proj_weight && g->text_proj_bias && g->text_att_weight &&
                  g->text_att_bias, "npa user queries: null gradient");
  NRL_REQUIRE(nheads == 2 || (g->news_proj_weight && g->news_proj_bias && g->news_att_weight && g->news_att_bias),
              "npa user queries: null news-query gradient");
  NRL_REQUIRE(d_text_queries != nullptr && (nheads == 2 || d_news_queries != nullptr), "npa user queries: null d_queries");
  if (batch == 0) return NRL_OK;
  const int Pmax = npa_pmax(p);
  NpaQueryWs w;
  NRL_TRY(carve_workspace(ws, ws_bytes, [&](Arena& ar) { npa_query_layout(ar, batch, a.U, Pmax, a.F, &w); }));
  hipStream_t st = (hipStream_t)stream;
  const size_t lds = (size_t)(a.U + 3 * Pmax + a.F) * sizeof(float);
  hipLaunchKernelGGL(npa_user_queries_bwd_rows_kernel, dim3((unsigned)batch, nheads), dim3(NPA_THREADS), lds, st, a,
                     d_text_queries, d_news_queries, w);
  NRL_LAUNCH_CHECK();
  NpaQueryGradArgs ga;
  ga.g[0] = NpaGradTargets{g->text_proj_weight, g->text_proj_bias, g->text_att_weight, g->text_att_bias};
  ga.g[1] = nheads == 3 ? NpaGradTargets{g->news_proj_weight, g->news_proj_bias, g->news_att_weight, g->news_att_bias}
                        : NpaGradTargets{nullptr, nullptr, nullptr, nullptr};
  ga.P[0] = p->text_query_dim; ga.P[1] = nheads == 3 ? p->news_query_dim : 0;
  ga.nheads[0] = 2; ga.nheads[1] = 1;
  ga.B = batch; ga.U = a.U; ga.F = a.F;
  const int rows = a.F + Pmax;
  hipLaunchKernelGGL(npa_user_queries_wgrad_kernel, dim3((unsigned)rows, 2), dim3(256), 0, st, ga, w);
  NRL_LAUNCH_CHECK();
  hipLaunchKernelGGL(npa_user_table_grad_kernel, dim3((unsigned)batch), dim3(64), 0, st, a, nheads, w, g->user_table);
  NRL_LAUNCH_CHECK();
  return NRL_OK;
}

int nrl_npa_cached_scores(const float* table, int64_t num_news, int32_t seq_len, int32_t num_filters, const int64_t* hist_idx,
                          int64_t n_hist, const int64_t* hist_offsets, const int64_t* cand_idx, int64_t n_cand,
                          const int64_t* cand_offsets, int64_t batch, const float* q_hist, const float* q_cand,
                          const float* q_news, int32_t max_hist, int32_t max_cand, float* user_vectors, float* scores,
                          void* stream) {
  NRL_REQUIRE(table && hist_offsets && cand_offsets && q_hist && q_cand && user_vectors && scores,
              "npa_cached_scores: null argument");
  NRL_REQUIRE((hist_idx || n_hist == 0) && (cand_idx || n_cand == 0), "npa_cached_scores: null index list");
  NRL_REQUIRE(num_news >= 0 && seq_len > 0 && n_hist >= 0 && n_cand >= 0 && batch >= 0 && max_hist >= 0 && max_cand >= 0,
              "npa_cached_scores: bad dimensions");
  NRL_REQUIRE(num_filters > 0 && num_filters % 4 == 0 && npa_ch(num_filters) <= NPA_MAX_CH,
              "npa_cached_scores: num_filters must be a multiple of 4, <= 1024");
  NRL_REQUIRE((((uintptr_t)table | (uintptr_t)q_hist | (uintptr_t)q_cand | (uintptr_t)q_news | (uintptr_t)user_vectors) & 15) == 0,
              "npa_cached_scores: table, queries and user vectors must be 16-byte aligned");
  NRL_REQUIRE(batch < (1LL << 31) && ceil_div(n_cand, NPA_WAVES) < (1LL << 31), "npa_cached_scores: batch too large");
  if (batch == 0) return NRL_OK;
  NpaCachedArgs a;
  a.table = table; a.num_news = num_news;
  a.hist_idx = hist_idx; a.hist_off = hist_offsets; a.cand_idx = cand_idx; a.cand_off = cand_offsets;
  a.n_hist = n_hist; a.n_cand = n_cand; a.B = batch;
  a.q_hist = q_hist; a.q_cand = q_cand; a.q_news = q_news;
  a.L = seq_len; a.F = num_filters; a.max_hist = max_hist; a.max_cand = max_cand;
  a.user = user_vectors; a.scores = scores;
  hipStream_t st = (hipStream_t)stream;
  switch (npa_ch(num_filters)) {
    case 1: return npa_cached_launch<1>(a, st);
    case 2: return npa_cached_launch<2>(a, st);
    case 3: return npa_cached_launch<3>(a, st);
    default: return npa_cached_launch<4>(a, st);
  }
}

int nrl_personalized_user_attention_fwd(const float* hist, const int64_t* hist_offsets, int64_t batch, int32_t max_hist,
                                        int32_t dim, const float* queries, float* out, void* stream) {
  NRL_REQUIRE(hist_offsets && queries && out && batch >= 0 && max_hist >= 0 && dim > 0,
              "personalized_user_attention_fwd: bad arguments");
  if (batch == 0) return NRL_OK;
  const size_t lds = (size_t)(max_hist + 1) * sizeof(float);
  NRL_REQUIRE(lds <= 64 * 1024, "personalized_user_attention: history too long");
  hipLaunchKernelGGL(npa_user_att_fwd_kernel, dim3((unsigned)batch), dim3(NPA_THREADS), lds, (hipStream_t)stream, hist,
                     hist_offsets, max_hist, dim, queries, out);
  NRL_LAUNCH_CHECK();
  return NRL_OK;
}

int nrl_personalized_user_attention_bwd(const float* hist, const int64_t* hist_offsets, int64_t batch, int32_t max_hist,
                                        int32_t dim, const float* queries, const float* d_out, float* d_hist,
                                        float* d_queries, void* stream) {
  NRL_REQUIRE(hist_offsets && queries && d_out && d_queries && batch >= 0 && max_hist >= 0 && dim > 0,
              "personalized_user_attention_bwd: bad arguments");
  if (batch == 0) return NRL_OK;
  const size_t lds = (size_t)(2 * max_hist + 2) * sizeof(float);
  NRL_REQUIRE(lds <= 64 * 1024, "personalized_user_attention: history too long");
  hipLaunchKernelGGL(npa_user_att_bwd_kernel, dim3((unsigned)batch), dim3(NPA_THREADS), lds, (hipStream_t)stream, hist,
                     hist_offsets, max_hist, dim, queries, d_out, d_hist, d_queries);
  NRL_LAUNCH_CHECK();
  return NRL_OK;
}

}  // extern "C"

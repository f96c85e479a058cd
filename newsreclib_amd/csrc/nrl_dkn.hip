// DKN (dkn_module.py:207-240): the knowledge-aware CNN news encoder (KCNN, news.py:186-299) and the candidate-aware user
// attention + DNN click predictor (user/dkn.py:40-107, click_predictor.py:14-45).
//   nrl_dkn_encoder_*  channel build (word rows | tanh(E[ids] T + b) | tanh(C[ids] T + b)) in the K-contiguous layout of
//                      KCWindow, one windowed GEMM per window (nrl_conv.h, pad = 0), bias + ReLU + max over the valid
//                      positions with a one-byte argmax; backward through the dense windowed dgrad / wgrad, the word and
//                      entity table gradients and a deterministic two-stage reduction for the transform's dT / db
//   nrl_dkn_click_*    one workgroup per impression: the user attention over its ragged history, the user vector, the
//                      predictor and the score mask; backward without float atomics (a fixed-order reduction over the
//                      batch for the parameter gradients)
//   nrl_dkn_user_query / nrl_dkn_cand_project  the two halves of the predictor's first layer, split by columns of pred_w1: the
//                      user's q = Wu u + b1 and the catalogue's P = rows Wc^T, for nrl_topk_relu_scores (nrl_topk.hip)
#include <math.h>

#include "nrl_api_internal.h"

namespace nrl {

constexpr int DKN_MAX_WIN = 4;
constexpr int DKN_THREADS = 256;

// ---- channel build ------------------------------------------------------------------------------------------------------
// out[m * ldo + j] = table[ids[m] * dim + j] (dim % 4 == 0, ldo % 4 == 0): the word channel of X, or one entity channel's
// lookup before the transform
__global__ __launch_bounds__(DKN_THREADS) void dkn_gather_kernel(const float* __restrict__ table, const int64_t* __restrict__ ids,
                                                                 int64_t n, int dim, float* __restrict__ out, int64_t ldo) {
  const int d4 = dim >> 2;
  const int64_t total = n * d4;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t m = i / d4;
    const int j = (int)(i - m * d4);
    reinterpret_cast<float4*>(out + m * ldo)[j] = reinterpret_cast<const float4*>(table + ids[m] * (int64_t)dim)[j];
  }
}

static int dkn_gather(const float* table, const int64_t* ids, int64_t n, int dim, float* out, int64_t ldo, hipStream_t st) {
  const int64_t total = n * (dim / 4);
  if (total == 0) return NRL_OK;
  const int64_t blocks = std::min<int64_t>(ceil_div(total, DKN_THREADS), 65536);
  hipLaunchKernelGGL(dkn_gather_kernel, dim3((unsigned)blocks), dim3(DKN_THREADS), 0, st, table, ids, n, dim, out, ldo);
  NRL_LAUNCH_CHECK();
  return NRL_OK;
}

// ---- max over time --------------------------------------------------------------------------------------------------------
// c (N * L, F) = conv + bias (pre-ReLU); one thread per (news, filter): out = relu(max over l in [0, L - W]),
// am = the first l attaining the max (rows past L - W read taps beyond the news: never valid conv outputs)
__global__ __launch_bounds__(DKN_THREADS) void dkn_maxpool_fwd_kernel(const float* __restrict__ c, int64_t N, int L, int F,
                                                                      int W, float* __restrict__ out, int64_t ldo,
                                                                      uint8_t* __restrict__ am, int64_t lda) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N * F) return;
  const int64_t n = i / F;
  const int f = (int)(i - n * F);
  const float* p = c + n * L * (int64_t)F + f;
  float best = p[0];
  int arg = 0;
  for (int l = 1; l <= L - W; ++l) {
    const float v = p[(int64_t)l * F];
    if (v > best) best = v, arg = l;
  }
  out[n * ldo + f] = fmaxf(best, 0.0f);
  am[n * lda + f] = (uint8_t)arg;
}

// dc (N * L, F): d_out at the argmax row when the pooled value is positive (the ReLU gate), zero elsewhere
__global__ __launch_bounds__(DKN_THREADS) void dkn_maxpool_bwd_kernel(const float* __restrict__ d_out, const float* __restrict__ out,
                                                                      int64_t ldo, const uint8_t* __restrict__ am, int64_t lda,
                                                                      int64_t N, int L, int F, float* __restrict__ dc) {
  const int64_t total = N * L * (int64_t)F;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t m = i / F;
    const int f = (int)(i - m * F);
    const int64_t n = m / L;
    const int l = (int)(m - n * L);
    float v = 0.0f;
    if (l == (int)am[n * lda + f] && out[n * ldo + f] > 0.0f) v = d_out[n * ldo + f];
    dc[i] = v;
  }
}

// ---- dgrad epilogue: dX of all windows summed; word columns -> dxw (M, D), entity columns -> de (M, (C-1) D) times
// (1 - y^2) of the saved tanh output once the last window has added its part
struct EpiDknDx {
  float* dxw;
  float* de;
  const float* x;       // X (M, inner)
  int D, inner, first, last;
  struct Row {
    float* w;
    float* e;
    const float* y;
  };
  __device__ __forceinline__ Row row(int64_t m) const {
    return Row{dxw + m * D, de + m * (int64_t)(inner - D), x + m * (int64_t)inner};
  }
  __device__ __forceinline__ void operator()(const Row& r, int64_t, int n, float v) const {
    float* dst = n < D ? r.w + n : r.e + (n - D);
    if (!first) v += *dst;
    if (last && n >= D) {
      const float y = r.y[n];
      v *= 1.0f - y * y;
    }
    *dst = v;
  }
};

// ---- transform weight gradient: dT (Ed, D) = sum_c sum_m E_c[id_m]^T de_c[m], db = sum_c sum_m de_c[m] -----------------
// Stage 1: workgroup (chunk of DKN_ROWS rows, slice of DKN_KS rows of dT) writes its partial sums; rows with entity id 0
// add into a column sum only (their table row is the same for all of them: the product with E_c[0] is taken once in
// stage 2), and only slice 0 reads them -- most positions of a title carry no entity.  Stage 2 sums the chunks in order: no float atomics, bit-reproducible.
constexpr int DKN_ROWS = 256;
constexpr int DKN_KS = 8;
constexpr int DKN_JPT = 2;      // columns per thread: D <= 512

__global__ __launch_bounds__(DKN_THREADS) void dkn_transform_wgrad_partial_kernel(
    const float* __restrict__ de, const int64_t* __restrict__ ent_ids, const float* __restrict__ ent,
    const float* __restrict__ ctx, int64_t M, int D, int Ed, int n_ch, float* __restrict__ part_t,
    float* __restrict__ part_z, float* __restrict__ part_b) {
  const int64_t chunk = blockIdx.x;
  const int k0 = blockIdx.y * DKN_KS;
  const int64_t m0 = chunk * DKN_ROWS, m1 = std::min<int64_t>(M, m0 + DKN_ROWS);
  float acc[DKN_JPT][DKN_KS], z0[DKN_JPT], z1[DKN_JPT], bs[DKN_JPT];
#pragma unroll
  for (int q = 0; q < DKN_JPT; ++q) {
    bs[q] = 0.f;
    z0[q] = z1[q] = 0.f;
#pragma unroll
    for (int k = 0; k < DKN_KS; ++k) acc[q][k] = 0.f;
  }
  const int ldd = n_ch * D;
  for (int64_t m = m0; m < m1; ++m) {
    const int64_t id = ent_ids[m];
    if (id == 0 && blockIdx.y != 0) continue;       // (the column sums of the id-0 rows and db: slice 0 only)
    for (int c = 0; c < n_ch; ++c) {
      const float* row = de + m * ldd + c * D;
      const float* e = (c == 0 ? ent : ctx) + id * Ed + k0;
      float ek[DKN_KS];
#pragma unroll
      for (int k = 0; k < DKN_KS; ++k) ek[k] = (id != 0 && k0 + k < Ed) ? e[k] : 0.f;
#pragma unroll
      for (int q = 0; q < DKN_JPT; ++q) {
        const int j = threadIdx.x + q * DKN_THREADS;
        if (j < D) {
          const float g = row[j];
          bs[q] += g;
          if (id == 0) {
            if (c == 0) z0[q] += g; else z1[q] += g;
          } else {
#pragma unroll
            for (int k = 0; k < DKN_KS; ++k) acc[q][k] = fmaf(ek[k], g, acc[q][k]);
          }
        }
      }
    }
  }
#pragma unroll
  for (int q = 0; q < DKN_JPT; ++q) {
    const int j = threadIdx.x + q * DKN_THREADS;
    if (j >= D) continue;
#pragma unroll
    for (int k = 0; k < DKN_KS; ++k)
      if (k0 + k < Ed) part_t[(chunk * Ed + k0 + k) * D + j] = acc[q][k];
    if (blockIdx.y == 0) {
      part_b[chunk * D + j] = bs[q];
      part_z[(chunk * 2 + 0) * D + j] = z0[q];
      part_z[(chunk * 2 + 1) * D + j] = z1[q];
    }
  }
}

// Stage 2: dT[k, j] += sum_chunks part_t + E[0, k] z_ent[j] + C[0, k] z_ctx[j];  db[j] += sum_chunks part_b
__global__ __launch_bounds__(DKN_THREADS) void dkn_transform_wgrad_reduce_kernel(
    const float* __restrict__ part_t, const float* __restrict__ part_z, const float* __restrict__ part_b, int64_t n_chunks,
    const float* __restrict__ ent, const float* __restrict__ ctx, int D, int Ed, int n_ch, float* __restrict__ dT,
    float* __restrict__ db) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < (int64_t)Ed * D) {
    const int k = (int)(i / D), j = (int)(i - (int64_t)k * D);
    float s = 0.f, z0 = 0.f, z1 = 0.f;
    for (int64_t c = 0; c < n_chunks; ++c) {
      s += part_t[(c * Ed + k) * D + j];
      z0 += part_z[(c * 2) * D + j];
      z1 += part_z[(c * 2 + 1) * D + j];
    }
    s = fmaf(ent[k], z0, s);
    if (n_ch > 1) s = fmaf(ctx[k], z1, s);
    dT[i] += s;
  } else if (i < (int64_t)Ed * D + D) {
    const int j = (int)(i - (int64_t)Ed * D);
    float s = 0.f;
    for (int64_t c = 0; c < n_chunks; ++c) s += part_b[c * D + j];
    db[j] += s;
  }
}

// (F, C, W, D) conv weight gradient += the (F, W, C, D) image gradient
__global__ __launch_bounds__(DKN_THREADS) void dkn_unpack_wgrad_kernel(const float* __restrict__ img, int F, int C, int W,
                                                                       int D, float* __restrict__ dw) {
  const int64_t total = (int64_t)F * C * W * D;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int d = (int)(i % D);
    int64_t r = i / D;
    const int t = (int)(r % W);
    r /= W;
    const int c = (int)(r % C);
    const int64_t f = r / C;
    dw[i] += img[((f * W + t) * C + c) * D + d];
  }
}

// ---- workspace ------------------------------------------------------------------------------------------------------------
struct DknShape {
  int64_t N, M;
  int L, D, Ed, C, F, nw, inner, Wmax;
  int W[DKN_MAX_WIN];
};

struct DknWs {
  float* x;          // (M, inner) channel stack, with Wmax rows of slack on both sides
  float* c;          // (M, F) conv output of one window / dc of one window (slack on both sides)
  float* e;          // (M, Ed) entity lookup (forward) / the entity rows' table gradient (backward)
  float* dxw;        // (M, D)
  float* de;         // (M, (C-1) D)
  float* wimg;       // (F, Wmax * inner) image gradient of one window
  float* part;       // stage-1 partials of dT / db
  uint16_t* planes;  // bf16 (hi, lo) planes of one conv weight image, then of T
  uint16_t* planes_t;
};

static size_t dkn_part_floats(const DknShape& s) {
  const int64_t ch = ceil_div(s.M, DKN_ROWS);
  return (size_t)ch * ((size_t)s.Ed * s.D + 3 * (size_t)s.D);
}

static size_t dkn_plane_elems(const DknShape& s) {
  size_t m = split_weight_elems(s.Ed, s.D);
  for (int i = 0; i < s.nw; ++i) {
    m = std::max(m, split_weight_elems(s.F, s.W[i] * s.inner));
    m = std::max(m, (size_t)s.inner * (size_t)((s.W[i] * s.F + 31) / 32 * 32) * 2 + 64);
  }
  return m;
}

// forward: x | c | e | planes | planes_t;  backward adds dxw | de | wimg | part (the forward's x must survive; c and e are reused)
static void dkn_layout(Arena& a, const DknShape& s, DknWs* w) {
  const size_t slack = (size_t)s.Wmax;
  w->x = a.take_after<float>(slack * s.inner, (size_t)(s.M + 2 * slack) * s.inner);
  w->c = a.take_after<float>(slack * s.F, (size_t)(s.M + 2 * slack) * s.F);
  w->e = a.take<float>((size_t)s.M * s.Ed);
  w->dxw = a.take<float>((size_t)s.M * s.D);
  w->de = a.take<float>((size_t)s.M * (s.inner - s.D));
  w->wimg = a.take<float>((size_t)s.F * s.Wmax * s.inner);
  w->part = a.take<float>(dkn_part_floats(s));
  w->planes = a.take<uint16_t>(dkn_plane_elems(s));
  w->planes_t = a.take<uint16_t>(dkn_plane_elems(s));
}

// click backward: d(user vector) rows + their column sum in row `batch` | dz | hr, packed floats
struct DknClickWs {
  float *dv, *dz, *hr;
};
static void dkn_click_layout(Arena& a, int64_t batch, int max_cand, int dim, int hidden, DknClickWs* w) {
  w->dv = a.take<float>((size_t)((batch + 1) * (int64_t)dim), sizeof(float));
  w->dz = a.take<float>((size_t)(batch * (int64_t)max_cand * hidden), sizeof(float));
  w->hr = a.take<float>((size_t)(batch * (int64_t)max_cand * hidden), sizeof(float));
}

static int dkn_check(const NrlDknParams* p, int64_t n_news, int L, DknShape* s) {
  NRL_REQUIRE(p != nullptr && p->word_table && p->entity_table && p->transform_matrix && p->transform_bias,
              "dkn encoder: null parameter");
  NRL_REQUIRE(p->num_windows >= 1 && p->num_windows <= DKN_MAX_WIN, "dkn encoder: 1 to 4 windows");
  NRL_REQUIRE(p->word_dim > 0 && p->word_dim % 4 == 0 && p->word_dim <= DKN_JPT * DKN_THREADS,
              "dkn encoder: text_embed_dim must be a positive multiple of 4, at most 512");
  NRL_REQUIRE(p->entity_dim > 0 && p->entity_dim % 4 == 0, "dkn encoder: entity_embed_dim must be a positive multiple of 4");
  NRL_REQUIRE(p->num_filters > 0 && p->num_filters % 4 == 0, "dkn encoder: num_filters must be a positive multiple of 4");
  NRL_REQUIRE(n_news >= 0 && L > 0 && L <= 255, "dkn encoder: 1 <= seq_len <= 255");
  s->N = n_news; s->L = L; s->M = n_news * L; s->D = p->word_dim; s->Ed = p->entity_dim;
  s->C = p->context_table != nullptr ? 3 : 2; s->F = p->num_filters; s->nw = p->num_windows; s->inner = s->C * s->D;
  s->Wmax = 0;
  for (int i = 0; i < s->nw; ++i) {
    NRL_REQUIRE(p->conv_image[i] && p->conv_bias[i], "dkn encoder: null conv parameter");
    NRL_REQUIRE(((uintptr_t)p->conv_image[i] & 15) == 0, "dkn encoder: conv image must be 16-byte aligned");
    NRL_REQUIRE(p->windows[i] >= 1 && p->windows[i] <= L, "dkn encoder: every window must be in [1, seq_len]");
    s->W[i] = p->windows[i];
    s->Wmax = std::max(s->Wmax, s->W[i]);
  }
  NRL_REQUIRE(((uintptr_t)p->transform_matrix & 15) == 0, "dkn encoder: transform_matrix must be 16-byte aligned");
  return NRL_OK;
}

}  // namespace nrl

using namespace nrl;

extern "C" {

size_t nrl_dkn_encoder_workspace_bytes(const NrlDknParams* p, int64_t n_news, int32_t seq_len) {
  DknShape s;
  if (dkn_check(p, n_news, seq_len, &s) != NRL_OK) return 0;
  return measure_workspace<DknWs>([&](Arena& a, auto* w) { dkn_layout(a, s, w); });
}

int nrl_dkn_encoder_fwd(const NrlDknParams* p, const int64_t* ids, const int64_t* entity_ids, int64_t n_news,
                        int32_t seq_len, float* out, uint8_t* argmax, void* ws, size_t ws_bytes, void* stream) {
  DknShape s;
  NRL_TRY(dkn_check(p, n_news, seq_len, &s));
  NRL_REQUIRE(ids && entity_ids && out && argmax, "dkn encoder fwd: null argument");
  if (s.M == 0) return NRL_OK;
  DknWs w;
  NRL_TRY(carve_workspace(ws, ws_bytes, [&](Arena& a) { dkn_layout(a, s, &w); }));
  hipStream_t st = (hipStream_t)stream;
  const Dropout nodrop = make_dropout(0.0, 0, 0);
  // X = [word rows | tanh(E[ids] T + b) | tanh(C[ids] T + b)]   (news.py:271-291)
  NRL_TRY(dkn_gather(p->word_table, ids, s.M, s.D, w.x, s.inner, st));
  SplitWeight sT{};
  if (cur_engine() == ENGINE_BF16X3) NRL_TRY(split_weight(p->transform_matrix, s.Ed, s.D, w.planes, &sT, st));
  for (int c = 1; c < s.C; ++c) {
    NRL_TRY(dkn_gather(c == 1 ? p->entity_table : p->context_table, entity_ids, s.M, s.Ed, w.e, s.Ed, st));
    // (M, Ed) x T (Ed, D): the dgrad form of a Linear with weight T (Ed, D)
    NRL_TRY(gemm_dgrad(w.e, p->transform_matrix, sT, EpiLinear{w.x + c * s.D, s.inner, p->transform_bias, 1, nodrop, s.inner},
                       s.M, s.Ed, s.D, st));
  }
  // per window: c = conv(X) + b (nrl_conv.h KCWindow, pad 0), then relu(max over the L - W + 1 valid rows)
  for (int i = 0; i < s.nw; ++i) {
    const int K = s.W[i] * s.inner;
    SplitWeight sc{};
    if (cur_engine() == ENGINE_BF16X3) NRL_TRY(split_weight(p->conv_image[i], s.F, K, w.planes_t, &sc, st));
    const KCWindow a{w.x, s.M, s.inner, s.L, s.W[i], 0};
    NRL_TRY(gemm_any(a, KCPlain{p->conv_image[i], K, s.F}, sc.hi, sc.lo, sc.ld, EpiLinear{w.c, s.F, p->conv_bias[i], 0, nodrop, s.F},
                     s.M, s.F, K, st));
    const int64_t nf = s.N * s.F;
    hipLaunchKernelGGL(dkn_maxpool_fwd_kernel, dim3((unsigned)ceil_div(nf, DKN_THREADS)), dim3(DKN_THREADS), 0, st, w.c, s.N,
                       s.L, s.F, s.W[i], out + i * s.F, (int64_t)s.nw * s.F, argmax + i * s.F, (int64_t)s.nw * s.F);
    NRL_LAUNCH_CHECK();
  }
  return NRL_OK;
}

int nrl_dkn_encoder_bwd(const NrlDknParams* p, const NrlDknGrads* g, const int64_t* ids, const int64_t* sorted_positions,
                        const int64_t* entity_ids, const int64_t* entity_sorted_positions, int64_t n_news, int32_t seq_len,
                        const float* out, const uint8_t* argmax, const float* d_out, void* ws, size_t ws_bytes,
                        void* stream) {
  DknShape s;
  NRL_TRY(dkn_check(p, n_news, seq_len, &s));
  NRL_REQUIRE(g && g->word_table && g->entity_table && g->transform_matrix && g->transform_bias,
              "dkn encoder bwd: null gradient");
  NRL_REQUIRE(s.C == 2 || g->context_table, "dkn encoder bwd: null context gradient");
  NRL_REQUIRE(ids && sorted_positions && entity_ids && entity_sorted_positions && out && argmax && d_out,
              "dkn encoder bwd: null argument");
  for (int i = 0; i < s.nw; ++i) NRL_REQUIRE(g->conv_weight[i] && g->conv_bias[i], "dkn encoder bwd: null conv gradient");
  if (s.M == 0) return NRL_OK;
  DknWs w;
  NRL_TRY(carve_workspace(ws, ws_bytes, [&](Arena& a) { dkn_layout(a, s, &w); }));
  hipStream_t st = (hipStream_t)stream;
  const Dropout nodrop = make_dropout(0.0, 0, 0);
  const int64_t ldo = (int64_t)s.nw * s.F;
  for (int i = 0; i < s.nw; ++i) {
    const int W = s.W[i], K = W * s.inner;
    // dc: one row per (news, filter) -- the argmax -- gated by the pooled value > 0
    const int64_t total = s.M * s.F;
    hipLaunchKernelGGL(dkn_maxpool_bwd_kernel, dim3((unsigned)std::min<int64_t>(ceil_div(total, DKN_THREADS), 65536)),
                       dim3(DKN_THREADS), 0, st, d_out + i * s.F, out + i * s.F, ldo, argmax + i * s.F, ldo, s.N, s.L, s.F,
                       w.c);
    NRL_LAUNCH_CHECK();
    // dW (image layout) and db: the windowed weight gradient (K = M, split-K partial sums added atomically)
    NRL_HIP(hipMemsetAsync(w.wimg, 0, (size_t)s.F * K * sizeof(float), st));
    NRL_TRY(gemm_wgrad_any(w.c, s.F, rc_window(w.x, s.inner, s.L, 0, 1, (int64_t)K), K, w.wimg, g->conv_bias[i], s.M, st));
    const int64_t nw_el = (int64_t)s.F * K;
    hipLaunchKernelGGL(dkn_unpack_wgrad_kernel, dim3((unsigned)std::min<int64_t>(ceil_div(nw_el, DKN_THREADS), 65536)),
                       dim3(DKN_THREADS), 0, st, w.wimg, s.F, s.C, W, s.D, g->conv_weight[i]);
    NRL_LAUNCH_CHECK();
    // dX += sum_{t', f} dc[m + t' - (W - 1), f] Wimg[f, (W-1-t') inner + j]   (reversed taps)
    const int KF = W * s.F, Kp = (KF + 31) / 32 * 32;
    uint16_t* hi = w.planes;
    if (cur_engine() == ENGINE_BF16X3) {
      const int64_t tot = (int64_t)s.inner * Kp;
      hipLaunchKernelGGL(split_conv_weight_t_kernel, dim3((unsigned)ceil_div(tot, 256)), dim3(256), 0, st, p->conv_image[i],
                         s.F, s.inner, W, Kp, hi);
      NRL_LAUNCH_CHECK();
    }
    const KCWindow a{w.c, s.M, s.F, s.L, W, W - 1};
    const RCConvT b_rc{p->conv_image[i], s.F, s.inner, W, (int64_t)s.inner};
    NRL_TRY(gemm_any(a, b_rc, hi, hi + 32, 2 * Kp, EpiDknDx{w.dxw, w.de, w.x, s.D, s.inner, i == 0, i == s.nw - 1}, s.M,
                     s.inner, KF, st));
  }
  // word channel -> the word table (padding row skipped)
  NRL_TRY(embedding_grad_sorted(w.dxw, ids, sorted_positions, s.M, s.D, g->word_table, st));
  // entity channels: dT / db (deterministic two-stage reduction) and the entity / context table gradients through T^T
  const int n_ch = s.C - 1;
  const int64_t n_chunks = ceil_div(s.M, DKN_ROWS);
  float* part_t = w.part;
  float* part_z = part_t + n_chunks * s.Ed * s.D;
  float* part_b = part_z + n_chunks * 2 * s.D;
  hipLaunchKernelGGL(dkn_transform_wgrad_partial_kernel, dim3((unsigned)n_chunks, (unsigned)ceil_div(s.Ed, DKN_KS)),
                     dim3(DKN_THREADS), 0, st, w.de, entity_ids, p->entity_table, p->context_table, s.M, s.D, s.Ed, n_ch,
                     part_t, part_z, part_b);
  NRL_LAUNCH_CHECK();
  const int64_t n_red = (int64_t)s.Ed * s.D + s.D;
  hipLaunchKernelGGL(dkn_transform_wgrad_reduce_kernel, dim3((unsigned)ceil_div(n_red, DKN_THREADS)), dim3(DKN_THREADS), 0, st,
                     part_t, part_z, part_b, n_chunks, p->entity_table, p->context_table, s.D, s.Ed, n_ch,
                     g->transform_matrix, g->transform_bias);
  NRL_LAUNCH_CHECK();
  SplitWeight sT{};
  if (cur_engine() == ENGINE_BF16X3) NRL_TRY(split_weight(p->transform_matrix, s.Ed, s.D, w.planes_t, &sT, st));
  for (int c = 0; c < n_ch; ++c) {
    // rows (M, Ed) = de_c (M, D) T^T, then the shared id-sorted order of the entity ids onto the table
    NRL_TRY(gemm_fwd(KCPlain{w.de + c * s.D, (int64_t)n_ch * s.D, s.M}, p->transform_matrix, sT,
                     EpiLinear{w.e, s.Ed, nullptr, 0, nodrop, s.Ed}, s.M, s.Ed, s.D, false, st));
    NRL_TRY(embedding_grad_sorted(w.e, entity_ids, entity_sorted_positions, s.M, s.Ed,
                                  c == 0 ? g->entity_table : g->context_table, st));
  }
  return NRL_OK;
}

}  // extern "C"

// ---- candidate-aware user attention + DNN click predictor -------------------------------------------------------------------
namespace nrl {

constexpr int DKN_MAX_HIST = 1024;
constexpr int DKN_MAX_DIM = 1024;
constexpr int DKN_MAX_HID = 64;
constexpr int DKN_WAVES = DKN_THREADS / 64;

// The attention DNN is affine (Linear -> Linear, user/dkn.py:42-45): its score of (cand j, hist i) is
// w2 . (W1[:, :dim] c_j + W1[:, dim:] h_i + b1) + b2 = v . h_i + (a term constant over i), which the softmax cancels.
// So one attention per impression, s_i = v . h_i with v = W1[:, dim:]^T w2, serves every valid candidate; the gradients
// of W1[:, :dim], b1 and b2 are then exactly zero (round-off in the reference).
struct DknSmem {
  float v[DKN_MAX_DIM];
  float u[DKN_MAX_DIM];
  float a[DKN_MAX_HIST];      // softmax weights
  float s[DKN_MAX_HIST];      // scores (forward) / d alpha (backward)
  float pre[DKN_MAX_HID];
  float red[DKN_WAVES];
};

// v, s_i, alpha_i and u of impression b; returns n_b
__device__ int dkn_attend(const NrlDknClickParams& p, const float* hist, const int64_t* hoff, int64_t b, int dim, DknSmem& sm) {
  const int Hd = p.hidden;
  const float* W1 = p.att_w1;
  for (int d = threadIdx.x; d < dim; d += DKN_THREADS) {
    float acc = 0.f;
    for (int k = 0; k < Hd; ++k) acc = fmaf(p.att_w2[k], W1[(int64_t)k * 2 * dim + dim + d], acc);
    sm.v[d] = acc;
  }
  __syncthreads();
  const int64_t h0 = hoff[b];
  const int nb = min((int)(hoff[b + 1] - h0), DKN_MAX_HIST);     // (the host refuses max_hist > DKN_MAX_HIST)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i = wave; i < nb; i += DKN_WAVES) {
    const float* h = hist + (h0 + i) * dim;
    float acc = 0.f;
    for (int d = lane; d < dim; d += 64) acc = fmaf(sm.v[d], h[d], acc);
    acc = wave_sum(acc);
    if (lane == 0) sm.s[i] = acc;
  }
  __syncthreads();
  float mx = -INFINITY;
  for (int i = threadIdx.x; i < nb; i += DKN_THREADS) mx = fmaxf(mx, sm.s[i]);
  mx = block_max<DKN_WAVES>(mx, sm.red);
  float part = 0.f;
  for (int i = threadIdx.x; i < nb; i += DKN_THREADS) {
    const float e = expf(sm.s[i] - mx);
    sm.a[i] = e;
    part += e;
  }
  const float tot = block_sum<DKN_WAVES>(part, sm.red);
  const float inv = nb > 0 ? 1.0f / tot : 0.f;
  for (int i = threadIdx.x; i < nb; i += DKN_THREADS) sm.a[i] *= inv;
  __syncthreads();
  for (int d = threadIdx.x; d < dim; d += DKN_THREADS) {
    float acc = 0.f;
    for (int i = 0; i < nb; ++i) acc = fmaf(sm.a[i], hist[(h0 + i) * dim + d], acc);
    sm.u[d] = acc;
  }
  __syncthreads();
  return nb;
}

// pre[k] = W1p[k] . [c; u] + b1p[k] of one candidate row
__device__ void dkn_pred_pre(const NrlDknClickParams& p, const float* c, int dim, DknSmem& sm) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int k = wave; k < p.hidden; k += DKN_WAVES) {
    const float* w = p.pred_w1 + (int64_t)k * 2 * dim;
    float acc = 0.f;
    for (int d = lane; d < dim; d += 64) acc = fmaf(w[d], c[d], fmaf(w[dim + d], sm.u[d], acc));
    acc = wave_sum(acc);
    if (lane == 0) sm.pre[k] = acc + p.pred_b1[k];
  }
  __syncthreads();
}

__global__ __launch_bounds__(DKN_THREADS) void dkn_click_fwd_kernel(NrlDknClickParams p, const float* __restrict__ hist,
                                                                    const int64_t* __restrict__ hoff, const float* __restrict__ cand,
                                                                    const int64_t* __restrict__ coff, int max_cand, int dim,
                                                                    float* __restrict__ scores, float* __restrict__ user) {
  __shared__ DknSmem sm;
  const int64_t b = blockIdx.x;
  dkn_attend(p, hist, hoff, b, dim, sm);
  for (int d = threadIdx.x; d < dim; d += DKN_THREADS) user[b * dim + d] = sm.u[d];
  const int64_t c0 = coff[b];
  const int nc = min((int)(coff[b + 1] - c0), max_cand);
  for (int j = 0; j < max_cand; ++j) {
    if (j >= nc) {                           // padded candidate: score 0 (dkn_module.py:237-238)
      if (threadIdx.x == 0) scores[b * max_cand + j] = 0.f;
      continue;
    }
    dkn_pred_pre(p, cand + (c0 + j) * dim, dim, sm);
    if (threadIdx.x == 0) {
      float sc = p.pred_b2[0];
      for (int k = 0; k < p.hidden; ++k) sc = fmaf(p.pred_w2[k], fmaxf(sm.pre[k], 0.f), sc);
      scores[b * max_cand + j] = sc;
    }
    __syncthreads();
  }
}

// Per impression: d_cand rows, d_hist rows, and for the parameter reduction dv (B, dim), dz / relu(pre) (B * max_cand, Hd)
__global__ __launch_bounds__(DKN_THREADS) void dkn_click_bwd_kernel(NrlDknClickParams p, const float* __restrict__ hist,
                                                                    const int64_t* __restrict__ hoff, const float* __restrict__ cand,
                                                                    const int64_t* __restrict__ coff, int max_cand, int dim,
                                                                    const float* __restrict__ d_scores, float* __restrict__ d_hist,
                                                                    float* __restrict__ d_cand, float* __restrict__ dv,
                                                                    float* __restrict__ dz, float* __restrict__ hrelu) {
  __shared__ DknSmem sm;
  __shared__ float dzs[DKN_MAX_HID];
  const int64_t b = blockIdx.x;
  const int nb = dkn_attend(p, hist, hoff, b, dim, sm);
  const int Hd = p.hidden;
  const int64_t c0 = coff[b];
  const int nc = min((int)(coff[b + 1] - c0), max_cand);
  float du[DKN_MAX_DIM / DKN_THREADS];
#pragma unroll
  for (int q = 0; q < DKN_MAX_DIM / DKN_THREADS; ++q) du[q] = 0.f;
  for (int j = 0; j < max_cand; ++j) {
    float* dzr = dz + (b * max_cand + j) * Hd;
    float* hr = hrelu + (b * max_cand + j) * Hd;
    if (j >= nc) {
      for (int k = threadIdx.x; k < Hd; k += DKN_THREADS) dzr[k] = 0.f, hr[k] = 0.f;
      continue;
    }
    const float* c = cand + (c0 + j) * dim;
    dkn_pred_pre(p, c, dim, sm);
    const float gsc = d_scores[b * max_cand + j];
    for (int k = threadIdx.x; k < Hd; k += DKN_THREADS) {
      const float pre = sm.pre[k];
      const float z = pre > 0.f ? gsc * p.pred_w2[k] : 0.f;
      dzs[k] = z;
      dzr[k] = z;
      hr[k] = fmaxf(pre, 0.f);
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < DKN_MAX_DIM / DKN_THREADS; ++q) {
      const int d = threadIdx.x + q * DKN_THREADS;
      if (d < dim) {
        float dc = 0.f, dd = 0.f;
        for (int k = 0; k < Hd; ++k) {
          const float* w = p.pred_w1 + (int64_t)k * 2 * dim;
          dc = fmaf(w[d], dzs[k], dc);
          dd = fmaf(w[dim + d], dzs[k], dd);
        }
        d_cand[(c0 + j) * dim + d] = dc;      // (the attention's share of d cand is exactly zero: see dkn_attend)
        du[q] += dd;
      }
    }
    __syncthreads();
  }
  // attention backward: d alpha_i = du . h_i; ds_i = alpha_i (d alpha_i - sum_k alpha_k d alpha_k)
#pragma unroll
  for (int q = 0; q < DKN_MAX_DIM / DKN_THREADS; ++q) {
    const int d = threadIdx.x + q * DKN_THREADS;
    if (d < dim) sm.u[d] = du[q];          // (u is no longer needed)
  }
  __syncthreads();
  const int64_t h0 = hoff[b];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i = wave; i < nb; i += DKN_WAVES) {
    const float* h = hist + (h0 + i) * dim;
    float acc = 0.f;
    for (int d = lane; d < dim; d += 64) acc = fmaf(sm.u[d], h[d], acc);
    acc = wave_sum(acc);
    if (lane == 0) sm.s[i] = acc;
  }
  __syncthreads();
  float part = 0.f;
  for (int i = threadIdx.x; i < nb; i += DKN_THREADS) part += sm.a[i] * sm.s[i];
  const float rho = block_sum<DKN_WAVES>(part, sm.red);
  for (int i = threadIdx.x; i < nb; i += DKN_THREADS) sm.s[i] = sm.a[i] * (sm.s[i] - rho);
  __syncthreads();
  for (int d = threadIdx.x; d < dim; d += DKN_THREADS) {
    float acc = 0.f;
    for (int i = 0; i < nb; ++i) {
      const float hv = hist[(h0 + i) * dim + d];
      d_hist[(h0 + i) * dim + d] = fmaf(sm.a[i], sm.u[d], sm.s[i] * sm.v[d]);
      acc = fmaf(sm.s[i], hv, acc);
    }
    dv[b * dim + d] = acc;
  }
}

// out[d] = sum_b x[b, d], in batch order
__global__ __launch_bounds__(DKN_THREADS) void dkn_column_sum_kernel(const float* __restrict__ x, int64_t B, int dim,
                                                                     float* __restrict__ out) {
  const int d = blockIdx.x * blockDim.x + threadIdx.x;
  if (d >= dim) return;
  float s = 0.f;
  for (int64_t b = 0; b < B; ++b) s += x[b * dim + d];
  out[d] = s;
}

// Parameter gradients, summed over the batch in a fixed order (one thread per output element):
//   att_w1[k, dim + d] += w2[k] sum_b dv_b[d];  att_w2[k] += W1[k, dim:] . sum_b dv_b   (W1[:, :dim], b1, b2: zero;
//   sum_b dv_b is row B of dv, dkn_column_sum_kernel)
//   pred_w1[k, :] += sum_{b, j} dz[b, j, k] [c_bj; u_b];  pred_b1 += sum dz;  pred_w2 += sum g relu(pre);  pred_b2 += sum g
__global__ __launch_bounds__(DKN_THREADS) void dkn_click_param_grad_kernel(
    NrlDknClickParams p, NrlDknClickGrads g, const float* __restrict__ cand, const int64_t* __restrict__ coff,
    const float* __restrict__ user, const float* __restrict__ d_scores, const float* __restrict__ dv,
    const float* __restrict__ dz, const float* __restrict__ hrelu, int64_t B, int max_cand, int dim) {
  const int Hd = p.hidden;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t n_w1 = (int64_t)Hd * 2 * dim;
  if (i < n_w1) {
    const int k = (int)(i / (2 * dim)), d = (int)(i - (int64_t)k * 2 * dim);
    float acc = 0.f;
    for (int64_t b = 0; b < B; ++b) {
      const int64_t c0 = coff[b];
      const int nc = min((int)(coff[b + 1] - c0), max_cand);
      for (int j = 0; j < nc; ++j) {
        const float x = d < dim ? cand[(c0 + j) * dim + d] : user[b * dim + d - dim];
        acc = fmaf(dz[(b * max_cand + j) * Hd + k], x, acc);
      }
    }
    g.pred_w1[i] += acc;
    if (d >= dim) g.att_w1[i] += p.att_w2[k] * dv[B * dim + d - dim];
    return;
  }
  const int64_t r = i - n_w1;
  if (r < Hd) {
    const int k = (int)r;
    float sb = 0.f, sw = 0.f, sa = 0.f;
    for (int64_t b = 0; b < B; ++b) {
      const int nc = (int)(coff[b + 1] - coff[b]);
      for (int j = 0; j < nc; ++j) {
        sb += dz[(b * max_cand + j) * Hd + k];
        sw = fmaf(d_scores[b * max_cand + j], hrelu[(b * max_cand + j) * Hd + k], sw);
      }
    }
    for (int d = 0; d < dim; ++d) sa = fmaf(p.att_w1[(int64_t)k * 2 * dim + dim + d], dv[B * dim + d], sa);
    g.pred_b1[k] += sb;
    g.pred_w2[k] += sw;
    g.att_w2[k] += sa;
  } else if (r == Hd) {
    float s = 0.f;
    for (int64_t b = 0; b < B; ++b) {
      const int nc = (int)(coff[b + 1] - coff[b]);
      for (int j = 0; j < nc; ++j) s += d_scores[b * max_cand + j];
    }
    g.pred_b2[0] += s;
  }
}

// ---- the factored click predictor: pre[j] = P[v, j] + q[b, j] with pred_w1 = [Wc | Wu] (full-catalogue top-k, nrl_topk.hip) ------
// One workgroup per user: the user vector of dkn_attend (the bits dkn_click_fwd_kernel writes) and
// q[b, j] = (sum_d Wu[j, d] u[d]) + b1[j], every j one wave's lane-strided fmaf chain and wave_sum: the order depends on dim alone.
__global__ __launch_bounds__(DKN_THREADS) void dkn_user_query_kernel(NrlDknClickParams p, const float* __restrict__ hist,
                                                                     const int64_t* __restrict__ hoff, int dim,
                                                                     float* __restrict__ user, float* __restrict__ q) {
  __shared__ DknSmem sm;
  const int64_t b = blockIdx.x;
  dkn_attend(p, hist, hoff, b, dim, sm);
  for (int d = threadIdx.x; d < dim; d += DKN_THREADS) user[b * dim + d] = sm.u[d];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int j = wave; j < p.hidden; j += DKN_WAVES) {
    const float* w = p.pred_w1 + (int64_t)j * 2 * dim + dim;
    float acc = 0.f;
    for (int d = lane; d < dim; d += 64) acc = fmaf(w[d], sm.u[d], acc);
    acc = wave_sum(acc);
    if (lane == 0) q[b * p.hidden + j] = acc + p.pred_b1[j];
  }
}

// out[n, j] = sum_d Wc[j, d] rows[n, d]: one thread per (row, NJ values of j), one fmaf chain over d = 0, 1, ... from +0 each, so
// the bits of an output depend on its row, Wc[j] and dim alone.  A workgroup owns DKN_PROJ_ROWS rows; chunks of DKN_PROJ_DK
// columns of the rows and of Wc pass through LDS (row stride DK + 1: the 64 lanes of a wave read 64 rows at one column from 64
// different banks; a wave's j is uniform, so Wc is read as a broadcast).
constexpr int DKN_PROJ_ROWS = 64;
constexpr int DKN_PROJ_DK = 32;
constexpr int DKN_PROJ_LD = DKN_PROJ_DK + 1;

template <int NJ>
__global__ __launch_bounds__(DKN_THREADS) void dkn_cand_project_kernel(const float* __restrict__ w1, int Hd,
                                                                       const float* __restrict__ rows, int64_t N, int dim,
                                                                       float* __restrict__ out) {
  __shared__ float xs[DKN_PROJ_ROWS * DKN_PROJ_LD];
  __shared__ float ws[DKN_MAX_HID * DKN_PROJ_LD];
  const int tid = threadIdx.x, r = tid & 63;
  const int jg = __builtin_amdgcn_readfirstlane(tid >> 6);           // this wave's j are jg, jg + 4, ...
  const int64_t n0 = (int64_t)blockIdx.x * DKN_PROJ_ROWS;
  float acc[NJ];
#pragma unroll
  for (int i = 0; i < NJ; ++i) acc[i] = 0.f;
  for (int d0 = 0; d0 < dim; d0 += DKN_PROJ_DK) {
    const int nd = min(DKN_PROJ_DK, dim - d0);
    for (int i = tid; i < DKN_PROJ_ROWS * DKN_PROJ_DK; i += DKN_THREADS) {
      const int rr = i / DKN_PROJ_DK, c = i % DKN_PROJ_DK;
      xs[rr * DKN_PROJ_LD + c] = (n0 + rr < N && c < nd) ? rows[(n0 + rr) * dim + d0 + c] : 0.f;
    }
    for (int i = tid; i < Hd * DKN_PROJ_DK; i += DKN_THREADS) {
      const int j = i / DKN_PROJ_DK, c = i % DKN_PROJ_DK;
      ws[j * DKN_PROJ_LD + c] = c < nd ? w1[(int64_t)j * 2 * dim + d0 + c] : 0.f;
    }
    __syncthreads();
    for (int c = 0; c < nd; ++c) {
      const float x = xs[r * DKN_PROJ_LD + c];
#pragma unroll
      for (int i = 0; i < NJ; ++i)
        if (jg + 4 * i < Hd) acc[i] = fmaf(ws[(jg + 4 * i) * DKN_PROJ_LD + c], x, acc[i]);
    }
    __syncthreads();
  }
  if (n0 + r < N) {
#pragma unroll
    for (int i = 0; i < NJ; ++i)
      if (jg + 4 * i < Hd) out[(n0 + r) * Hd + jg + 4 * i] = acc[i];
  }
}

static int dkn_click_check(const NrlDknClickParams* p, int64_t B, int max_hist, int max_cand, int dim) {
  NRL_REQUIRE(p && p->att_w1 && p->att_w2 && p->pred_w1 && p->pred_b1 && p->pred_w2 && p->pred_b2, "dkn click: null parameter");
  NRL_REQUIRE(p->hidden >= 1 && p->hidden <= DKN_MAX_HID, "dkn click: hidden_dim_dnn must be in [1, 64]");
  NRL_REQUIRE(dim >= 1 && dim <= DKN_MAX_DIM, "dkn click: news vector width must be in [1, 1024]");
  NRL_REQUIRE(max_hist >= 0 && max_hist <= DKN_MAX_HIST, "dkn click: at most 1024 history news per impression");
  NRL_REQUIRE(B >= 0 && max_cand >= 0 && B < (1LL << 31), "dkn click: bad batch shape");
  return NRL_OK;
}

}  // namespace nrl

extern "C" {

size_t nrl_dkn_click_workspace_bytes(int64_t batch, int32_t max_cand, int32_t dim, int32_t hidden) {
  return measure_workspace<DknClickWs>([&](Arena& a, auto* w) { dkn_click_layout(a, batch, max_cand, dim, hidden, w); });
}

int nrl_dkn_click_fwd(const NrlDknClickParams* p, const float* hist, const int64_t* hist_offsets, int32_t max_hist,
                      const float* cand, const int64_t* cand_offsets, int64_t batch, int32_t max_cand, int32_t dim,
                      float* scores, float* user, void* stream) {
  NRL_TRY(dkn_click_check(p, batch, max_hist, max_cand, dim));
  NRL_REQUIRE(hist_offsets && cand_offsets && scores && user, "dkn click fwd: null argument");
  if (batch == 0) return NRL_OK;
  hipLaunchKernelGGL(dkn_click_fwd_kernel, dim3((unsigned)batch), dim3(DKN_THREADS), 0, (hipStream_t)stream, *p, hist,
                     hist_offsets, cand, cand_offsets, max_cand, dim, scores, user);
  NRL_LAUNCH_CHECK();
  return NRL_OK;
}

int nrl_dkn_user_query(const NrlDknClickParams* p, const float* hist, const int64_t* hist_offsets, int32_t max_hist, int64_t B,
                       int32_t dim, float* user, float* q, void* stream) {
  NRL_TRY(dkn_click_check(p, B, max_hist, 0, dim));
  NRL_REQUIRE(hist_offsets && user && q, "dkn user query: null hist_offsets, user or q");
  if (B == 0) return NRL_OK;
  hipLaunchKernelGGL(dkn_user_query_kernel, dim3((unsigned)B), dim3(DKN_THREADS), 0, (hipStream_t)stream, *p, hist, hist_offsets,
                     dim, user, q);
  NRL_LAUNCH_CHECK();
  return NRL_OK;
}

int nrl_dkn_cand_project(const NrlDknClickParams* p, const float* rows, int64_t N, int32_t dim, float* out, void* stream) {
  NRL_TRY(dkn_click_check(p, 0, 0, 0, dim));
  NRL_REQUIRE(N >= 0 && N < ((int64_t)1 << 31), "dkn cand project: N in [0, 2^31) rows (got %lld)", (long long)N);
  if (N == 0) return NRL_OK;
  NRL_REQUIRE(rows && out, "dkn cand project: null rows or out");
  const dim3 grid((unsigned)ceil_div(N, DKN_PROJ_ROWS)), block(DKN_THREADS);
  hipStream_t st = (hipStream_t)stream;
  if (p->hidden <= 16)
    hipLaunchKernelGGL(dkn_cand_project_kernel<4>, grid, block, 0, st, p->pred_w1, p->hidden, rows, N, dim, out);
  else if (p->hidden <= 32)
    hipLaunchKernelGGL(dkn_cand_project_kernel<8>, grid, block, 0, st, p->pred_w1, p->hidden, rows, N, dim, out);
  else
    hipLaunchKernelGGL(dkn_cand_project_kernel<16>, grid, block, 0, st, p->pred_w1, p->hidden, rows, N, dim, out);
  NRL_LAUNCH_CHECK();
  return NRL_OK;
}

int nrl_dkn_click_bwd(const NrlDknClickParams* p, const NrlDknClickGrads* g, const float* hist, const int64_t* hist_offsets,
                      int32_t max_hist, const float* cand, const int64_t* cand_offsets, int64_t batch, int32_t max_cand,
                      int32_t dim, const float* user, const float* d_scores, float* d_hist, float* d_cand, void* ws,
                      size_t ws_bytes, void* stream) {
  NRL_TRY(dkn_click_check(p, batch, max_hist, max_cand, dim));
  NRL_REQUIRE(g && g->att_w1 && g->att_w2 && g->pred_w1 && g->pred_b1 && g->pred_w2 && g->pred_b2,
              "dkn click bwd: null gradient");
  NRL_REQUIRE(hist_offsets && cand_offsets && user && d_scores && d_hist && d_cand, "dkn click bwd: null argument");
  if (batch == 0) return NRL_OK;
  DknClickWs w;
  NRL_TRY(carve_workspace(ws, ws_bytes, [&](Arena& a) { dkn_click_layout(a, batch, max_cand, dim, p->hidden, &w); }));
  hipStream_t st = (hipStream_t)stream;
  float *const dv = w.dv, *const dz = w.dz, *const hr = w.hr;
  hipLaunchKernelGGL(dkn_click_bwd_kernel, dim3((unsigned)batch), dim3(DKN_THREADS), 0, st, *p, hist, hist_offsets, cand,
                     cand_offsets, max_cand, dim, d_scores, d_hist, d_cand, dv, dz, hr);
  NRL_LAUNCH_CHECK();
  hipLaunchKernelGGL(dkn_column_sum_kernel, dim3((unsigned)ceil_div(dim, DKN_THREADS)), dim3(DKN_THREADS), 0, st, dv, batch,
                     dim, dv + batch * dim);
  NRL_LAUNCH_CHECK();
  const int64_t n = (int64_t)p->hidden * 2 * dim + p->hidden + 1;
  hipLaunchKernelGGL(dkn_click_param_grad_kernel, dim3((unsigned)ceil_div(n, DKN_THREADS)), dim3(DKN_THREADS), 0, st, *p, *g,
                     cand, cand_offsets, user, d_scores, dv, dz, hr, batch, max_cand, dim);
  NRL_LAUNCH_CHECK();
  return NRL_OK;
}

}  // extern "C"

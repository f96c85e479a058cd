// Full-catalogue ranking: for B users and a table of V news, either the k rows each user scores highest (nrl_topk_*) or where a
// ragged per-user list of held-out rows lands among all of them (nrl_catalogue_*_ranks), leaving out a ragged per-user exclusion
// list (the history) and the rows an `eligible` mask removes.  The (B, V) score matrix is never written: every workgroup walks its
// slice of the table once, tile by tile, and keeps per user only what its consumer needs.
//
// ONE WALK (tk_walk), seven tile producers, four consumers; fifteen of the seventeen walk kernels are its instantiations and nothing
// else (tkr_scores_kernel keeps its own text, for its speed: see there; tkz_sum_kernel runs the walk with its user loop unrolled).  The sixth producer, TkBiasProducer (the dot product plus
// a per-(user, class) bias: tkb_scores_kernel, tkbc_count_kernel, tkbcap_scores_kernel), is TkDot's column with one add behind it;
// the seventh, TksProducer (Gumbel top-k: the dot product times inv_temp plus a hashed Gumbel variable per (seed, user key, row):
// tks_scores_kernel under TkSelect, nrl_topk_sampled_scores), is TkDot's column with a multiply, the noise and an add behind it:
//                      plain dot product   MINER interests      MANNeR ensemble     DKN factored DNN    NPA pooling
//   producer           TkDot               TkiProducer<GATE>    TkeProducer         TkrProducer         TkpProducer
//   TkSelect (top-k)   tk_scores_kernel    tki_scores_kernel    tke_scores_kernel   tkr_scores_kernel   tkp_scores_kernel
//   TkCount  (rank)    tkc_count_kernel    tkic_count_kernel    tkec_count_kernel   tkrc_count_kernel   tkpc_count_kernel
//   TkSelectCapped     tkcap_scores_kernel -                    tkecap_scores_kernel -                  -
//     (top-k, at most m rows per class; k <= 64; merged by tk_merge_capped_kernel)
//   TkLogZ (sums)      tkz_sum_kernel      -                    -                   -                   -
//     (nrl_catalogue_logz: per user n, max t, sum exp(t - max), sum (t - max) exp(t - max) over t = score * inv_temp, the policy of
//     the sampled entry; its slices are the statistics chunks, a function of V alone; folded by tkz_finish_kernel)
// tkw_scores_kernel / tkwc_count_kernel (nrl_topk_window_scores / nrl_catalogue_window_ranks: a time window per user) run TkDot with
// TkSelect / TkCount under a walk of their own, tkw_walk: tk_walk with the window ANDed into the eligibility the consumer sees and
// table tiles outside every window of the workgroup skipped.  The plain kernels' text is untouched by it; see its section.
// 256 threads, one workgroup per (slice of V, tile of users).  Per table tile of TK_BV = 128 rows:
//   * the PRODUCER leaves the tile's scores in LDS.  TkDot: exact-fp32 MFMA (v_mfma_f32_16x16x4_f32) over LDS tiles of both
//     operands (k-major, double-buffered, register-staged global loads as nrl_gemm.h); every score is ONE accumulator chain over
//     k = 0, 4, 8, ... from +0, zero-filled up to the next multiple of TK_BK: its bits are a function of the two rows and D alone,
//     whatever B, V, k, the slicing or the GEMM engine setting (which this unit does not read).  The others: that product over the
//     K interest rows of a user with an aggregation behind it; over up to three tables into a tile of weighted z-scores (after a
//     statistics pass, tke_stats_kernel / tke_finish_kernel); b2 + sum_j w2[j] relu(proj[v, j] + q[u, j]) in plain fp32 vector
//     code; per token a two-operand product folded into an online softmax in registers.  Each section below says how;
//   * the CONSUMER sees one user's 128 scores at a time, by the wave that serves the user: a lane owns two columns and builds the
//     64-bit entry (order-preserving score key << 32 | ~row: larger = better, so equal scores rank by ascending row, and 0 = empty
//     slot) of the columns that are inside V and eligible.  TkSelect compares it with the user's current k-th entry; nearly always
//     no lane survives and the user costs a few instructions.  When lanes survive, the user's exclusion list (its first TK_XCAP
//     entries cached in LDS, longer lists read from global memory) clears the bits of excluded rows inside this tile, the user's
//     list is loaded into registers (entry p in lane p & 63) and the survivors are inserted one by one with ballots and lane
//     shifts.  The top k of a set under a strict total order does not depend on the insertion order, so the result is a pure
//     function of the score bits and the rows.  TkCount counts the entries above each target's entry, and the population.
// A producer does not know its consumer, so a score has the same bits in the list and in the rank; what a rank entry computes
// outside the walk -- the targets' own scores, one *_target_kernel per scorer -- runs the same chain on the same operands.
//   tk_merge_kernel    one wave per user: validates the user's offsets and exclusion indices (status flags), merges the `slices`
//       partial lists with the same insertion and writes (row, score) or (-1, -inf);
//   tkc_finish_kernel  one wave per user: the same flags, the sum of the slices' counts, each target's validity, the outputs.
// The stages (exclusion cache, eligibility, tile product, per-user selection or count, flush) are inlined device functions of
// pointers and counts; the producers and consumers are structs of pointers into LDS that call them.  On the host each scorer's
// own checks and fields are one function each, shared by its two entries.
// No float atomics, no allocation, no host read-back; the workspace holds the partial lists, O(B * slices * k), or the counts.
// Behind the walk kernels, mmr_rerank_kernel (nrl_mmr_rerank) re-ranks a pool any of the top-k entries returned by greedy MMR: it is
// no walk (one workgroup per user, the pool's Gram matrix by tk_tile_accumulate<1, true>, then k steps) and needs no workspace.
// cal_rerank_kernel (nrl_calibrated_rerank) is that kernel with a class-calibration term; its mu == 0 form has no Gram stage.
// dpp_rerank_kernel (nrl_dpp_rerank) is its workgroup running the greedy MAP inference of a determinantal point process instead.
#include <math.h>

#include "nrl_common.h"

namespace nrl {

using tk_f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int TK_THREADS = 256;
constexpr int TK_BU = 64;                      // users per workgroup: 2 waves x 2 MFMA blocks
constexpr int TK_BV = 128;                     // table rows per tile: 2 waves x 4 MFMA blocks
constexpr int TK_BK = 16;
constexpr int TK_LDA = TK_BU + 16;             // == 16 (mod 32): conflict-free fragment reads (nrl_gemm.h LdsLd)
constexpr int TK_LDB = TK_BV + 16;
constexpr int TK_SCLD = TK_BV + 4;             // score tile: 4 rows apart = 16 banks apart for the accumulator stores
constexpr int TK_XCAP = 64;                    // exclusion entries per user cached in LDS
constexpr int TK_USERS_PER_WAVE = TK_BU / 4;
constexpr int TK_TARGET_BLOCKS = 512;          // two resident workgroups on each of the 256 CUs

// dynamic LDS of a scores kernel: `tiles` score tiles (2 with a gate), and what TkSelect carves behind the producer's share: per
// user of the workgroup a list of k entries and the exclusion cache (start, TK_XCAP rows, length); then the eligibility bytes.
// 64 users, one tile: 50 KB + 512 B per k, so two workgroups per CU up to k = 60 and more than 64 KB from k = 29 on.
constexpr size_t tk_lds_bytes(int tiles, int users, int k) {
  return (size_t)tiles * TK_BU * TK_SCLD * 4 + (size_t)users * k * 8 + (size_t)users * 8 + (size_t)users * TK_XCAP * 4 + (size_t)users * 4 +
         TK_BV;
}
static_assert(2 * TK_BK * (TK_LDA + TK_LDB) <= TK_BU * TK_SCLD, "the operand tiles live inside the score tile");
static_assert(2 * TK_BK * (2 * TK_LDA + TK_LDB) <= 2 * TK_BU * TK_SCLD, "with a gate the three operand tiles live inside the two score tiles");
constexpr size_t TKE_STATS_LDS = (size_t)TK_BU * NRL_TOPK_MAX_MODELS * 2 * 4;      // the ensemble kernel's (mean, sd) per user and table
static_assert(tk_lds_bytes(2, TK_BU, NRL_TOPK_MAX_K) + TKE_STATS_LDS <= 160 * 1024,
              "the largest layout fits the dynamic LDS the launch may request");

struct TkArgs {
  const float* user;
  const float* table;
  int64_t B;
  int32_t V, D, k;
  const int64_t* excl_idx;
  const int64_t* excl_off;
  const uint8_t* eligible;
  int32_t slices, tiles_per_slice;
  unsigned long long* partial;                 // (B, slices, k) entries
  int64_t* out_idx;
  float* out_score;
  int32_t* status;
};
// the arguments of a kernel that serves one scorer: a consumer's base (TkArgs, or TkcArgs for the rank) and the scorer's own fields
template <class Base, class Fields>
struct TkWith : Base, Fields {};

__device__ __forceinline__ float tk_unkey(uint32_t key) {      // the score of a score_key
  return __uint_as_float((key & 0x80000000u) ? (key ^ 0x80000000u) : ~key);
}
__device__ __forceinline__ unsigned long long tk_entry(float s, uint32_t v) {
  return ((unsigned long long)score_key(s) << 32) | (uint32_t)~v;
}

__device__ __forceinline__ unsigned long long tk_shfl(unsigned long long x, int src) {
  const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)x, src, 64), hi = (uint32_t)__shfl((int)(uint32_t)(x >> 32), src, 64);
  return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ unsigned long long tk_shfl_up1(unsigned long long x) {
  const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)x, 1, 64), hi = (uint32_t)__shfl_up((int)(uint32_t)(x >> 32), 1, 64);
  return ((unsigned long long)hi << 32) | lo;
}

// A descending list of up to 128 entries held by one wave: position p in lane p & 63 of e0 (p < 64) or e1.  Positions from k on
// hold what fell off the end (all below the k-th entry) and are never read.
struct TkList {
  unsigned long long e0, e1;
  __device__ __forceinline__ unsigned long long kth(int k) const { return tk_shfl(k <= 64 ? e0 : e1, (k - 1) & 63); }
  // nk (wave-uniform) is above the k-th entry and differs from every entry
  __device__ __forceinline__ void insert(unsigned long long nk, int lane, bool two) {
    const bool g0 = e0 > nk;
    int pos = __popcll(__ballot(g0));
    const unsigned long long up0 = tk_shfl_up1(e0);
    if (two) {
      const bool g1 = e1 > nk;
      pos += __popcll(__ballot(g1));
      unsigned long long up1 = tk_shfl_up1(e1);
      const unsigned long long last0 = tk_shfl(e0, 63);
      if (lane == 0) up1 = last0;
      e1 = g1 ? e1 : (lane + 64 == pos ? nk : up1);
    }
    e0 = g0 ? e0 : (lane == pos ? nk : up0);
  }
  // inserts the lanes' entries c whose bit is set in m, as long as they stay above the k-th entry; NaN scores are only reported
  __device__ __forceinline__ bool take(unsigned long long c, unsigned long long m, int k, int lane, bool& nan) {
    bool changed = false;
    unsigned long long thr = kth(k);
    while (m) {
      const int b = __ffsll((long long)m) - 1;
      m &= m - 1;
      const unsigned long long nk = tk_shfl(c, b);
      if (nk <= thr) continue;
      if ((uint32_t)(nk >> 32) == 0xFFFFFFFFu) {
        nan = true;
        continue;
      }
      insert(nk, lane, k > 64);
      thr = kth(k);
      m &= __ballot(c > thr);
      changed = true;
    }
    return changed;
  }
};

// a user's exclusion range: false when the offsets decrease or leave [0, excl_off[B]]
__device__ __forceinline__ bool tk_excl_range(const TkArgs& A, int64_t u, int64_t& s, int64_t& n) {
  s = 0;
  n = 0;
  if (!A.excl_off) return true;
  const int64_t a = A.excl_off[u], b = A.excl_off[u + 1], end = A.excl_off[A.B];
  if (a < 0 || b < a || b > end) return false;
  s = a;
  n = A.excl_idx ? b - a : 0;
  return true;
}

// ---- the stages of a scores kernel ---------------------------------------------------------------------------------------------
// Exclusion cache of a tile of `slots` users of which the first `nu`, from user u0 on, exist: xs[slots] the start of the user's
// exclusion list, xn[slots] its length (0: none, or bad offsets), xl[slots][TK_XCAP] its first rows (-1: none, or outside V).
__device__ __forceinline__ void tk_cache_exclusions(const TkArgs& A, int64_t u0, int nu, int slots, int64_t* xs, int32_t* xn,
                                                    int32_t* xl) {
  const int tid = threadIdx.x;
  if (tid < slots) {
    int64_t s = 0, n = 0;
    if (tid < nu && !tk_excl_range(A, u0 + tid, s, n)) n = 0;                // the merge kernel flags and blanks such a user
    xs[tid] = s;
    xn[tid] = (int32_t)(n < 0x7FFFFFFF ? n : 0x7FFFFFFF);
  }
  __syncthreads();
  for (int i = tid; i < slots * TK_XCAP; i += TK_THREADS) {
    const int ul = i / TK_XCAP, j = i % TK_XCAP;
    int32_t x = -1;
    if (j < xn[ul]) {
      const int64_t r = A.excl_idx[xs[ul] + j];
      if (r >= 0 && r < A.V) x = (int32_t)r;
    }
    xl[i] = x;
  }
}

// el[TK_BV]: column v0 + c of the table tile is inside V and eligible
__device__ __forceinline__ void tk_fill_eligible(const uint8_t* eligible, int v0, int V, uint8_t* el) {
  const int tid = threadIdx.x;
  if (tid < TK_BV) {
    const int64_t v = (int64_t)v0 + tid;
    el[tid] = (v < V && (!eligible || eligible[v])) ? 1 : 0;
  }
}

// The 64 x 128 products of NA row operands (pa[a]: this thread's staging row, tid >> 2, of operand a; zero when !ua_ok) with the
// table rows v0 ... v0 + 127, `ldt` floats apart and D deep (ldt > D: a table whose rows are one token of a (V, L, F) map), left in
// `acc`: the lane holds tile row wm * 32 + i * 16 + 4 g + r, column wn * 64 + j * 16 + l15 in acc[a][i][j][r].  `lds` holds the
// operand tiles, NA x [2][TK_BK][TK_LDA] and then [2][TK_BK][TK_LDB], all staged against ONE pass over the table tile.  Ends with
// the workgroup synchronised: `lds` is free.
// ROWS: tile column c is not table row v0 + c but table row rows[v0 + c] (v0 + c < V, the length of `rows`), read in place at
// table + rows[v0 + c] * ldt, and a zero row where that index is outside [0, table_rows): the products of a gathered table
// without the gather.
template <int NA, bool ROWS = false>
__device__ __forceinline__ void tk_tile_accumulate(const float* const (&pa)[NA], bool ua_ok, const float* table, int64_t ldt, int v0,
                                                   int V, int D, float* lds, tk_f32x4 (&acc)[NA][2][4],
                                                   const int64_t* rows = nullptr, int64_t table_rows = 0) {
  float* const As = lds;
  float* const Bs = As + NA * 2 * TK_BK * TK_LDA;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int l15 = lane & 15, g = lane >> 4;
  // staging assignment: one float4 of every row-operand tile and two of the table tile per thread and k-tile
  const int srow = tid >> 2, skc = (tid & 3) * 4;
  const int nkt = (D + TK_BK - 1) / TK_BK;
  const float* pb[2];
  bool vb_ok[2];
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const int64_t v = (int64_t)v0 + srow + c * 64;
    if constexpr (ROWS) {
      const int64_t r = v < V ? rows[v] : -1;
      vb_ok[c] = r >= 0 && r < table_rows;
      pb[c] = table + (vb_ok[c] ? r : 0) * ldt;
    } else {
      vb_ok[c] = v < V;
      pb[c] = table + (int64_t)(vb_ok[c] ? v : V - 1) * ldt;
    }
  }
  float4 ra[NA], rb[2];
  auto load_tiles = [&](int k0) {                    // unconditional loads from clamped addresses; masked when staged
    const int kk = k0 + skc < D ? k0 + skc : D - 4;
#pragma unroll
    for (int a = 0; a < NA; ++a) ra[a] = ld4(pa[a] + kk);
#pragma unroll
    for (int c = 0; c < 2; ++c) rb[c] = ld4(pb[c] + kk);
  };
  auto store_tiles = [&](int buf, int k0) {
    const bool kok = k0 + skc < D;
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int a = 0; a < NA; ++a) {
      float* as = As + (2 * a + buf) * TK_BK * TK_LDA;
      const float4 x = (kok && ua_ok) ? ra[a] : z;
      as[(skc + 0) * TK_LDA + srow] = x.x;
      as[(skc + 1) * TK_LDA + srow] = x.y;
      as[(skc + 2) * TK_LDA + srow] = x.z;
      as[(skc + 3) * TK_LDA + srow] = x.w;
    }
    float* bs = Bs + buf * TK_BK * TK_LDB;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const float4 b = (kok && vb_ok[c]) ? rb[c] : z;
      const int row = srow + c * 64;
      bs[(skc + 0) * TK_LDB + row] = b.x;
      bs[(skc + 1) * TK_LDB + row] = b.y;
      bs[(skc + 2) * TK_LDB + row] = b.z;
      bs[(skc + 3) * TK_LDB + row] = b.w;
    }
  };

#pragma unroll
  for (int a = 0; a < NA; ++a)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[a][i][j] = tk_f32x4{0.f, 0.f, 0.f, 0.f};

  load_tiles(0);
  store_tiles(0, 0);
  __syncthreads();
  for (int kt = 0; kt < nkt; ++kt) {
    const int buf = kt & 1;
    if (kt + 1 < nkt) load_tiles((kt + 1) * TK_BK);
    const float* bs = Bs + buf * TK_BK * TK_LDB + wn * 64 + l15;
#pragma unroll
    for (int ks = 0; ks < TK_BK / 4; ++ks) {
      float x[NA][2], b[4];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int a = 0; a < NA; ++a) x[a][i] = As[(2 * a + buf) * TK_BK * TK_LDA + wm * 32 + l15 + (4 * ks + g) * TK_LDA + i * 16];
#pragma unroll
      for (int j = 0; j < 4; ++j) b[j] = bs[(4 * ks + g) * TK_LDB + j * 16];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int a = 0; a < NA; ++a) acc[a][i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(x[a][i], b[j], acc[a][i][j], 0, 0, 0);
    }
    if (kt + 1 < nkt) store_tiles(buf ^ 1, (kt + 1) * TK_BK);
    __syncthreads();
  }
}

// one operand's fragments of tk_tile_accumulate -> a score tile [TK_BU][TK_SCLD]
__device__ __forceinline__ void tk_store_fragments(const tk_f32x4 (&x)[2][4], float* tile) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm = wave >> 1, wn = wave & 1, l15 = lane & 15, g = lane >> 4;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) tile[(wm * 32 + i * 16 + 4 * g + r) * TK_SCLD + wn * 64 + j * 16 + l15] = x[i][j][r];
}

// The products of tk_tile_accumulate over a (V, D) table into NA score tiles [TK_BU][TK_SCLD] from `sc` on: until the scores exist
// the same LDS holds the operand tiles.  Ends with the tiles written and the workgroup synchronised.
template <int NA>
__device__ __forceinline__ void tk_tile_product(const float* const (&pa)[NA], bool ua_ok, const float* table, int v0, int V, int D,
                                                float* sc) {
  tk_f32x4 acc[NA][2][4];
  tk_tile_accumulate<NA>(pa, ua_ok, table, D, v0, V, D, sc, acc);
#pragma unroll
  for (int a = 0; a < NA; ++a) tk_store_fragments(acc[a], sc + a * TK_BU * TK_SCLD);
  __syncthreads();
}

// The bits of m0 (columns 0 ... 63 of the table tile at v0) and m1 (64 ... 127) of the rows on one user's exclusion list are cleared,
// by one wave: xn / xs / xl the user's entries of the exclusion cache, longer lists read on from global memory.
__device__ __forceinline__ void tk_clear_excluded(const int32_t* xn, const int64_t* xs, const int32_t* xl, const int64_t* excl_idx,
                                                  int v0, int lane, unsigned long long& m0, unsigned long long& m1) {
  const int n = *xn;
  for (int base = 0; base < n; base += 64) {         // excluded rows inside this tile lose their bit
    const int i = base + lane;
    int64_t x = -1;
    if (i < n) x = i < TK_XCAP ? (int64_t)xl[i] : excl_idx[*xs + i];
    const int64_t rel64 = x - v0;
    const bool inr = x >= 0 && rel64 >= 0 && rel64 < TK_BV;
    const int rel = inr ? (int)rel64 : 0;
    unsigned long long hit = __ballot(inr);
    while (hit) {
      const int b = __ffsll((long long)hit) - 1;
      hit &= hit - 1;
      const int r = __shfl(rel, b, 64);
      if (r < 64)
        m0 &= ~(1ull << r);
      else
        m1 &= ~(1ull << (r - 64));
    }
  }
}

// One user against one table tile, by one wave: `row` the user's 128 scores, L its list of k entries, xn / xs / xl its entries of
// the exclusion cache, e_0 / e_1 the lane's eligibility of columns lane and 64 + lane.
__device__ __forceinline__ void tk_select_user(const float* row, unsigned long long* L, const int32_t* xn, const int64_t* xs,
                                               const int32_t* xl, const int64_t* excl_idx, int v0, bool e_0, bool e_1, int k, int lane,
                                               bool& nan) {
  const unsigned long long thr = L[k - 1];
  const unsigned long long c0 = e_0 ? tk_entry(row[lane], (uint32_t)v0 + lane) : 0ull;
  const unsigned long long c1 = e_1 ? tk_entry(row[64 + lane], (uint32_t)v0 + 64 + lane) : 0ull;
  unsigned long long m0 = __ballot(c0 > thr), m1 = __ballot(c1 > thr);
  if (!(m0 | m1)) return;
  tk_clear_excluded(xn, xs, xl, excl_idx, v0, lane, m0, m1);
  if (!(m0 | m1)) return;
  TkList S;
  S.e0 = lane < k ? L[lane] : 0ull;
  S.e1 = lane + 64 < k ? L[lane + 64] : 0ull;
  bool changed = S.take(c0, m0, k, lane, nan);
  changed |= S.take(c1, m1 & __ballot(c1 > S.kth(k)), k, lane, nan);
  if (changed) {
    if (lane < k) L[lane] = S.e0;
    if (lane + 64 < k) L[lane + 64] = S.e1;
    wave_lds_sync();
  }
}

// a user's k entries, by the wave that owns them, to its slot of `partial`
__device__ __forceinline__ void tk_flush_user(const unsigned long long* L, unsigned long long* P, int k, int lane) {
  for (int p = lane; p < k; p += 64) P[p] = L[p];
}

// ---- the walk: one skeleton for every (tile producer, consumer) pair ---------------------------------------------------------------
// A workgroup serves one (slice of V, tile of users) and walks the slice's table tiles once.  What differs between the walk
// kernels is chosen at compile time by two types and never branched on at run time (tkr_scores_kernel alone is written out):
//   the PRODUCER (one per scorer) owns the score tile(s) at the front of the dynamic LDS and whatever else of the scorer's lives in
//     LDS, contiguously; `rest` is the first byte after that.  slots(): the users of a tile.  stage(A, u0, nu): before the walk, its
//     operands (per-thread row pointers, or rows staged in LDS: the consumer's prologue publishes them).  tile(A, v0, nu): the
//     scores of the tile's users for table rows v0 ... v0 + 127, workgroup synchronised at the end.  row(ul): user ul's 128 scores.
//     skip(ul): the user takes no part.  first / end / STEP: which users of the tile a wave serves (TkBlocked or TkStrided);
//   the CONSUMER (TkSelect, TkCount) carves its arrays from `rest` on, 8-byte members first so that any slots() keeps every member
//     aligned.  `el`: the eligibility bytes.  prologue(A, u0, nu, slots): by the workgroup, ends with its arrays published except
//     for what only the first tile's barriers need to publish.  user(row, ul, ...): one user against one table tile, by the wave
//     that serves the user.  flush(A, ul, u, sl, lane): the user's result for slice sl, by the same wave.
// Both consumers therefore see the same score bits: there is one producer per scorer, and it does not know who consumes.

// the slice of table tiles of a workgroup: first row and number of tiles
__device__ __forceinline__ void tk_slice(const TkArgs& A, int sl, int& v_begin, int& nvt) {
  v_begin = sl * A.tiles_per_slice * TK_BV;                                  // < V < 2^31
  const int64_t v_stop = (int64_t)v_begin + (int64_t)A.tiles_per_slice * TK_BV;
  const int v_end = v_stop < A.V ? (int)v_stop : A.V;
  nvt = (v_end - v_begin + TK_BV - 1) / TK_BV;
}

// wave w serves users 16 w ... 16 w + 15 of the tile
struct TkBlocked {
  static constexpr int STEP = 1;
  __device__ __forceinline__ static int first(int wave) { return wave * TK_USERS_PER_WAVE; }
  __device__ __forceinline__ static int end(int wave, int nu) {
    return first(wave) + TK_USERS_PER_WAVE < nu ? first(wave) + TK_USERS_PER_WAVE : nu;
  }
};
// wave w serves users w, w + 4, ... of the tile
struct TkStrided {
  static constexpr int STEP = 4;
  __device__ __forceinline__ static int first(int wave) { return wave; }
  __device__ __forceinline__ static int end(int, int nu) { return nu; }
};

template <class Args, class Producer, class Consumer>
__device__ __forceinline__ void tk_walk(const Args& A, Producer& P, Consumer& C) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int slots = P.slots();
  // the slice is the fast index: the workgroups resident together share their table slice across the user tiles
  const int sl = (int)(blockIdx.x % (unsigned)A.slices);
  const int64_t u0 = (int64_t)(blockIdx.x / (unsigned)A.slices) * slots;     // first user of the tile
  const int nu = A.B - u0 < slots ? (int)(A.B - u0) : slots;                 // its users (>= 1)
  int v_begin, nvt;
  tk_slice(A, sl, v_begin, nvt);

  P.stage(A, u0, nu);
  C.prologue(A, u0, nu, slots);                       // (its barriers also publish what the producer staged in LDS)
  const int ul_begin = Producer::first(wave), ul_end = Producer::end(wave, nu);
  bool nan = false;

  for (int vt = 0; vt < nvt; ++vt) {
    const int v0 = v_begin + vt * TK_BV;
    tk_fill_eligible(A.eligible, v0, A.V, C.el);
    P.tile(A, v0, nu);

    const bool e_0 = C.el[lane] != 0, e_1 = C.el[64 + lane] != 0;
    for (int ul = ul_begin; ul < ul_end; ul += Producer::STEP) {
      if (P.skip(ul)) continue;
      C.user(P.row(ul), ul, A.excl_idx, v0, e_0, e_1, lane, nan);
    }
    __syncthreads();                                  // the score tiles and `el` are free for the next tile's operands
  }

  if (nan && lane == 0) atomicOr(A.status, NRL_TOPK_E_NAN);
  wave_lds_sync();
  for (int ul = ul_begin; ul < ul_end; ul += Producer::STEP) C.flush(A, ul, u0 + ul, sl, lane);
}

constexpr size_t TK_TILE_BYTES = (size_t)TK_BU * TK_SCLD * 4;
static_assert(TK_TILE_BYTES % 16 == 0, "what follows the score tiles is 16-byte aligned");

// The selecting consumer: per user of the tile a list of k entries, kept while the slice streams past, and the exclusion cache.
struct TkSelect {
  unsigned long long* lists;                   // [slots][k]
  int64_t* xs;                                 // [slots] exclusion cache: start
  int32_t* xl;                                 // [slots][TK_XCAP] exclusion cache: first rows
  int32_t* xn;                                 // [slots] exclusion cache: length
  uint8_t* el;                                 // [TK_BV]
  int k;
  __device__ __forceinline__ TkSelect(unsigned char* p, int slots, int k_) : k(k_) {
    lists = reinterpret_cast<unsigned long long*>(p);
    xs = reinterpret_cast<int64_t*>(lists + slots * k);
    xl = reinterpret_cast<int32_t*>(xs + slots);
    xn = xl + slots * TK_XCAP;
    el = reinterpret_cast<uint8_t*>(xn + slots);
  }
  __device__ __forceinline__ void prologue(const TkArgs& A, int64_t u0, int nu, int slots) const {
    for (int i = threadIdx.x; i < slots * k; i += TK_THREADS) lists[i] = 0ull;
    tk_cache_exclusions(A, u0, nu, slots, xs, xn, xl);                       // (its barrier also publishes `lists`)
  }
  __device__ __forceinline__ void user(const float* row, int ul, const int64_t* excl_idx, int v0, bool e_0, bool e_1, int lane,
                                       bool& nan) const {
    tk_select_user(row, lists + ul * k, xn + ul, xs + ul, xl + ul * TK_XCAP, excl_idx, v0, e_0, e_1, k, lane, nan);
  }
  __device__ __forceinline__ void flush(const TkArgs& A, int ul, int64_t u, int sl, int lane) const {
    tk_flush_user(lists + ul * k, A.partial + (u * A.slices + sl) * k, k, lane);
  }
};
static_assert(tk_lds_bytes(0, 1, 1) == 8 + 8 + TK_XCAP * 4 + 4 + TK_BV, "tk_lds_bytes counts the members of TkSelect");

// The producer of the plain dot product: tile row r is user u0 + r, zero past the last user.
struct TkDot : TkBlocked {
  float* sc;                                   // [TK_BU][TK_SCLD]; until the scores exist, the operand tiles
  unsigned char* rest;
  const float* pa[1];
  bool ua_ok;
  __device__ __forceinline__ explicit TkDot(unsigned char* p) : sc(reinterpret_cast<float*>(p)), rest(p + TK_TILE_BYTES) {}
  __device__ __forceinline__ int slots() const { return TK_BU; }
  __device__ __forceinline__ void stage(const TkArgs& A, int64_t u0, int nu) {
    const int srow = threadIdx.x >> 2;
    ua_ok = srow < nu;
    pa[0] = A.user + (ua_ok ? u0 + srow : A.B - 1) * A.D;
  }
  __device__ __forceinline__ void tile(const TkArgs& A, int v0, int) const { tk_tile_product<1>(pa, ua_ok, A.table, v0, A.V, A.D, sc); }
  __device__ __forceinline__ const float* row(int ul) const { return sc + ul * TK_SCLD; }
  __device__ __forceinline__ bool skip(int) const { return false; }
};

__global__ __launch_bounds__(TK_THREADS) void tk_scores_kernel(TkArgs A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char tk_smem[];
  TkDot P(tk_smem);
  TkSelect C(P.rest, TK_BU, A.k);
  tk_walk(A, P, C);
}

// one wave per user: status flags, merge of the user's partial lists, output
__global__ __launch_bounds__(64) void tk_merge_kernel(TkArgs A) {
  const int64_t u = blockIdx.x;
  const int lane = threadIdx.x, k = A.k;
  int64_t s, n;
  const bool ok = tk_excl_range(A, u, s, n);
  TkList S;
  S.e0 = S.e1 = 0ull;
  if (!ok) {
    if (lane == 0) atomicOr(A.status, NRL_TOPK_E_OFFSETS);
  } else {
    int bad = 0;
    for (int64_t i = lane; i < n; i += 64) {
      const int64_t x = A.excl_idx[s + i];
      bad |= (x < 0 || x >= A.V);
    }
    if (__ballot(bad) && lane == 0) atomicOr(A.status, NRL_TOPK_E_EXCLUDE);
    const unsigned long long* P = A.partial + u * A.slices * k;
    const int64_t total = (int64_t)A.slices * k;
    bool nan = false;
    for (int64_t base = 0; base < total; base += 64) {
      const unsigned long long c = base + lane < total ? P[base + lane] : 0ull;
      const unsigned long long m = __ballot(c > S.kth(k));
      if (m) S.take(c, m, k, lane, nan);
    }
  }
  for (int p = lane; p < k; p += 64) {
    const unsigned long long e = p < 64 ? S.e0 : S.e1;
    A.out_idx[u * k + p] = e ? (int64_t)(uint32_t)~(uint32_t)e : -1;
    A.out_score[u * k + p] = e ? tk_unkey((uint32_t)(e >> 32)) : -INFINITY;
  }
}

// ---- class-capped selection: the k best rows with at most m of any one class ----------------------------------------------------------
// Every table row has a class (row_class[v], any int32) and a user's list takes a row, walking the family's order from the best
// row down, only while fewer than m rows of its class are in it.  That list is the top k of the union of the classes' own top-m
// sets, so like the plain top-k it does not depend on the order in which the rows are seen: TkSelectCapped streams the tiles
// past it and tk_merge_capped_kernel merges the slices' lists by the same insertion (a row of the global answer has, class by
// class, no more better-ranked rivals inside its slice than it has globally, so it is in its slice's answer).
//   * TkCapList: one descending list of up to NRL_TOPK_CAP_MAX_K = 64 entries, position p in lane p, every entry with the class
//     of its row beside it (`tag`; an empty slot, entry 0, has no class; positions from k on hold what fell off and are masked out
//     of every count).  A candidate x of class c above the k-th entry: with g the class-c entries better than x, g >= m drops x;
//     otherwise, when the list already holds m entries of class c, the worst of them (position w) leaves and x enters at its
//     place pos <= w; otherwise x enters and the last entry falls off (w = 63).  Both are ONE lane-select: positions below pos
//     and above w keep their entry, pos takes x, the positions between take their upper neighbour;
//   * the tags are not stored: the lists in LDS, the partial lists and so the workspace and the LDS layout are those of TkSelect,
//     and a list's tags are re-read from row_class[row] when it is loaded into registers (V * 4 bytes, resident in L2);
//   * the threshold pruning is TkSelect's (a candidate not above the k-th entry is dropped first), against the capped list's
//     k-th entry, which is lower: more lanes survive the ballot and are then dropped by their class, one at a time.
// With m >= k no class ever fills up before the list does and every step is TkList's: the bits of the uncapped entry.
struct TkCapFields {
  const int32_t* row_class;                    // (V) the class of every table row
  int32_t m;                                   // the rows of one class a list may hold
};

struct TkCapList {
  unsigned long long e;
  int32_t tag;
  __device__ __forceinline__ unsigned long long kth(int k) const { return tk_shfl(e, k - 1); }
  // nk (wave-uniform, of class c) is above the k-th entry and differs from every entry; false: its class is full of better rows
  __device__ __forceinline__ bool insert(unsigned long long nk, int32_t c, int k, int m, int lane) {
    const bool g = e > nk;                             // (false in the empty slots and from k on: those are below the k-th)
    const bool same = lane < k && e != 0ull && tag == c;
    if (__popcll(__ballot(same && g)) >= m) return false;
    const unsigned long long held = __ballot(same);
    const int pos = __popcll(__ballot(g));
    const int w = __popcll(held) >= m ? 63 - __clzll((long long)held) : 63;
    const unsigned long long up = tk_shfl_up1(e);
    const int32_t tup = __shfl_up(tag, 1, 64);
    const bool keep = lane < pos || lane > w;
    e = keep ? e : (lane == pos ? nk : up);
    tag = keep ? tag : (lane == pos ? c : tup);
    return true;
  }
  // TkList::take over entries c with classes t
  __device__ __forceinline__ bool take(unsigned long long c, int32_t t, unsigned long long msk, int k, int m, int lane, bool& nan) {
    bool changed = false;
    unsigned long long thr = kth(k);
    while (msk) {
      const int b = __ffsll((long long)msk) - 1;
      msk &= msk - 1;
      const unsigned long long nk = tk_shfl(c, b);
      if (nk <= thr) continue;
      if ((uint32_t)(nk >> 32) == 0xFFFFFFFFu) {
        nan = true;
        continue;
      }
      if (!insert(nk, __shfl(t, b, 64), k, m, lane)) continue;
      thr = kth(k);
      msk &= __ballot(c > thr);
      changed = true;
    }
    return changed;
  }
  // the list of k <= 64 entries at L, its tags read from row_class
  __device__ __forceinline__ void load(const unsigned long long* L, const int32_t* row_class, int k, int lane) {
    e = lane < k ? L[lane] : 0ull;
    tag = e ? row_class[(uint32_t)~(uint32_t)e] : 0;
  }
};

// tk_select_user under the cap
__device__ __forceinline__ void tk_select_user_capped(const float* row, unsigned long long* L, const int32_t* xn, const int64_t* xs,
                                                      const int32_t* xl, const int64_t* excl_idx, const int32_t* row_class, int v0,
                                                      bool e_0, bool e_1, int k, int m, int lane, bool& nan) {
  const unsigned long long thr = L[k - 1];
  const unsigned long long c0 = e_0 ? tk_entry(row[lane], (uint32_t)v0 + lane) : 0ull;
  const unsigned long long c1 = e_1 ? tk_entry(row[64 + lane], (uint32_t)v0 + 64 + lane) : 0ull;
  unsigned long long m0 = __ballot(c0 > thr), m1 = __ballot(c1 > thr);
  if (!(m0 | m1)) return;
  tk_clear_excluded(xn, xs, xl, excl_idx, v0, lane, m0, m1);
  if (!(m0 | m1)) return;
  const int32_t t0 = ((m0 >> lane) & 1) ? row_class[(int64_t)v0 + lane] : 0;           // (a set bit: the column is inside V)
  const int32_t t1 = ((m1 >> lane) & 1) ? row_class[(int64_t)v0 + 64 + lane] : 0;
  TkCapList S;
  S.load(L, row_class, k, lane);
  bool changed = S.take(c0, t0, m0, k, m, lane, nan);
  changed |= S.take(c1, t1, m1 & __ballot(c1 > S.kth(k)), k, m, lane, nan);
  if (changed) {
    if (lane < k) L[lane] = S.e;
    wave_lds_sync();
  }
}

// The capped selecting consumer: TkSelect's arrays, prologue and flush; only what a user does with a tile differs.
struct TkSelectCapped : TkSelect {
  TkCapFields F;
  __device__ __forceinline__ TkSelectCapped(unsigned char* p, int slots, int k_, const TkCapFields& f) : TkSelect(p, slots, k_), F(f) {}
  __device__ __forceinline__ void user(const float* row, int ul, const int64_t* excl_idx, int v0, bool e_0, bool e_1, int lane,
                                       bool& nan) const {
    tk_select_user_capped(row, lists + ul * k, xn + ul, xs + ul, xl + ul * TK_XCAP, excl_idx, F.row_class, v0, e_0, e_1, k, F.m, lane,
                          nan);
  }
};

__global__ __launch_bounds__(TK_THREADS) void tkcap_scores_kernel(TkWith<TkArgs, TkCapFields> A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char tk_smem[];
  TkDot P(tk_smem);
  TkSelectCapped C(P.rest, TK_BU, A.k, A);
  tk_walk(A, P, C);
}

// tk_merge_kernel under the cap (k <= 64): the same flags, the slices' lists merged by the capped insertion
__global__ __launch_bounds__(64) void tk_merge_capped_kernel(TkWith<TkArgs, TkCapFields> A) {
  const int64_t u = blockIdx.x;
  const int lane = threadIdx.x, k = A.k;
  int64_t s, n;
  const bool ok = tk_excl_range(A, u, s, n);
  TkCapList S;
  S.e = 0ull;
  S.tag = 0;
  if (!ok) {
    if (lane == 0) atomicOr(A.status, NRL_TOPK_E_OFFSETS);
  } else {
    int bad = 0;
    for (int64_t i = lane; i < n; i += 64) {
      const int64_t x = A.excl_idx[s + i];
      bad |= (x < 0 || x >= A.V);
    }
    if (__ballot(bad) && lane == 0) atomicOr(A.status, NRL_TOPK_E_EXCLUDE);
    const unsigned long long* P = A.partial + u * A.slices * k;
    const int64_t total = (int64_t)A.slices * k;
    bool nan = false;
    for (int64_t base = 0; base < total; base += 64) {
      const unsigned long long c = base + lane < total ? P[base + lane] : 0ull;
      const unsigned long long msk = __ballot(c > S.kth(k));
      if (!msk) continue;
      const int32_t t = ((msk >> lane) & 1) ? A.row_class[(uint32_t)~(uint32_t)c] : 0;
      S.take(c, t, msk, k, A.m, lane, nan);
    }
  }
  if (lane < k) {
    A.out_idx[u * k + lane] = S.e ? (int64_t)(uint32_t)~(uint32_t)S.e : -1;
    A.out_score[u * k + lane] = S.e ? tk_unkey((uint32_t)(S.e >> 32)) : -INFINITY;
  }
}

// ---- class-biased scores: the dot product plus a per-(user, class) additive term ------------------------------------------------------
// score(u, v) = fl32(dot(u, v) + bias[u, c]), c = bias_class[v]: the accumulator chain of TkDot, bit for bit, and then ONE fp32 add
// (never a further k step of the chain).  bias (B, S) fp32, S <= NRL_TOPK_MAX_BIAS_CLASSES; a class id outside [0, S) is scored
// with bias +0 and sets NRL_TOPK_E_CLASS.  The soft counterpart of the class cap above, and SentiDebias's combined score.
//   * the bias rows of the workgroup's 64 users are staged once, [TK_BU][ld] behind the score tile; column S of every row is +0 and
//     is where a bad class id points, so the add has no branch;
//   * per table tile the 128 class ids (already mapped into [0, S]) are staged behind them, and the add is done on the accumulator
//     fragments before they are stored: no second pass over the tile and no further barrier.  A lane reads, per fragment register,
//     bias[4 g + r][class of column l15]: within the 32 lanes a ds_read_b32 banks together that is two rows (g and g + 1) times up
//     to 16 classes; equal classes are one address (a broadcast), and ld = 4 (mod 8) puts the two rows 16 banks apart, so up to
//     16 classes never conflict and more can only where two columns' classes are 16 (other row) or 32 (same row) apart.
struct TkbFields {
  const float* bias;                           // (B, S)
  const int32_t* bias_class;                   // (V) the class of every table row, for the bias
  int32_t S;
};

constexpr int tkb_ld(int S) { return (S + 4) / 8 * 8 + 4; }                  // the smallest ld >= S + 1 with ld = 4 (mod 8)
constexpr size_t tkb_extra_lds(int S) { return (size_t)TK_BU * tkb_ld(S) * 4 + TK_BV * 4; }
static_assert(tkb_ld(1) == 4 && tkb_ld(3) == 4 && tkb_ld(4) == 12 && tkb_ld(19) == 20 && tkb_ld(NRL_TOPK_MAX_BIAS_CLASSES) == 68,
              "room for the zero column, 16 banks between rows 4 apart");
static_assert(tkb_extra_lds(1) % 16 == 0 && tkb_extra_lds(NRL_TOPK_MAX_BIAS_CLASSES) % 16 == 0 && (TK_BU * 8 * 4) % 16 == 0,
              "what follows the bias rows and the class ids is 16-byte aligned, for every S");
static_assert(tk_lds_bytes(1, TK_BU, NRL_TOPK_MAX_K) + tkb_extra_lds(NRL_TOPK_MAX_BIAS_CLASSES) <= 160 * 1024,
              "the largest layout fits the dynamic LDS the launch may request");

// the class of table row v as the add reads it: S (the zero column) for an id outside [0, S), which is flagged
__device__ __forceinline__ int tkb_class(const TkbFields& F, int64_t v, bool& bad) {
  const int32_t c = F.bias_class[v];
  bad = c < 0 || c >= F.S;
  return bad ? F.S : c;
}

// The producer of the class-biased kernels: TkDot's tile, every element with its (user, class) bias added once.
struct TkBiasProducer : TkBlocked {
  float* sc;                                   // [TK_BU][TK_SCLD]; until the scores exist, the operand tiles
  float* bl;                                   // [TK_BU][ld] the users' bias rows; column S (and the rows past B) +0
  int32_t* cl;                                 // [TK_BV] the tile's class ids in [0, S]
  unsigned char* rest;
  const TkbFields& F;
  int ld;
  const float* pa[1];
  bool ua_ok;
  __device__ __forceinline__ TkBiasProducer(unsigned char* p, const TkbFields& f)
      : sc(reinterpret_cast<float*>(p)), bl(sc + TK_BU * TK_SCLD), cl(reinterpret_cast<int32_t*>(bl + TK_BU * tkb_ld(f.S))),
        rest(p + TK_TILE_BYTES + tkb_extra_lds(f.S)), F(f), ld(tkb_ld(f.S)) {}
  __device__ __forceinline__ int slots() const { return TK_BU; }
  __device__ __forceinline__ void stage(const TkArgs& A, int64_t u0, int nu) {
    const int srow = threadIdx.x >> 2;
    ua_ok = srow < nu;
    pa[0] = A.user + (ua_ok ? u0 + srow : A.B - 1) * A.D;
    for (int i = threadIdx.x; i < TK_BU * ld; i += TK_THREADS) {             // (the consumer's prologue publishes the rows)
      const int ul = i / ld, c = i % ld;
      bl[i] = (ul < nu && c < F.S) ? F.bias[(u0 + ul) * F.S + c] : 0.f;
    }
  }
  __device__ __forceinline__ void tile(const TkArgs& A, int v0, int) const {
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid < TK_BV) {                                // (rows past V: any class, eligibility drops them)
      const int64_t v = (int64_t)v0 + tid;
      bool bad = false;
      cl[tid] = v < A.V ? tkb_class(F, v, bad) : F.S;
      if (__ballot(bad) && lane == 0) atomicOr(A.status, NRL_TOPK_E_CLASS);
    }
    tk_f32x4 acc[1][2][4];
    tk_tile_accumulate<1>(pa, ua_ok, A.table, A.D, v0, A.V, A.D, sc, acc);   // (its barriers publish `cl`)
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1, l15 = lane & 15, g = lane >> 4;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float* const b = bl + cl[wn * 64 + j * 16 + l15];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[0][i][j][r] = __fadd_rn(acc[0][i][j][r], b[(wm * 32 + i * 16 + 4 * g + r) * ld]);
    }
    tk_store_fragments(acc[0], sc);
    __syncthreads();
  }
  __device__ __forceinline__ const float* row(int ul) const { return sc + ul * TK_SCLD; }
  __device__ __forceinline__ bool skip(int) const { return false; }
};

__global__ __launch_bounds__(TK_THREADS) void tkb_scores_kernel(TkWith<TkArgs, TkbFields> A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char tk_smem[];
  TkBiasProducer P(tk_smem, A);
  TkSelect C(P.rest, TK_BU, A.k);
  tk_walk(A, P, C);
}

__global__ __launch_bounds__(TK_THREADS) void tkbcap_scores_kernel(TkWith<TkWith<TkArgs, TkbFields>, TkCapFields> A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char tk_smem[];
  TkBiasProducer P(tk_smem, A);
  TkSelectCapped C(P.rest, TK_BU, A.k, A);
  tk_walk(A, P, C);
}

// ---- multi-interest scores (MINER) ---------------------------------------------------------------------------------------------
// A user is K interest rows; a table row's score is an aggregate of the K dot products (ops_miner.SCORE_MODES: 0 max, 1 mean,
// 2 softmax-weighted by the K gate logits).  The row operand of the tile product is the (B * K, D) interest matrix: the 64 rows of
// a workgroup hold Ut = 64 / K whole users (rows from Ut * K on are zero and belong to nobody), and once the 64 x 128 tile of s_j
// is in LDS the K rows of every user are reduced per column, in ascending j, into the user's first row: the one stage that is
// this kernel's own.  The scan, the exclusion and the insertion then run over Ut users, and tk_merge_kernel finishes.
// GATE (mode 2) runs the gate rows as a second row operand against the SAME staged table tile into a second score tile.
struct TkiFields {                             // beside them `user` is the interests and B counts users
  const float* gate;
  int32_t K, Ut, mode;
};

// the aggregate of one user's K scores of one column (stride TK_SCLD apart); lg: the gate logits of the same positions
template <bool GATE>
__device__ __forceinline__ float tki_aggregate(const float* s, const float* lg, int K, int mode) {
  if constexpr (GATE) {
    float m = lg[0];
    for (int j = 1; j < K; ++j) m = fmaxf(m, lg[j * TK_SCLD]);
    float num = 0.f, den = 0.f;
    for (int j = 0; j < K; ++j) {              // a NaN logit, or inf - inf, makes e (and the score) NaN
      const float e = expf(__fsub_rn(lg[j * TK_SCLD], m));
      const float es = __fmul_rn(e, s[j * TK_SCLD]);
      num = j ? __fadd_rn(num, es) : es;
      den = j ? __fadd_rn(den, e) : e;
    }
    return num / den;
  }
  float a = s[0];
  if (mode == 0) {
    bool bad = a != a;
    for (int j = 1; j < K; ++j) {
      const float x = s[j * TK_SCLD];
      bad |= x != x;
      a = fmaxf(a, x);
    }
    return bad ? __uint_as_float(0x7FC00000u) : a;
  }
  for (int j = 1; j < K; ++j) a = __fadd_rn(a, s[j * TK_SCLD]);
  return a / (float)K;
}

// The tile producer of the multi-interest kernels (scores and count): the products of the staged interest (and gate) rows with the
// table tile at v0 into the score tile(s) from `sc` on, then the aggregation: the K rows of each of the tile's `nu` users, one column
// per thread, into the user's first row (nobody else reads or writes them).  Ends with the workgroup synchronised.
template <bool GATE>
__device__ __forceinline__ void tki_tile(const float* const (&pa)[GATE ? 2 : 1], bool ua_ok, const float* table, int v0, int V, int D,
                                         float* sc, int nu, int K, int mode) {
  const float* const lg = sc + TK_BU * TK_SCLD;
  tk_tile_product<GATE ? 2 : 1>(pa, ua_ok, table, v0, V, D, sc);
  for (int i = threadIdx.x; i < nu * TK_BV; i += TK_THREADS) {
    const int at = (i / TK_BV) * K * TK_SCLD + (i % TK_BV);
    sc[at] = tki_aggregate<GATE>(sc + at, lg + at, K, mode);
  }
  __syncthreads();
}

// The producer of the multi-interest kernels: tile row r is interest row u0 * K + r of the (B * K, D) matrix while r < nu * K, zero
// from there on; a user's scores are in the first of its K rows.
template <bool GATE>
struct TkiProducer : TkStrided {
  static constexpr int NA = GATE ? 2 : 1;
  float* sc;                                   // [TK_BU][TK_SCLD] the s_j; with a gate the l_j follow
  unsigned char* rest;
  const TkiFields& F;
  const float* pa[NA];
  bool ua_ok;
  __device__ __forceinline__ TkiProducer(unsigned char* p, const TkiFields& f)
      : sc(reinterpret_cast<float*>(p)), rest(p + NA * TK_TILE_BYTES), F(f) {}
  __device__ __forceinline__ int slots() const { return F.Ut; }
  __device__ __forceinline__ void stage(const TkArgs& A, int64_t u0, int nu) {
    const int srow = threadIdx.x >> 2;
    ua_ok = srow < nu * F.K;
    const int64_t ua = ua_ok ? u0 * F.K + srow : 0;
    pa[0] = A.user + ua * A.D;
    if constexpr (GATE) pa[1] = F.gate + ua * A.D;
  }
  __device__ __forceinline__ void tile(const TkArgs& A, int v0, int nu) const {
    tki_tile<GATE>(pa, ua_ok, A.table, v0, A.V, A.D, sc, nu, F.K, F.mode);
  }
  __device__ __forceinline__ const float* row(int ul) const { return sc + ul * F.K * TK_SCLD; }
  __device__ __forceinline__ bool skip(int) const { return false; }
};

template <bool GATE>
__global__ __launch_bounds__(TK_THREADS) void tki_scores_kernel(TkWith<TkArgs, TkiFields> A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char tk_smem[];
  TkiProducer<GATE> P(tk_smem, A);
  TkSelect C(P.rest, A.Ut, A.k);
  tk_walk(A, P, C);
}

// ---- z-scored ensemble scores (MANNeR) ------------------------------------------------------------------------------------------
// T <= 3 sub-models, each a (B, D) user matrix and a (V, D) table.  The score of (u, v) is sum_t w_t (s_t - mu_t[u]) / sd_t[u], where
// mu_t / sd_t are the mean and the unbiased standard deviation of s_t[u, .] over the user's population (eligible, inside V, not
// excluded, not NaN).  Two passes over the tables:
//   tke_stats_kernel   one workgroup per (tile of 64 users, statistics chunk): per t and table tile the tile product, then per user
//       the tile's (n, mean, M2) over the population, folded into the chunk's running moments by the pairwise update;
//   tke_finish_kernel  one wave per user folds the chunks in ascending order, writes (mean, sd), flags what cannot be standardised;
//   tke_scores_kernel  tk_scores_kernel with a second score tile that collects the weighted z-scores of the T products.
// The chunks depend on V alone (never on B or `slices`), so a user's statistics are a function of its rows, the tables, the mask,
// its exclusion set and V.
struct TkeFields {                             // beside them `user` / `table` are those of sub-model 0
  const float* users[NRL_TOPK_MAX_MODELS];
  const float* tables[NRL_TOPK_MAX_MODELS];
  float w[NRL_TOPK_MAX_MODELS];
  int32_t T, chunks, tiles_per_chunk;
  float* out_stats;                            // (B, T, 2): mean, sd
  float* moments;                              // (B, NRL_TOPK_STAT_CHUNKS, T, 3): n (int32 bits), mean, M2
};

__device__ __forceinline__ const float* tke_pick(const float* const (&p)[NRL_TOPK_MAX_MODELS], int t) {
  return t == 0 ? p[0] : (t == 1 ? p[1] : p[2]);
}

// (n, mean, M2) of b folded into a (Chan et al.); both sides non-empty
__device__ __forceinline__ void tke_fold(int& n, float& mean, float& m2, int nb, float mb, float m2b) {
  const int na = n;
  n = na + nb;
  const float d = __fsub_rn(mb, mean);
  mean = __fadd_rn(mean, __fdiv_rn(__fmul_rn(d, (float)nb), (float)n));
  m2 = __fadd_rn(__fadd_rn(m2, m2b), __fdiv_rn(__fmul_rn(__fmul_rn(__fmul_rn(d, d), (float)na), (float)nb), (float)n));
}

__global__ __launch_bounds__(TK_THREADS) void tke_stats_kernel(TkWith<TkArgs, TkeFields> A) {
  __shared__ __attribute__((aligned(16))) float sc[TK_BU * TK_SCLD];
  __shared__ int32_t xl[TK_BU * TK_XCAP];
  __shared__ int64_t xs[TK_BU];
  __shared__ int32_t xn[TK_BU];
  __shared__ uint8_t el[TK_BV];
  __shared__ int32_t mn[TK_BU * NRL_TOPK_MAX_MODELS];
  __shared__ float mm[TK_BU * NRL_TOPK_MAX_MODELS], m2[TK_BU * NRL_TOPK_MAX_MODELS];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int V = A.V, T = A.T;
  const int ch = (int)(blockIdx.x % (unsigned)A.chunks);
  const int64_t u0 = (int64_t)(blockIdx.x / (unsigned)A.chunks) * TK_BU;
  const int nu = A.B - u0 < TK_BU ? (int)(A.B - u0) : TK_BU;
  const int v_begin = ch * A.tiles_per_chunk * TK_BV;
  const int64_t v_stop = (int64_t)v_begin + (int64_t)A.tiles_per_chunk * TK_BV;
  const int v_end = v_stop < V ? (int)v_stop : V;
  const int nvt = (v_end - v_begin + TK_BV - 1) / TK_BV;

  for (int i = tid; i < TK_BU * NRL_TOPK_MAX_MODELS; i += TK_THREADS) {
    mn[i] = 0;
    mm[i] = 0.f;
    m2[i] = 0.f;
  }
  tk_cache_exclusions(A, u0, nu, TK_BU, xs, xn, xl);

  const int ul_begin = wave * TK_USERS_PER_WAVE, ul_end = ul_begin + TK_USERS_PER_WAVE < nu ? ul_begin + TK_USERS_PER_WAVE : nu;
  const int srow = tid >> 2;
  const bool ua_ok = srow < nu;
  bool nan = false;

  for (int t = 0; t < T; ++t) {
    const float* const pa[1] = {tke_pick(A.users, t) + (ua_ok ? u0 + srow : A.B - 1) * A.D};
    const float* const table = tke_pick(A.tables, t);
    for (int vt = 0; vt < nvt; ++vt) {
      const int v0 = v_begin + vt * TK_BV;
      tk_fill_eligible(A.eligible, v0, V, el);
      tk_tile_product<1>(pa, ua_ok, table, v0, V, A.D, sc);

      const bool e_0 = el[lane] != 0, e_1 = el[64 + lane] != 0;
      for (int ul = ul_begin; ul < ul_end; ++ul) {
        unsigned long long m0 = __ballot(e_0), m1 = __ballot(e_1);
        tk_clear_excluded(xn + ul, xs + ul, xl + ul * TK_XCAP, A.excl_idx, v0, lane, m0, m1);
        const float x0 = sc[ul * TK_SCLD + lane], x1 = sc[ul * TK_SCLD + 64 + lane];
        bool b0 = (m0 >> lane) & 1, b1 = (m1 >> lane) & 1;
        if (__ballot((b0 && x0 != x0) || (b1 && x1 != x1))) nan = true;
        b0 = b0 && x0 == x0;
        b1 = b1 && x1 == x1;
        const int nb = __popcll(__ballot(b0)) + __popcll(__ballot(b1));
        if (nb == 0) continue;
        const float mb = __fdiv_rn(wave_sum(__fadd_rn(b0 ? x0 : 0.f, b1 ? x1 : 0.f)), (float)nb);
        const float d0 = b0 ? __fsub_rn(x0, mb) : 0.f, d1 = b1 ? __fsub_rn(x1, mb) : 0.f;
        const float m2b = wave_sum(__fadd_rn(__fmul_rn(d0, d0), __fmul_rn(d1, d1)));
        const int at = ul * NRL_TOPK_MAX_MODELS + t;
        int n = mn[at];
        float mean = mm[at], M2 = m2[at];
        if (n == 0) {
          n = nb;
          mean = mb;
          M2 = m2b;
        } else {
          tke_fold(n, mean, M2, nb, mb, m2b);
        }
        if (lane == 0) {
          mn[at] = n;
          mm[at] = mean;
          m2[at] = M2;
        }
      }
      __syncthreads();                                // the score tile and `el` are free for the next tile's operands
    }
  }

  if (nan && lane == 0) atomicOr(A.status, NRL_TOPK_E_NAN);
  for (int i = tid; i < nu * T; i += TK_THREADS) {
    const int ul = i / T, t = i % T, at = ul * NRL_TOPK_MAX_MODELS + t;
    float* const o = A.moments + (((u0 + ul) * NRL_TOPK_STAT_CHUNKS + ch) * T + t) * 3;
    o[0] = __int_as_float(mn[at]);
    o[1] = mm[at];
    o[2] = m2[at];
  }
}

// a user's statistics can standardise: every sd positive and finite
__device__ __forceinline__ bool tke_sd_ok(float sd) { return sd > 0.f && sd < INFINITY; }

__global__ __launch_bounds__(64) void tke_finish_kernel(TkWith<TkArgs, TkeFields> A) {
  const int64_t u = blockIdx.x;
  const int lane = threadIdx.x, T = A.T;
  bool bad = false;
  if (lane < T) {
    int n = 0;
    float mean = 0.f, M2 = 0.f;
    for (int c = 0; c < A.chunks; ++c) {
      const float* const m = A.moments + ((u * NRL_TOPK_STAT_CHUNKS + c) * T + lane) * 3;
      const int nb = __float_as_int(m[0]);
      if (nb == 0) continue;
      if (n == 0) {
        n = nb;
        mean = m[1];
        M2 = m[2];
      } else {
        tke_fold(n, mean, M2, nb, m[1], m[2]);
      }
    }
    const float nanv = __uint_as_float(0x7FC00000u);
    const float sd = n >= 2 ? __fsqrt_rn(__fdiv_rn(M2, (float)(n - 1))) : nanv;
    A.out_stats[(u * T + lane) * 2] = n ? mean : nanv;
    A.out_stats[(u * T + lane) * 2 + 1] = sd;
    bad = !tke_sd_ok(sd);
  }
  if (__ballot(bad) && lane == 0) atomicOr(A.status, NRL_TOPK_E_STATS);
}

// One sub-model's share w ((s - mean) / sd) of an ensemble score, folded into `acc` (the first share starts the sum): every
// operation rounded to fp32 on its own.  Written once for the tile and for the target kernel, with contraction switched off: the
// __f*_rn intrinsics are plain operators, and where the product feeds the sum directly the compiler would otherwise fuse the two
// into an fma in one kernel and not in the other, one ulp apart.
__device__ __forceinline__ float tke_fold_z(float acc, bool first, float w, float s, float mean, float sd) {
#pragma clang fp contract(off)
  const float z = w * ((s - mean) / sd);
  return first ? z : acc + z;
}

// The tile producer of the ensemble kernels (scores and count): per sub-model t in ascending order the product of the staged rows
// `urow` of users[t] with the tile of tables[t] at v0 into `sc`, folded into the ensemble tile `zs` as w_t (s - mu_t) / sd_t with
// the workgroup's statistics st[TK_BU][T][2], one rounded operation at a time.  Ends with `zs` complete, `sc` free and the
// workgroup synchronised.
__device__ __forceinline__ void tke_tile(const float* const (&users)[NRL_TOPK_MAX_MODELS], const float* const (&tables)[NRL_TOPK_MAX_MODELS],
                                         const float (&wt)[NRL_TOPK_MAX_MODELS], int T, int64_t urow, bool ua_ok, int v0, int V, int D,
                                         float* sc, float* zs, const float* st) {
  const int tid = threadIdx.x;
  for (int t = 0; t < T; ++t) {
    const float* const pa[1] = {tke_pick(users, t) + urow * D};
    tk_tile_product<1>(pa, ua_ok, tke_pick(tables, t), v0, V, D, sc);
    const float w = t == 0 ? wt[0] : (t == 1 ? wt[1] : wt[2]);
    for (int i = tid; i < TK_BU * TK_BV; i += TK_THREADS) {
      const int ul = i / TK_BV, at = ul * TK_SCLD + (i % TK_BV);
      const float* const s2 = st + (ul * T + t) * 2;
      zs[at] = tke_fold_z(t ? zs[at] : 0.f, t == 0, w, sc[at], s2[0], s2[1]);
    }
    __syncthreads();                                  // the ensemble tile is complete; tile 0 is free for the next operands
  }
}

// The workgroup's copy st[TK_BU][T][2] of the (mean, sd) of its `nu` users from u0 on; a refused user (and a slot without one) is
// marked by sd = 0 in its first entry.  The caller's next barrier publishes it.
__device__ __forceinline__ void tke_stage_stats(const float* out_stats, int64_t u0, int nu, int T, float* st) {
  const int tid = threadIdx.x;
  if (tid < TK_BU) {
    bool ok = tid < nu;
    for (int t = 0; t < T; ++t) {
      const float mean = ok ? out_stats[((u0 + tid) * T + t) * 2] : 0.f, sd = ok ? out_stats[((u0 + tid) * T + t) * 2 + 1] : 1.f;
      st[(tid * T + t) * 2] = mean;
      st[(tid * T + t) * 2 + 1] = sd;
      ok = ok && tke_sd_ok(sd);
    }
    if (!ok) st[tid * T * 2 + 1] = 0.f;
  }
}

// The producer of the ensemble kernels: tile row r is user u0 + r of every sub-model, zero past the last; the raw tile, the ensemble
// tile a user's scores are read from, then the workgroup's statistics.  A user whose statistics cannot standardise is skipped: its
// list stays empty and the merge writes -1 / -inf; its counters stay 0, so the population comes out 0.
struct TkeProducer : TkBlocked {
  float* sc;                                   // [TK_BU][TK_SCLD] the raw scores of one table
  float* zs;                                   // [TK_BU][TK_SCLD] the ensemble scores
  float* st;                                   // [TK_BU][T][2] mean, sd; sd 0: the user is refused
  unsigned char* rest;
  const TkeFields& E;
  int64_t urow;
  bool ua_ok;
  __device__ __forceinline__ TkeProducer(unsigned char* p, const TkeFields& e)
      : sc(reinterpret_cast<float*>(p)), zs(sc + TK_BU * TK_SCLD), st(zs + TK_BU * TK_SCLD),
        rest(p + 2 * TK_TILE_BYTES + (size_t)TK_BU * e.T * 2 * 4), E(e) {}
  __device__ __forceinline__ int slots() const { return TK_BU; }
  __device__ __forceinline__ void stage(const TkArgs& A, int64_t u0, int nu) {
    tke_stage_stats(E.out_stats, u0, nu, E.T, st);
    const int srow = threadIdx.x >> 2;
    ua_ok = srow < nu;
    urow = ua_ok ? u0 + srow : A.B - 1;
  }
  __device__ __forceinline__ void tile(const TkArgs& A, int v0, int) const {
    tke_tile(E.users, E.tables, E.w, E.T, urow, ua_ok, v0, A.V, A.D, sc, zs, st);
  }
  __device__ __forceinline__ const float* row(int ul) const { return zs + ul * TK_SCLD; }
  __device__ __forceinline__ bool skip(int ul) const { return st[ul * E.T * 2 + 1] == 0.f; }
};

__global__ __launch_bounds__(TK_THREADS) void tke_scores_kernel(TkWith<TkArgs, TkeFields> A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char tk_smem[];
  TkeProducer P(tk_smem, A);
  TkSelect C(P.rest, TK_BU, A.k);
  tk_walk(A, P, C);
}

__global__ __launch_bounds__(TK_THREADS) void tkecap_scores_kernel(TkWith<TkWith<TkArgs, TkeFields>, TkCapFields> A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char tk_smem[];
  TkeProducer P(tk_smem, A);
  TkSelectCapped C(P.rest, TK_BU, A.k, A);
  tk_walk(A, P, C);
}

// ---- factored DNN scores (DKN) ---------------------------------------------------------------------------------------------------
// DKN's click predictor Linear(2 dim, Hd) -> ReLU -> Linear(Hd, 1) on [cand; user] with its first layer split by columns:
// score(u, v) = b2 + sum_j w2[j] relu(proj[v, j] + q[u, j]), proj (V, Hd) the catalogue's share and q (B, Hd) the user's with the
// bias (nrl_dkn_cand_project / nrl_dkn_user_query).  tk_scores_kernel with another tile producer: no GEMM, B V Hd add / select / fma.
//   * q of the workgroup's 64 users and w2 are staged once (row stride Hd rounded up to 4: a wave reads one user's q as 16-byte
//     broadcasts); per table tile the 128 proj rows, contiguous in memory, are staged into the LDS of the score tile with the
//     odd row stride Hd | 1: lane l reads rows l and 64 + l at the same j, 32 lanes of a ds_read_b32 group then hit 32 banks;
//   * wave w produces the scores of its own users 16 w ... 16 w + 15 (the ones it selects for): a lane holds 16 x 2 chains
//     s = b2; s = fmaf(w2[j], h_j, s) in ascending j, h_j = x < 0 ? 0 : x (a NaN x stays NaN), x = proj[v, j] + q[u, j];
//   * the proj tile is dead once every chain is complete; the scores overwrite it and the selection runs as everywhere.
struct TkrFields {                             // beside them `user` is q, `table` is proj, D is Hd
  const float* w2;
  const float* b2;
};

constexpr int tkr_ldp(int Hd) { return Hd | 1; }
constexpr int tkr_ldq(int Hd) { return (Hd + 3) & ~3; }
constexpr size_t tkr_extra_lds(int Hd) { return (size_t)(TK_BU + 1) * tkr_ldq(Hd) * 4; }      // q rows, then w2
static_assert(TK_BV * tkr_ldp(NRL_TOPK_MAX_HIDDEN) <= TK_BU * TK_SCLD, "the proj tile lives inside the score tile");
static_assert(tk_lds_bytes(1, TK_BU, NRL_TOPK_MAX_K) + tkr_extra_lds(NRL_TOPK_MAX_HIDDEN) <= 160 * 1024 &&
                  tkr_extra_lds(1) % 16 == 0 && tkr_extra_lds(NRL_TOPK_MAX_HIDDEN) % 16 == 0,
              "the largest layout fits; under the walk the q rows follow the score tile (16-byte aligned) and, whole float4s,"
              " keep the consumer's arrays aligned");

__device__ __forceinline__ float tkr_step(float w, float p, float q, float s) {
  const float x = __fadd_rn(p, q);
  return fmaf(w, x < 0.f ? 0.f : x, s);
}

// The tile producer of the DNN count kernel, in three pieces (tkr_scores_kernel has its own copy: below).
// q of the tile's `nu` users from u0 on and w2 into LDS: qs[TK_BU][ldq], zero past Hd and past the last user, then w2s[ldq]
__device__ __forceinline__ void tkr_stage_users(const float* q, const float* w2, int64_t u0, int nu, int Hd, float* qs, float* w2s) {
  const int tid = threadIdx.x, ldq = tkr_ldq(Hd);
  for (int i = tid; i < TK_BU * ldq; i += TK_THREADS) {
    const int ul = i / ldq, j = i - ul * ldq;
    qs[i] = (ul < nu && j < Hd) ? q[(u0 + ul) * Hd + j] : 0.f;
  }
  for (int i = tid; i < ldq; i += TK_THREADS) w2s[i] = i < Hd ? w2[i] : 0.f;
}

// a thread's staging walk over a proj tile: element e = tid, tid + 256, ... of the tile is column e % Hd of tile row e / Hd
struct TkrWalk {
  int row0, col0, drow, dcol;
};
__device__ __forceinline__ TkrWalk tkr_walk(int Hd) {
  const int tid = threadIdx.x, row0 = tid / Hd, drow = TK_THREADS / Hd;
  return TkrWalk{row0, tid - row0 * Hd, drow, TK_THREADS - drow * Hd};
}

// The scores of the wave's 16 users (tile rows ul_begin ...; `qw` their q rows) for the 128 proj rows from v0 on, left in the score
// tile `sc`, which holds the staged proj tile until every chain is complete.  Ends with the workgroup synchronised.
__device__ __forceinline__ void tkr_tile(const float* table, int v0, int V, int Hd, const TkrWalk& W, float* sc, const float* qw,
                                         const float* w2s, float b2, int ul_begin) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int ldp = tkr_ldp(Hd), ldq = tkr_ldq(Hd);
  const float* const p0 = sc + lane * ldp;                                   // this lane's two proj rows
  const float* const p1 = sc + (64 + lane) * ldp;
  {
    const float* const src = table + (int64_t)v0 * Hd;                       // the tile's rows are contiguous
    const int inside = (V - v0 < TK_BV ? V - v0 : TK_BV) * Hd;               // rows from V on are zero (and not eligible)
    int row = W.row0, col = W.col0;
    for (int e = tid; e < TK_BV * Hd; e += TK_THREADS) {
      sc[row * ldp + col] = e < inside ? src[e] : 0.f;
      row += W.drow;
      col += W.dcol;
      if (col >= Hd) {
        col -= Hd;
        ++row;
      }
    }
  }
  __syncthreads();

  float acc[TK_USERS_PER_WAVE][2];
#pragma unroll
  for (int u = 0; u < TK_USERS_PER_WAVE; ++u) acc[u][0] = acc[u][1] = b2;
  int j = 0;
  for (; j + 4 <= Hd; j += 4) {
    const float a0[4] = {p0[j], p0[j + 1], p0[j + 2], p0[j + 3]}, a1[4] = {p1[j], p1[j + 1], p1[j + 2], p1[j + 3]};
    const float4 w = *reinterpret_cast<const float4*>(w2s + j);
    const float wj[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int u = 0; u < TK_USERS_PER_WAVE; ++u) {
      const float4 q4 = *reinterpret_cast<const float4*>(qw + u * ldq + j);
      const float qj[4] = {q4.x, q4.y, q4.z, q4.w};
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        acc[u][0] = tkr_step(wj[t], a0[t], qj[t], acc[u][0]);
        acc[u][1] = tkr_step(wj[t], a1[t], qj[t], acc[u][1]);
      }
    }
  }
  for (; j < Hd; ++j) {
    const float a0 = p0[j], a1 = p1[j], w = w2s[j];
#pragma unroll
    for (int u = 0; u < TK_USERS_PER_WAVE; ++u) {
      const float q = qw[u * ldq + j];
      acc[u][0] = tkr_step(w, a0, q, acc[u][0]);
      acc[u][1] = tkr_step(w, a1, q, acc[u][1]);
    }
  }
  __syncthreads();                                    // every chain is complete: the proj tile gives way to the scores
#pragma unroll
  for (int u = 0; u < TK_USERS_PER_WAVE; ++u) {
    sc[(ul_begin + u) * TK_SCLD + lane] = acc[u][0];
    sc[(ul_begin + u) * TK_SCLD + 64 + lane] = acc[u][1];
  }
  __syncthreads();
}

// The producer of the DNN count kernel: the score tile, then the q rows of the tile's users and w2.  Blocked mapping, and it needs
// it: a wave computes the scores of the users it serves.
struct TkrProducer : TkBlocked {
  float* sc;                                   // [TK_BU][TK_SCLD]; before: proj tile [TK_BV][ldp]
  float* qs;                                   // [TK_BU][ldq], zero past Hd and past the last user
  float* w2s;                                  // [ldq]
  unsigned char* rest;
  const TkrFields& F;
  TkrWalk W;
  const float* qw;                             // the q rows of the users this wave serves, the first of which is ul_begin
  int ul_begin;
  float b2;
  __device__ __forceinline__ TkrProducer(unsigned char* p, const TkrFields& f, int Hd)
      : sc(reinterpret_cast<float*>(p)), qs(sc + TK_BU * TK_SCLD), w2s(qs + TK_BU * tkr_ldq(Hd)),
        rest(p + TK_TILE_BYTES + tkr_extra_lds(Hd)), F(f) {}
  __device__ __forceinline__ int slots() const { return TK_BU; }
  __device__ __forceinline__ void stage(const TkArgs& A, int64_t u0, int nu) {
    tkr_stage_users(A.user, F.w2, u0, nu, A.D, qs, w2s);
    b2 = F.b2[0];
    W = tkr_walk(A.D);
    ul_begin = first(__builtin_amdgcn_readfirstlane(threadIdx.x >> 6));
    qw = qs + ul_begin * tkr_ldq(A.D);
  }
  __device__ __forceinline__ void tile(const TkArgs& A, int v0, int) const {
    tkr_tile(A.table, v0, A.V, A.D, W, sc, qw, w2s, b2, ul_begin);
  }
  __device__ __forceinline__ const float* row(int ul) const { return sc + ul * TK_SCLD; }
  __device__ __forceinline__ bool skip(int) const { return false; }
};

// tkr_scores_kernel is the one walk kernel that is NOT an instantiation of tk_walk: it keeps its own text -- the skeleton, the slice
// range and DKN's tile producer inline -- and compiles to the instructions it always had.  DUPLICATED rather than shared: with this
// kernel going through TkrProducer (tkr_stage_users / tkr_walk / tkr_tile) the compiler scheduled its scalar code differently and
// the whole call measured 3 - 8 % slower at B = 512, V = 65,536, Hd = 16, as it had when the producer was first factored out
// (profiles/topk_walk_refactor_before_after.txt, profiles/topk_scores_refactor_before_after.txt).  Its LDS order is the earlier
// one too: lists after `el`, then q and w2 (tk_lds_bytes(1, TK_BU, 1) and TK_BU * 8 are multiples of 16, so the q rows are
// 16-byte aligned for every k).  The chain must stay that of tkr_tile, line for line:
// tests/test_gpu_catalogue_rank_scorers.py::test_consistency_with_topk_on_real_values compares the score bits of the two.
static_assert(tk_lds_bytes(1, TK_BU, 1) % 16 == 0 && (TK_BU * 8) % 16 == 0, "tkr_scores_kernel's q rows follow its lists, 16-byte aligned");
__global__ __launch_bounds__(TK_THREADS) void tkr_scores_kernel(TkWith<TkArgs, TkrFields> A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char tk_smem[];
  float* const sc = reinterpret_cast<float*>(tk_smem);                       // [TK_BU][TK_SCLD]; before: proj tile [TK_BV][ldp]
  int32_t* const xl = reinterpret_cast<int32_t*>(sc + TK_BU * TK_SCLD);      // [TK_BU][TK_XCAP]
  int64_t* const xs = reinterpret_cast<int64_t*>(xl + TK_BU * TK_XCAP);      // [TK_BU]
  int32_t* const xn = reinterpret_cast<int32_t*>(xs + TK_BU);                // [TK_BU]
  uint8_t* const el = reinterpret_cast<uint8_t*>(xn + TK_BU);                // [TK_BV]
  unsigned long long* const lists = reinterpret_cast<unsigned long long*>(el + TK_BV);      // [TK_BU][k]
  const int Hd = A.D, ldp = tkr_ldp(Hd), ldq = tkr_ldq(Hd);
  float* const qs = reinterpret_cast<float*>(lists + TK_BU * A.k);           // [TK_BU][ldq], zero past Hd and past the last user
  float* const w2s = qs + TK_BU * ldq;                                       // [ldq]

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int k = A.k, V = A.V;
  const int sl = (int)(blockIdx.x % (unsigned)A.slices);
  const int64_t u0 = (int64_t)(blockIdx.x / (unsigned)A.slices) * TK_BU;
  const int nu = A.B - u0 < TK_BU ? (int)(A.B - u0) : TK_BU;
  const int v_begin = sl * A.tiles_per_slice * TK_BV;
  const int64_t v_stop = (int64_t)v_begin + (int64_t)A.tiles_per_slice * TK_BV;
  const int v_end = v_stop < V ? (int)v_stop : V;
  const int nvt = (v_end - v_begin + TK_BV - 1) / TK_BV;

  for (int i = tid; i < TK_BU * k; i += TK_THREADS) lists[i] = 0ull;
  for (int i = tid; i < TK_BU * ldq; i += TK_THREADS) {
    const int ul = i / ldq, j = i - ul * ldq;
    qs[i] = (ul < nu && j < Hd) ? A.user[(u0 + ul) * Hd + j] : 0.f;
  }
  for (int i = tid; i < ldq; i += TK_THREADS) w2s[i] = i < Hd ? A.w2[i] : 0.f;
  const float b2 = A.b2[0];
  tk_cache_exclusions(A, u0, nu, TK_BU, xs, xn, xl);

  const int ul_begin = wave * TK_USERS_PER_WAVE, ul_end = ul_begin + TK_USERS_PER_WAVE < nu ? ul_begin + TK_USERS_PER_WAVE : nu;
  // staging walk: element e = tid, tid + 256, ... of the tile is column e % Hd of tile row e / Hd
  const int row0 = tid / Hd, col0 = tid - row0 * Hd, drow = TK_THREADS / Hd, dcol = TK_THREADS - drow * Hd;
  const float* const p0 = sc + lane * ldp;                                   // this lane's two proj rows
  const float* const p1 = sc + (64 + lane) * ldp;
  const float* const qw = qs + ul_begin * ldq;                               // this wave's 16 q rows
  bool nan = false;

  for (int vt = 0; vt < nvt; ++vt) {
    const int v0 = v_begin + vt * TK_BV;
    tk_fill_eligible(A.eligible, v0, V, el);
    {
      const float* const src = A.table + (int64_t)v0 * Hd;                   // the tile's rows are contiguous
      const int inside = (V - v0 < TK_BV ? V - v0 : TK_BV) * Hd;             // rows from V on are zero (and not eligible)
      int row = row0, col = col0;
      for (int e = tid; e < TK_BV * Hd; e += TK_THREADS) {
        sc[row * ldp + col] = e < inside ? src[e] : 0.f;
        row += drow;
        col += dcol;
        if (col >= Hd) {
          col -= Hd;
          ++row;
        }
      }
    }
    __syncthreads();

    float acc[TK_USERS_PER_WAVE][2];
#pragma unroll
    for (int u = 0; u < TK_USERS_PER_WAVE; ++u) acc[u][0] = acc[u][1] = b2;
    int j = 0;
    for (; j + 4 <= Hd; j += 4) {
      const float a0[4] = {p0[j], p0[j + 1], p0[j + 2], p0[j + 3]}, a1[4] = {p1[j], p1[j + 1], p1[j + 2], p1[j + 3]};
      const float4 w = *reinterpret_cast<const float4*>(w2s + j);
      const float wj[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
      for (int u = 0; u < TK_USERS_PER_WAVE; ++u) {
        const float4 q4 = *reinterpret_cast<const float4*>(qw + u * ldq + j);
        const float qj[4] = {q4.x, q4.y, q4.z, q4.w};
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          acc[u][0] = tkr_step(wj[t], a0[t], qj[t], acc[u][0]);
          acc[u][1] = tkr_step(wj[t], a1[t], qj[t], acc[u][1]);
        }
      }
    }
    for (; j < Hd; ++j) {
      const float a0 = p0[j], a1 = p1[j], w = w2s[j];
#pragma unroll
      for (int u = 0; u < TK_USERS_PER_WAVE; ++u) {
        const float q = qw[u * ldq + j];
        acc[u][0] = tkr_step(w, a0, q, acc[u][0]);
        acc[u][1] = tkr_step(w, a1, q, acc[u][1]);
      }
    }
    __syncthreads();                                  // every chain is complete: the proj tile gives way to the scores
#pragma unroll
    for (int u = 0; u < TK_USERS_PER_WAVE; ++u) {
      sc[(ul_begin + u) * TK_SCLD + lane] = acc[u][0];
      sc[(ul_begin + u) * TK_SCLD + 64 + lane] = acc[u][1];
    }
    __syncthreads();

    const bool e_0 = el[lane] != 0, e_1 = el[64 + lane] != 0;
    for (int ul = ul_begin; ul < ul_end; ++ul)
      tk_select_user(sc + ul * TK_SCLD, lists + ul * k, xn + ul, xs + ul, xl + ul * TK_XCAP, A.excl_idx, v0, e_0, e_1, k, lane, nan);
    __syncthreads();                                  // the score tile and `el` are free for the next proj tile
  }

  if (nan && lane == 0) atomicOr(A.status, NRL_TOPK_E_NAN);
  wave_lds_sync();
  for (int ul = ul_begin; ul < ul_end; ++ul) tk_flush_user(lists + ul * k, A.partial + ((u0 + ul) * A.slices + sl) * k, k, lane);
}

// ---- personalized-pooling scores (NPA) --------------------------------------------------------------------------------------------
// NPA's eval-mode score from the cached conv feature maps c (V, L, F): with a[u, v, t] = c[v, t] . q[u] (q the user's tanh'd text
// query) and s[u, v, t] = c[v, t] . user[u], score(u, v) = sum_t softmax_t(a[u, v, :])[t] s[u, v, t]: the dot product of the user
// vector with the news vector pooled by the user's own attention, without forming the pooled vector.  tk_scores_kernel with
// another tile producer:
//   * tokens t = 0 ... L - 1 in ascending order; per token ONE pass of tk_tile_accumulate<2> with the row operands q and user over
//     the table rows features + (v L + t) F (row stride L F, depth F), so a and s of a position come out of the same staged tile;
//   * the two accumulator fragments stay in registers, 32 (u, v) positions per thread, and are folded into an online-softmax
//     state (m, l, o) per position: m' = max(m, a); r = exp(m - m'); p = exp(a - m'); l = l r + p; o = o r + p s, with the
//     exponential of npa_cached_pool.  A NaN logit leaves m alone (fmaxf) and makes p, hence l and o, NaN; so does inf - inf;
//   * after the last token o / l goes to the score tile and the selection runs as everywhere.
// LDS: the three operand tiles (38 KB) take the place of the one score tile (33 KB) of tk_lds_bytes(1, ...), so two workgroups
// fit a CU up to k = 50; (B, V, L) is never written.  Registers: 32 positions x (2 accumulators + 3 state) and the staging; the
// second launch bound holds the compiler to two waves per SIMD (231 VGPRs, no scratch; without it 269 and one wave: a quarter slower).
struct TkpFields {                             // beside them `user` is q, `table` the feature maps, D is F
  const float* uvec;
  int32_t L;
};

constexpr int TKP_OPERAND_FLOATS = 2 * TK_BK * (2 * TK_LDA + TK_LDB);
constexpr size_t TKP_EXTRA_LDS = (size_t)(TKP_OPERAND_FLOATS - TK_BU * TK_SCLD) * 4;
static_assert(TKP_OPERAND_FLOATS >= TK_BU * TK_SCLD && TKP_EXTRA_LDS % 16 == 0, "the score tile lives inside the operand tiles");
static_assert(tk_lds_bytes(1, TK_BU, NRL_TOPK_MAX_K) + TKP_EXTRA_LDS <= 160 * 1024, "the largest layout fits");

// The tile producer of the pooling kernels (scores, count and target): per token one pass of tk_tile_accumulate<2> with the row
// operands q (pa[0]) and user (pa[1]) over the feature maps, folded into the online softmax in registers; o / l is left in the
// score tile `sc`, which holds the operand tiles until then.  ROWS / rows / table_rows as for tk_tile_accumulate.  Ends with the
// workgroup synchronised.
template <bool ROWS>
__device__ __forceinline__ void tkp_tile(const float* const (&pa)[2], bool ua_ok, const float* table, int64_t ldt, int v0, int V, int L,
                                         int F, float* sc, const int64_t* rows = nullptr, int64_t table_rows = 0) {
  tk_f32x4 m[2][4], l[2][4], o[2][4];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      m[i][j] = tk_f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
      l[i][j] = o[i][j] = tk_f32x4{0.f, 0.f, 0.f, 0.f};
    }
  for (int t = 0; t < L; ++t) {
    tk_f32x4 acc[2][2][4];                          // [0]: the logits a, [1]: the values s
    tk_tile_accumulate<2, ROWS>(pa, ua_ok, table + (int64_t)t * F, ldt, v0, V, F, sc, acc, rows, table_rows);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float a = acc[0][i][j][r], mo = m[i][j][r];
          const float mn = fmaxf(mo, a);            // a NaN logit leaves the maximum alone and arrives through p
          const float keep = __expf(mo - mn), p = __expf(a - mn);
          l[i][j][r] = fmaf(l[i][j][r], keep, p);
          o[i][j][r] = fmaf(o[i][j][r], keep, __fmul_rn(p, acc[1][i][j][r]));
          m[i][j][r] = mn;
        }
  }
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) o[i][j][r] = __fdiv_rn(o[i][j][r], l[i][j][r]);
  tk_store_fragments(o, sc);                        // (the last pass ended synchronised: the operand tiles are dead)
  __syncthreads();
}

// The producer of the pooling kernels: tile row r is (q, user) of user u0 + r, zero past the last user; the three operand tiles,
// of which the score tile takes the place once the last token is folded.
struct TkpProducer : TkBlocked {
  float* sc;                                   // operand tiles; afterwards [TK_BU][TK_SCLD] scores
  unsigned char* rest;
  const TkpFields& F;
  const float* pa[2];
  bool ua_ok;
  __device__ __forceinline__ TkpProducer(unsigned char* p, const TkpFields& f)
      : sc(reinterpret_cast<float*>(p)), rest(p + (size_t)TKP_OPERAND_FLOATS * 4), F(f) {}
  __device__ __forceinline__ int slots() const { return TK_BU; }
  __device__ __forceinline__ void stage(const TkArgs& A, int64_t u0, int nu) {
    const int srow = threadIdx.x >> 2;
    ua_ok = srow < nu;
    const int64_t ua = (ua_ok ? u0 + srow : A.B - 1) * A.D;
    pa[0] = A.user + ua;
    pa[1] = F.uvec + ua;
  }
  __device__ __forceinline__ void tile(const TkArgs& A, int v0, int) const {
    tkp_tile<false>(pa, ua_ok, A.table, (int64_t)F.L * A.D, v0, A.V, F.L, A.D, sc);
  }
  __device__ __forceinline__ const float* row(int ul) const { return sc + ul * TK_SCLD; }
  __device__ __forceinline__ bool skip(int) const { return false; }
};

__global__ __launch_bounds__(TK_THREADS, 2) void tkp_scores_kernel(TkWith<TkArgs, TkpFields> A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char tk_smem[];
  TkpProducer P(tk_smem, A);
  TkSelect C(P.rest, TK_BU, A.k);
  tk_walk(A, P, C);
}

// ---- full-catalogue rank of held-out rows ------------------------------------------------------------------------------------------
// The consumer that counts instead of selects: for a ragged per-user list of target rows (the held-out clicks), 1 + the number of
// rows of the user's population (eligible, inside V, not excluded, not NaN) whose entry is above the target's, and the population.
//   tkc_init_kernel     one wave per target slot: blanks the slot's outputs and owner and gathers the target's table row into a
//       (n_targets, D) workspace table (zeros for a row outside V);
//   tkc_owner_kernel    one thread per user: a user whose target range is sound claims its slots (ranges can overlap only where the
//       offsets decrease somewhere; the later user then owns the slot);
//   tkc_target_kernel   one workgroup per 64 slots: the tile product of the owners' user rows (row operand, by pointer) with the
//       gathered rows; slot j's score is the tile's diagonal -- the bits tk_scores_kernel computes for that (user, row);
//   tkc_count_kernel    tk_scores_kernel's walk with another consumer: per (user, table tile) the entries, the exclusion sweep, the
//       NaN drop, then popc of the survivors into the user's population counter and, per target, popc of `entry > target entry`;
//   tkc_finish_kernel   one wave per user: status flags, the sum over the slices, each target's validity, the outputs.
// Counts are integers: nothing depends on the order of any sum.
struct TkcArgs : TkArgs {                      // k, partial and out_idx are unused
  const int64_t* tgt_idx;
  const int64_t* tgt_off;
  int64_t n_targets;
  float* gathered;                             // (n_targets, D)
  float* tscore;                               // (n_targets)
  int32_t* owner;                              // (n_targets): the user that owns the slot, -1 none
  int32_t* pcnt;                               // (B, slices) population per slice
  int32_t* tcnt;                               // (n_targets, slices) rows above the target per slice
  int32_t* out_rank;
  int32_t* out_ranked;
};

constexpr int TKC_T = NRL_RANK_MAX_TARGETS;
constexpr int TKC_CLD = TKC_T + 1;             // a user's counters: one per target, then the population

// The LDS a count kernel keeps beside its score tiles, for a tile of `slots` users (TK_BU, or the whole users of a multi-interest
// tile): the exclusion cache and the eligibility bytes of the scores kernels, then what the counting consumer owns.  8-byte
// members first, so any `slots` keeps every member aligned; `p` is 8-byte aligned.
struct TkcLds {
  unsigned long long* te;                      // [slots][TKC_T] target entries
  int64_t* xs;                                 // [slots] exclusion cache: start
  int64_t* ts;                                 // [slots] first target slot
  int32_t* xl;                                 // [slots][TK_XCAP] exclusion cache: first rows
  int32_t* xn;                                 // [slots] exclusion cache: length
  int32_t* cnt;                                // [slots][TKC_CLD] counters
  int32_t* tn;                                 // [slots] target slots (0: none, or a bad range)
  uint8_t* el;                                 // [TK_BV]
  __device__ __forceinline__ TkcLds(unsigned char* p, int slots) {
    te = reinterpret_cast<unsigned long long*>(p);
    xs = reinterpret_cast<int64_t*>(te + slots * TKC_T);
    ts = xs + slots;
    xl = reinterpret_cast<int32_t*>(ts + slots);
    xn = xl + slots * TK_XCAP;
    cnt = xn + slots;
    tn = cnt + slots * TKC_CLD;
    el = reinterpret_cast<uint8_t*>(tn + slots);
  }
};
constexpr size_t tkc_lds_bytes(int slots) {
  return (size_t)slots * (TKC_T * 8 + 8 + 8 + TK_XCAP * 4 + 4 + TKC_CLD * 4 + 4) + TK_BV;
}
// dynamic LDS of tkc_count_kernel: score tile, then the layout above (33 KB + 41.9 KB)
constexpr size_t TKC_LDS = TK_TILE_BYTES + tkc_lds_bytes(TK_BU);
static_assert(2 * TKC_LDS <= 160 * 1024, "two workgroups of the count kernel fit a CU");

// a user's target range: false when the offsets decrease, leave [0, n_targets] or span more than TKC_T slots
__device__ __forceinline__ bool tkc_tgt_range(const TkcArgs& A, int64_t u, int64_t& s, int& n) {
  s = 0;
  n = 0;
  if (!A.tgt_off) return true;
  const int64_t a = A.tgt_off[u], b = A.tgt_off[u + 1];
  if (a < 0 || b < a || b > A.n_targets || b - a > TKC_T) return false;
  s = a;
  n = (int)(b - a);
  return true;
}

// ---- the counting consumer: what a count kernel runs where a scores kernel runs tk_select_user / tk_flush_user -------------------
// Prologue, by the workgroup, for the tile's `nu` users from u0 on: zero counters, target ranges, the exclusion cache, and every
// slot's entry -- ~0 (above every entry: it counts nothing) where the user does not own the slot or the row is outside V.  Ends
// with the workgroup synchronised.
__device__ __forceinline__ void tkc_prologue(const TkcArgs& A, int64_t u0, int nu, int slots, const TkcLds& S) {
  const int tid = threadIdx.x;
  for (int i = tid; i < slots * TKC_CLD; i += TK_THREADS) S.cnt[i] = 0;
  if (tid < slots) {
    int64_t s = 0;
    int n = 0;
    if (tid < nu && !tkc_tgt_range(A, u0 + tid, s, n)) n = 0;                // the finish kernel flags and blanks such a user
    S.ts[tid] = s;
    S.tn[tid] = n;
  }
  tk_cache_exclusions(A, u0, nu, slots, S.xs, S.xn, S.xl);                   // (its barrier also publishes `cnt`, `ts` and `tn`)
  for (int i = tid; i < slots * TKC_T; i += TK_THREADS) {
    const int ul = i / TKC_T, t = i % TKC_T;
    unsigned long long e = ~0ull;
    if (t < S.tn[ul]) {
      const int64_t j = S.ts[ul] + t, row = A.tgt_idx[j];
      if (A.owner[j] == (int32_t)(u0 + ul) && row >= 0 && row < A.V) e = tk_entry(A.tscore[j], (uint32_t)row);
    }
    S.te[i] = e;
  }
  __syncthreads();
}

// One user (slot `ul` of the tile) against one table tile, by the wave that owns the user: `row` the user's 128 scores, e_0 / e_1
// the lane's eligibility of columns lane and 64 + lane.  Entries, the exclusion sweep, the NaN drop (flagged), then popc of the
// survivors into the population counter and, per target, popc of `entry > target entry`: one LDS update per user and tile.
__device__ __forceinline__ void tkc_count_user(const float* row, const TkcLds& S, int ul, const int64_t* excl_idx, int v0, bool e_0,
                                               bool e_1, int lane, bool& nan) {
  unsigned long long c0 = e_0 ? tk_entry(row[lane], (uint32_t)v0 + lane) : 0ull;
  unsigned long long c1 = e_1 ? tk_entry(row[64 + lane], (uint32_t)v0 + 64 + lane) : 0ull;
  unsigned long long m0 = __ballot(e_0), m1 = __ballot(e_1);
  tk_clear_excluded(S.xn + ul, S.xs + ul, S.xl + ul * TK_XCAP, excl_idx, v0, lane, m0, m1);
  const unsigned long long n0 = m0 & __ballot((uint32_t)(c0 >> 32) == 0xFFFFFFFFu), n1 = m1 & __ballot((uint32_t)(c1 >> 32) == 0xFFFFFFFFu);
  if (n0 | n1) nan = true;                            // a NaN score of a row of the population: flagged and left out
  m0 &= ~n0;
  m1 &= ~n1;
  if (!((m0 >> lane) & 1)) c0 = 0ull;
  if (!((m1 >> lane) & 1)) c1 = 0ull;
  // lane t collects target t's count, lane TKC_T the population
  int add = lane == TKC_T ? __popcll(m0) + __popcll(m1) : 0;
  const int nt = S.tn[ul];
  for (int t = 0; t < nt; ++t) {
    const unsigned long long e = S.te[ul * TKC_T + t];        // wave-uniform
    const int above = __popcll(__ballot(c0 > e)) + __popcll(__ballot(c1 > e));
    if (lane == t) add = above;
  }
  if (lane < nt || lane == TKC_T) S.cnt[ul * TKC_CLD + lane] += add;
}

// Epilogue of user u (slot `ul` of the tile) by the wave that owns it: the slice's population and the counts of the slots it owns
__device__ __forceinline__ void tkc_flush_user(const TkcArgs& A, const TkcLds& S, int ul, int64_t u, int sl, int lane) {
  if (lane == TKC_T) A.pcnt[u * A.slices + sl] = S.cnt[ul * TKC_CLD + TKC_T];
  if (lane < S.tn[ul] && S.te[ul * TKC_T + lane] != ~0ull) A.tcnt[(S.ts[ul] + lane) * A.slices + sl] = S.cnt[ul * TKC_CLD + lane];
}

// the counting consumer of the walk
struct TkCount {
  const TkcLds S;
  uint8_t* el;
  __device__ __forceinline__ TkCount(unsigned char* p, int slots) : S(p, slots), el(S.el) {}
  __device__ __forceinline__ void prologue(const TkcArgs& A, int64_t u0, int nu, int slots) const { tkc_prologue(A, u0, nu, slots, S); }
  __device__ __forceinline__ void user(const float* row, int ul, const int64_t* excl_idx, int v0, bool e_0, bool e_1, int lane,
                                       bool& nan) const {
    tkc_count_user(row, S, ul, excl_idx, v0, e_0, e_1, lane, nan);
  }
  __device__ __forceinline__ void flush(const TkcArgs& A, int ul, int64_t u, int sl, int lane) const {
    tkc_flush_user(A, S, ul, u, sl, lane);
  }
};

__global__ __launch_bounds__(64) void tkc_init_kernel(TkcArgs A) {
  const int64_t j = blockIdx.x;
  const int lane = threadIdx.x;
  const int64_t row = A.tgt_idx[j];
  const bool ok = row >= 0 && row < A.V;
  if (lane == 0) {
    A.owner[j] = -1;
    A.out_rank[j] = 0;
    A.out_score[j] = -INFINITY;
  }
  if (!A.gathered) return;                            // (a scorer whose target scores read the table in place)
  const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int c = lane * 4; c < A.D; c += 256) st4(A.gathered + j * A.D + c, ok ? ld4(A.table + row * A.D + c) : z);
}

__global__ __launch_bounds__(256) void tkc_owner_kernel(TkcArgs A) {
  const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (u >= A.B) return;
  int64_t s;
  int n;
  if (!tkc_tgt_range(A, u, s, n)) return;
  for (int t = 0; t < n; ++t) atomicMax(A.owner + s + t, (int32_t)u);
}

__global__ __launch_bounds__(TK_THREADS) void tkc_target_kernel(TkcArgs A) {
  __shared__ __attribute__((aligned(16))) float sc[TK_BU * TK_SCLD];
  const int tid = threadIdx.x;
  const int64_t j0 = (int64_t)blockIdx.x * TK_BU;
  // staging: tile row r is the user row of the owner of slot j0 + r, zero where nobody owns it; the table tile starts at the
  // gathered row j0, so slot j0 + r is column r
  const int srow = tid >> 2;
  const int own = j0 + srow < A.n_targets ? A.owner[j0 + srow] : -1;
  const bool ua_ok = own >= 0;
  const float* const pa[1] = {A.user + (int64_t)(ua_ok ? own : 0) * A.D};
  tk_tile_product<1>(pa, ua_ok, A.gathered, (int)j0, (int)A.n_targets, A.D, sc);
  if (tid < TK_BU && j0 + tid < A.n_targets) A.tscore[j0 + tid] = sc[tid * TK_SCLD + tid];
}

__global__ __launch_bounds__(TK_THREADS) void tkc_count_kernel(TkcArgs A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char tk_smem[];
  TkDot P(tk_smem);
  TkCount C(P.rest, TK_BU);
  tk_walk(A, P, C);
}

// ---- the count walk under the other scorers ------------------------------------------------------------------------------------------
// Each is the walk under its scorer's producer -- the one its scores kernel runs, so a score's bits cannot differ between the
// top-k list and the rank -- with the counting consumer, and a target kernel that computes the slots' scores by the same chain.

// The class bias.  The score tile, the bias rows and class ids, then the consumer's arrays: 74.9 KB + 1.5 KB (S <= 3) ... 17.5 KB.
static_assert(TKC_LDS + tkb_extra_lds(NRL_TOPK_MAX_BIAS_CLASSES) <= 160 * 1024, "the biased count kernel's largest layout fits");
static_assert(2 * (TKC_LDS + tkb_extra_lds(8)) <= 160 * 1024, "up to 8 classes two workgroups of it fit a CU");

// tkc_target_kernel, then the one add of the producer: slot j's score is the diagonal plus bias[owner, class of the target row]
__global__ __launch_bounds__(TK_THREADS) void tkbc_target_kernel(TkWith<TkcArgs, TkbFields> A) {
  __shared__ __attribute__((aligned(16))) float sc[TK_BU * TK_SCLD];
  const int tid = threadIdx.x;
  const int64_t j0 = (int64_t)blockIdx.x * TK_BU;
  const int srow = tid >> 2;
  const int own = j0 + srow < A.n_targets ? A.owner[j0 + srow] : -1;
  const bool ua_ok = own >= 0;
  const float* const pa[1] = {A.user + (int64_t)(ua_ok ? own : 0) * A.D};
  tk_tile_product<1>(pa, ua_ok, A.gathered, (int)j0, (int)A.n_targets, A.D, sc);
  if (tid < TK_BU && j0 + tid < A.n_targets) {
    // (its own staging row is another slot's: the owner is read again.  The walk flags a bad class id of any row inside V.)
    const int jown = A.owner[j0 + tid];
    const int64_t row = A.tgt_idx[j0 + tid];
    float b = 0.f;
    if (jown >= 0 && row >= 0 && row < A.V) {
      bool bad;
      const int c = tkb_class(A, row, bad);
      if (!bad) b = A.bias[(int64_t)jown * A.S + c];
    }
    A.tscore[j0 + tid] = __fadd_rn(sc[tid * TK_SCLD + tid], b);
  }
}

__global__ __launch_bounds__(TK_THREADS) void tkbc_count_kernel(TkWith<TkcArgs, TkbFields> A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char tk_smem[];
  TkBiasProducer P(tk_smem, A);
  TkCount C(P.rest, TK_BU);
  tk_walk(A, P, C);
}

// MINER.  A workgroup holds Ut = 64 / K users, so the consumer's arrays are [Ut][...].
constexpr size_t tkic_lds_bytes(bool gate, int Ut) { return (gate ? 2 : 1) * TK_TILE_BYTES + tkc_lds_bytes(Ut); }
static_assert(2 * tkic_lds_bytes(false, TK_BU) <= 160 * 1024, "max / mean: two workgroups of the interest count kernel fit a CU");
static_assert(tkic_lds_bytes(true, TK_BU) <= 160 * 1024, "weighted: the second score tile leaves room for one workgroup per CU");

// One workgroup per Ut slots from j0 on: tile rows i K ... i K + K - 1 are the K interest (and gate) rows of the owner of slot
// j0 + i, the table tile is the gathered target rows from j0 on, so slot j0 + i's K products are column i of those rows; the
// aggregate over them is the score tki_scores_kernel computes for that (user, row).  K = 1: tkc_target_kernel.
template <bool GATE>
__global__ __launch_bounds__(TK_THREADS) void tkic_target_kernel(TkWith<TkcArgs, TkiFields> A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char tk_smem[];
  constexpr int NA = GATE ? 2 : 1;
  float* const sc = reinterpret_cast<float*>(tk_smem);                       // [TK_BU][TK_SCLD] the s_j; with a gate the l_j follow
  const float* const lg = sc + TK_BU * TK_SCLD;
  const int tid = threadIdx.x, K = A.K, Ut = A.Ut;
  const int64_t j0 = (int64_t)blockIdx.x * Ut;
  const int srow = tid >> 2, i = srow / K;
  const int own = (i < Ut && j0 + i < A.n_targets) ? A.owner[j0 + i] : -1;
  const bool ua_ok = own >= 0;
  const int64_t ua = ua_ok ? (int64_t)own * K + (srow - i * K) : 0;
  const float* pa[NA];
  pa[0] = A.user + ua * A.D;
  if constexpr (GATE) pa[1] = A.gate + ua * A.D;
  tk_tile_product<NA>(pa, ua_ok, A.gathered, (int)j0, (int)A.n_targets, A.D, sc);
  if (tid < Ut && j0 + tid < A.n_targets) {
    const int at = tid * K * TK_SCLD + tid;
    A.tscore[j0 + tid] = tki_aggregate<GATE>(sc + at, lg + at, K, A.mode);
  }
}

template <bool GATE>
__global__ __launch_bounds__(TK_THREADS) void tkic_count_kernel(TkWith<TkcArgs, TkiFields> A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char tk_smem[];
  TkiProducer<GATE> P(tk_smem, A);
  TkCount C(P.rest, A.Ut);
  tk_walk(A, P, C);
}

// DKN.  The q rows and w2 follow the score tile (16-byte aligned), then the consumer's arrays.
constexpr size_t tkrc_lds_bytes(int Hd) { return TK_TILE_BYTES + tkr_extra_lds(Hd) + tkc_lds_bytes(TK_BU); }
static_assert(tkrc_lds_bytes(NRL_TOPK_MAX_HIDDEN) <= 160 * 1024 && 2 * tkrc_lds_bytes(20) <= 160 * 1024,
              "the largest layout fits (91.1 KB at Hd = 64: one workgroup per CU); two workgroups fit a CU up to Hd = 20");

// one thread per slot: the chain of tkr_tile for (owner, target row), read in place -- no gather, no tile
__global__ __launch_bounds__(256) void tkrc_target_kernel(TkWith<TkcArgs, TkrFields> A) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= A.n_targets) return;
  const int own = A.owner[j], Hd = A.D;
  const int64_t row = A.tgt_idx[j];
  float s = 0.f;
  if (own >= 0 && row >= 0 && row < A.V) {
    const float* const p = A.table + row * Hd;
    const float* const q = A.user + (int64_t)own * Hd;
    s = A.b2[0];
    for (int c = 0; c < Hd; ++c) s = tkr_step(A.w2[c], p[c], q[c], s);
  }
  A.tscore[j] = s;
}

__global__ __launch_bounds__(TK_THREADS) void tkrc_count_kernel(TkWith<TkcArgs, TkrFields> A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char tk_smem[];
  TkrProducer P(tk_smem, A, A.D);
  TkCount C(P.rest, TK_BU);
  tk_walk(A, P, C);
}

// NPA.  The operand tiles (38 KB) and the consumer's arrays (41.9 KB) are 79.9 KB: two workgroups fit a CU with all
// NRL_RANK_MAX_TARGETS targets.
constexpr size_t TKPC_LDS = (size_t)TKP_OPERAND_FLOATS * 4 + tkc_lds_bytes(TK_BU);
static_assert(((size_t)TKP_OPERAND_FLOATS * 4) % 16 == 0 && 2 * TKPC_LDS <= 160 * 1024,
              "two workgroups of the pooled count kernel fit a CU (under 80 KB each)");

// One workgroup per 64 slots from j0 on: tile row r is (q, user) of the owner of slot j0 + r, tile column c the feature map of
// target row tgt_idx[j0 + c], read in place (nothing is gathered: a map is L F floats); slot j0 + r's score is the diagonal.
__global__ __launch_bounds__(TK_THREADS, 2) void tkpc_target_kernel(TkWith<TkcArgs, TkpFields> A) {
  __shared__ __attribute__((aligned(16))) float sc[TKP_OPERAND_FLOATS];
  const int tid = threadIdx.x, F = A.D;
  const int64_t j0 = (int64_t)blockIdx.x * TK_BU;
  const int srow = tid >> 2;
  const int own = j0 + srow < A.n_targets ? A.owner[j0 + srow] : -1;
  const bool ua_ok = own >= 0;
  const int64_t ua = (int64_t)(ua_ok ? own : 0) * F;
  const float* const pa[2] = {A.user + ua, A.uvec + ua};
  tkp_tile<true>(pa, ua_ok, A.table, (int64_t)A.L * F, (int)j0, (int)A.n_targets, A.L, F, sc, A.tgt_idx, A.V);
  if (tid < TK_BU && j0 + tid < A.n_targets) A.tscore[j0 + tid] = sc[tid * TK_SCLD + tid];
}

__global__ __launch_bounds__(TK_THREADS, 2) void tkpc_count_kernel(TkWith<TkcArgs, TkpFields> A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char tk_smem[];
  TkpProducer P(tk_smem, A);
  TkCount C(P.rest, TK_BU);
  tk_walk(A, P, C);
}

// MANNeR.  The statistics pass runs first, as for the top-k; the raw tile, the ensemble tile and the workgroup's statistics
// (67.5 KB) and the consumer's arrays (41.9 KB) are 109.4 KB: one workgroup per CU.
constexpr size_t TKEC_LDS = 2 * TK_TILE_BYTES + TKE_STATS_LDS + tkc_lds_bytes(TK_BU);
static_assert((2 * TK_TILE_BYTES + TKE_STATS_LDS) % 16 == 0 && TKEC_LDS <= 160 * 1024,
              "the two score tiles and the statistics leave room for one workgroup per CU");

// one wave per target slot: the target's rows of tables 1 ... T - 1 into blocks 1 ... T - 1 of the (T, n_targets, D) gathered
// workspace (tkc_init_kernel filled block 0 from table 0); zeros for a row outside V
__global__ __launch_bounds__(64) void tkec_gather_kernel(TkWith<TkcArgs, TkeFields> A) {
  const int64_t j = blockIdx.x;
  const int lane = threadIdx.x, t = 1 + (int)blockIdx.y;
  const int64_t row = A.tgt_idx[j];
  const bool ok = row >= 0 && row < A.V;
  const float* const table = tke_pick(A.tables, t);
  float* const dst = A.gathered + ((int64_t)t * A.n_targets + j) * A.D;
  const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int c = lane * 4; c < A.D; c += 256) st4(dst + c, ok ? ld4(table + row * A.D + c) : z);
}

// One workgroup per 64 slots from j0 on, as tkc_target_kernel: per sub-model the tile product of the owners' rows of users[t] with
// the gathered rows of tables[t]; the diagonal is the raw score tke_scores_kernel computes for that (user, row), folded with the
// owner's statistics by the same operations in the same order.  NaN where the owner's statistics cannot standardise: the finish
// kernel leaves such a slot at rank 0 / -inf.
__global__ __launch_bounds__(TK_THREADS) void tkec_target_kernel(TkWith<TkcArgs, TkeFields> A) {
  __shared__ __attribute__((aligned(16))) float sc[TK_BU * TK_SCLD];
  const int tid = threadIdx.x, T = A.T;
  const int64_t j0 = (int64_t)blockIdx.x * TK_BU;
  const int srow = tid >> 2;
  const int own = j0 + srow < A.n_targets ? A.owner[j0 + srow] : -1;
  const bool ua_ok = own >= 0;
  // thread i < 64 folds slot j0 + i (its own staging row is another slot's: the owner is read again)
  const bool mine = tid < TK_BU && j0 + tid < A.n_targets;
  const int jown = mine ? A.owner[j0 + tid] : -1;
  bool ok = true;
  float zsum = 0.f;
  for (int t = 0; t < T; ++t) {
    const float* const pa[1] = {tke_pick(A.users, t) + (int64_t)(ua_ok ? own : 0) * A.D};
    tk_tile_product<1>(pa, ua_ok, A.gathered + (int64_t)t * A.n_targets * A.D, (int)j0, (int)A.n_targets, A.D, sc);
    if (jown >= 0) {
      const float mean = A.out_stats[((int64_t)jown * T + t) * 2], sd = A.out_stats[((int64_t)jown * T + t) * 2 + 1];
      const float w = t == 0 ? A.w[0] : (t == 1 ? A.w[1] : A.w[2]);
      zsum = tke_fold_z(zsum, t == 0, w, sc[tid * TK_SCLD + tid], mean, sd);
      ok = ok && tke_sd_ok(sd);
    }
    __syncthreads();                                  // the diagonal is read; the tile is free for the next operands
  }
  if (mine) A.tscore[j0 + tid] = ok ? zsum : __uint_as_float(0x7FC00000u);
}

__global__ __launch_bounds__(TK_THREADS) void tkec_count_kernel(TkWith<TkcArgs, TkeFields> A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char tk_smem[];
  TkeProducer P(tk_smem, A);
  TkCount C(P.rest, TK_BU);
  tk_walk(A, P, C);
}

__device__ __forceinline__ int tkc_wave_sum(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// per-user time windows (the section below): row v is in user u's population only when win_lo[u] <= row_time[v] <= win_hi[u]
struct TkwFields {
  const int32_t* row_time;                     // (V)
  const int32_t* win_lo;                       // (B) closed bounds; lo > hi: an empty window
  const int32_t* win_hi;
};

// one wave per user; W: the windowed entry's one extra test of a target (null for every other entry)
__device__ __forceinline__ void tkc_finish_user(const TkcArgs& A, const TkwFields* W) {
  const int64_t u = blockIdx.x;
  const int lane = threadIdx.x;
  int64_t xs, xn, ts;
  int nt;
  const bool excl_ok = tk_excl_range(A, u, xs, xn);
  const bool tgt_ok = tkc_tgt_range(A, u, ts, nt);
  if (lane == 0 && !excl_ok) atomicOr(A.status, NRL_TOPK_E_OFFSETS);
  if (lane == 0 && !tgt_ok) atomicOr(A.status, NRL_RANK_E_TARGETS);
  int pop = 0;
  for (int s = lane; s < A.slices; s += 64) pop += A.pcnt[u * A.slices + s];
  pop = tkc_wave_sum(pop);
  if (lane == 0) A.out_ranked[u] = excl_ok ? pop : 0;
  if (!excl_ok) return;                               // (the slots it owns keep rank 0 / -inf)

  // lane t < nt: target slot ts + t, when this user owns it
  const bool mine = lane < nt && A.owner[ts + lane] == (int32_t)u;
  const int64_t row = mine ? A.tgt_idx[ts + lane] : -1;
  const bool inside = row >= 0 && row < A.V;
  if (__ballot(mine && !inside) && lane == 0) atomicOr(A.status, NRL_RANK_E_TARGET_ROW);
  bool excluded = false;
  int bad = 0;
  for (int64_t base = 0; base < xn; base += 64) {
    const int64_t x = base + lane < xn ? A.excl_idx[xs + base + lane] : -1;
    bad |= base + lane < xn && (x < 0 || x >= A.V);
    for (int t = 0; t < nt; ++t) {
      const int64_t rt = ((int64_t)__shfl((int)(row >> 32), t, 64) << 32) | (uint32_t)__shfl((int)(uint32_t)row, t, 64);
      const bool hit = __ballot(x >= 0 && x == rt) != 0ull;
      if (lane == t) excluded |= hit;
    }
  }
  if (__ballot(bad) && lane == 0) atomicOr(A.status, NRL_TOPK_E_EXCLUDE);
  if (!mine || !inside || excluded || (A.eligible && !A.eligible[row])) return;
  if (W) {                                            // a target outside its owner's window: rank 0 / -inf, no flag
    const int32_t t = W->row_time[row];
    if (t < W->win_lo[u] || t > W->win_hi[u]) return;
  }
  const float s = A.tscore[ts + lane];
  if (s != s) return;
  int above = 0;
  for (int i = 0; i < A.slices; ++i) above += A.tcnt[(ts + lane) * A.slices + i];
  A.out_rank[ts + lane] = 1 + above;
  A.out_score[ts + lane] = tk_unkey(score_key(s));    // (-0 comes back as +0, as from tk_merge_kernel)
}

__global__ __launch_bounds__(64) void tkc_finish_kernel(TkcArgs A) { tkc_finish_user(A, nullptr); }

// ---- per-user time windows: nrl_topk_window_scores, nrl_catalogue_window_ranks ----------------------------------------------------
// Row v belongs to user u's population iff it does under the plain entries' rules and win_lo[u] <= row_time[v] <= win_hi[u] (int32,
// closed; lo > hi is an empty window: an empty list, population 0, every rank 0 and no flag).  The window is a property of the WALK:
// TkDot, TkSelect and TkCount run as they are, so a score has the bits of the plain entries, and tkw_walk is tk_walk with
//   * the users' bounds staged once (lo / hi [slots]; an empty window for the slots past the last user) and their union
//     [min lo, max hi] over the non-empty windows, read back from LDS behind the prologue's barrier: the same in every thread;
//   * per table tile the 128 row times staged next to `el` by the threads that fill `el`; the wave that serves user ul ANDs
//     lo <= t <= hi into the two eligibility booleans of its lanes before the consumer sees them;
//   * the TILE SKIP: a thread whose row is inside V, eligible and inside the union window writes the tile's number into hit[vt & 1];
//     after one barrier every thread reads the same word, and a tile nobody marked is left before its product, its table read and
//     its per-user loop.  Such a tile holds no row of any user's population, so it contributes no entry and no count: the skip
//     cannot change a result.  Two words, by the tile's parity: a thread that has skipped tile vt marks tile vt + 1 in the other
//     word while a slower one still reads vt's, and nobody reaches tile vt + 2 before everyone passed the barrier of vt + 1.  A
//     workgroup whose windows are all empty walks no tile and flushes empty lists / zero counts.
// A user whose window misses the tile costs its wave two loads and a ballot.  The merge is tk_merge_kernel (a partial list never
// holds a row outside the window), the target scores are tkc_target_kernel's, and the finish makes the one extra test above.
struct TkWindow {
  int32_t* tt;                                 // [TK_BV] row times of the table tile
  int32_t* lo;                                 // [slots]
  int32_t* hi;                                 // [slots]
  int32_t* hit;                                // [2] (+ 2 words of padding): the last tile somebody marked, by parity
  __device__ __forceinline__ TkWindow(unsigned char* p, int slots) {
    tt = reinterpret_cast<int32_t*>(p);
    lo = tt + TK_BV;
    hi = lo + slots;
    hit = hi + slots;
  }
};
// behind the consumer's arrays, which end 4-byte aligned for any `slots` and 16-byte aligned for TK_BU
constexpr size_t tkw_lds_bytes(int slots) { return (size_t)TK_BV * 4 + (size_t)slots * 8 + 16; }
static_assert(tk_lds_bytes(1, TK_BU, 1) % 16 == 0 && (TK_BU * 8) % 16 == 0 && TKC_LDS % 16 == 0 && tkw_lds_bytes(TK_BU) % 16 == 0,
              "the window's arrays start and end 16-byte aligned behind either consumer, for every k");
// 1040 B: two workgroups of the scores kernel fit a CU up to k = 58 (plain: 60), more than 64 KB from k = 27 on (plain: 29)
static_assert(2 * (tk_lds_bytes(1, TK_BU, 58) + tkw_lds_bytes(TK_BU)) <= 160 * 1024 &&
                  2 * (tk_lds_bytes(1, TK_BU, 59) + tkw_lds_bytes(TK_BU)) > 160 * 1024,
              "two workgroups of the windowed scores kernel fit a CU up to k = 58");
static_assert(tk_lds_bytes(1, TK_BU, 26) + tkw_lds_bytes(TK_BU) <= 64 * 1024 && tk_lds_bytes(1, TK_BU, 27) + tkw_lds_bytes(TK_BU) > 64 * 1024,
              "the windowed scores kernel needs the LDS attribute from k = 27 on");
static_assert(2 * (TKC_LDS + tkw_lds_bytes(TK_BU)) <= 160 * 1024, "two workgroups of the windowed count kernel fit a CU");
static_assert(tk_lds_bytes(1, TK_BU, NRL_TOPK_MAX_K) + tkw_lds_bytes(TK_BU) <= 160 * 1024, "the largest windowed layout fits");

constexpr int32_t TKW_MIN = -0x7FFFFFFF - 1, TKW_MAX = 0x7FFFFFFF;

template <class Args, class Producer, class Consumer>
__device__ __forceinline__ void tkw_walk(const Args& A, Producer& P, Consumer& C, const TkWindow& W) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int slots = P.slots();
  const int sl = (int)(blockIdx.x % (unsigned)A.slices);
  const int64_t u0 = (int64_t)(blockIdx.x / (unsigned)A.slices) * slots;
  const int nu = A.B - u0 < slots ? (int)(A.B - u0) : slots;
  int v_begin, nvt;
  tk_slice(A, sl, v_begin, nvt);

  P.stage(A, u0, nu);
  if (tid < slots) {
    W.lo[tid] = tid < nu ? A.win_lo[u0 + tid] : TKW_MAX;
    W.hi[tid] = tid < nu ? A.win_hi[u0 + tid] : TKW_MIN;
  }
  if (tid < 2) W.hit[tid] = 0;
  C.prologue(A, u0, nu, slots);                       // (its barrier also publishes lo, hi and hit)
  int32_t ulo = TKW_MAX, uhi = TKW_MIN;               // the union of the non-empty windows, from LDS: the same in every thread
  for (int i = 0; i < nu; ++i) {
    const int32_t l = W.lo[i], h = W.hi[i];
    if (l <= h) {
      ulo = l < ulo ? l : ulo;
      uhi = h > uhi ? h : uhi;
    }
  }
  ulo = __builtin_amdgcn_readfirstlane(ulo);
  uhi = __builtin_amdgcn_readfirstlane(uhi);
  if (ulo > uhi) nvt = 0;                             // every window is empty
  const int ul_begin = Producer::first(wave), ul_end = Producer::end(wave, nu);
  bool nan = false;

  for (int vt = 0; vt < nvt; ++vt) {
    const int v0 = v_begin + vt * TK_BV;
    if (tid < TK_BV) {
      const int64_t v = (int64_t)v0 + tid;
      const bool e = v < A.V && (!A.eligible || A.eligible[v]);
      const int32_t t = v < A.V ? A.row_time[v] : 0;
      C.el[tid] = e ? 1 : 0;
      W.tt[tid] = t;
      if (e && ulo <= t && t <= uhi) W.hit[vt & 1] = vt + 1;
    }
    __syncthreads();
    if (W.hit[vt & 1] != vt + 1) continue;            // (uniform: one LDS word behind a barrier)
    P.tile(A, v0, nu);

    const bool e_0 = C.el[lane] != 0, e_1 = C.el[64 + lane] != 0;
    const int32_t t_0 = W.tt[lane], t_1 = W.tt[64 + lane];
    for (int ul = ul_begin; ul < ul_end; ul += Producer::STEP) {
      if (P.skip(ul)) continue;
      const int32_t lo = W.lo[ul], hi = W.hi[ul];
      const bool w_0 = e_0 && lo <= t_0 && t_0 <= hi, w_1 = e_1 && lo <= t_1 && t_1 <= hi;
      if (!__ballot(w_0 || w_1)) continue;
      C.user(P.row(ul), ul, A.excl_idx, v0, w_0, w_1, lane, nan);
    }
    __syncthreads();                                  // the score tile, `el` and `tt` are free for the next tile
  }

  if (nan && lane == 0) atomicOr(A.status, NRL_TOPK_E_NAN);
  wave_lds_sync();
  for (int ul = ul_begin; ul < ul_end; ul += Producer::STEP) C.flush(A, ul, u0 + ul, sl, lane);
}

__global__ __launch_bounds__(TK_THREADS) void tkw_scores_kernel(TkWith<TkArgs, TkwFields> A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char tk_smem[];
  TkDot P(tk_smem);
  TkSelect C(P.rest, TK_BU, A.k);
  TkWindow W(P.rest + tk_lds_bytes(0, TK_BU, A.k), TK_BU);
  tkw_walk(A, P, C, W);
}

__global__ __launch_bounds__(TK_THREADS) void tkwc_count_kernel(TkWith<TkcArgs, TkwFields> A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char tk_smem[];
  TkDot P(tk_smem);
  TkCount C(P.rest, TK_BU);
  TkWindow W(P.rest + tkc_lds_bytes(TK_BU), TK_BU);
  tkw_walk(A, P, C, W);
}

__global__ __launch_bounds__(64) void tkwc_finish_kernel(TkWith<TkcArgs, TkwFields> A) { tkc_finish_user(A, &A); }

// ---- Gumbel top-k: nrl_topk_sampled_scores, nrl_gumbel_noise ----------------------------------------------------------------------------
// One Plackett-Luce draw without replacement from softmax(s * inv_temp) per user: the k rows with the largest
// z = fadd_rn(fmul_rn(s, inv_temp), g), g a standard Gumbel variable per (seed, user key, row) from the counter-based hash of the
// dropout masks (the header has the normative statement).  The noise is a property of the PRODUCER: TksProducer is TkDot's tile with the
// perturbation on the accumulator fragments before they are stored, the way TkBiasProducer adds its bias, so tk_walk, TkSelect, the
// partial lists and tk_merge_kernel run as they are over z instead of s.
//   * where: behind the MFMA chain, in registers.  A lane holds 32 elements of the tile (8 users x 4 columns), so the hash and the two
//     logs are spread evenly over all 256 threads whatever the number of users, and the tile is written once.  The alternative -- the
//     serving wave rewrites its user's row in place -- costs a second LDS read and write of every element (64 KB per tile) for the
//     same arithmetic and leaves the lanes of a short user tile idle; it would save nothing: columns past V and users past B are
//     perturbed here too (harmless: they are never consumed) rather than branched around;
//   * ku, the 64 users' hashed keys, are staged once per workgroup (256 B behind the score tile; the consumer's prologue publishes
//     them); k0, the per-call key, comes from the host.  A lane reads 8 of them per tile: 4 addresses per wave and read, a broadcast;
//   * the lists hold z only.  The raw scores of the selected rows are computed afterwards by tks_raw_kernel: tkc_target_kernel's
//     diagonal of the tile product of (owner's row, selected row), the selected rows read in place through out_idx
//     (tk_tile_accumulate<1, true>: nothing is gathered, no workspace beyond the partial lists) -- the same chain on the same
//     operands, so the bits nrl_topk_scores reports for that pair.
struct TksFields {
  const int64_t* user_key;                     // (B)
  uint32_t k0;                                 // the per-call key (tks_call_key)
  float inv_temp;
};

__host__ __device__ __forceinline__ uint32_t tks_call_key(uint64_t seed) {
  return lowbias32((uint32_t)(seed & 0xFFFFFFFFu) ^ lowbias32((uint32_t)(seed >> 32) + 0x9E3779B9u));
}
__host__ __device__ __forceinline__ uint32_t tks_user_key(uint32_t k0, uint64_t key) {
  return lowbias32((uint32_t)(key & 0xFFFFFFFFu) ^ lowbias32((uint32_t)(key >> 32) ^ k0));
}
// u = (2 m + 1) 2^-24 with m the top 23 bits of the pair's hash: exact in fp32 and inside [2^-24, 1 - 2^-24]
__device__ __forceinline__ float tks_uniform(uint32_t ku, uint32_t row) {
  const uint32_t m = lowbias32(row * 0x9E3779B1u + ku) >> 9;
  return (float)(2u * m + 1u) * 0x1p-24f;
}
// g = -log(-log(u)) in fp32 by an accurate logf, twice.  Never the fast intrinsic: its absolute error near u = 1 exceeds -log(u)
// itself, and those are the rows that receive the largest perturbations.  And not the library's logf either: its errors of up to
// 2 ulp in -log(u) and in g add up to 2^-21.9 max(1, |g|) (measured), which four times over is above the 2^-20 the noise test
// allows.  tks_logf is the float64 log rounded once to fp32, a logf within half an ulp and a bit; through both, 2^-23.
__device__ __forceinline__ float tks_logf(float x) { return (float)log((double)x); }
__device__ __forceinline__ float tks_gumbel(float u) { return -tks_logf(-tks_logf(u)); }
// the perturbed key of a pair: two roundings, never an fma (the unit is compiled with contraction on, and __fmul_rn is a plain `*`)
__device__ __forceinline__ float tks_perturb(float s, float inv_temp, float g) {
#pragma clang fp contract(off)
  const float scaled = s * inv_temp;
  return scaled + g;
}

constexpr size_t TKS_EXTRA_LDS = (size_t)TK_BU * 4;                          // ku
static_assert(TKS_EXTRA_LDS % 16 == 0, "what follows the hashed keys is 16-byte aligned");
// 256 B: two workgroups of the sampled scores kernel fit a CU up to k = 59 (plain: 60), more than 64 KB from k = 28 on (plain: 29)
static_assert(2 * (tk_lds_bytes(1, TK_BU, 59) + TKS_EXTRA_LDS) <= 160 * 1024 && 2 * (tk_lds_bytes(1, TK_BU, 60) + TKS_EXTRA_LDS) > 160 * 1024,
              "two workgroups of the sampled scores kernel fit a CU up to k = 59");
static_assert(tk_lds_bytes(1, TK_BU, 27) + TKS_EXTRA_LDS <= 64 * 1024 && tk_lds_bytes(1, TK_BU, 28) + TKS_EXTRA_LDS > 64 * 1024,
              "the sampled scores kernel needs the LDS attribute from k = 28 on");
static_assert(tk_lds_bytes(1, TK_BU, NRL_TOPK_MAX_K) + TKS_EXTRA_LDS <= 160 * 1024, "the largest sampled layout fits");

// The producer of the sampled kernel: TkDot's tile, every element scaled by inv_temp and perturbed by its pair's Gumbel noise.
struct TksProducer : TkBlocked {
  float* sc;                                   // [TK_BU][TK_SCLD]; until the keys exist, the operand tiles
  uint32_t* kul;                               // [TK_BU] the users' hashed keys
  unsigned char* rest;
  const TksFields& F;
  const float* pa[1];
  bool ua_ok;
  __device__ __forceinline__ TksProducer(unsigned char* p, const TksFields& f)
      : sc(reinterpret_cast<float*>(p)), kul(reinterpret_cast<uint32_t*>(p + TK_TILE_BYTES)), rest(p + TK_TILE_BYTES + TKS_EXTRA_LDS),
        F(f) {}
  __device__ __forceinline__ int slots() const { return TK_BU; }
  __device__ __forceinline__ void stage(const TkArgs& A, int64_t u0, int nu) {
    const int srow = threadIdx.x >> 2;
    ua_ok = srow < nu;
    pa[0] = A.user + (ua_ok ? u0 + srow : A.B - 1) * A.D;
    if (threadIdx.x < TK_BU)                          // (the consumer's prologue publishes the keys)
      kul[threadIdx.x] = (int)threadIdx.x < nu ? tks_user_key(F.k0, (uint64_t)F.user_key[u0 + threadIdx.x]) : 0u;
  }
  __device__ __forceinline__ void tile(const TkArgs& A, int v0, int) const {
    const int tid = threadIdx.x, lane = tid & 63;
    tk_f32x4 acc[1][2][4];
    tk_tile_accumulate<1>(pa, ua_ok, A.table, A.D, v0, A.V, A.D, sc, acc);
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1, l15 = lane & 15, g = lane >> 4;
    uint32_t ku[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) ku[i][r] = kul[wm * 32 + i * 16 + 4 * g + r];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t row = (uint32_t)v0 + wn * 64 + j * 16 + l15;
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[0][i][j][r] = tks_perturb(acc[0][i][j][r], F.inv_temp, tks_gumbel(tks_uniform(ku[i][r], row)));
    }
    tk_store_fragments(acc[0], sc);
    __syncthreads();
  }
  __device__ __forceinline__ const float* row(int ul) const { return sc + ul * TK_SCLD; }
  __device__ __forceinline__ bool skip(int) const { return false; }
};

__global__ __launch_bounds__(TK_THREADS) void tks_scores_kernel(TkWith<TkArgs, TksFields> A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char tk_smem[];
  TksProducer P(tk_smem, A);
  TkSelect C(P.rest, TK_BU, A.k);
  tk_walk(A, P, C);
}

// The raw scores of the selected rows, one workgroup per 64 slots of the (B, k) lists: tile row r is the user row of slot j0 + r
// (user (j0 + r) / k), tile column c is table row out_idx[j0 + c] read in place (a zero row for -1), and slot j0 + r's score is the
// diagonal: the bits tk_scores_kernel computes for that (user, row), reported as tk_merge_kernel reports them (-0 as +0).
struct TksRawArgs {
  const float* user;
  const float* table;
  const int64_t* idx;                          // (B, k) the merged lists' rows
  float* out_score;                            // (B, k)
  int64_t V;
  int32_t n, D, k;                             // n = B * k slots
};
__global__ __launch_bounds__(TK_THREADS) void tks_raw_kernel(TksRawArgs A) {
  __shared__ __attribute__((aligned(16))) float sc[TK_BU * TK_SCLD];
  const int tid = threadIdx.x;
  const int j0 = (int)blockIdx.x * TK_BU;
  if (A.V == 0) {                                     // (uniform: no table to read, every slot is empty)
    if (tid < TK_BU && j0 + tid < A.n) A.out_score[j0 + tid] = -INFINITY;
    return;
  }
  const int srow = tid >> 2;
  const bool ua_ok = j0 + srow < A.n;
  const float* const pa[1] = {A.user + (int64_t)(ua_ok ? (j0 + srow) / A.k : 0) * A.D};
  tk_f32x4 acc[1][2][4];
  tk_tile_accumulate<1, true>(pa, ua_ok, A.table, A.D, j0, A.n, A.D, sc, acc, A.idx, A.V);
  tk_store_fragments(acc[0], sc);
  __syncthreads();
  if (tid < TK_BU && j0 + tid < A.n)
    A.out_score[j0 + tid] = A.idx[j0 + tid] >= 0 ? tk_unkey(score_key(sc[tid * TK_SCLD + tid])) : -INFINITY;
}

// the public statement of the noise: element i is the pair (user_key[i], row[i]) under the call key k0
__global__ __launch_bounds__(256) void tks_noise_kernel(const int64_t* user_key, const int64_t* row, int64_t n, uint32_t k0, float* out_u,
                                                        float* out_g) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float u = tks_uniform(tks_user_key(k0, (uint64_t)user_key[i]), (uint32_t)row[i]);
  if (out_u) out_u[i] = u;
  if (out_g) out_g[i] = tks_gumbel(u);
}

// ---- several Gumbel top-k draws per walk: nrl_topk_sampled_draws --------------------------------------------------------------------
// R draws of nrl_topk_sampled_scores, draw r under seed + r (mod 2^64), from ONE pass over the table: the dot products of draw r and
// draw r + 1 are the same bits and only the noise differs, so the MFMA chain, the table reads and the operand staging are paid once
// per tile and a draw costs its noise, a store of the tile and its selection.  tkd_walk is a walk of its own beside tk_walk (whose
// text, like TkDot's, TkSelect's and TksProducer's, is untouched):
//   * per table tile tk_tile_accumulate<1> runs once and the accumulator fragments stay in registers; for r = 0 ... R - 1 a COPY of
//     them is perturbed with draw r's noise (tks_perturb / tks_gumbel / tks_uniform as they stand, the same operands in the same
//     order as TksProducer::tile), stored to the one score tile, and each wave selects its users' rows into list (user, r) with
//     tk_select_user.  Two barriers per draw: the tile published, the tile free;
//   * the exclusion cache, the eligibility bytes and the slice plan belong to the user and the tile, not to the draw: filled once;
//   * the hashed user keys of all draws, kud[R][64], are staged in the prologue; the per-draw call keys k0[r] = tks_call_key(seed + r)
//     come from the host in the kernel arguments;
//   * LDS: TkSelect carves its members for lists of R k entries (list (ul, r) at lists + (ul R + r) k), so the layout is
//     tk_lds_bytes(1, TK_BU, R k) + R * 256; the partial lists are (B, slices, R, k);
//   * tkd_merge_kernel, one wave per (user, draw): the flags and the merge of tk_merge_kernel over that draw's partial lists (the
//     flags are raised once per draw of a user instead of once: an OR either way);
//   * the raw scores are tks_raw_kernel over the (B, R k) lists: its k only divides a slot number by the slots per user.
// A NaN key is seen per draw exactly where the single entry sees it, so the status word is the OR of the R single calls' words.
constexpr size_t tkd_lds_bytes(int R, int k) { return tk_lds_bytes(1, TK_BU, R * k) + (size_t)R * TK_BU * 4; }
static_assert(NRL_TOPK_MAX_DRAWS * TK_BU * 4 % 16 == 0 && (TK_BU * 4) % 16 == 0, "what follows the hashed keys is 16-byte aligned");
static_assert(tkd_lds_bytes(NRL_TOPK_MAX_DRAWS, NRL_TOPK_MAX_K / NRL_TOPK_MAX_DRAWS) == 124800 &&
                  tkd_lds_bytes(NRL_TOPK_MAX_DRAWS, NRL_TOPK_MAX_K / NRL_TOPK_MAX_DRAWS) <= 160 * 1024,
              "the largest layout of the draws kernel (32 draws of 4) fits");
static_assert(tkd_lds_bytes(1, NRL_TOPK_MAX_K) <= tkd_lds_bytes(NRL_TOPK_MAX_DRAWS, NRL_TOPK_MAX_K / NRL_TOPK_MAX_DRAWS),
              "no R with R k <= NRL_TOPK_MAX_K needs more than 32 draws of 4");
// two workgroups per CU: 512 R k + 256 R <= 30,848 -- R k <= 59 for one draw, 58 for two, 50 for five draws of 10
static_assert(2 * tkd_lds_bytes(1, 59) <= 160 * 1024 && 2 * tkd_lds_bytes(1, 60) > 160 * 1024, "one draw: two workgroups per CU up to k = 59");
static_assert(2 * tkd_lds_bytes(2, 29) <= 160 * 1024 && 2 * tkd_lds_bytes(2, 30) > 160 * 1024, "two draws: up to k = 29");
static_assert(2 * tkd_lds_bytes(5, 10) <= 160 * 1024 && 2 * tkd_lds_bytes(6, 10) > 160 * 1024, "k = 10: up to five draws");
static_assert(2 * tkd_lds_bytes(13, 4) <= 160 * 1024 && 2 * tkd_lds_bytes(14, 4) > 160 * 1024, "k = 4: up to thirteen draws");

struct TkdFields {
  const int64_t* user_key;                     // (B)
  float inv_temp;
  int32_t R, R_all, r0;                        // this launch serves draws r0 ... r0 + R - 1 of the call's R_all
  uint32_t k0[NRL_TOPK_MAX_DRAWS];             // tks_call_key(seed + r0 + r)
};

__device__ __forceinline__ void tkd_walk(const TkWith<TkArgs, TkdFields>& A, unsigned char* smem) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int R = A.R, k = A.k, rk = R * k;
  float* const sc = reinterpret_cast<float*>(smem);                          // [TK_BU][TK_SCLD]; until the keys exist, the operand tiles
  uint32_t* const kud = reinterpret_cast<uint32_t*>(smem + TK_TILE_BYTES);   // [R][TK_BU] the users' hashed keys per draw
  TkSelect C(smem + TK_TILE_BYTES + (size_t)R * TK_BU * 4, TK_BU, rk);
  const int sl = (int)(blockIdx.x % (unsigned)A.slices);
  const int64_t u0 = (int64_t)(blockIdx.x / (unsigned)A.slices) * TK_BU;
  const int nu = A.B - u0 < TK_BU ? (int)(A.B - u0) : TK_BU;
  int v_begin, nvt;
  tk_slice(A, sl, v_begin, nvt);

  const int srow = tid >> 2;
  const bool ua_ok = srow < nu;
  const float* const pa[1] = {A.user + (ua_ok ? u0 + srow : A.B - 1) * A.D};
  if (tid < TK_BU) {
    const uint64_t key = tid < nu ? (uint64_t)A.user_key[u0 + tid] : 0ull;
    for (int r = 0; r < R; ++r) kud[r * TK_BU + tid] = tid < nu ? tks_user_key(A.k0[r], key) : 0u;
  }
  C.prologue(A, u0, nu, TK_BU);                       // (its barrier also publishes the keys)
  const int ul_begin = TkBlocked::first(wave), ul_end = TkBlocked::end(wave, nu);
  const int wm = wave >> 1, wn = wave & 1, l15 = lane & 15, g = lane >> 4;
  bool nan = false;

  for (int vt = 0; vt < nvt; ++vt) {
    const int v0 = v_begin + vt * TK_BV;
    tk_fill_eligible(A.eligible, v0, A.V, C.el);
    tk_f32x4 acc[1][2][4];
    tk_tile_accumulate<1>(pa, ua_ok, A.table, A.D, v0, A.V, A.D, sc, acc);   // (its barriers publish `el`)
    const bool e_0 = C.el[lane] != 0, e_1 = C.el[64 + lane] != 0;
    for (int r = 0; r < R; ++r) {
      const uint32_t* const kul = kud + r * TK_BU;
      uint32_t ku[2][4];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q) ku[i][q] = kul[wm * 32 + i * 16 + 4 * g + q];
      tk_f32x4 z[2][4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint32_t row = (uint32_t)v0 + wn * 64 + j * 16 + l15;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int q = 0; q < 4; ++q) z[i][j][q] = tks_perturb(acc[0][i][j][q], A.inv_temp, tks_gumbel(tks_uniform(ku[i][q], row)));
      }
      tk_store_fragments(z, sc);
      __syncthreads();
      for (int ul = ul_begin; ul < ul_end; ++ul)
        tk_select_user(sc + ul * TK_SCLD, C.lists + (ul * R + r) * k, C.xn + ul, C.xs + ul, C.xl + ul * TK_XCAP, A.excl_idx, v0, e_0, e_1,
                       k, lane, nan);
      __syncthreads();                                // the score tile is free for the next draw, or the next tile's operands
    }
  }

  if (nan && lane == 0) atomicOr(A.status, NRL_TOPK_E_NAN);
  wave_lds_sync();
  for (int ul = ul_begin; ul < ul_end; ++ul)
    tk_flush_user(C.lists + ul * rk, A.partial + ((u0 + ul) * A.slices + sl) * rk, rk, lane);
}

__global__ __launch_bounds__(TK_THREADS) void tkd_scores_kernel(TkWith<TkArgs, TkdFields> A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char tk_smem[];
  tkd_walk(A, tk_smem);
}

// one wave per (user, draw): tk_merge_kernel's flags and merge over draw r's partial lists, written to list (u, r0 + r) of (B, R_all, k)
__global__ __launch_bounds__(64) void tkd_merge_kernel(TkWith<TkArgs, TkdFields> A) {
  const int64_t u = blockIdx.x / (unsigned)A.R;
  const int r = (int)(blockIdx.x % (unsigned)A.R);
  const int lane = threadIdx.x, k = A.k;
  int64_t s, n;
  const bool ok = tk_excl_range(A, u, s, n);
  TkList S;
  S.e0 = S.e1 = 0ull;
  if (!ok) {
    if (lane == 0) atomicOr(A.status, NRL_TOPK_E_OFFSETS);
  } else {
    int bad = 0;
    for (int64_t i = lane; i < n; i += 64) {
      const int64_t x = A.excl_idx[s + i];
      bad |= (x < 0 || x >= A.V);
    }
    if (__ballot(bad) && lane == 0) atomicOr(A.status, NRL_TOPK_E_EXCLUDE);
    bool nan = false;
    for (int sl = 0; sl < A.slices; ++sl) {
      const unsigned long long* P = A.partial + ((u * A.slices + sl) * A.R + r) * k;
      for (int base = 0; base < k; base += 64) {
        const unsigned long long c = base + lane < k ? P[base + lane] : 0ull;
        const unsigned long long m = __ballot(c > S.kth(k));
        if (m) S.take(c, m, k, lane, nan);
      }
    }
  }
  const int64_t o = (u * A.R_all + A.r0 + r) * k;
  for (int p = lane; p < k; p += 64) {
    const unsigned long long e = p < 64 ? S.e0 : S.e1;
    A.out_idx[o + p] = e ? (int64_t)(uint32_t)~(uint32_t)e : -1;
    A.out_score[o + p] = e ? tk_unkey((uint32_t)(e >> 32)) : -INFINITY;
  }
}

// ---- class exposure of lists: nrl_list_class_exposure ----------------------------------------------------------------------------------
// out[b, s] = fl32((sum over the slots (l, j) of user b in ascending order of (double)pos_weight[j] where the slot's row has class s)
// / L).  One wave per user; lane s owns class s and adds in float64 in slot order, so no atomics and one order.  64 slots at a time:
// lane i reads slot base + i's row and its class once, and the slots that count are broadcast one by one.
struct TkxArgs {
  const int64_t* list_idx;                     // (B, L, k)
  const int32_t* row_class;                    // (V)
  const float* pos_weight;                     // (k)
  int64_t V;
  int32_t L, k, S;
  float* out;                                  // (B, S)
  int32_t* status;
};
__global__ __launch_bounds__(64) void tkx_exposure_kernel(TkxArgs A) {
  const int64_t u = blockIdx.x;
  const int lane = threadIdx.x;
  const int64_t n = (int64_t)A.L * A.k;
  const int64_t* const list = A.list_idx + u * n;
  double sum = 0.0;
  int flags = 0;
  for (int64_t base = 0; base < n; base += 64) {
    const int64_t i = base + lane;
    int cls = -1;
    if (i < n) {
      const int64_t row = list[i];
      if (row >= 0 && row < A.V) {
        const int32_t c = A.row_class[row];
        if (c >= 0 && c < A.S)
          cls = c;
        else
          flags |= NRL_TOPK_E_CLASS;
      } else if (row != -1) {
        flags |= NRL_MMR_E_ROW;
      }
    }
    unsigned long long m = __ballot(cls >= 0);
    while (m) {
      const int b = __ffsll((long long)m) - 1;
      m &= m - 1;
      const int c = __shfl(cls, b, 64);
      const double w = (double)A.pos_weight[(int)((base + b) % A.k)];
      if (c == lane) sum += w;
    }
  }
  if (lane < A.S) A.out[u * A.S + lane] = (float)(sum / (double)A.L);
  const unsigned long long f1 = __ballot(flags & NRL_MMR_E_ROW), f2 = __ballot(flags & NRL_TOPK_E_CLASS);
  if (lane == 0 && (f1 | f2)) atomicOr(A.status, (f1 ? NRL_MMR_E_ROW : 0) | (f2 ? NRL_TOPK_E_CLASS : 0));
}

// ---- the log-partition of the sampled policy: nrl_catalogue_logz, nrl_list_logprob -----------------------------------------------------
// What the Plackett-Luce policy of nrl_topk_sampled_scores needs to say how probable a drawn list was: per user, over the rows of the
// user's population whose scaled score t = fmul_rn(s, inv_temp) (the first rounding of tks_perturb) is finite, minus the rows of an
// optional per-user drop list: n, m = max t, S = sum exp(t - m), W = sum (t - m) exp(t - m).  TkLogZ is the SUMMING consumer of the
// walk, under TkDot (tkz_sum_kernel); tkz_finish_kernel folds the chunks.
//   * the slices of this walk are the statistics chunks of tke_statistics, a function of V alone, so the order of every reduction is:
//     a user's outputs have the same bits whatever B, its place in the batch and the mask's form (null or all ones);
//   * no cross-lane reduction per (user, table tile): where TkSelect nearly always leaves a user after a few instructions, this
//     consumer has work for every user of every tile.  A lane owns columns lane and 64 + lane as elsewhere and keeps its own running
//     (m, S, W) of each of its wave's 16 users IN REGISTERS (48 VGPRs); per tile the wave only counts (ballots: the population and
//     the dropped rows).  Registers need the user loop unrolled, so the kernel runs tkz_walk, tk_walk's skeleton with that loop
//     unrolled over TK_USERS_PER_WAVE and predicated; tk_walk's text is untouched.  The states in LDS instead (st[3][64][64], 48 KB,
//     through tk_walk itself) gave the same bits at one workgroup per CU instead of two and 1.36 - 1.42x the time.
//     flush reduces the 64 lane states once, by a butterfly over lane distances 1, 2, ..., 32 whose merge is symmetric bit for bit,
//     and writes the chunk's (n, dropped, m, S, W);
//   * rescaling a state from m to m' > m: r = exp(m - m'), S' = S r, W' = (W + (m - m') S) r; a state that underflows (r == 0) is 0;
//   * mask order: exclusion sweep, drop sweep (tk_clear_excluded over the drop list: its first TK_XCAP entries cached in LDS, the
//     rest read from global memory), NaN drop (NRL_TOPK_E_NAN), non-finite drop (NRL_POLICY_E_INF).  `dropped` counts the drop
//     rows that were eligible, not excluded and finite, once each;
//   * every add and multiply below is one rounded fp32 operation (contraction off, as tke_fold_z); tkz_exp is the fast exponential:
//     for a sum of exponentials a term's ABSOLUTE error counts and |x| e^x <= 1 / e for x <= 0, so v_exp_f32 of x log2(e) is as good
//     here as the library's expf (DESIGN.md 7y has both measured);
//   * tkz_finish_kernel, one wave per user: the flags of tk_merge_kernel, then the chunks folded in ascending order in float64 (at most
//     64) and each output rounded to fp32 once.
// LDS of tkz_sum_kernel: the score tile (33 KB), the two caches (16.75 KB each), the counters: 67.1 KB, two workgroups per CU.
struct TkzFields {
  const int64_t* drop_idx;                     // (B, kd) or null: -1 an empty slot
  int32_t kd;
  float inv_temp;
  float* parts;                                // (B, chunks, TKZ_WORDS): n, dropped (int32 bits), m, S, W
  float *out_max, *out_logsum, *out_entropy;   // (B)
  int32_t *out_pop, *out_dropped;              // (B); out_dropped may be null
};
constexpr int TKZ_WORDS = 5;

constexpr size_t tkz_lds_bytes(int slots) {
  return (size_t)slots * (8 + 8) + (size_t)slots * TK_XCAP * 4 * 2 + (size_t)slots * (4 + 4 + 8) + TK_BV;
}
constexpr size_t TKZ_LDS = TK_TILE_BYTES + tkz_lds_bytes(TK_BU);
static_assert(2 * TKZ_LDS <= 160 * 1024, "two workgroups of the summing kernel fit a CU");

__device__ __forceinline__ float tkz_exp(float x) { return __expf(x); }
// the scaled score: the first rounding of tks_perturb, -0 as +0 (so that a maximum has one bit pattern)
__device__ __forceinline__ float tkz_scale(float s, float inv_temp) {
#pragma clang fp contract(off)
  const float t = s * inv_temp;
  return t == 0.f ? 0.f : t;
}

struct TkzState {                              // m == -inf: empty, and then S == W == 0
  float m, S, W;
};
// the state rescaled to the maximum m2 > a.m (finite)
__device__ __forceinline__ void tkz_rescale(TkzState& a, float m2) {
#pragma clang fp contract(off)
  if (a.m != -INFINITY) {
    const float d = a.m - m2, r = tkz_exp(d);
    if (r > 0.f) {
      a.W = (a.W + d * a.S) * r;
      a.S = a.S * r;
    } else {
      a.S = a.W = 0.f;
    }
  }
  a.m = m2;
}
// one more term t <= a.m (finite)
__device__ __forceinline__ void tkz_term(TkzState& a, float t) {
#pragma clang fp contract(off)
  const float x = t - a.m, e = tkz_exp(x);
  a.S = a.S + e;
  if (e > 0.f) a.W = a.W + x * e;
}
// the two columns of a lane: the valid ones among t0, t1, in that order
__device__ __forceinline__ void tkz_add2(TkzState& a, bool b0, float t0, bool b1, float t1) {
  float mt = b0 ? t0 : -INFINITY;
  if (b1 && t1 > mt) mt = t1;
  if (mt == -INFINITY) return;
  if (mt > a.m) tkz_rescale(a, mt);
  if (b0) tkz_term(a, t0);
  if (b1) tkz_term(a, t1);
}
// two states as one; merge(a, b) and merge(b, a) have the same bits
__device__ __forceinline__ TkzState tkz_merge(const TkzState& a, const TkzState& b) {
#pragma clang fp contract(off)
  if (b.m == -INFINITY) return a;
  if (a.m == -INFINITY) return b;
  TkzState o;
  o.m = a.m > b.m ? a.m : b.m;
  const float da = a.m - o.m, db = b.m - o.m, ra = tkz_exp(da), rb = tkz_exp(db);
  const float Sa = ra > 0.f ? a.S * ra : 0.f, Sb = rb > 0.f ? b.S * rb : 0.f;
  const float Wa = ra > 0.f ? (a.W + da * a.S) * ra : 0.f, Wb = rb > 0.f ? (b.W + db * b.S) * rb : 0.f;
  o.S = Sa + Sb;
  o.W = Wa + Wb;
  return o;
}

// The summing consumer: per user of the tile two counters, the exclusion cache and the drop cache; the lane states are the caller's
// registers, handed to user() and flush().
struct TkLogZ {
  int64_t* xs;                                 // [slots] exclusion cache: start
  int64_t* ds;                                 // [slots] drop cache: start (u * kd)
  int32_t* xl;                                 // [slots][TK_XCAP] exclusion cache: first rows
  int32_t* dl;                                 // [slots][TK_XCAP] drop cache: first rows
  int32_t* xn;                                 // [slots] exclusion cache: length
  int32_t* dn;                                 // [slots] drop cache: length (kd, 0 for a slot without a user)
  int32_t* cnt;                                // [slots][2] population, dropped rows
  uint8_t* el;                                 // [TK_BV]
  const TkzFields& F;
  int slots;
  bool inf = false;
  __device__ __forceinline__ TkLogZ(unsigned char* p, int slots_, const TkzFields& f) : F(f), slots(slots_) {
    xs = reinterpret_cast<int64_t*>(p);
    ds = xs + slots;
    xl = reinterpret_cast<int32_t*>(ds + slots);
    dl = xl + slots * TK_XCAP;
    xn = dl + slots * TK_XCAP;
    dn = xn + slots;
    cnt = dn + slots;
    el = reinterpret_cast<uint8_t*>(cnt + 2 * slots);
  }
  __device__ __forceinline__ void prologue(const TkArgs& A, int64_t u0, int nu, int) const {
    const int tid = threadIdx.x;
    for (int i = tid; i < 2 * slots; i += TK_THREADS) cnt[i] = 0;
    if (tid < slots) {
      ds[tid] = (u0 + tid) * (int64_t)F.kd;
      dn[tid] = tid < nu ? F.kd : 0;
    }
    tk_cache_exclusions(A, u0, nu, slots, xs, xn, xl);                       // (its barrier also publishes `ds` and `dn`)
    for (int i = tid; i < slots * TK_XCAP; i += TK_THREADS) {
      const int ul = i / TK_XCAP, j = i % TK_XCAP;
      int32_t x = -1;
      if (j < dn[ul]) {
        const int64_t r = F.drop_idx[ds[ul] + j];
        if (r >= 0 && r < A.V) x = (int32_t)r;
      }
      dl[i] = x;
    }
  }
  // one user against one table tile, by the wave that serves the user; a: the lane's state of that user
  __device__ __forceinline__ void user(const float* row, int ul, const int64_t* excl_idx, int v0, bool e_0, bool e_1, int lane, bool& nan,
                                       TkzState& a) {
    const float t0 = tkz_scale(row[lane], F.inv_temp), t1 = tkz_scale(row[64 + lane], F.inv_temp);
    unsigned long long m0 = __ballot(e_0), m1 = __ballot(e_1);
    tk_clear_excluded(xn + ul, xs + ul, xl + ul * TK_XCAP, excl_idx, v0, lane, m0, m1);
    const unsigned long long a0 = m0, a1 = m1;
    tk_clear_excluded(dn + ul, ds + ul, dl + ul * TK_XCAP, F.drop_idx, v0, lane, m0, m1);
    const unsigned long long q0 = __ballot(t0 != t0), q1 = __ballot(t1 != t1);
    if ((m0 & q0) | (m1 & q1)) nan = true;            // a NaN scaled score of a row of the population: flagged and left out
    m0 &= ~q0;
    m1 &= ~q1;
    const unsigned long long i0 = __ballot(fabsf(t0) == INFINITY), i1 = __ballot(fabsf(t1) == INFINITY);
    if ((m0 & i0) | (m1 & i1)) inf = true;            // an infinite one: flagged and left out
    m0 &= ~i0;
    m1 &= ~i1;
    const int np = __popcll(m0) + __popcll(m1);
    const int nd = __popcll(a0 & ~m0 & ~(q0 | i0)) + __popcll(a1 & ~m1 & ~(q1 | i1));
    if ((np | nd) && lane == 0) {
      cnt[2 * ul] += np;
      cnt[2 * ul + 1] += nd;
    }
    if (np) tkz_add2(a, (m0 >> lane) & 1, t0, (m1 >> lane) & 1, t1);
  }
  __device__ __forceinline__ void flush(const TkArgs& A, int ul, int64_t u, int sl, int lane, TkzState a) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const TkzState b{__shfl_xor(a.m, off, 64), __shfl_xor(a.S, off, 64), __shfl_xor(a.W, off, 64)};
      a = tkz_merge(a, b);
    }
    if (lane == 0) {
      float* const o = F.parts + (u * A.slices + sl) * TKZ_WORDS;
      o[0] = __int_as_float(cnt[2 * ul]);
      o[1] = __int_as_float(cnt[2 * ul + 1]);
      o[2] = a.m;
      o[3] = a.S;
      o[4] = a.W;
      if (inf) atomicOr(A.status, NRL_POLICY_E_INF);
    }
    inf = false;
  }
};
static_assert(tkz_lds_bytes(1) == 8 + 8 + 2 * TK_XCAP * 4 + 4 + 4 + 8 + TK_BV, "tkz_lds_bytes counts the members of TkLogZ");

// tkz_walk: tk_walk for TkDot under TkLogZ with the user loop unrolled over the wave's TK_USERS_PER_WAVE users and predicated, so that
// user i's lane state a[i] is indexed by a compile-time constant and stays in registers (no scratch).  The stages, their order and
// the barriers are tk_walk's.
__global__ __launch_bounds__(TK_THREADS) void tkz_sum_kernel(TkWith<TkArgs, TkzFields> A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char tk_smem[];
  TkDot P(tk_smem);
  TkLogZ C(P.rest, TK_BU, A);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int sl = (int)(blockIdx.x % (unsigned)A.slices);
  const int64_t u0 = (int64_t)(blockIdx.x / (unsigned)A.slices) * TK_BU;
  const int nu = A.B - u0 < TK_BU ? (int)(A.B - u0) : TK_BU;
  int v_begin, nvt;
  tk_slice(A, sl, v_begin, nvt);
  P.stage(A, u0, nu);
  C.prologue(A, u0, nu, TK_BU);
  const int ul_begin = TkDot::first(wave), ul_end = TkDot::end(wave, nu);
  bool nan = false;
  TkzState a[TK_USERS_PER_WAVE];
#pragma unroll
  for (int i = 0; i < TK_USERS_PER_WAVE; ++i) a[i] = TkzState{-INFINITY, 0.f, 0.f};
  for (int vt = 0; vt < nvt; ++vt) {
    const int v0 = v_begin + vt * TK_BV;
    tk_fill_eligible(A.eligible, v0, A.V, C.el);
    P.tile(A, v0, nu);
    const bool e_0 = C.el[lane] != 0, e_1 = C.el[64 + lane] != 0;
#pragma unroll
    for (int i = 0; i < TK_USERS_PER_WAVE; ++i)
      if (ul_begin + i < ul_end) C.user(P.row(ul_begin + i), ul_begin + i, A.excl_idx, v0, e_0, e_1, lane, nan, a[i]);
    __syncthreads();
  }
  if (nan && lane == 0) atomicOr(A.status, NRL_TOPK_E_NAN);
  wave_lds_sync();
#pragma unroll
  for (int i = 0; i < TK_USERS_PER_WAVE; ++i)
    if (ul_begin + i < ul_end) C.flush(A, ul_begin + i, u0 + ul_begin + i, sl, lane, a[i]);
}

// one wave per user: status flags, the fold of the user's chunks in float64, the outputs
__global__ __launch_bounds__(64) void tkz_finish_kernel(TkWith<TkArgs, TkzFields> A) {
#pragma clang fp contract(off)
  const int64_t u = blockIdx.x;
  const int lane = threadIdx.x;
  int64_t s, n;
  const bool ok = tk_excl_range(A, u, s, n);
  if (!ok) {
    if (lane == 0) atomicOr(A.status, NRL_TOPK_E_OFFSETS);
  } else {
    int bad = 0;
    for (int64_t i = lane; i < n; i += 64) {
      const int64_t x = A.excl_idx[s + i];
      bad |= (x < 0 || x >= A.V);
    }
    if (__ballot(bad) && lane == 0) atomicOr(A.status, NRL_TOPK_E_EXCLUDE);
  }
  if (lane != 0) return;
  int64_t pop = 0, dropped = 0;
  double m = -INFINITY, S = 0.0, W = 0.0;
  for (int c = 0; ok && c < A.slices; ++c) {
    const float* const p = A.parts + (u * A.slices + c) * TKZ_WORDS;
    const int nb = __float_as_int(p[0]);
    dropped += __float_as_int(p[1]);
    if (nb == 0) continue;
    pop += nb;
    const double mb = p[2], Sb = p[3], Wb = p[4];
    if (m == -INFINITY) {
      m = mb;
      S = Sb;
      W = Wb;
      continue;
    }
    const double m2 = m > mb ? m : mb, da = m - m2, db = mb - m2, ra = exp(da), rb = exp(db);
    const double Wa = ra > 0.0 ? (W + da * S) * ra : 0.0, Wc = rb > 0.0 ? (Wb + db * Sb) * rb : 0.0;
    S = (ra > 0.0 ? S * ra : 0.0) + (rb > 0.0 ? Sb * rb : 0.0);
    W = Wa + Wc;
    m = m2;
  }
  const double ls = pop ? log(S) : -INFINITY, h = pop ? ls - W / S : 0.0;
  A.out_max[u] = (float)m;
  A.out_logsum[u] = (float)ls;
  A.out_entropy[u] = (float)(h > 0.0 ? h : 0.0);
  A.out_pop[u] = (int32_t)pop;
  if (A.out_dropped) A.out_dropped[u] = (int32_t)dropped;
}

// The log-probabilities of the lists, one wave per user, in float64 and in the TAIL form: with a_j the scaled score of slot j, the
// denominator of slot j is R_j = exp(tail_max + tail_logsum) + sum_{i >= j} exp(a_i), accumulated from the last slot backwards
// (positive terms only: Z - sum_{i < j} cancels to nothing once the first slots hold the mass), and log p_j = a_j - log R_j.  log R_j
// is carried as a running log-sum-exp, L' = max(L, a) + log1p(exp(-|L - a|)), i.e. against the running maximum rather than one M for
// the whole list: the same sum, and no term underflows however far the scores spread.  Where slot j is all that is left, L' = a_j
// and log p_j is exactly 0.  `score` are the raw scores tks_raw_kernel wrote.
struct TkzListArgs {
  const int64_t* idx;                          // (B, k): rows, -1 in trailing empty slots
  const float* score;                          // (B, k)
  const float *tail_max, *tail_logsum;         // (B)
  const int32_t *tail_pop, *tail_dropped;      // (B)
  float *out_logp, *out_total;                 // (B, k), (B)
  int32_t* status;
  int64_t V;
  int32_t k;
  float inv_temp;
};
__global__ __launch_bounds__(64) void tkz_list_kernel(TkzListArgs A) {
  __shared__ double sa[NRL_TOPK_MAX_K];
  const int64_t u = blockIdx.x;
  const int lane = threadIdx.x, k = A.k;
  const int64_t* const L = A.idx + u * k;
  const int64_t r0 = lane < k ? L[lane] : -1, r1 = lane + 64 < k ? L[lane + 64] : -1;
  const unsigned long long f0 = __ballot(r0 != -1), f1 = __ballot(r1 != -1);
  const int cnt = __popcll(f0) + __popcll(f1);
  // valid: no hole before a row, every row inside [0, V), no row twice, and every row found in the user's population
  const unsigned long long w0 = cnt >= 64 ? ~0ull : (1ull << cnt) - 1, w1 = cnt <= 64 ? 0ull : (cnt >= 128 ? ~0ull : (1ull << (cnt - 64)) - 1);
  bool bad = (r0 != -1 && (r0 < 0 || r0 >= A.V)) || (r1 != -1 && (r1 < 0 || r1 >= A.V));
  for (int j = 0; j < cnt; ++j) {
    const int64_t v = (int64_t)tk_shfl((unsigned long long)(j < 64 ? r0 : r1), j & 63);
    bad |= (lane != j && r0 == v) || (lane + 64 != j && r1 == v);
  }
  const bool valid = f0 == w0 && f1 == w1 && !__ballot(bad) && A.tail_dropped[u] == cnt;
  if (!valid) {
    const float nanv = __uint_as_float(0x7FC00000u);
    for (int p = lane; p < k; p += 64) A.out_logp[u * k + p] = nanv;
    if (lane == 0) {
      A.out_total[u] = nanv;
      atomicOr(A.status, NRL_POLICY_E_LIST);
    }
    return;
  }
  for (int p = lane; p < cnt; p += 64) sa[p] = (double)tkz_scale(A.score[u * k + p], A.inv_temp);
  __syncthreads();
  if (lane == 0) {
    double L = A.tail_pop[u] > 0 ? (double)A.tail_max[u] + (double)A.tail_logsum[u] : -INFINITY;
    for (int j = cnt - 1; j >= 0; --j) {
      const double a = sa[j];
      if (L == -INFINITY) {
        L = a;
      } else {
        const double hi = L > a ? L : a, lo = L > a ? a : L;
        L = hi + log1p(exp(lo - hi));
      }
      sa[j] = a - L;
    }
  }
  __syncthreads();
  for (int p = lane; p < k; p += 64) A.out_logp[u * k + p] = p < cnt ? (float)sa[p] : 0.f;
  if (lane == 0) {
    double total = 0.0;
    for (int j = 0; j < cnt; ++j) total += sa[j];
    A.out_total[u] = (float)total;
  }
}

// ---- greedy MMR re-ranking of a pool (nrl_mmr_rerank) ------------------------------------------------------------------------------
// One workgroup per user.  The pool's Gram matrix is ceil(N / 64) calls of tk_tile_accumulate<1, true>: the A rows are pool slots
// 64 h ... 64 h + 63 read in place, the gathered B rows the whole pool, so G[i][j] is the chain of nrl_topk_scores over the two
// table rows and bit-symmetric.  Each call stages its operands inside the tile it then writes; the two [TK_BU][TK_SCLD] tiles are
// contiguous, so sim[i][j] is at i * TK_SCLD + j for every i.  Behind them:
//   wk[2][4] u64    the waves' best entries of a step, double-buffered by the step's parity (one barrier a step)
//   rows[128] i64   the slots' table rows;  scs[128] their scores;  rn[128] 1 / sqrt(G[i][i]);  objs[2][128] the slots' objectives
// rel, pen and the live / selected flags of slot i live in the registers of thread i.  The greedy loop reads sim[c][i], the ROW of
// the slot just selected: lane i reads word c * 132 + i, consecutive lanes consecutive banks, no conflict (the column, i * 132 + c,
// would put lanes 8 apart on one bank).  Every scalar operation below is one correctly rounded fp32 operation and none contracts.
constexpr int MMR_MAX_POOL = NRL_MMR_MAX_POOL;
constexpr size_t MMR_SLOT_BYTES = 2 * 4 * 8 + (size_t)MMR_MAX_POOL * (8 + 4 + 4 + 2 * 4);
constexpr size_t mmr_lds_bytes(int halves) { return (size_t)halves * TK_TILE_BYTES + MMR_SLOT_BYTES; }
static_assert(MMR_MAX_POOL == TK_BV && MMR_MAX_POOL == 2 * TK_BU, "a pool is one tile of gathered rows and at most two tiles of A rows");
static_assert(MMR_MAX_POOL <= TK_THREADS, "one thread per slot");
static_assert(2 * mmr_lds_bytes(2) <= 160 * 1024, "two workgroups of the largest layout fit a CU");

struct MmrArgs {
  const int64_t* pool_idx;
  const float* pool_score;
  const float* table;
  int32_t N, D, k;
  int64_t V;
  float lambda;
  int32_t similarity, normalize;
  int64_t* out_idx;
  float* out_score;
  float* out_mmr;
  int32_t* status;
};

// plain fp32 operations that stay single: the unit is compiled with contraction on (__fsqrt_rn would be the approximate
// v_sqrt_f32 here; sqrtf and the division are the correctly rounded expansions)
__device__ __forceinline__ float mmr_mul(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}
__device__ __forceinline__ float mmr_sub(float a, float b) {
#pragma clang fp contract(off)
  return a - b;
}
__device__ __forceinline__ float mmr_div(float a, float b) {
#pragma clang fp contract(off)
  return a / b;
}
__device__ __forceinline__ unsigned long long mmr_wave_max(unsigned long long x, int lane) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long y = tk_shfl(x, lane ^ off);
    x = y > x ? y : x;
  }
  return x;
}

__global__ __launch_bounds__(TK_THREADS) void mmr_rerank_kernel(MmrArgs A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char tk_smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int N = A.N, k = A.k;
  const int halves = (N + TK_BU - 1) / TK_BU;
  const int64_t u = blockIdx.x;
  float* const sim = reinterpret_cast<float*>(tk_smem);
  unsigned long long* const wk = reinterpret_cast<unsigned long long*>(tk_smem + (size_t)halves * TK_TILE_BYTES);
  int64_t* const rows = reinterpret_cast<int64_t*>(wk + 8);
  float* const scs = reinterpret_cast<float*>(rows + MMR_MAX_POOL);
  float* const rn = scs + MMR_MAX_POOL;
  float* const objs = rn + MMR_MAX_POOL;
  const int64_t* const pool = A.pool_idx + u * N;

  // the slots: thread i owns slot i
  bool live = false;
  float score = 0.f;
  int flags = 0;
  if (tid < MMR_MAX_POOL) {
    int64_t row = -1;
    if (tid < N) {
      row = pool[tid];
      score = A.pool_score[u * N + tid];
    }
    const bool row_ok = row >= 0 && row < A.V;
    const bool fin = fabsf(score) < INFINITY;
    if (row != -1 && !row_ok) flags |= NRL_MMR_E_ROW;
    if (row_ok && !fin) flags |= NRL_TOPK_E_NAN;
    live = row_ok && fin;
    rows[tid] = live ? row : -1;
    scs[tid] = score;
    rn[tid] = 0.f;
  }
  __syncthreads();

  // the Gram matrix
  if (A.V > 0) {
    for (int h = 0; h < halves; ++h) {
      const int64_t ar = rows[h * TK_BU + (tid >> 2)];                        // (-1: an empty, bad or non-finite slot)
      const bool ua_ok = ar >= 0;
      const float* const pa[1] = {A.table + (ua_ok ? ar : 0) * A.D};
      float* const tile = sim + h * TK_BU * TK_SCLD;
      tk_f32x4 acc[1][2][4];
      tk_tile_accumulate<1, true>(pa, ua_ok, A.table, A.D, 0, N, A.D, tile, acc, pool, A.V);
      tk_store_fragments(acc[0], tile);
      __syncthreads();
    }
  }

  // the diagonal: a slot whose own product is not finite is dead; r
  if (tid < N && live) {
    const float g = sim[tid * TK_SCLD + tid];
    if (!(fabsf(g) < INFINITY)) {
      live = false;
      flags |= NRL_TOPK_E_NAN;
    } else {
      rn[tid] = g == 0.f ? 0.f : mmr_div(1.f, __builtin_sqrtf(g));
    }
  }
  {
    int f = flags;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) f |= __shfl_xor(f, off, 64);
    if (f && lane == 0) atomicOr(A.status, f);
  }
  // relevance: the extremes of the live scores as keys (-0 counts as +0), through the waves' slots of wk
  const uint32_t key = score_key(score);
  if (A.normalize) {
    uint32_t lo = live ? key : 0xFFFFFFFFu, hi = live ? key : 0u;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const uint32_t l2 = (uint32_t)__shfl_xor((int)lo, off, 64), h2 = (uint32_t)__shfl_xor((int)hi, off, 64);
      lo = l2 < lo ? l2 : lo;
      hi = h2 > hi ? h2 : hi;
    }
    if (lane == 0) wk[wave] = ((unsigned long long)hi << 32) | lo;
  }
  __syncthreads();                                    // publishes rn and the extremes
  float rel = score;
  if (A.normalize) {
    uint32_t lo = 0xFFFFFFFFu, hi = 0u;
#pragma unroll
    for (int w = 0; w < TK_THREADS / 64; ++w) {
      const unsigned long long e = wk[w];
      const uint32_t l2 = (uint32_t)e, h2 = (uint32_t)(e >> 32);
      lo = l2 < lo ? l2 : lo;
      hi = h2 > hi ? h2 : hi;
    }
    if (hi == lo || hi == 0u) {
      rel = 0.f;
    } else {
      const float s_min = tk_unkey(lo), s_max = tk_unkey(hi);
      rel = mmr_div(mmr_sub(score, s_min), mmr_sub(s_max, s_min));
    }
  }
  if (A.similarity == 0) {
    for (int e = tid; e < N * TK_BV; e += TK_THREADS) {
      const int i = e / TK_BV, j = e % TK_BV;
      float* const p = sim + i * TK_SCLD + j;
      *p = mmr_mul(*p, mmr_mul(rn[i], rn[j]));
    }
  }
  __syncthreads();                                    // sim is final; wk is free for the steps

  const float lrel = mmr_mul(A.lambda, rel), om = mmr_sub(1.f, A.lambda);
  float pen = 0.f;
  bool sel = false;
  int c = -1, t = 0;
  for (; t < k; ++t) {
    if (t > 0) {
      const float s = tid < N ? sim[c * TK_SCLD + tid] : 0.f;
      pen = t == 1 ? s : fmaxf(pen, s);
    }
    const float obj = mmr_sub(lrel, mmr_mul(om, pen));
    unsigned long long e = 0ull;
    if (live && !sel) e = obj != obj ? ((1ull << 32) | (uint32_t)~(uint32_t)tid) : tk_entry(obj, (uint32_t)tid);
    e = mmr_wave_max(e, lane);
    const int par = t & 1;
    if (lane == 0) wk[par * 4 + wave] = e;
    if (tid < MMR_MAX_POOL) objs[par * MMR_MAX_POOL + tid] = obj;
    __syncthreads();
    unsigned long long best = wk[par * 4];
#pragma unroll
    for (int w = 1; w < TK_THREADS / 64; ++w) {
      const unsigned long long y = wk[par * 4 + w];
      best = y > best ? y : best;
    }
    if (best == 0ull) break;                          // the live slots have run out (uniform)
    c = (int)~(uint32_t)best;
    if (tid == c) sel = true;
    if (tid == 0) {
      A.out_idx[u * k + t] = rows[c];
      A.out_score[u * k + t] = scs[c];
      A.out_mmr[u * k + t] = objs[par * MMR_MAX_POOL + c];
    }
  }
  for (int p = t + tid; p < k; p += TK_THREADS) {
    A.out_idx[u * k + p] = -1;
    A.out_score[u * k + p] = -INFINITY;
    A.out_mmr[u * k + p] = -INFINITY;
  }
}

// ---- calibrated greedy re-ranking of a pool (nrl_calibrated_rerank) ----------------------------------------------------------------
// mmr_rerank_kernel's workgroup (one per user, thread i owns slot i) with a third term in the objective: gamma times the
// Personalization value the list would have after adding a slot of class c, cal_c.  GRAM = false is the mu == 0 form: no Gram
// matrix, no tile LDS, the table is never read.  Dynamic LDS, behind the `halves` Gram tiles of the GRAM form:
//   wk[2][4] u64     the waves' best entries of a step, double-buffered by the step's parity
//   rows[128] i64    the slots' table rows (the Gram stage gathers by them)
//   rn[128] f32      1 / sqrt(G[i][i])
//   cls[128] i32     the slots' classes, -1 where the slot is dead or its class is outside [0, S)
//   tgt[64] f32      the user's target with the refused entries as +0
//   cnt[2][64] f32   n_j, one copy per wave that owns slots;  cal[2][64] f32  cal_c, likewise
// Only waves 0 and 1 own slots (N <= 128).  Each keeps the class state for itself: lane j holds n_j in a register and stores it
// to its wave's cnt row, lane c < S sums its two chains over broadcast reads of cnt and tgt (every lane the same word: no
// conflict) and stores cal_c, lane i reads cal[class_i].  A wave's LDS operations complete in order, so inside one wave these
// stores and reads need a compiler fence and no barrier; the redundant copy costs no time, the two waves run side by side.  That
// leaves ONE barrier a step, the one that publishes the waves' best entries, as in mmr_rerank_kernel.  The winner's thread
// writes the step's outputs from its own registers, so there is no objs array.  The gathered read cal[class_i] is a ds_read_b32:
// lanes of one 32-lane half conflict when their classes differ by 32 (same class: a broadcast), so it is conflict-free for
// S <= 32 and at worst 2-way above.
constexpr int CAL_MAX_CLASSES = NRL_CAL_MAX_CLASSES;
constexpr int CAL_SLOT_WAVES = MMR_MAX_POOL / 64;
constexpr size_t CAL_SLOT_BYTES = 2 * 4 * 8 + (size_t)MMR_MAX_POOL * (8 + 4 + 4) + (size_t)CAL_MAX_CLASSES * 4 * (1 + 2 * CAL_SLOT_WAVES);
constexpr size_t cal_lds_bytes(int halves) { return (size_t)halves * TK_TILE_BYTES + CAL_SLOT_BYTES; }
static_assert(CAL_MAX_CLASSES == 64, "lane j of a wave owns class j");
static_assert(2 * cal_lds_bytes(2) <= 160 * 1024, "two workgroups of the largest layout fit a CU");

struct CalArgs {
  const int64_t* pool_idx;
  const float* pool_score;
  const float* table;
  int32_t N, D, k;
  int64_t V;
  const int32_t* row_class;
  const float* target;
  int32_t S;
  float lambda, mu, gamma;
  int32_t similarity, normalize;
  int64_t* out_idx;
  float* out_score;
  float* out_obj;
  float* out_cal;
  int32_t* status;
};

__device__ __forceinline__ float cal_add(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}

template <bool GRAM>
__global__ __launch_bounds__(TK_THREADS) void cal_rerank_kernel(CalArgs A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char tk_smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int N = A.N, k = A.k, S = A.S;
  const int halves = GRAM ? (N + TK_BU - 1) / TK_BU : 0;
  const int64_t u = blockIdx.x;
  float* const sim = reinterpret_cast<float*>(tk_smem);
  unsigned long long* const wk = reinterpret_cast<unsigned long long*>(tk_smem + (size_t)halves * TK_TILE_BYTES);
  int64_t* const rows = reinterpret_cast<int64_t*>(wk + 8);
  float* const rn = reinterpret_cast<float*>(rows + MMR_MAX_POOL);
  int32_t* const cls = reinterpret_cast<int32_t*>(rn + MMR_MAX_POOL);
  float* const tgt = reinterpret_cast<float*>(cls + MMR_MAX_POOL);
  float* const cnt = tgt + CAL_MAX_CLASSES;
  float* const cal = cnt + CAL_SLOT_WAVES * CAL_MAX_CLASSES;
  const int64_t* const pool = A.pool_idx + u * N;

  // the slots: thread i owns slot i; the target: thread j its entry j
  bool live = false;
  float score = 0.f;
  int64_t row = -1;
  int flags = 0;
  if (tid < MMR_MAX_POOL) {
    if (tid < N) {
      row = pool[tid];
      score = A.pool_score[u * N + tid];
    }
    const bool row_ok = row >= 0 && row < A.V;
    const bool fin = fabsf(score) < INFINITY;
    if (row != -1 && !row_ok) flags |= NRL_MMR_E_ROW;
    if (row_ok && !fin) flags |= NRL_TOPK_E_NAN;
    live = row_ok && fin;
    rows[tid] = live ? row : -1;
    rn[tid] = 0.f;
  }
  if (tid < CAL_MAX_CLASSES) {
    float g = 0.f;
    if (tid < S) {
      g = A.target[u * S + tid];
      if (!(fabsf(g) < INFINITY && g >= 0.f)) {
        g = 0.f;
        flags |= NRL_CAL_E_TARGET;
      }
    }
    tgt[tid] = g;
  }
  __syncthreads();

  if (GRAM) {
    // the Gram matrix, as in mmr_rerank_kernel
    if (A.V > 0) {
      for (int h = 0; h < halves; ++h) {
        const int64_t ar = rows[h * TK_BU + (tid >> 2)];                      // (-1: an empty, bad or non-finite slot)
        const bool ua_ok = ar >= 0;
        const float* const pa[1] = {A.table + (ua_ok ? ar : 0) * A.D};
        float* const tile = sim + h * TK_BU * TK_SCLD;
        tk_f32x4 acc[1][2][4];
        tk_tile_accumulate<1, true>(pa, ua_ok, A.table, A.D, 0, N, A.D, tile, acc, pool, A.V);
        tk_store_fragments(acc[0], tile);
        __syncthreads();
      }
    }
    // the diagonal: a slot whose own product is not finite is dead; r
    if (tid < N && live) {
      const float g = sim[tid * TK_SCLD + tid];
      if (!(fabsf(g) < INFINITY)) {
        live = false;
        flags |= NRL_TOPK_E_NAN;
      } else {
        rn[tid] = g == 0.f ? 0.f : mmr_div(1.f, __builtin_sqrtf(g));
      }
    }
  }
  // the class of a live slot
  int cl = -1;
  if (live) {
    cl = A.row_class[row];
    if (cl < 0 || cl >= S) {
      cl = -1;
      flags |= NRL_TOPK_E_CLASS;
    }
  }
  if (tid < MMR_MAX_POOL) cls[tid] = cl;
  {
    int f = flags;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) f |= __shfl_xor(f, off, 64);
    if (f && lane == 0) atomicOr(A.status, f);
  }
  // relevance: the extremes of the live scores as keys (-0 counts as +0), through the waves' slots of wk
  const uint32_t key = score_key(score);
  if (A.normalize) {
    uint32_t lo = live ? key : 0xFFFFFFFFu, hi = live ? key : 0u;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const uint32_t l2 = (uint32_t)__shfl_xor((int)lo, off, 64), h2 = (uint32_t)__shfl_xor((int)hi, off, 64);
      lo = l2 < lo ? l2 : lo;
      hi = h2 > hi ? h2 : hi;
    }
    if (lane == 0) wk[wave] = ((unsigned long long)hi << 32) | lo;
  }
  __syncthreads();                                    // publishes rn, cls and the extremes
  float rel = score;
  if (A.normalize) {
    uint32_t lo = 0xFFFFFFFFu, hi = 0u;
#pragma unroll
    for (int w = 0; w < TK_THREADS / 64; ++w) {
      const unsigned long long e = wk[w];
      const uint32_t l2 = (uint32_t)e, h2 = (uint32_t)(e >> 32);
      lo = l2 < lo ? l2 : lo;
      hi = h2 > hi ? h2 : hi;
    }
    if (hi == lo || hi == 0u) {
      rel = 0.f;
    } else {
      const float s_min = tk_unkey(lo), s_max = tk_unkey(hi);
      rel = mmr_div(mmr_sub(score, s_min), mmr_sub(s_max, s_min));
    }
  }
  if (GRAM && A.similarity == 0) {
    for (int e = tid; e < N * TK_BV; e += TK_THREADS) {
      const int i = e / TK_BV, j = e % TK_BV;
      float* const p = sim + i * TK_SCLD + j;
      *p = mmr_mul(*p, mmr_mul(rn[i], rn[j]));
    }
  }
  __syncthreads();                                    // sim is final; wk is free for the steps

  const float lrel = mmr_mul(A.lambda, rel);
  const bool slot_wave = wave < CAL_SLOT_WAVES && wave * 64 < N;           // (uniform: this wave owns slots)
  float* const my_cnt = cnt + (wave & (CAL_SLOT_WAVES - 1)) * CAL_MAX_CLASSES;
  float* const my_cal = cal + (wave & (CAL_SLOT_WAVES - 1)) * CAL_MAX_CLASSES;
  float pen = 0.f, nj = 0.f;
  bool sel = false;
  int c = -1, t = 0;
  for (; t < k; ++t) {
    if (t > 0) {
      if (GRAM) {
        const float s = tid < N ? sim[c * TK_SCLD + tid] : 0.f;
        pen = t == 1 ? s : fmaxf(pen, s);
      }
      if (lane == cls[c]) nj += 1.f;                  // (cls[c] == -1: the winner counts for no class)
    }
    float calv = 0.f;
    if (slot_wave) {
      my_cnt[lane] = nj;
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      if (lane < S) {
        float m = 0.f, x = 0.f;
        for (int j = 0; j < S; ++j) {
          const float n1 = my_cnt[j] + (j == lane ? 1.f : 0.f), g = tgt[j];
          m = cal_add(m, fminf(n1, g));
          x = cal_add(x, fmaxf(n1, g));
        }
        my_cal[lane] = mmr_div(m, x);
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      if (cl >= 0) calv = my_cal[cl];
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    }
    const float obj = cal_add(mmr_sub(lrel, mmr_mul(A.mu, pen)), mmr_mul(A.gamma, calv));
    unsigned long long e = 0ull;
    if (live && !sel) e = obj != obj ? ((1ull << 32) | (uint32_t)~(uint32_t)tid) : tk_entry(obj, (uint32_t)tid);
    e = mmr_wave_max(e, lane);
    const int par = t & 1;
    if (lane == 0) wk[par * 4 + wave] = e;
    __syncthreads();
    unsigned long long best = wk[par * 4];
#pragma unroll
    for (int w = 1; w < TK_THREADS / 64; ++w) {
      const unsigned long long y = wk[par * 4 + w];
      best = y > best ? y : best;
    }
    if (best == 0ull) break;                          // the live slots have run out (uniform)
    c = (int)~(uint32_t)best;
    if (tid == c) {
      sel = true;
      A.out_idx[u * k + t] = row;
      A.out_score[u * k + t] = score;
      A.out_obj[u * k + t] = obj;
      A.out_cal[u * k + t] = calv;
    }
  }
  for (int p = t + tid; p < k; p += TK_THREADS) {
    A.out_idx[u * k + p] = -1;
    A.out_score[u * k + p] = -INFINITY;
    A.out_obj[u * k + p] = -INFINITY;
    A.out_cal[u * k + p] = -INFINITY;
  }
}

// ---- greedy DPP re-ranking of a pool (nrl_dpp_rerank) ------------------------------------------------------------------------------
// mmr_rerank_kernel's workgroup (one per user, thread i owns slot i) running the fast greedy MAP inference of a determinantal point
// process (Chen, Zhang, Zhou 2018): an incremental Cholesky factorisation of L = diag(q) sim diag(q), formed in place over the Gram
// tiles in the pass that applies the cosine scaling.  Dynamic LDS, behind the `halves` Gram tiles:
//   wk[2][4] u64     the waves' best entries of a step, double-buffered by the parity of the barrier count
//   rows[128] i64    the slots' table rows (the Gram stage gathers by them)
//   rn[128] f32      1 / sqrt(G[i][i]);  qs[128] f32  the slots' qualities, +0 where the slot is dead
//   cv[k][128] f32   the Cholesky rows, step-major and sized from k at launch: cv[s][i] = e_i of step s
// d2_i, thr_i and the live / selected flags of slot i live in the registers of thread i.  After the barrier of step t has named the
// winner c, thread i walks s = 0 ... t - 1 reading cv[s][i] (lane i word s * 128 + i: consecutive lanes consecutive banks) and
// cv[s][c] (every lane the same word: a broadcast), then L[c][i], the ROW of the winner as MMR reads sim[c][i], and stores
// cv[t][i].  Thread i alone writes column i of cv, and cv[t][.] is first read after the NEXT step's barrier, so a step costs ONE
// barrier, the one that publishes the waves' best entries; the winner's d2 travels in the key of its entry (it is positive, so
// tk_unkey returns its bits).  When no slot is eligible the fill phase lists the rest by pool score through the same entries.
constexpr int DPP_MAX_K = NRL_DPP_MAX_K;
constexpr size_t DPP_SLOT_BYTES = 2 * 4 * 8 + (size_t)MMR_MAX_POOL * (8 + 4 + 4);
constexpr size_t dpp_lds_bytes(int halves, int k) { return (size_t)halves * TK_TILE_BYTES + DPP_SLOT_BYTES + (size_t)k * MMR_MAX_POOL * 4; }
static_assert(DPP_MAX_K <= MMR_MAX_POOL, "a list is no longer than a pool");
static_assert((2 * TK_TILE_BYTES + DPP_SLOT_BYTES) % 16 == 0, "the Cholesky rows start 16-byte aligned");
static_assert(dpp_lds_bytes(2, DPP_MAX_K) <= 160 * 1024, "the largest layout (two tiles, 64 Cholesky rows, the slots) fits a CU");
static_assert(2 * dpp_lds_bytes(2, 16) <= 160 * 1024, "up to k = 16 two workgroups of the largest pool fit a CU");

struct DppArgs {
  const int64_t* pool_idx;
  const float* pool_score;
  const float* quality;
  const float* table;
  int32_t N, D, k;
  int64_t V;
  float alpha, eps;
  int32_t similarity, normalize;
  int64_t* out_idx;
  float* out_score;
  float* out_gain;
  int32_t* status;
};

__global__ __launch_bounds__(TK_THREADS) void dpp_rerank_kernel(DppArgs A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char tk_smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int N = A.N, k = A.k;
  const int halves = (N + TK_BU - 1) / TK_BU;
  const int64_t u = blockIdx.x;
  float* const sim = reinterpret_cast<float*>(tk_smem);
  unsigned long long* const wk = reinterpret_cast<unsigned long long*>(tk_smem + (size_t)halves * TK_TILE_BYTES);
  int64_t* const rows = reinterpret_cast<int64_t*>(wk + 8);
  float* const rn = reinterpret_cast<float*>(rows + MMR_MAX_POOL);
  float* const qs = rn + MMR_MAX_POOL;
  float* const cv = qs + MMR_MAX_POOL;
  const int64_t* const pool = A.pool_idx + u * N;

  // the slots: thread i owns slot i
  bool live = false;
  float score = 0.f, q = 0.f;
  int64_t row = -1;
  int flags = 0;
  if (tid < MMR_MAX_POOL) {
    if (tid < N) {
      row = pool[tid];
      score = A.pool_score[u * N + tid];
    }
    const bool row_ok = row >= 0 && row < A.V;
    const bool fin = fabsf(score) < INFINITY;
    if (row != -1 && !row_ok) flags |= NRL_MMR_E_ROW;
    if (row_ok && !fin) flags |= NRL_TOPK_E_NAN;
    live = row_ok && fin;
    if (live && A.quality) {
      q = A.quality[u * N + tid];
      if (!(q >= 0.f && q < INFINITY)) {
        live = false;
        flags |= NRL_DPP_E_QUALITY;
      }
    }
    rows[tid] = live ? row : -1;
    rn[tid] = 0.f;
  }
  __syncthreads();

  // the Gram matrix, as in mmr_rerank_kernel
  if (A.V > 0) {
    for (int h = 0; h < halves; ++h) {
      const int64_t ar = rows[h * TK_BU + (tid >> 2)];                        // (-1: an empty, bad or non-finite slot)
      const bool ua_ok = ar >= 0;
      const float* const pa[1] = {A.table + (ua_ok ? ar : 0) * A.D};
      float* const tile = sim + h * TK_BU * TK_SCLD;
      tk_f32x4 acc[1][2][4];
      tk_tile_accumulate<1, true>(pa, ua_ok, A.table, A.D, 0, N, A.D, tile, acc, pool, A.V);
      tk_store_fragments(acc[0], tile);
      __syncthreads();
    }
  }

  // the diagonal: a slot whose own product is not finite is dead; r
  if (tid < N && live) {
    const float g = sim[tid * TK_SCLD + tid];
    if (!(fabsf(g) < INFINITY)) {
      live = false;
      flags |= NRL_TOPK_E_NAN;
    } else {
      rn[tid] = g == 0.f ? 0.f : mmr_div(1.f, __builtin_sqrtf(g));
    }
  }
  // without a given quality: relevance as in mmr_rerank_kernel (the extremes of the live scores as keys, through the waves' slots
  // of wk), then q = exp(alpha rel)
  const bool from_rel = A.quality == nullptr;
  if (from_rel && A.normalize) {
    const uint32_t key = score_key(score);
    uint32_t lo = live ? key : 0xFFFFFFFFu, hi = live ? key : 0u;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const uint32_t l2 = (uint32_t)__shfl_xor((int)lo, off, 64), h2 = (uint32_t)__shfl_xor((int)hi, off, 64);
      lo = l2 < lo ? l2 : lo;
      hi = h2 > hi ? h2 : hi;
    }
    if (lane == 0) wk[wave] = ((unsigned long long)hi << 32) | lo;
    __syncthreads();                                  // publishes the extremes (uniform branch)
  }
  if (from_rel) {
    float rel = score;
    if (A.normalize) {
      uint32_t lo = 0xFFFFFFFFu, hi = 0u;
#pragma unroll
      for (int w = 0; w < TK_THREADS / 64; ++w) {
        const unsigned long long e = wk[w];
        const uint32_t l2 = (uint32_t)e, h2 = (uint32_t)(e >> 32);
        lo = l2 < lo ? l2 : lo;
        hi = h2 > hi ? h2 : hi;
      }
      if (hi == lo || hi == 0u) {
        rel = 0.f;
      } else {
        const float s_min = tk_unkey(lo), s_max = tk_unkey(hi);
        rel = mmr_div(mmr_sub(score, s_min), mmr_sub(s_max, s_min));
      }
    }
    q = expf(mmr_mul(A.alpha, rel));
  }
  if (tid < MMR_MAX_POOL) qs[tid] = live ? q : 0.f;
  __syncthreads();                                    // publishes rn and qs; the extremes in wk have been read

  // the kernel matrix, in place: L[i][j] = (q_i q_j) sim[i][j]
  const bool cosine = A.similarity == 0;
  for (int e = tid; e < N * TK_BV; e += TK_THREADS) {
    const int i = e / TK_BV, j = e % TK_BV;
    float* const p = sim + i * TK_SCLD + j;
    float s = *p;
    if (cosine) s = mmr_mul(s, mmr_mul(rn[i], rn[j]));
    *p = mmr_mul(mmr_mul(qs[i], qs[j]), s);
  }
  __syncthreads();                                    // L is final; wk is free for the steps

  float d2 = 0.f, thr = 0.f;
  if (tid < N && live) {
    d2 = sim[tid * TK_SCLD + tid];
    if (!(fabsf(d2) < INFINITY)) {
      live = false;
      flags |= NRL_TOPK_E_NAN;
    }
    thr = mmr_mul(A.eps, d2);
  }
  {
    int f = flags;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) f |= __shfl_xor(f, off, 64);
    if (f && lane == 0) atomicOr(A.status, f);
  }

  // a step's ONE barrier: the largest of the threads' entries, through the waves' slots of wk; par counts the barriers
  int par = 0;
  auto best_entry = [&](unsigned long long e) {
    e = mmr_wave_max(e, lane);
    if (lane == 0) wk[par * 4 + wave] = e;
    __syncthreads();
    unsigned long long best = wk[par * 4];
#pragma unroll
    for (int w = 1; w < TK_THREADS / 64; ++w) {
      const unsigned long long y = wk[par * 4 + w];
      best = y > best ? y : best;
    }
    par ^= 1;
    return best;
  };

  // the DPP phase
  bool sel = false;
  int c = -1, t = 0;
  float d2c = 0.f;
  for (; t < k; ++t) {
    if (t > 0 && tid < N && live && !sel) {
      float acc = 0.f;
      for (int s = 0; s < t - 1; ++s) acc = cal_add(acc, mmr_mul(cv[s * MMR_MAX_POOL + c], cv[s * MMR_MAX_POOL + tid]));
      const float e = mmr_div(mmr_sub(sim[c * TK_SCLD + tid], acc), __builtin_sqrtf(d2c));
      cv[(t - 1) * MMR_MAX_POOL + tid] = e;
      d2 = mmr_sub(d2, mmr_mul(e, e));
    }
    const bool eligible = live && !sel && d2 > 0.f && d2 >= thr;
    const unsigned long long best = best_entry(eligible ? tk_entry(d2, (uint32_t)tid) : 0ull);
    if (best == 0ull) break;                          // no slot is eligible: the DPP phase is over for good (uniform)
    c = (int)~(uint32_t)best;
    d2c = tk_unkey((uint32_t)(best >> 32));           // (d2_c > 0: the key gives its bits back)
    if (tid == c) {
      sel = true;
      A.out_idx[u * k + t] = row;
      A.out_score[u * k + t] = score;
      A.out_gain[u * k + t] = d2;
    }
  }
  // the fill phase: the live slots left over, by (pool score descending, slot ascending)
  for (const int t0 = t; t < k; ++t) {
    const unsigned long long best = best_entry(live && !sel ? tk_entry(score, (uint32_t)tid) : 0ull);
    if (best == 0ull) break;                          // the live slots have run out (uniform)
    if (tid == (int)~(uint32_t)best) {
      sel = true;
      A.out_idx[u * k + t] = row;
      A.out_score[u * k + t] = score;
      A.out_gain[u * k + t] = 0.f;
      if (t == t0) atomicOr(A.status, NRL_DPP_E_RANK);
    }
  }
  for (int p = t + tid; p < k; p += TK_THREADS) {
    A.out_idx[u * k + p] = -1;
    A.out_score[u * k + p] = -INFINITY;
    A.out_gain[u * k + p] = -INFINITY;
  }
}

static bool tk_shape_ok(int64_t B, int64_t V, int32_t D, int32_t k) {
  return B >= 0 && V >= 0 && V < ((int64_t)1 << 31) && D > 0 && D % 4 == 0 && D <= NRL_TOPK_MAX_D && k >= 1 && k <= NRL_TOPK_MAX_K;
}

// how many pieces of V run in parallel per user tile (`lists`: what the workspace is sized for) and the table tiles of each
// (`bu` users per workgroup: TK_BU, or the whole users of a multi-interest tile)
static void tk_plan(int64_t B, int64_t V, int32_t slices, int64_t bu, int64_t& lists, int64_t& used, int64_t& tiles_per_slice) {
  const int64_t nvt = ceil_div(V, TK_BV), ut = ceil_div(B, bu);
  int64_t want = slices > 0 ? slices : ceil_div(TK_TARGET_BLOCKS, ut > 0 ? ut : 1);
  if (want > nvt) want = nvt;
  if (want < 1) want = 1;
  lists = want;
  tiles_per_slice = nvt > 0 ? ceil_div(nvt, want) : 1;
  used = nvt > 0 ? ceil_div(nvt, tiles_per_slice) : 0;
}

// the checks both entries make, in this order; `who` is the entry's name in the message
static int tk_check(const char* who, int64_t B, int64_t V, int32_t D, int32_t k, const int64_t* excl_idx, const int64_t* excl_off) {
  NRL_REQUIRE(k >= 1 && k <= NRL_TOPK_MAX_K, "%s: k in [1, %d] (got %d)", who, NRL_TOPK_MAX_K, k);
  NRL_REQUIRE(D > 0 && D % 4 == 0 && D <= NRL_TOPK_MAX_D, "%s: D a multiple of 4 in [4, %d] (got %d)", who, NRL_TOPK_MAX_D, D);
  NRL_REQUIRE(V < ((int64_t)1 << 31), "%s: at most 2^31 - 1 table rows (got %lld)", who, (long long)V);
  NRL_REQUIRE(B < ((int64_t)1 << 31), "%s: at most 2^31 - 1 users per call (got %lld)", who, (long long)B);
  NRL_REQUIRE((excl_idx == nullptr) == (excl_off == nullptr) || excl_off, "%s: excl_idx without excl_off", who);
  return NRL_OK;
}

// the arguments every kernel of the unit reads, in the order of TkArgs; the launcher sets the two slice fields
static TkArgs tk_args(const float* user, const float* table, int64_t B, int64_t V, int32_t D, int32_t k, const int64_t* excl_idx,
                      const int64_t* excl_off, const uint8_t* eligible, unsigned long long* partial, int64_t* out_idx,
                      float* out_score, int32_t* status) {
  return TkArgs{user, table, B, (int32_t)V, D, k, excl_idx, excl_off, eligible, 0, 0, partial, out_idx, out_score, status};
}

// the merge that follows a scores kernel: the plain one, or the one under a class cap
struct TkMerge {
  int operator()(const TkArgs& A, hipStream_t st) const {
    tk_merge_kernel<<<(unsigned)A.B, 64, 0, st>>>(A);
    NRL_LAUNCH_CHECK();
    return NRL_OK;
  }
};
struct TkMergeCapped {
  TkCapFields F;
  int operator()(const TkArgs& A, hipStream_t st) const {
    tk_merge_capped_kernel<<<(unsigned)A.B, 64, 0, st>>>(TkWith<TkArgs, TkCapFields>{A, F});
    NRL_LAUNCH_CHECK();
    return NRL_OK;
  }
};

// the checks of a capped entry, after those of the entry it caps
static int tk_cap_check(const char* who, int64_t V, int32_t k, const int32_t* row_class, int32_t max_per_class) {
  NRL_REQUIRE(k <= NRL_TOPK_CAP_MAX_K, "%s: k in [1, %d] under a class cap (got %d)", who, NRL_TOPK_CAP_MAX_K, k);
  NRL_REQUIRE(row_class || V == 0, "%s: row_class is required", who);
  NRL_REQUIRE(max_per_class >= 1, "%s: max_per_class >= 1 (got %d)", who, max_per_class);
  return NRL_OK;
}

// plans the slices, runs `kernel` (`tiles` score tiles, `bu` users per workgroup, `extra_lds` bytes of its own after the layout of
// tk_lds_bytes) over them and then the merge
template <class Args, class Merge = TkMerge>
static int tk_launch(const char* who, void (*kernel)(Args), Args& A, int32_t slices, int tiles, int bu, void* stream,
                     size_t extra_lds = 0, Merge merge = Merge{}) {
  int64_t lists, used, tps;
  tk_plan(A.B, A.V, slices, bu, lists, used, tps);
  const int64_t blocks = ceil_div(A.B, bu) * used;
  NRL_REQUIRE(blocks < ((int64_t)1 << 31), "%s: grid too large (%lld workgroups)", who, (long long)blocks);
  A.slices = (int32_t)used;
  A.tiles_per_slice = (int32_t)tps;
  hipStream_t st = (hipStream_t)stream;
  if (used > 0) {
    const size_t smem = tk_lds_bytes(tiles, bu, A.k) + extra_lds;
    // more than 64 KB of dynamic LDS needs the attribute; it belongs to the current device, so it is set per call
    if (smem > 64 * 1024) NRL_HIP(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    kernel<<<(unsigned)blocks, TK_THREADS, smem, st>>>(A);
    NRL_LAUNCH_CHECK();
  }
  return merge(A, st);
}

// The launches of a rank entry: slots and owners, `target` (the entry's target kernel: a callable that launches it), the count
// kernel with `smem` bytes of dynamic LDS over `blocks` workgroups, the finish.
struct TkcFinish {
  void operator()(const TkcArgs& A, hipStream_t st) const { tkc_finish_kernel<<<(unsigned)A.B, 64, 0, st>>>(A); }
};
struct TkcFinishWindow {
  TkwFields F;
  void operator()(const TkcArgs& A, hipStream_t st) const {
    tkwc_finish_kernel<<<(unsigned)A.B, 64, 0, st>>>(TkWith<TkcArgs, TkwFields>{A, F});
  }
};
template <class Args, class Target, class Finish = TkcFinish>
static int tkc_launch(void (*count)(Args), Args& A, int64_t blocks, size_t smem, void* stream, Target target,
                      Finish finish = Finish{}) {
  hipStream_t st = (hipStream_t)stream;
  if (A.n_targets > 0) {
    tkc_init_kernel<<<(unsigned)A.n_targets, 64, 0, st>>>(static_cast<const TkcArgs&>(A));
    NRL_LAUNCH_CHECK();
    tkc_owner_kernel<<<(unsigned)ceil_div(A.B, 256), 256, 0, st>>>(static_cast<const TkcArgs&>(A));
    NRL_LAUNCH_CHECK();
    if (A.V > 0) NRL_TRY(target(st));
  }
  if (blocks > 0) {
    // more than 64 KB of dynamic LDS needs the attribute; it belongs to the current device, so it is set per call
    NRL_HIP(hipFuncSetAttribute((const void*)count, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    count<<<(unsigned)blocks, TK_THREADS, smem, st>>>(A);
    NRL_LAUNCH_CHECK();
  }
  finish(static_cast<const TkcArgs&>(A), st);
  NRL_LAUNCH_CHECK();
  return NRL_OK;
}

// the checks of a windowed entry, after those of the entry it windows
static int tk_window_check(const char* who, int64_t B, int64_t V, const TkwFields& win) {
  NRL_REQUIRE(win.row_time || V == 0, "%s: row_time is required", who);
  NRL_REQUIRE((win.win_lo && win.win_hi) || B == 0, "%s: win_lo and win_hi are required", who);
  return NRL_OK;
}

}  // namespace nrl

using namespace nrl;

extern "C" {

// k packed (score, index) keys per (user, slice list); never empty
static void tk_layout(Arena& a, int64_t B, int64_t V, int32_t k, int32_t slices, int64_t bu, unsigned long long** partial) {
  int64_t lists, used, tps;
  tk_plan(B, V, slices, bu, lists, used, tps);
  const size_t keys = (size_t)B * (size_t)lists * (size_t)k;
  *partial = a.take<unsigned long long>(keys > 0 ? keys : 1);
}

size_t nrl_topk_scores_workspace_bytes(int64_t B, int64_t V, int32_t D, int32_t k, int32_t slices) {
  if (!tk_shape_ok(B, V, D, k) || slices < 0) return 256;
  return measure_workspace<unsigned long long*>([&](Arena& a, auto* w) { tk_layout(a, B, V, k, slices, TK_BU, w); });
}

// nrl_topk_scores (`cap` and `win` null), nrl_topk_scores_capped and nrl_topk_window_scores: one sequence of checks, one layout; the
// cap or the window picks the kernels
static int tk_scores_entry(const char* who, const float* user_vec, const float* table, int64_t B, int64_t V, int32_t D, int32_t k,
                           const TkCapFields* cap, const TkwFields* win, const int64_t* excl_idx, const int64_t* excl_off, const uint8_t* eligible,
                           int32_t slices, int64_t* out_idx, float* out_score, int32_t* status, void* ws, size_t ws_bytes,
                           void* stream) {
  NRL_REQUIRE(B >= 0 && V >= 0 && D >= 0 && slices >= 0, "%s: negative size", who);
  NRL_TRY(tk_check(who, B, V, D, k, excl_idx, excl_off));
  NRL_REQUIRE(status, "%s: the status word is required", who);
  if (cap) NRL_TRY(tk_cap_check(who, V, k, cap->row_class, cap->m));
  if (B == 0) return NRL_OK;
  NRL_REQUIRE(out_idx && out_score && user_vec && (V == 0 || table), "%s: null argument", who);
  if (win) NRL_TRY(tk_window_check(who, B, V, *win));
  unsigned long long* partial;
  NRL_TRY(carve_workspace(ws, ws_bytes, [&](Arena& a) { tk_layout(a, B, V, k, slices, TK_BU, &partial); }));
  TkArgs A = tk_args(user_vec, table, B, V, D, k, excl_idx, excl_off, eligible, partial, out_idx, out_score, status);
  if (win) {
    TkWith<TkArgs, TkwFields> W{A, *win};
    return tk_launch(who, tkw_scores_kernel, W, slices, 1, TK_BU, stream, tkw_lds_bytes(TK_BU));
  }
  if (!cap) return tk_launch(who, tk_scores_kernel, A, slices, 1, TK_BU, stream);
  TkWith<TkArgs, TkCapFields> C{A, *cap};
  return tk_launch(who, tkcap_scores_kernel, C, slices, 1, TK_BU, stream, 0, TkMergeCapped{*cap});
}

int nrl_topk_scores(const float* user_vec, const float* table, int64_t B, int64_t V, int32_t D, int32_t k, const int64_t* excl_idx,
                    const int64_t* excl_off, const uint8_t* eligible, int32_t slices, int64_t* out_idx, float* out_score,
                    int32_t* status, void* ws, size_t ws_bytes, void* stream) {
  return tk_scores_entry("topk_scores", user_vec, table, B, V, D, k, nullptr, nullptr, excl_idx, excl_off, eligible, slices, out_idx, out_score,
                         status, ws, ws_bytes, stream);
}

int nrl_topk_scores_capped(const float* user_vec, const float* table, int64_t B, int64_t V, int32_t D, int32_t k,
                           const int32_t* row_class, int32_t max_per_class, const int64_t* excl_idx, const int64_t* excl_off,
                           const uint8_t* eligible, int32_t slices, int64_t* out_idx, float* out_score, int32_t* status, void* ws,
                           size_t ws_bytes, void* stream) {
  const TkCapFields cap{row_class, max_per_class};
  return tk_scores_entry("topk_scores_capped", user_vec, table, B, V, D, k, &cap, nullptr, excl_idx, excl_off, eligible, slices, out_idx,
                         out_score, status, ws, ws_bytes, stream);
}

int nrl_topk_window_scores(const float* user_vec, const float* table, int64_t B, int64_t V, int32_t D, int32_t k,
                           const int32_t* row_time, const int32_t* win_lo, const int32_t* win_hi, const int64_t* excl_idx,
                           const int64_t* excl_off, const uint8_t* eligible, int32_t slices, int64_t* out_idx, float* out_score,
                           int32_t* status, void* ws, size_t ws_bytes, void* stream) {
  const TkwFields win{row_time, win_lo, win_hi};
  return tk_scores_entry("topk_window_scores", user_vec, table, B, V, D, k, nullptr, &win, excl_idx, excl_off, eligible, slices,
                         out_idx, out_score, status, ws, ws_bytes, stream);
}

// nrl_topk_sampled_scores: the checks and the layout of nrl_topk_scores, then its own; tks_scores_kernel over the slices, the plain
// merge (out_key takes the place of out_score), then the raw scores of the merged rows
struct TkMergeSampled {
  float* out_score;
  int operator()(const TkArgs& A, hipStream_t st) const {
    NRL_TRY(TkMerge{}(A, st));
    const int64_t n = A.B * A.k;
    tks_raw_kernel<<<(unsigned)ceil_div(n, TK_BU), TK_THREADS, 0, st>>>(TksRawArgs{A.user, A.table, A.out_idx, out_score, A.V, (int32_t)n, A.D, A.k});
    NRL_LAUNCH_CHECK();
    return NRL_OK;
  }
};

size_t nrl_topk_sampled_scores_workspace_size(int64_t B, int64_t V, int32_t D, int32_t k, int32_t slices) {
  return nrl_topk_scores_workspace_bytes(B, V, D, k, slices);                // (the raw scores read their rows in place)
}

int nrl_topk_sampled_scores(const float* user_vec, const float* table, int64_t B, int64_t V, int32_t D, int32_t k,
                            const int64_t* user_key, uint64_t seed, float inv_temp, const int64_t* excl_idx, const int64_t* excl_off,
                            const uint8_t* eligible, int32_t slices, int64_t* out_idx, float* out_key, float* out_score, int32_t* status,
                            void* ws, size_t ws_bytes, void* stream) {
  const char* who = "topk_sampled_scores";
  NRL_REQUIRE(B >= 0 && V >= 0 && D >= 0 && slices >= 0, "%s: negative size", who);
  NRL_TRY(tk_check(who, B, V, D, k, excl_idx, excl_off));
  NRL_REQUIRE(status, "%s: the status word is required", who);
  NRL_REQUIRE(inv_temp >= 0.f && inv_temp < INFINITY, "%s: inv_temp finite and >= 0 (got %g)", who, (double)inv_temp);
  NRL_REQUIRE(B * (int64_t)k < ((int64_t)1 << 31), "%s: at most 2^31 - 1 list slots per call (got %lld)", who, (long long)(B * k));
  if (B == 0) return NRL_OK;
  NRL_REQUIRE(out_idx && out_key && out_score && user_vec && (V == 0 || table), "%s: null argument", who);
  NRL_REQUIRE(user_key, "%s: user_key is required", who);
  unsigned long long* partial;
  NRL_TRY(carve_workspace(ws, ws_bytes, [&](Arena& a) { tk_layout(a, B, V, k, slices, TK_BU, &partial); }));
  TkWith<TkArgs, TksFields> A{tk_args(user_vec, table, B, V, D, k, excl_idx, excl_off, eligible, partial, out_idx, out_key, status),
                              TksFields{user_key, tks_call_key(seed), inv_temp}};
  return tk_launch(who, tks_scores_kernel, A, slices, 1, TK_BU, stream, TKS_EXTRA_LDS, TkMergeSampled{out_score});
}

int nrl_gumbel_noise(const int64_t* user_key, const int64_t* row, int64_t n, uint64_t seed, float* out_u, float* out_g, void* stream) {
  NRL_REQUIRE(n >= 0 && ceil_div(n, 256) < ((int64_t)1 << 31), "gumbel_noise: n in [0, 2^39) (got %lld)", (long long)n);
  if (n == 0) return NRL_OK;
  NRL_REQUIRE(user_key && row && (out_u || out_g), "gumbel_noise: null argument");
  tks_noise_kernel<<<(unsigned)ceil_div(n, 256), 256, 0, (hipStream_t)stream>>>(user_key, row, n, tks_call_key(seed), out_u, out_g);
  NRL_LAUNCH_CHECK();
  return NRL_OK;
}

// nrl_topk_sampled_draws: the checks of nrl_topk_sampled_scores, then its own; the R draws in groups of tkd_group draws per walk
// (tkd_scores_kernel, tkd_merge_kernel; no output bit depends on the grouping), then tks_raw_kernel over all B R k slots
size_t nrl_topk_sampled_draws_workspace_size(int64_t B, int64_t V, int32_t D, int32_t k, int32_t R, int32_t slices) {
  if (R < 1 || R > NRL_TOPK_MAX_DRAWS || k < 1 || k > NRL_TOPK_MAX_K) return 256;
  return nrl_topk_scores_workspace_bytes(B, V, D, R * k, slices);            // (R lists of k entries are one list of R k)
}

// draws per walk: the most that leave two workgroups resident per CU, at least one.  Measured (B = 512, V = 65,536,
// k = 10): 8 draws in walks of 4 or 5 take 0.68 - 0.73x the time of 8 single calls, in walks of 6 or 8 (one workgroup per CU)
// 0.94 - 1.04x -- a second resident workgroup is worth more than the walks it costs.
static int32_t tkd_group(int32_t k, int32_t R) {
  int32_t G = 1;
  while (G < R && 2 * tkd_lds_bytes(G + 1, k) <= 160 * 1024) ++G;
  return G;
}

int nrl_topk_sampled_draws(const float* user_vec, const float* table, int64_t B, int64_t V, int32_t D, int32_t k, int32_t R,
                           const int64_t* excl_idx, const int64_t* excl_off, const uint8_t* eligible, const int64_t* user_key,
                           uint64_t seed, float inv_temp, int32_t slices, int64_t* out_idx, float* out_key, float* out_score,
                           int32_t* status, void* ws, size_t ws_bytes, void* stream) {
  const char* who = "topk_sampled_draws";
  NRL_REQUIRE(B >= 0 && V >= 0 && D >= 0 && slices >= 0, "%s: negative size", who);
  NRL_TRY(tk_check(who, B, V, D, k, excl_idx, excl_off));
  NRL_REQUIRE(status, "%s: the status word is required", who);
  NRL_REQUIRE(inv_temp >= 0.f && inv_temp < INFINITY, "%s: inv_temp finite and >= 0 (got %g)", who, (double)inv_temp);
  NRL_REQUIRE(B * (int64_t)k < ((int64_t)1 << 31), "%s: at most 2^31 - 1 list slots per call (got %lld)", who, (long long)(B * k));
  NRL_REQUIRE(R >= 1 && R <= NRL_TOPK_MAX_DRAWS, "%s: R in [1, %d] (got %d)", who, NRL_TOPK_MAX_DRAWS, R);
  NRL_REQUIRE(R * k <= NRL_TOPK_MAX_K, "%s: R * k at most %d (got %d)", who, NRL_TOPK_MAX_K, R * k);
  NRL_REQUIRE(B * (int64_t)R * k < ((int64_t)1 << 31), "%s: at most 2^31 - 1 list slots per call (got %lld)", who,
              (long long)(B * R * k));
  if (B == 0) return NRL_OK;
  NRL_REQUIRE(out_idx && out_key && out_score && user_vec && (V == 0 || table), "%s: null argument", who);
  NRL_REQUIRE(user_key, "%s: user_key is required", who);
  unsigned long long* partial;
  NRL_TRY(carve_workspace(ws, ws_bytes, [&](Arena& a) { tk_layout(a, B, V, R * k, slices, TK_BU, &partial); }));
  int64_t lists, used, tps;
  tk_plan(B, V, slices, TK_BU, lists, used, tps);
  const int64_t blocks = ceil_div(B, TK_BU) * used;
  NRL_REQUIRE(blocks < ((int64_t)1 << 31), "%s: grid too large (%lld workgroups)", who, (long long)blocks);
  hipStream_t st = (hipStream_t)stream;
  const int32_t G = tkd_group(k, R);
  for (int32_t r0 = 0; r0 < R; r0 += G) {
    TkWith<TkArgs, TkdFields> A;
    static_cast<TkArgs&>(A) = tk_args(user_vec, table, B, V, D, k, excl_idx, excl_off, eligible, partial, out_idx, out_key, status);
    A.slices = (int32_t)used;
    A.tiles_per_slice = (int32_t)tps;
    A.user_key = user_key;
    A.inv_temp = inv_temp;
    A.R = R - r0 < G ? R - r0 : G;
    A.R_all = R;
    A.r0 = r0;
    for (int32_t r = 0; r < NRL_TOPK_MAX_DRAWS; ++r) A.k0[r] = r < A.R ? tks_call_key(seed + (uint64_t)(r0 + r)) : 0u;
    if (used > 0) {
      const size_t smem = tkd_lds_bytes(A.R, k);
      // more than 64 KB of dynamic LDS needs the attribute; it belongs to the current device, so it is set per call
      if (smem > 64 * 1024)
        NRL_HIP(hipFuncSetAttribute((const void*)tkd_scores_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
      tkd_scores_kernel<<<(unsigned)blocks, TK_THREADS, smem, st>>>(A);
      NRL_LAUNCH_CHECK();
    }
    tkd_merge_kernel<<<(unsigned)(B * A.R), 64, 0, st>>>(A);
    NRL_LAUNCH_CHECK();
  }
  const int64_t n = B * (int64_t)R * k;
  tks_raw_kernel<<<(unsigned)ceil_div(n, TK_BU), TK_THREADS, 0, st>>>(TksRawArgs{user_vec, table, out_idx, out_score, V, (int32_t)n, D, R * k});
  NRL_LAUNCH_CHECK();
  return NRL_OK;
}

int nrl_list_class_exposure(const int64_t* list_idx, const int32_t* row_class, const float* pos_weight, int64_t B, int32_t L, int32_t k,
                            int64_t V, int32_t S, float* out, int32_t* status, void* stream) {
  const char* who = "list_class_exposure";
  NRL_REQUIRE(B >= 0 && V >= 0, "%s: negative size", who);
  NRL_REQUIRE(S >= 1 && S <= NRL_TOPK_MAX_BIAS_CLASSES, "%s: S in [1, %d] (got %d)", who, NRL_TOPK_MAX_BIAS_CLASSES, S);
  NRL_REQUIRE(k >= 1 && k <= NRL_TOPK_MAX_K, "%s: k in [1, %d] (got %d)", who, NRL_TOPK_MAX_K, k);
  NRL_REQUIRE(L >= 1, "%s: L >= 1 (got %d)", who, L);
  NRL_REQUIRE(B < ((int64_t)1 << 31), "%s: at most 2^31 - 1 users per call (got %lld)", who, (long long)B);
  NRL_REQUIRE(status, "%s: the status word is required", who);
  if (B == 0) return NRL_OK;
  NRL_REQUIRE(list_idx && pos_weight && out && (V == 0 || row_class), "%s: null argument", who);
  tkx_exposure_kernel<<<(unsigned)B, 64, 0, (hipStream_t)stream>>>(TkxArgs{list_idx, row_class, pos_weight, V, L, k, S, out, status});
  NRL_LAUNCH_CHECK();
  return NRL_OK;
}

// nrl_catalogue_logz: the chunks of tke_statistics (a function of V alone: no `slices`), tkz_sum_kernel over them, tkz_finish_kernel
static void tkz_plan(int64_t V, int32_t& chunks, int32_t& tiles_per_chunk) {
  const int64_t nvt = ceil_div(V, TK_BV);
  tiles_per_chunk = (int32_t)(nvt > 0 ? ceil_div(nvt, NRL_TOPK_STAT_CHUNKS) : 1);
  chunks = (int32_t)(nvt > 0 ? ceil_div(nvt, tiles_per_chunk) : 0);
}
// (n, dropped, m, S, W) per (user, chunk); never empty
static void tkz_layout(Arena& a, int64_t B, int64_t V, float** parts) {
  int32_t chunks, tpc;
  tkz_plan(V, chunks, tpc);
  const size_t words = (size_t)B * (size_t)chunks * TKZ_WORDS;
  *parts = a.take<float>(words > 0 ? words : 1);
}

size_t nrl_catalogue_logz_workspace_size(int64_t B, int64_t V, int32_t D) {
  if (!tk_shape_ok(B, V, D, 1)) return 256;
  return measure_workspace<float*>([&](Arena& a, auto* w) { tkz_layout(a, B, V, w); });
}

int nrl_catalogue_logz(const float* user_vec, const float* table, int64_t B, int64_t V, int32_t D, float inv_temp,
                       const int64_t* excl_idx, const int64_t* excl_off, const uint8_t* eligible, const int64_t* drop_idx, int32_t kd,
                       float* out_max, float* out_logsum, float* out_entropy, int32_t* out_pop, int32_t* out_dropped, int32_t* status,
                       void* ws, size_t ws_bytes, void* stream) {
  const char* who = "catalogue_logz";
  NRL_REQUIRE(B >= 0 && V >= 0 && D >= 0, "%s: negative size", who);
  NRL_TRY(tk_check(who, B, V, D, 1, excl_idx, excl_off));
  NRL_REQUIRE(inv_temp >= 0.f && inv_temp < INFINITY, "%s: inv_temp finite and >= 0 (got %g)", who, (double)inv_temp);
  NRL_REQUIRE(kd >= 0 && kd <= NRL_TOPK_MAX_K, "%s: kd in [0, %d] (got %d)", who, NRL_TOPK_MAX_K, kd);
  NRL_REQUIRE(status, "%s: the status word is required", who);
  if (B == 0) return NRL_OK;
  NRL_REQUIRE(out_max && out_logsum && out_entropy && out_pop && user_vec && (V == 0 || table), "%s: null argument", who);
  NRL_REQUIRE(kd == 0 || (drop_idx && out_dropped), "%s: kd > 0 needs drop_idx and out_dropped", who);
  float* parts;
  NRL_TRY(carve_workspace(ws, ws_bytes, [&](Arena& a) { tkz_layout(a, B, V, &parts); }));
  TkWith<TkArgs, TkzFields> A;
  static_cast<TkArgs&>(A) = tk_args(user_vec, table, B, V, D, 1, excl_idx, excl_off, eligible, nullptr, nullptr, nullptr, status);
  static_cast<TkzFields&>(A) = TkzFields{kd > 0 ? drop_idx : nullptr, kd, inv_temp, parts, out_max, out_logsum, out_entropy, out_pop, out_dropped};
  tkz_plan(V, A.slices, A.tiles_per_slice);
  const int64_t blocks = ceil_div(B, TK_BU) * A.slices;
  NRL_REQUIRE(blocks < ((int64_t)1 << 31), "%s: grid too large (%lld workgroups)", who, (long long)blocks);
  hipStream_t st = (hipStream_t)stream;
  if (blocks > 0) {
    // more than 64 KB of dynamic LDS needs the attribute; it belongs to the current device, so it is set per call
    NRL_HIP(hipFuncSetAttribute((const void*)tkz_sum_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    tkz_sum_kernel<<<(unsigned)blocks, TK_THREADS, TKZ_LDS, st>>>(A);
    NRL_LAUNCH_CHECK();
  }
  tkz_finish_kernel<<<(unsigned)B, 64, 0, st>>>(A);
  NRL_LAUNCH_CHECK();
  return NRL_OK;
}

// nrl_list_logprob: the raw scores of the listed rows as nrl_topk_sampled_scores computes those of the drawn rows, then tkz_list_kernel
int nrl_list_logprob(const float* user_vec, const float* table, int64_t B, int64_t V, int32_t D, float inv_temp, const int64_t* list_idx,
                     int32_t k, const float* tail_max, const float* tail_logsum, const int32_t* tail_pop, const int32_t* tail_dropped,
                     float* out_score, float* out_logp, float* out_total, int32_t* status, void* stream) {
  const char* who = "list_logprob";
  NRL_REQUIRE(B >= 0 && V >= 0 && D >= 0, "%s: negative size", who);
  NRL_TRY(tk_check(who, B, V, D, k, nullptr, nullptr));
  NRL_REQUIRE(inv_temp >= 0.f && inv_temp < INFINITY, "%s: inv_temp finite and >= 0 (got %g)", who, (double)inv_temp);
  NRL_REQUIRE(status, "%s: the status word is required", who);
  NRL_REQUIRE(B * (int64_t)k < ((int64_t)1 << 31), "%s: at most 2^31 - 1 list slots per call (got %lld)", who, (long long)(B * k));
  if (B == 0) return NRL_OK;
  NRL_REQUIRE(list_idx && tail_max && tail_logsum && tail_pop && tail_dropped && out_score && out_logp && out_total && user_vec &&
                  (V == 0 || table),
              "%s: null argument", who);
  hipStream_t st = (hipStream_t)stream;
  const int64_t n = B * k;
  tks_raw_kernel<<<(unsigned)ceil_div(n, TK_BU), TK_THREADS, 0, st>>>(TksRawArgs{user_vec, table, list_idx, out_score, V, (int32_t)n, D, k});
  NRL_LAUNCH_CHECK();
  tkz_list_kernel<<<(unsigned)B, 64, 0, st>>>(
      TkzListArgs{list_idx, out_score, tail_max, tail_logsum, tail_pop, tail_dropped, out_logp, out_total, status, V, k, inv_temp});
  NRL_LAUNCH_CHECK();
  return NRL_OK;
}

// the workspace of nrl_catalogue_ranks: the gathered target rows and their scores and owners, then the per-slice counts
struct TkcWs {
  float *gathered, *tscore;
  int32_t *owner, *pcnt, *tcnt;
};
static void tkc_layout(Arena& a, int64_t B, int64_t V, int32_t D, int64_t n_targets, int32_t slices, int64_t bu, TkcWs* w) {
  int64_t lists, used, tps;
  tk_plan(B, V, slices, bu, lists, used, tps);
  const size_t n = (size_t)n_targets;
  w->gathered = a.take<float>(n * (size_t)D > 0 ? n * (size_t)D : 1);
  w->tscore = a.take<float>(n > 0 ? n : 1);
  w->owner = a.take<int32_t>(n > 0 ? n : 1);
  w->pcnt = a.take<int32_t>((size_t)B * (size_t)lists > 0 ? (size_t)B * (size_t)lists : 1);
  w->tcnt = a.take<int32_t>(n * (size_t)lists > 0 ? n * (size_t)lists : 1);
}

size_t nrl_catalogue_ranks_workspace_size(int64_t B, int64_t V, int32_t D, int64_t n_targets, int32_t slices) {
  if (!tk_shape_ok(B, V, D, 1) || slices < 0 || n_targets < 0 || n_targets >= ((int64_t)1 << 31)) return 256;
  return measure_workspace<TkcWs>([&](Arena& a, auto* w) { tkc_layout(a, B, V, D, n_targets, slices, TK_BU, w); });
}

// the checks every rank entry makes after its own shape checks, in this order; `who` is the entry's name in the message
static int tkc_check(const char* who, int64_t n_targets, const int64_t* tgt_idx, const int64_t* tgt_off, const int32_t* status) {
  NRL_REQUIRE(n_targets < ((int64_t)1 << 31), "%s: at most 2^31 - 1 targets per call (got %lld)", who, (long long)n_targets);
  NRL_REQUIRE(tgt_off || (!tgt_idx && n_targets == 0), "%s: tgt_idx without tgt_off", who);
  NRL_REQUIRE(status, "%s: the status word is required", who);
  return NRL_OK;
}

// Carves the workspace (D floats per gathered target row), plans the slices for `bu` users per workgroup and fills the arguments
// every kernel of a rank entry reads; `gather`: the target kernel reads gathered rows.
static int tkc_prepare(const char* who, TkcArgs& A, const float* user, const float* table, int64_t B, int64_t V, int32_t D,
                       int32_t ws_D, bool gather, const int64_t* tgt_idx, const int64_t* tgt_off, int64_t n_targets,
                       const int64_t* excl_idx, const int64_t* excl_off, const uint8_t* eligible, int32_t slices, int64_t bu,
                       int32_t* out_rank, float* out_score, int32_t* out_ranked, int32_t* status, void* ws, size_t ws_bytes,
                       int64_t* blocks) {
  TkcWs w;
  NRL_TRY(carve_workspace(ws, ws_bytes, [&](Arena& a) { tkc_layout(a, B, V, ws_D, n_targets, slices, bu, &w); }));
  int64_t lists, used, tps;
  tk_plan(B, V, slices, bu, lists, used, tps);
  *blocks = ceil_div(B, bu) * used;
  NRL_REQUIRE(*blocks < ((int64_t)1 << 31), "%s: grid too large (%lld workgroups)", who, (long long)*blocks);
  static_cast<TkArgs&>(A) = tk_args(user, table, B, V, D, 1, excl_idx, excl_off, eligible, nullptr, nullptr, out_score, status);
  A.slices = (int32_t)used;
  A.tiles_per_slice = (int32_t)tps;
  A.tgt_idx = tgt_idx;
  A.tgt_off = tgt_off;
  A.n_targets = n_targets;
  A.gathered = gather ? w.gathered : nullptr;
  A.tscore = w.tscore;
  A.owner = w.owner;
  A.pcnt = w.pcnt;
  A.tcnt = w.tcnt;
  A.out_rank = out_rank;
  A.out_ranked = out_ranked;
  return NRL_OK;
}

// nrl_catalogue_ranks (`win` null) and nrl_catalogue_window_ranks: one sequence of checks, one layout; the window picks the kernels
static int tkc_ranks_entry(const char* who, const float* user_vec, const float* table, int64_t B, int64_t V, int32_t D,
                           const int64_t* tgt_idx, const int64_t* tgt_off, int64_t n_targets, const TkwFields* win,
                           const int64_t* excl_idx, const int64_t* excl_off, const uint8_t* eligible, int32_t slices,
                           int32_t* out_rank, float* out_score, int32_t* out_ranked, int32_t* status, void* ws, size_t ws_bytes,
                           void* stream) {
  NRL_REQUIRE(B >= 0 && V >= 0 && D >= 0 && slices >= 0 && n_targets >= 0, "%s: negative size", who);
  NRL_TRY(tk_check(who, B, V, D, 1, excl_idx, excl_off));
  NRL_TRY(tkc_check(who, n_targets, tgt_idx, tgt_off, status));
  if (B == 0) return NRL_OK;
  NRL_REQUIRE(out_ranked && user_vec && (V == 0 || table) && (n_targets == 0 || (tgt_idx && out_rank && out_score)),
              "%s: null argument", who);
  if (win) NRL_TRY(tk_window_check(who, B, V, *win));
  TkWith<TkcArgs, TkwFields> A{};
  int64_t blocks;
  NRL_TRY(tkc_prepare(who, A, user_vec, table, B, V, D, D, true, tgt_idx, tgt_off, n_targets, excl_idx, excl_off, eligible, slices,
                      TK_BU, out_rank, out_score, out_ranked, status, ws, ws_bytes, &blocks));
  auto target = [&](hipStream_t st) {
    tkc_target_kernel<<<(unsigned)ceil_div(n_targets, TK_BU), TK_THREADS, 0, st>>>(A);
    NRL_LAUNCH_CHECK();
    return NRL_OK;
  };
  if (!win) return tkc_launch(tkc_count_kernel, static_cast<TkcArgs&>(A), blocks, TKC_LDS, stream, target);
  static_cast<TkwFields&>(A) = *win;
  return tkc_launch(tkwc_count_kernel, A, blocks, TKC_LDS + tkw_lds_bytes(TK_BU), stream, target, TkcFinishWindow{*win});
}

int nrl_catalogue_ranks(const float* user_vec, const float* table, int64_t B, int64_t V, int32_t D, const int64_t* tgt_idx,
                        const int64_t* tgt_off, int64_t n_targets, const int64_t* excl_idx, const int64_t* excl_off,
                        const uint8_t* eligible, int32_t slices, int32_t* out_rank, float* out_score, int32_t* out_ranked,
                        int32_t* status, void* ws, size_t ws_bytes, void* stream) {
  return tkc_ranks_entry("catalogue_ranks", user_vec, table, B, V, D, tgt_idx, tgt_off, n_targets, nullptr, excl_idx, excl_off,
                         eligible, slices, out_rank, out_score, out_ranked, status, ws, ws_bytes, stream);
}

int nrl_catalogue_window_ranks(const float* user_vec, const float* table, int64_t B, int64_t V, int32_t D, const int64_t* tgt_idx,
                               const int64_t* tgt_off, int64_t n_targets, const int32_t* row_time, const int32_t* win_lo,
                               const int32_t* win_hi, const int64_t* excl_idx, const int64_t* excl_off, const uint8_t* eligible,
                               int32_t slices, int32_t* out_rank, float* out_score, int32_t* out_ranked, int32_t* status, void* ws,
                               size_t ws_bytes, void* stream) {
  const TkwFields win{row_time, win_lo, win_hi};
  return tkc_ranks_entry("catalogue_window_ranks", user_vec, table, B, V, D, tgt_idx, tgt_off, n_targets, &win, excl_idx, excl_off,
                         eligible, slices, out_rank, out_score, out_ranked, status, ws, ws_bytes, stream);
}

// ---- the other scorers: each one's own checks and its fields, written once for its two entries ------------------------------------
// The order in which an entry's checks fire is part of its contract (a caller sees the first that fails), and a scorer's checks do
// not all sit together in it: those of its sizes come before tk_check, those of its operands after.  Hence up to two functions
// per scorer; `who` is the entry's name in the message.

// MINER
static int tki_check(const char* who, int32_t K, int32_t mode, const float* gate) {
  NRL_REQUIRE(K >= 1 && K <= NRL_TOPK_MAX_INTERESTS, "%s: K in [1, %d] (got %d)", who, NRL_TOPK_MAX_INTERESTS, K);
  NRL_REQUIRE(mode >= 0 && mode <= 2, "%s: mode 0 (max), 1 (mean) or 2 (weighted) (got %d)", who, mode);
  NRL_REQUIRE(mode != 2 || gate, "%s: mode 2 (weighted) needs the gate rows", who);
  return NRL_OK;
}
// Ut = TK_BU / K users per workgroup: the plan of these entries is their own, and never needs more lists (or counts) than the
// workspace of the plain entries holds for the same sizes (Ut <= TK_BU)
static TkiFields tki_fields(const float* gate, int32_t K, int32_t mode) { return TkiFields{mode == 2 ? gate : nullptr, K, TK_BU / K, mode}; }

int nrl_topk_interest_scores(const float* interests, const float* gate, const float* table, int64_t B, int32_t K, int64_t V, int32_t D,
                             int32_t k, int32_t mode, const int64_t* excl_idx, const int64_t* excl_off, const uint8_t* eligible,
                             int32_t slices, int64_t* out_idx, float* out_score, int32_t* status, void* ws, size_t ws_bytes,
                             void* stream) {
  NRL_REQUIRE(B >= 0 && V >= 0 && D >= 0 && slices >= 0, "topk_interest_scores: negative size");
  NRL_TRY(tki_check("topk_interest_scores", K, mode, gate));
  NRL_TRY(tk_check("topk_interest_scores", B, V, D, k, excl_idx, excl_off));
  if (B == 0) return NRL_OK;
  TkWith<TkArgs, TkiFields> A;
  static_cast<TkiFields&>(A) = tki_fields(gate, K, mode);
  unsigned long long* partial;
  NRL_TRY(carve_workspace(ws, ws_bytes, [&](Arena& a) { tk_layout(a, B, V, k, slices, A.Ut, &partial); }));
  NRL_REQUIRE(status, "topk_interest_scores: the status word is required");
  NRL_REQUIRE(out_idx && out_score && interests && (V == 0 || table), "topk_interest_scores: null argument");
  static_cast<TkArgs&>(A) = tk_args(interests, table, B, V, D, k, excl_idx, excl_off, eligible, partial, out_idx, out_score, status);
  return mode == 2 ? tk_launch("topk_interest_scores", tki_scores_kernel<true>, A, slices, 2, A.Ut, stream)
                   : tk_launch("topk_interest_scores", tki_scores_kernel<false>, A, slices, 1, A.Ut, stream);
}

int nrl_catalogue_interest_ranks(const float* interests, const float* gate, const float* table, int64_t B, int32_t K, int64_t V,
                                 int32_t D, int32_t mode, const int64_t* tgt_idx, const int64_t* tgt_off, int64_t n_targets,
                                 const int64_t* excl_idx, const int64_t* excl_off, const uint8_t* eligible, int32_t slices,
                                 int32_t* out_rank, float* out_score, int32_t* out_ranked, int32_t* status, void* ws,
                                 size_t ws_bytes, void* stream) {
  NRL_REQUIRE(B >= 0 && V >= 0 && D >= 0 && slices >= 0 && n_targets >= 0, "catalogue_interest_ranks: negative size");
  NRL_TRY(tki_check("catalogue_interest_ranks", K, mode, gate));
  NRL_TRY(tk_check("catalogue_interest_ranks", B, V, D, 1, excl_idx, excl_off));
  NRL_TRY(tkc_check("catalogue_interest_ranks", n_targets, tgt_idx, tgt_off, status));
  if (B == 0) return NRL_OK;
  NRL_REQUIRE(out_ranked && interests && (V == 0 || table) && (n_targets == 0 || (tgt_idx && out_rank && out_score)),
              "catalogue_interest_ranks: null argument");
  TkWith<TkcArgs, TkiFields> A;
  static_cast<TkiFields&>(A) = tki_fields(gate, K, mode);
  int64_t blocks;
  NRL_TRY(tkc_prepare("catalogue_interest_ranks", A, interests, table, B, V, D, D, true, tgt_idx, tgt_off, n_targets, excl_idx,
                      excl_off, eligible, slices, A.Ut, out_rank, out_score, out_ranked, status, ws, ws_bytes, &blocks));
  const unsigned tgrid = (unsigned)ceil_div(n_targets, A.Ut);
  if (mode == 2)
    return tkc_launch(tkic_count_kernel<true>, A, blocks, tkic_lds_bytes(true, A.Ut), stream, [&](hipStream_t st) {
      NRL_HIP(hipFuncSetAttribute((const void*)tkic_target_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
      tkic_target_kernel<true><<<tgrid, TK_THREADS, 2 * TK_TILE_BYTES, st>>>(A);
      NRL_LAUNCH_CHECK();
      return NRL_OK;
    });
  return tkc_launch(tkic_count_kernel<false>, A, blocks, tkic_lds_bytes(false, A.Ut), stream, [&](hipStream_t st) {
    tkic_target_kernel<false><<<tgrid, TK_THREADS, TK_TILE_BYTES, st>>>(A);
    NRL_LAUNCH_CHECK();
    return NRL_OK;
  });
}

// DKN (no D in its tk_check: Hd takes its place and has its own bounds)
static int tkr_check_sizes(const char* who, int32_t Hd) {
  NRL_REQUIRE(Hd >= 1 && Hd <= NRL_TOPK_MAX_HIDDEN, "%s: Hd in [1, %d] (got %d)", who, NRL_TOPK_MAX_HIDDEN, Hd);
  return NRL_OK;
}
static int tkr_check_operands(const char* who, const float* w2, const float* b2) {
  NRL_REQUIRE(w2, "%s: w2 is required", who);
  NRL_REQUIRE(b2, "%s: b2 is required (a device pointer)", who);
  return NRL_OK;
}

int nrl_topk_relu_scores(const float* q, const float* proj, const float* w2, const float* b2, int64_t B, int64_t V, int32_t Hd,
                         int32_t k, const int64_t* excl_idx, const int64_t* excl_off, const uint8_t* eligible, int32_t slices,
                         int64_t* out_idx, float* out_score, int32_t* status, void* ws, size_t ws_bytes, void* stream) {
  NRL_REQUIRE(B >= 0 && V >= 0 && slices >= 0, "topk_relu_scores: negative size");
  NRL_TRY(tkr_check_sizes("topk_relu_scores", Hd));
  NRL_TRY(tk_check("topk_relu_scores", B, V, 4, k, excl_idx, excl_off));
  NRL_REQUIRE(status, "topk_relu_scores: the status word is required");
  NRL_TRY(tkr_check_operands("topk_relu_scores", w2, b2));
  if (B == 0) return NRL_OK;
  NRL_REQUIRE(out_idx && out_score && q && (V == 0 || proj), "topk_relu_scores: null argument");
  unsigned long long* partial;
  NRL_TRY(carve_workspace(ws, ws_bytes, [&](Arena& a) { tk_layout(a, B, V, k, slices, TK_BU, &partial); }));
  TkWith<TkArgs, TkrFields> A;
  static_cast<TkArgs&>(A) = tk_args(q, proj, B, V, Hd, k, excl_idx, excl_off, eligible, partial, out_idx, out_score, status);
  static_cast<TkrFields&>(A) = TkrFields{w2, b2};
  return tk_launch("topk_relu_scores", tkr_scores_kernel, A, slices, 1, TK_BU, stream, tkr_extra_lds(Hd));
}

int nrl_catalogue_relu_ranks(const float* q, const float* proj, const float* w2, const float* b2, int64_t B, int64_t V, int32_t Hd,
                             const int64_t* tgt_idx, const int64_t* tgt_off, int64_t n_targets, const int64_t* excl_idx,
                             const int64_t* excl_off, const uint8_t* eligible, int32_t slices, int32_t* out_rank, float* out_score,
                             int32_t* out_ranked, int32_t* status, void* ws, size_t ws_bytes, void* stream) {
  NRL_REQUIRE(B >= 0 && V >= 0 && slices >= 0 && n_targets >= 0, "catalogue_relu_ranks: negative size");
  NRL_TRY(tkr_check_sizes("catalogue_relu_ranks", Hd));
  NRL_TRY(tk_check("catalogue_relu_ranks", B, V, 4, 1, excl_idx, excl_off));
  NRL_TRY(tkc_check("catalogue_relu_ranks", n_targets, tgt_idx, tgt_off, status));
  NRL_TRY(tkr_check_operands("catalogue_relu_ranks", w2, b2));
  if (B == 0) return NRL_OK;
  NRL_REQUIRE(out_ranked && q && (V == 0 || proj) && (n_targets == 0 || (tgt_idx && out_rank && out_score)),
              "catalogue_relu_ranks: null argument");
  // the layout of nrl_catalogue_ranks_workspace_size(B, V, 4, ...): nothing is gathered, the target kernel reads proj in place
  TkWith<TkcArgs, TkrFields> A;
  int64_t blocks;
  NRL_TRY(tkc_prepare("catalogue_relu_ranks", A, q, proj, B, V, Hd, 4, false, tgt_idx, tgt_off, n_targets, excl_idx, excl_off,
                      eligible, slices, TK_BU, out_rank, out_score, out_ranked, status, ws, ws_bytes, &blocks));
  static_cast<TkrFields&>(A) = TkrFields{w2, b2};
  return tkc_launch(tkrc_count_kernel, A, blocks, tkrc_lds_bytes(Hd), stream, [&](hipStream_t st) {
    tkrc_target_kernel<<<(unsigned)ceil_div(n_targets, 256), 256, 0, st>>>(A);
    NRL_LAUNCH_CHECK();
    return NRL_OK;
  });
}

// NPA (no D in its tk_check: F takes its place and has its own bounds)
static int tkp_check_sizes(const char* who, int32_t L, int32_t F) {
  NRL_REQUIRE(L >= 1 && L <= NRL_TOPK_MAX_TOKENS, "%s: L in [1, %d] tokens (got %d)", who, NRL_TOPK_MAX_TOKENS, L);
  NRL_REQUIRE(F >= 4 && F % 4 == 0 && F <= NRL_TOPK_MAX_D, "%s: F a multiple of 4 in [4, %d] (got %d)", who, NRL_TOPK_MAX_D, F);
  return NRL_OK;
}
static int tkp_check_operands(const char* who, const float* q, const float* user, const float* features) {
  NRL_REQUIRE((((uintptr_t)q | (uintptr_t)user | (uintptr_t)features) & 15) == 0, "%s: q, user and features must be 16-byte aligned", who);
  return NRL_OK;
}

int nrl_topk_pooled_scores(const float* q, const float* user, const float* features, int64_t B, int64_t V, int32_t L, int32_t F,
                           int32_t k, const int64_t* excl_idx, const int64_t* excl_off, const uint8_t* eligible, int32_t slices,
                           int64_t* out_idx, float* out_score, int32_t* status, void* ws, size_t ws_bytes, void* stream) {
  NRL_REQUIRE(B >= 0 && V >= 0 && slices >= 0, "topk_pooled_scores: negative size");
  NRL_TRY(tkp_check_sizes("topk_pooled_scores", L, F));
  NRL_TRY(tk_check("topk_pooled_scores", B, V, 4, k, excl_idx, excl_off));
  NRL_REQUIRE(status, "topk_pooled_scores: the status word is required");
  if (B == 0) return NRL_OK;
  NRL_REQUIRE(out_idx && out_score && q && user && (V == 0 || features), "topk_pooled_scores: null argument");
  NRL_TRY(tkp_check_operands("topk_pooled_scores", q, user, features));
  unsigned long long* partial;
  NRL_TRY(carve_workspace(ws, ws_bytes, [&](Arena& a) { tk_layout(a, B, V, k, slices, TK_BU, &partial); }));
  TkWith<TkArgs, TkpFields> A;
  static_cast<TkArgs&>(A) = tk_args(q, features, B, V, F, k, excl_idx, excl_off, eligible, partial, out_idx, out_score, status);
  static_cast<TkpFields&>(A) = TkpFields{user, L};
  return tk_launch("topk_pooled_scores", tkp_scores_kernel, A, slices, 1, TK_BU, stream, TKP_EXTRA_LDS);
}

int nrl_catalogue_pooled_ranks(const float* q, const float* user, const float* features, int64_t B, int64_t V, int32_t L, int32_t F,
                               const int64_t* tgt_idx, const int64_t* tgt_off, int64_t n_targets, const int64_t* excl_idx,
                               const int64_t* excl_off, const uint8_t* eligible, int32_t slices, int32_t* out_rank, float* out_score,
                               int32_t* out_ranked, int32_t* status, void* ws, size_t ws_bytes, void* stream) {
  NRL_REQUIRE(B >= 0 && V >= 0 && slices >= 0 && n_targets >= 0, "catalogue_pooled_ranks: negative size");
  NRL_TRY(tkp_check_sizes("catalogue_pooled_ranks", L, F));
  NRL_TRY(tk_check("catalogue_pooled_ranks", B, V, 4, 1, excl_idx, excl_off));
  NRL_TRY(tkc_check("catalogue_pooled_ranks", n_targets, tgt_idx, tgt_off, status));
  if (B == 0) return NRL_OK;
  NRL_REQUIRE(out_ranked && q && user && (V == 0 || features) && (n_targets == 0 || (tgt_idx && out_rank && out_score)),
              "catalogue_pooled_ranks: null argument");
  NRL_TRY(tkp_check_operands("catalogue_pooled_ranks", q, user, features));
  // the layout of nrl_catalogue_ranks_workspace_size(B, V, 4, ...): nothing is gathered, the target kernel reads the maps in place
  TkWith<TkcArgs, TkpFields> A;
  int64_t blocks;
  NRL_TRY(tkc_prepare("catalogue_pooled_ranks", A, q, features, B, V, F, 4, false, tgt_idx, tgt_off, n_targets, excl_idx, excl_off,
                      eligible, slices, TK_BU, out_rank, out_score, out_ranked, status, ws, ws_bytes, &blocks));
  static_cast<TkpFields&>(A) = TkpFields{user, L};
  return tkc_launch(tkpc_count_kernel, A, blocks, TKPC_LDS, stream, [&](hipStream_t st) {
    tkpc_target_kernel<<<(unsigned)ceil_div(n_targets, TK_BU), TK_THREADS, 0, st>>>(A);
    NRL_LAUNCH_CHECK();
    return NRL_OK;
  });
}

// MANNeR
static int tke_check_sizes(const char* who, int32_t T) {
  NRL_REQUIRE(T >= 1 && T <= NRL_TOPK_MAX_MODELS, "%s: T in [1, %d] sub-models (got %d)", who, NRL_TOPK_MAX_MODELS, T);
  return NRL_OK;
}
static int tke_check_operands(const char* who, const float* const* users, const float* const* tables, const float* weights, int32_t T,
                              int64_t V) {
  NRL_REQUIRE(users && tables && weights, "%s: null users / tables / weights array", who);
  for (int t = 0; t < T; ++t) NRL_REQUIRE(users[t] && (V == 0 || tables[t]), "%s: null user matrix or table of sub-model %d", who, t);
  return NRL_OK;
}
static int tke_check_stats(const char* who, const float* out_stats, const float* moments) {
  NRL_REQUIRE(out_stats && moments, "%s: out_stats and the moments scratch are required", who);
  return NRL_OK;
}
// (the statistics pass sets the two chunk fields)
static TkeFields tke_fields(const float* const* users, const float* const* tables, const float* weights, int32_t T, float* out_stats,
                            float* moments) {
  TkeFields E;
  for (int t = 0; t < NRL_TOPK_MAX_MODELS; ++t) {
    E.users[t] = users[t < T ? t : 0];
    E.tables[t] = tables[t < T ? t : 0];
    E.w[t] = t < T ? weights[t] : 0.f;
  }
  E.T = T;
  E.chunks = E.tiles_per_chunk = 0;
  E.out_stats = out_stats;
  E.moments = moments;
  return E;
}

// The statistics pass of both ensemble entries: plans the chunks (into E, which the entry's walk kernel is then handed) and runs
// tke_stats_kernel and tke_finish_kernel over them
static int tke_statistics(const char* who, const TkArgs& base, TkeFields& E, void* stream) {
  // the statistics chunks: a function of V alone, so that the order of every reduction is
  const int64_t nvt = ceil_div((int64_t)base.V, TK_BV);
  E.tiles_per_chunk = (int32_t)(nvt > 0 ? ceil_div(nvt, NRL_TOPK_STAT_CHUNKS) : 1);
  E.chunks = (int32_t)(nvt > 0 ? ceil_div(nvt, E.tiles_per_chunk) : 0);
  const int64_t blocks = ceil_div(base.B, TK_BU) * E.chunks;
  NRL_REQUIRE(blocks < ((int64_t)1 << 31), "%s: grid too large (%lld workgroups)", who, (long long)blocks);
  const TkWith<TkArgs, TkeFields> A{base, E};
  hipStream_t st = (hipStream_t)stream;
  if (blocks > 0) {
    tke_stats_kernel<<<(unsigned)blocks, TK_THREADS, 0, st>>>(A);
    NRL_LAUNCH_CHECK();
  }
  tke_finish_kernel<<<(unsigned)A.B, 64, 0, st>>>(A);
  NRL_LAUNCH_CHECK();
  return NRL_OK;
}

// nrl_topk_ensemble_scores (`cap` null) and nrl_topk_ensemble_scores_capped: the statistics pass does not know the cap
static int tke_scores_entry(const char* who, const float* const* users, const float* const* tables, const float* weights, int32_t T,
                            int64_t B, int64_t V, int32_t D, int32_t k, const TkCapFields* cap, const int64_t* excl_idx,
                            const int64_t* excl_off, const uint8_t* eligible, int32_t slices, int64_t* out_idx, float* out_score,
                            float* out_stats, float* moments, int32_t* status, void* ws, size_t ws_bytes, void* stream) {
  NRL_REQUIRE(B >= 0 && V >= 0 && D >= 0 && slices >= 0, "%s: negative size", who);
  NRL_TRY(tke_check_sizes(who, T));
  NRL_TRY(tk_check(who, B, V, D, k, excl_idx, excl_off));
  NRL_TRY(tke_check_operands(who, users, tables, weights, T, V));
  NRL_REQUIRE(status, "%s: the status word is required", who);
  NRL_TRY(tke_check_stats(who, out_stats, moments));
  if (cap) NRL_TRY(tk_cap_check(who, V, k, cap->row_class, cap->m));
  if (B == 0) return NRL_OK;
  NRL_REQUIRE(out_idx && out_score, "%s: null argument", who);
  unsigned long long* partial;
  NRL_TRY(carve_workspace(ws, ws_bytes, [&](Arena& a) { tk_layout(a, B, V, k, slices, TK_BU, &partial); }));
  TkWith<TkArgs, TkeFields> A;
  static_cast<TkArgs&>(A) = tk_args(users[0], tables[0], B, V, D, k, excl_idx, excl_off, eligible, partial, out_idx, out_score, status);
  static_cast<TkeFields&>(A) = tke_fields(users, tables, weights, T, out_stats, moments);
  NRL_TRY(tke_statistics(who, A, A, stream));
  const size_t stats_lds = (size_t)TK_BU * T * 2 * 4;
  if (!cap) return tk_launch(who, tke_scores_kernel, A, slices, 2, TK_BU, stream, stats_lds);
  TkWith<TkWith<TkArgs, TkeFields>, TkCapFields> C{A, *cap};
  return tk_launch(who, tkecap_scores_kernel, C, slices, 2, TK_BU, stream, stats_lds, TkMergeCapped{*cap});
}

int nrl_topk_ensemble_scores(const float* const* users, const float* const* tables, const float* weights, int32_t T, int64_t B,
                             int64_t V, int32_t D, int32_t k, const int64_t* excl_idx, const int64_t* excl_off,
                             const uint8_t* eligible, int32_t slices, int64_t* out_idx, float* out_score, float* out_stats,
                             float* moments, int32_t* status, void* ws, size_t ws_bytes, void* stream) {
  return tke_scores_entry("topk_ensemble_scores", users, tables, weights, T, B, V, D, k, nullptr, excl_idx, excl_off, eligible, slices,
                          out_idx, out_score, out_stats, moments, status, ws, ws_bytes, stream);
}

int nrl_topk_ensemble_scores_capped(const float* const* users, const float* const* tables, const float* weights, int32_t T, int64_t B,
                                    int64_t V, int32_t D, int32_t k, const int32_t* row_class, int32_t max_per_class,
                                    const int64_t* excl_idx, const int64_t* excl_off, const uint8_t* eligible, int32_t slices,
                                    int64_t* out_idx, float* out_score, float* out_stats, float* moments, int32_t* status, void* ws,
                                    size_t ws_bytes, void* stream) {
  const TkCapFields cap{row_class, max_per_class};
  return tke_scores_entry("topk_ensemble_scores_capped", users, tables, weights, T, B, V, D, k, &cap, excl_idx, excl_off, eligible,
                          slices, out_idx, out_score, out_stats, moments, status, ws, ws_bytes, stream);
}

size_t nrl_catalogue_ensemble_ranks_workspace_size(int32_t T, int64_t B, int64_t V, int32_t D, int64_t n_targets, int32_t slices) {
  if (!tk_shape_ok(B, V, D, 1) || T < 1 || T > NRL_TOPK_MAX_MODELS || slices < 0 || n_targets < 0 || n_targets >= ((int64_t)1 << 31))
    return 256;
  return measure_workspace<TkcWs>([&](Arena& a, auto* w) { tkc_layout(a, B, V, T * D, n_targets, slices, TK_BU, w); });
}

int nrl_catalogue_ensemble_ranks(const float* const* users, const float* const* tables, const float* weights, int32_t T, int64_t B,
                                 int64_t V, int32_t D, const int64_t* tgt_idx, const int64_t* tgt_off, int64_t n_targets,
                                 const int64_t* excl_idx, const int64_t* excl_off, const uint8_t* eligible, int32_t slices,
                                 int32_t* out_rank, float* out_score, int32_t* out_ranked, float* out_stats, float* moments,
                                 int32_t* status, void* ws, size_t ws_bytes, void* stream) {
  NRL_REQUIRE(B >= 0 && V >= 0 && D >= 0 && slices >= 0 && n_targets >= 0, "catalogue_ensemble_ranks: negative size");
  NRL_TRY(tke_check_sizes("catalogue_ensemble_ranks", T));
  NRL_TRY(tk_check("catalogue_ensemble_ranks", B, V, D, 1, excl_idx, excl_off));
  NRL_TRY(tkc_check("catalogue_ensemble_ranks", n_targets, tgt_idx, tgt_off, status));
  NRL_TRY(tke_check_operands("catalogue_ensemble_ranks", users, tables, weights, T, V));
  NRL_TRY(tke_check_stats("catalogue_ensemble_ranks", out_stats, moments));
  if (B == 0) return NRL_OK;
  NRL_REQUIRE(out_ranked && (n_targets == 0 || (tgt_idx && out_rank && out_score)), "catalogue_ensemble_ranks: null argument");
  // the layout of nrl_catalogue_ranks with T gathered blocks: (T, n_targets, D)
  TkWith<TkcArgs, TkeFields> A;
  int64_t blocks;
  NRL_TRY(tkc_prepare("catalogue_ensemble_ranks", A, users[0], tables[0], B, V, D, T * D, true, tgt_idx, tgt_off, n_targets, excl_idx,
                      excl_off, eligible, slices, TK_BU, out_rank, out_score, out_ranked, status, ws, ws_bytes, &blocks));
  static_cast<TkeFields&>(A) = tke_fields(users, tables, weights, T, out_stats, moments);
  NRL_TRY(tke_statistics("catalogue_ensemble_ranks", A, A, stream));
  return tkc_launch(tkec_count_kernel, A, blocks, TKEC_LDS, stream, [&](hipStream_t st) {
    if (T > 1) {
      tkec_gather_kernel<<<dim3((unsigned)n_targets, (unsigned)(T - 1)), 64, 0, st>>>(A);
      NRL_LAUNCH_CHECK();
    }
    tkec_target_kernel<<<(unsigned)ceil_div(n_targets, TK_BU), TK_THREADS, 0, st>>>(A);
    NRL_LAUNCH_CHECK();
    return NRL_OK;
  });
}

// The class bias: the dot product's entries with (bias, bias_class, S) behind D
static int tkb_check(const char* who, const float* bias, const int32_t* bias_class, int32_t S, int64_t V) {
  NRL_REQUIRE(S >= 1 && S <= NRL_TOPK_MAX_BIAS_CLASSES, "%s: S in [1, %d] (got %d)", who, NRL_TOPK_MAX_BIAS_CLASSES, S);
  NRL_REQUIRE(bias, "%s: bias is required", who);
  NRL_REQUIRE(bias_class || V == 0, "%s: row_class is required", who);
  return NRL_OK;
}

// nrl_topk_bias_scores (`cap` null) and nrl_topk_bias_scores_capped: tk_scores_entry with the bias fields
static int tkb_scores_entry(const char* who, const float* user_vec, const float* table, int64_t B, int64_t V, int32_t D,
                            const TkbFields& bias, int32_t k, const TkCapFields* cap, const int64_t* excl_idx, const int64_t* excl_off,
                            const uint8_t* eligible, int32_t slices, int64_t* out_idx, float* out_score, int32_t* status, void* ws,
                            size_t ws_bytes, void* stream) {
  NRL_REQUIRE(B >= 0 && V >= 0 && D >= 0 && slices >= 0, "%s: negative size", who);
  NRL_TRY(tk_check(who, B, V, D, k, excl_idx, excl_off));
  NRL_REQUIRE(status, "%s: the status word is required", who);
  NRL_TRY(tkb_check(who, bias.bias, bias.bias_class, bias.S, V));
  if (cap) NRL_TRY(tk_cap_check(who, V, k, cap->row_class, cap->m));
  if (B == 0) return NRL_OK;
  NRL_REQUIRE(out_idx && out_score && user_vec && (V == 0 || table), "%s: null argument", who);
  unsigned long long* partial;
  NRL_TRY(carve_workspace(ws, ws_bytes, [&](Arena& a) { tk_layout(a, B, V, k, slices, TK_BU, &partial); }));
  TkWith<TkArgs, TkbFields> A;
  static_cast<TkArgs&>(A) = tk_args(user_vec, table, B, V, D, k, excl_idx, excl_off, eligible, partial, out_idx, out_score, status);
  static_cast<TkbFields&>(A) = bias;
  if (!cap) return tk_launch(who, tkb_scores_kernel, A, slices, 1, TK_BU, stream, tkb_extra_lds(bias.S));
  TkWith<TkWith<TkArgs, TkbFields>, TkCapFields> C{A, *cap};
  return tk_launch(who, tkbcap_scores_kernel, C, slices, 1, TK_BU, stream, tkb_extra_lds(bias.S), TkMergeCapped{*cap});
}

int nrl_topk_bias_scores(const float* user_vec, const float* table, int64_t B, int64_t V, int32_t D, const float* bias,
                         const int32_t* row_class, int32_t S, int32_t k, const int64_t* excl_idx, const int64_t* excl_off,
                         const uint8_t* eligible, int32_t slices, int64_t* out_idx, float* out_score, int32_t* status, void* ws,
                         size_t ws_bytes, void* stream) {
  return tkb_scores_entry("topk_bias_scores", user_vec, table, B, V, D, TkbFields{bias, row_class, S}, k, nullptr, excl_idx, excl_off,
                          eligible, slices, out_idx, out_score, status, ws, ws_bytes, stream);
}

int nrl_topk_bias_scores_capped(const float* user_vec, const float* table, int64_t B, int64_t V, int32_t D, const float* bias,
                                const int32_t* row_class, int32_t S, int32_t k, const int32_t* cap_class, int32_t max_per_class,
                                const int64_t* excl_idx, const int64_t* excl_off, const uint8_t* eligible, int32_t slices,
                                int64_t* out_idx, float* out_score, int32_t* status, void* ws, size_t ws_bytes, void* stream) {
  const TkCapFields cap{cap_class, max_per_class};
  return tkb_scores_entry("topk_bias_scores_capped", user_vec, table, B, V, D, TkbFields{bias, row_class, S}, k, &cap, excl_idx,
                          excl_off, eligible, slices, out_idx, out_score, status, ws, ws_bytes, stream);
}

int nrl_catalogue_bias_ranks(const float* user_vec, const float* table, int64_t B, int64_t V, int32_t D, const float* bias,
                             const int32_t* row_class, int32_t S, const int64_t* tgt_idx, const int64_t* tgt_off, int64_t n_targets,
                             const int64_t* excl_idx, const int64_t* excl_off, const uint8_t* eligible, int32_t slices,
                             int32_t* out_rank, float* out_score, int32_t* out_ranked, int32_t* status, void* ws, size_t ws_bytes,
                             void* stream) {
  NRL_REQUIRE(B >= 0 && V >= 0 && D >= 0 && slices >= 0 && n_targets >= 0, "catalogue_bias_ranks: negative size");
  NRL_TRY(tk_check("catalogue_bias_ranks", B, V, D, 1, excl_idx, excl_off));
  NRL_TRY(tkc_check("catalogue_bias_ranks", n_targets, tgt_idx, tgt_off, status));
  NRL_TRY(tkb_check("catalogue_bias_ranks", bias, row_class, S, V));
  if (B == 0) return NRL_OK;
  NRL_REQUIRE(out_ranked && user_vec && (V == 0 || table) && (n_targets == 0 || (tgt_idx && out_rank && out_score)),
              "catalogue_bias_ranks: null argument");
  TkWith<TkcArgs, TkbFields> A;
  int64_t blocks;
  NRL_TRY(tkc_prepare("catalogue_bias_ranks", A, user_vec, table, B, V, D, D, true, tgt_idx, tgt_off, n_targets, excl_idx, excl_off,
                      eligible, slices, TK_BU, out_rank, out_score, out_ranked, status, ws, ws_bytes, &blocks));
  static_cast<TkbFields&>(A) = TkbFields{bias, row_class, S};
  return tkc_launch(tkbc_count_kernel, A, blocks, TKC_LDS + tkb_extra_lds(S), stream, [&](hipStream_t st) {
    tkbc_target_kernel<<<(unsigned)ceil_div(n_targets, TK_BU), TK_THREADS, 0, st>>>(A);
    NRL_LAUNCH_CHECK();
    return NRL_OK;
  });
}

// ---- nrl_mmr_rerank (header: semantics) --------------------------------------------------------------------------------------------
int nrl_mmr_rerank(const int64_t* pool_idx, const float* pool_score, const float* table, int64_t B, int32_t N, int64_t V, int32_t D,
                   int32_t k, float lambda, int32_t similarity, int32_t normalize, int64_t* out_idx, float* out_score, float* out_mmr,
                   int32_t* status, void* stream) {
  NRL_REQUIRE(B >= 0 && N >= 0 && V >= 0 && D >= 0 && k >= 0, "mmr_rerank: negative size");
  NRL_REQUIRE(N >= 1 && N <= NRL_MMR_MAX_POOL, "mmr_rerank: N in [1, %d] (got %d)", NRL_MMR_MAX_POOL, N);
  NRL_REQUIRE(k >= 1 && k <= N, "mmr_rerank: k in [1, N = %d] (got %d)", N, k);
  NRL_REQUIRE(D > 0 && D % 4 == 0 && D <= NRL_TOPK_MAX_D, "mmr_rerank: D a multiple of 4 in [4, %d] (got %d)", NRL_TOPK_MAX_D, D);
  NRL_REQUIRE(V < ((int64_t)1 << 31), "mmr_rerank: at most 2^31 - 1 table rows (got %lld)", (long long)V);
  NRL_REQUIRE(B < ((int64_t)1 << 31), "mmr_rerank: at most 2^31 - 1 users per call (got %lld)", (long long)B);
  NRL_REQUIRE(lambda >= 0.f && lambda <= 1.f, "mmr_rerank: lambda in [0, 1] (got %g)", (double)lambda);
  NRL_REQUIRE((similarity == 0 || similarity == 1) && (normalize == 0 || normalize == 1),
              "mmr_rerank: similarity (0 cosine, 1 dot) and normalize in {0, 1} (got %d, %d)", similarity, normalize);
  NRL_REQUIRE(status, "mmr_rerank: the status word is required");
  if (B == 0) return NRL_OK;
  NRL_REQUIRE(pool_idx && pool_score && out_idx && out_score && out_mmr && (V == 0 || table), "mmr_rerank: null argument");
  const MmrArgs A{pool_idx, pool_score, table, N, D, k, V, lambda, similarity, normalize, out_idx, out_score, out_mmr, status};
  const size_t smem = mmr_lds_bytes((N + TK_BU - 1) / TK_BU);
  // more than 64 KB of dynamic LDS needs the attribute; it belongs to the current device, so it is set per call
  if (smem > 64 * 1024)
    NRL_HIP(hipFuncSetAttribute((const void*)mmr_rerank_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  mmr_rerank_kernel<<<(unsigned)B, TK_THREADS, smem, (hipStream_t)stream>>>(A);
  NRL_LAUNCH_CHECK();
  return NRL_OK;
}

// ---- nrl_calibrated_rerank (header: semantics) -------------------------------------------------------------------------------------
int nrl_calibrated_rerank(const int64_t* pool_idx, const float* pool_score, const float* table, int64_t B, int32_t N, int64_t V,
                          int32_t D, const int32_t* row_class, const float* target, int32_t S, int32_t k, float lambda, float mu,
                          float gamma, int32_t similarity, int32_t normalize, int64_t* out_idx, float* out_score, float* out_obj,
                          float* out_cal, int32_t* status, void* stream) {
  NRL_REQUIRE(B >= 0 && N >= 0 && V >= 0 && S >= 0 && k >= 0, "calibrated_rerank: negative size");
  NRL_REQUIRE(N >= 1 && N <= NRL_MMR_MAX_POOL, "calibrated_rerank: N in [1, %d] (got %d)", NRL_MMR_MAX_POOL, N);
  NRL_REQUIRE(k >= 1 && k <= N, "calibrated_rerank: k in [1, N = %d] (got %d)", N, k);
  NRL_REQUIRE(S >= 1 && S <= NRL_CAL_MAX_CLASSES, "calibrated_rerank: S in [1, %d] (got %d)", NRL_CAL_MAX_CLASSES, S);
  NRL_REQUIRE(V < ((int64_t)1 << 31), "calibrated_rerank: at most 2^31 - 1 table rows (got %lld)", (long long)V);
  NRL_REQUIRE(B < ((int64_t)1 << 31), "calibrated_rerank: at most 2^31 - 1 users per call (got %lld)", (long long)B);
  NRL_REQUIRE(lambda >= 0.f && lambda <= 1.f, "calibrated_rerank: lambda in [0, 1] (got %g)", (double)lambda);
  NRL_REQUIRE(mu >= 0.f && mu <= 1.f, "calibrated_rerank: mu in [0, 1] (got %g)", (double)mu);
  NRL_REQUIRE(gamma >= 0.f && gamma <= 1.f, "calibrated_rerank: gamma in [0, 1] (got %g)", (double)gamma);
  NRL_REQUIRE(normalize == 0 || normalize == 1, "calibrated_rerank: normalize in {0, 1} (got %d)", normalize);
  const bool gram = mu != 0.f;
  if (gram) {
    NRL_REQUIRE(D > 0 && D % 4 == 0 && D <= NRL_TOPK_MAX_D, "calibrated_rerank: with mu != 0, D a multiple of 4 in [4, %d] (got %d)",
                NRL_TOPK_MAX_D, D);
    NRL_REQUIRE(similarity == 0 || similarity == 1, "calibrated_rerank: with mu != 0, similarity (0 cosine, 1 dot) in {0, 1} (got %d)",
                similarity);
  }
  NRL_REQUIRE(status, "calibrated_rerank: the status word is required");
  if (B == 0) return NRL_OK;
  NRL_REQUIRE(pool_idx && pool_score && target && out_idx && out_score && out_obj && out_cal && (V == 0 || row_class) &&
                  (V == 0 || !gram || table),
              "calibrated_rerank: null argument");
  const CalArgs A{pool_idx, pool_score, table,     N,          D,       k,         V,       row_class, target, S,
                  lambda,   mu,         gamma,     similarity, normalize, out_idx, out_score, out_obj, out_cal, status};
  if (gram) {
    const size_t smem = cal_lds_bytes((N + TK_BU - 1) / TK_BU);
    // more than 64 KB of dynamic LDS needs the attribute; it belongs to the current device, so it is set per call
    if (smem > 64 * 1024)
      NRL_HIP(hipFuncSetAttribute((const void*)cal_rerank_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    cal_rerank_kernel<true><<<(unsigned)B, TK_THREADS, smem, (hipStream_t)stream>>>(A);
  } else {
    cal_rerank_kernel<false><<<(unsigned)B, TK_THREADS, cal_lds_bytes(0), (hipStream_t)stream>>>(A);
  }
  NRL_LAUNCH_CHECK();
  return NRL_OK;
}

// ---- nrl_dpp_rerank (header: semantics) --------------------------------------------------------------------------------------------
int nrl_dpp_rerank(const int64_t* pool_idx, const float* pool_score, const float* quality, const float* table, int64_t B, int32_t N,
                   int64_t V, int32_t D, int32_t k, float alpha, float eps, int32_t similarity, int32_t normalize, int64_t* out_idx,
                   float* out_score, float* out_gain, int32_t* status, void* stream) {
  NRL_REQUIRE(B >= 0 && N >= 0 && V >= 0 && D >= 0 && k >= 0, "dpp_rerank: negative size");
  NRL_REQUIRE(N >= 1 && N <= NRL_MMR_MAX_POOL, "dpp_rerank: N in [1, %d] (got %d)", NRL_MMR_MAX_POOL, N);
  NRL_REQUIRE(k >= 1 && k <= N && k <= NRL_DPP_MAX_K, "dpp_rerank: k in [1, min(N = %d, %d)] (got %d)", N, NRL_DPP_MAX_K, k);
  NRL_REQUIRE(alpha >= 0.f && alpha < INFINITY, "dpp_rerank: alpha finite and >= 0 (got %g)", (double)alpha);
  NRL_REQUIRE(eps >= 0.f && eps < 1.f, "dpp_rerank: eps in [0, 1) (got %g)", (double)eps);
  NRL_REQUIRE(D > 0 && D % 4 == 0 && D <= NRL_TOPK_MAX_D, "dpp_rerank: D a multiple of 4 in [4, %d] (got %d)", NRL_TOPK_MAX_D, D);
  NRL_REQUIRE(V < ((int64_t)1 << 31), "dpp_rerank: at most 2^31 - 1 table rows (got %lld)", (long long)V);
  NRL_REQUIRE(B < ((int64_t)1 << 31), "dpp_rerank: at most 2^31 - 1 users per call (got %lld)", (long long)B);
  NRL_REQUIRE((similarity == 0 || similarity == 1) && (normalize == 0 || normalize == 1),
              "dpp_rerank: similarity (0 cosine, 1 dot) and normalize in {0, 1} (got %d, %d)", similarity, normalize);
  NRL_REQUIRE(status, "dpp_rerank: the status word is required");
  if (B == 0) return NRL_OK;
  NRL_REQUIRE(pool_idx && pool_score && out_idx && out_score && out_gain && (V == 0 || table), "dpp_rerank: null argument");
  const DppArgs A{pool_idx, pool_score, quality, table, N, D, k, V, alpha, eps, similarity, normalize, out_idx, out_score, out_gain, status};
  const size_t smem = dpp_lds_bytes((N + TK_BU - 1) / TK_BU, k);
  // more than 64 KB of dynamic LDS needs the attribute; it belongs to the current device, so it is set per call
  if (smem > 64 * 1024)
    NRL_HIP(hipFuncSetAttribute((const void*)dpp_rerank_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  dpp_rerank_kernel<<<(unsigned)B, TK_THREADS, smem, (hipStream_t)stream>>>(A);
  NRL_LAUNCH_CHECK();
  return NRL_OK;
}

}  // extern "C"

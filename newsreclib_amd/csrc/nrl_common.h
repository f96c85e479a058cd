// Shared device/host helpers for the gfx950 NRMS kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/newsreclib_amd.h"
#include "nrl_arena.h"

namespace nrl {

// ---- error plumbing (thread-local message behind nrl_last_error) -----------------------------
void set_error(const char* fmt, ...);

#define NRL_REQUIRE(cond, ...)            \
  do {                                    \
    if (!(cond)) {                        \
      ::nrl::set_error(__VA_ARGS__);      \
      return NRL_E_INVALID;               \
    }                                     \
  } while (0)

#define NRL_HIP(call)                                                              \
  do {                                                                             \
    hipError_t e__ = (call);                                                       \
    if (e__ != hipSuccess) {                                                       \
      ::nrl::set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e__), __FILE__, __LINE__); \
      return NRL_E_HIP;                                                            \
    }                                                                              \
  } while (0)

#define NRL_LAUNCH_CHECK() NRL_HIP(hipGetLastError())

#define NRL_TRY(expr)            \
  do {                           \
    int rc__ = (expr);           \
    if (rc__ != NRL_OK) return rc__; \
  } while (0)

// ---- workspaces (nrl_arena.h) --------------------------------------------------------------------
// The one workspace check of every entry point.  `layout(Arena&)` names the regions; it runs once measuring and, when the
// caller's buffer holds that many bytes, once more carving.  Null / misaligned: NRL_E_INVALID; short: NRL_E_WORKSPACE.
template <class Layout>
static inline int carve_workspace(void* ws, size_t ws_bytes, Layout&& layout) {
  NRL_REQUIRE(ws != nullptr && ((uintptr_t)ws & 255) == 0, "workspace must be 256-byte aligned");
  Arena need;
  layout(need);
  if (ws_bytes < need.bytes()) {
    set_error("workspace too small: %zu < %zu bytes", ws_bytes, need.bytes());
    return NRL_E_WORKSPACE;
  }
  Arena a(ws);
  layout(a);
  return NRL_OK;
}

// the `*_workspace_bytes` side: the same layout on a measuring arena, its pointers thrown away
template <class Ws, class Layout>
static inline size_t measure_workspace(Layout&& layout) {
  Arena a;
  Ws w;
  layout(a, &w);
  return a.bytes();
}

// ---- dropout keep mask (normative statement in oracle/nrms_oracle.py) -------------------------
__host__ __device__ __forceinline__ uint32_t lowbias32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7FEB352Du;
  x ^= x >> 15;
  x *= 0x846CA68Bu;
  x ^= x >> 16;
  return x;
}

__host__ __device__ __forceinline__ uint32_t dropout_key(uint64_t seed, uint32_t stream) {
  uint32_t s = lowbias32(stream + 0x9E3779B9u);
  s = lowbias32((uint32_t)(seed >> 32) ^ s);
  s = lowbias32((uint32_t)(seed & 0xFFFFFFFFu) ^ s);
  return s;
}

struct Dropout {
  uint32_t key;
  uint32_t thresh;  // keep iff hash >= thresh
  float scale;      // 1/(1-p); p == 0 -> thresh 0, scale 1 (every element kept)
  __device__ __forceinline__ float mult(uint32_t flat_idx) const {
    return lowbias32(flat_idx * 0x9E3779B1u + key) >= thresh ? scale : 0.0f;
  }
};

inline Dropout make_dropout(double p, uint64_t seed, uint32_t stream) {
  Dropout d;
  d.key = dropout_key(seed, stream);
  if (p <= 0.0) {
    d.thresh = 0u;
    d.scale = 1.0f;
  } else {
    d.thresh = (uint32_t)(p * 4294967296.0);
    d.scale = (float)(1.0 / (1.0 - p));
  }
  return d;
}

// ---- small device helpers ----------------------------------------------------------------------
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}

// Reductions over a workgroup of WAVES waves in a fixed order (xor tree within a wave, then the waves in order); every thread
// gets the result.  `red` holds WAVES floats of LDS; the leading barrier lets it be reused by the next call.  The sum starts
// from +0: a block of all -0 gives +0.
template <int WAVES>
__device__ __forceinline__ float block_sum(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float s = 0.f;
#pragma unroll
  for (int w = 0; w < WAVES; ++w) s += red[w];
  return s;
}
template <int WAVES>
__device__ __forceinline__ float block_max(float v, float* red) {
  v = wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float s = red[0];
#pragma unroll
  for (int w = 1; w < WAVES; ++w) s = fmaxf(s, red[w]);
  return s;
}

// dot4 keeps this expression order: contraction sees the same tree everywhere
__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }
__device__ __forceinline__ float dot4(float4 a, float4 b) { return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w; }

// order-preserving key of a score: a > b  <=>  key(a) > key(b); -0 == +0, NaN = 0xFFFFFFFF above +inf
__device__ __forceinline__ uint32_t score_key(float s) {
  if (s != s) return 0xFFFFFFFFu;
  if (s == 0.f) s = 0.f;
  const uint32_t b = __float_as_uint(s);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// one wave: its LDS operations complete in order, the compiler must not move them across
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

static inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
static inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

}  // namespace nrl

// Device prelude shared by re_kernels.hip and mf_kernels.hip: build stamp, launch check, the pointwise losses and
// their host-side dispatch, and the fixed-order wave reductions every fused solver is built from.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

// Build id (photon_ml_amd/ops/build.py: content hash of the sources + compile command, -DPML_BUILD_ID=...): the
// loaders compare it with the tree's sources and refuse a stale library.
#ifndef PML_BUILD_ID
#define PML_BUILD_ID "unstamped-build!"
#endif
__attribute__((used)) static const char pml_build_stamp[] = "PML_BUILD_ID=" PML_BUILD_ID;

#define LAUNCH_CHECK()                                         \
  do {                                                         \
    hipError_t e_ = hipGetLastError();                         \
    if (e_ != hipSuccess) return (int)e_;                      \
  } while (0)

enum { LOSS_LOGISTIC = 0, LOSS_POISSON = 1, LOSS_SQUARED = 2, LOSS_HINGE = 3 };

// Run-time loss -> template argument: fn(L) with L() a constexpr int. Callers validate ``loss`` first; NL = 3 never
// instantiates the hinge (the TRON kernels: its second derivative is 0), NL = 4 does (L-BFGS / OWL-QN).
template <int NL = 3, typename F>
static inline void with_loss(int loss, F&& fn) {
  static_assert(NL == 3 || NL == 4, "three smooth losses, or those and the smoothed hinge");
  if (loss == LOSS_LOGISTIC) fn(std::integral_constant<int, LOSS_LOGISTIC>{});
  else if (loss == LOSS_POISSON) fn(std::integral_constant<int, LOSS_POISSON>{});
  else if (NL == 3 || loss == LOSS_SQUARED) fn(std::integral_constant<int, LOSS_SQUARED>{});
  else if constexpr (NL == 4) fn(std::integral_constant<int, LOSS_HINGE>{});
}

template <int LOSS>
__device__ __forceinline__ void loss_t(double z, double y, double& l, double& dl, double& d2) {
  if constexpr (LOSS == LOSS_LOGISTIC) {
    // one exp, one log1p, one reciprocal, no branches (as pointwise_loss in glm_kernels.hip):
    // e = exp(-|z|) serves the sigmoid and log(1 + exp(+-z)) = max(+-z, 0) + log1p(e)
    const double e = exp(-fabs(z));
    const double lp = log1p(e);
    const double r = 1.0 / (1.0 + e);
    const double s = z >= 0.0 ? r : e * r;
    const bool pos = y > 0.5;
    const double zz = pos ? -z : z;
    l = (zz > 0.0 ? zz : 0.0) + lp;
    dl = pos ? s - 1.0 : s;
    d2 = s * (1.0 - s);
  } else if constexpr (LOSS == LOSS_POISSON) {
    const double e = exp(z);
    l = e - y * z; dl = e - y; d2 = e;
  } else if constexpr (LOSS == LOSS_HINGE) {
    // Rennie & Srebro smoothed hinge (function/losses.py, pointwise_loss in glm_kernels.hip): once differentiable
    const double yy = y < 0.5 ? -1.0 : 1.0;
    const double t = yy * z;
    l = t <= 0.0 ? 0.5 - t : (t < 1.0 ? 0.5 * (1.0 - t) * (1.0 - t) : 0.0);
    dl = (t < 0.0 ? -1.0 : (t < 1.0 ? t - 1.0 : 0.0)) * yy;
    d2 = 0.0;
  } else {
    const double d = z - y;
    l = 0.5 * d * d; dl = d; d2 = 1.0;
  }
}

// weight x per-row term with an exact 0 for zero-weight rows whatever the term (wx in glm_kernels.hip): a
// zero-weight row whose exp overflowed (a partial score, an overshooting trial step) must not turn 0 x inf into NaN
__device__ __forceinline__ double wx(double w, double x) { return w != 0.0 ? w * x : 0.0; }

template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v) {
  const long long b = __builtin_bit_cast(long long, v);
  const int lo = __builtin_amdgcn_update_dpp(0, (int)b, CTRL, 0xF, 0xF, true);
  const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), CTRL, 0xF, 0xF, true);
  return __builtin_bit_cast(double, ((long long)hi << 32) | (long long)(unsigned int)lo);
}

__device__ __forceinline__ double readlane_f64(double v, int l) {
  const long long b = __builtin_bit_cast(long long, v);
  const int lo = __builtin_amdgcn_readlane((int)b, l);
  const int hi = __builtin_amdgcn_readlane((int)(b >> 32), l);
  return __builtin_bit_cast(double, ((long long)hi << 32) | (long long)(unsigned int)lo);
}

// Sum over the 4 lanes of a quad, in every lane of the quad (fixed order).
__device__ __forceinline__ double quad_total(double v) {
  v += dpp_f64<0xB1>(v);    // quad_perm [1,0,3,2]
  v += dpp_f64<0x4E>(v);    // quad_perm [2,3,0,1]
  return v;
}

// Sum over the 16 lanes of a DPP row, in every lane of the row (fixed-order butterflies: deterministic).
__device__ __forceinline__ double row16_total(double v) {
  v = quad_total(v);
  v += dpp_f64<0x141>(v);   // row_half_mirror
  v += dpp_f64<0x140>(v);   // row_mirror
  return v;
}

// Sum over the 64 lanes of a wave, returned (bitwise identical) in every lane: the row sums (every lane then holds
// its row's sum), then the four of them in a fixed order.
__device__ __forceinline__ double wave_total(double v) {
  v = row16_total(v);
  return (readlane_f64(v, 0) + readlane_f64(v, 16)) + (readlane_f64(v, 32) + readlane_f64(v, 48));
}

// LDS hand-off between the lanes of one wave: in-order LDS per wave + a compiler fence.
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// A workgroup-uniform value re-tagged as wave-uniform (readfirstlane): it is held in SGPRs, not VGPRs.
__device__ __forceinline__ long long uniform_i64(long long v) {
  const int lo = __builtin_amdgcn_readfirstlane((int)v);
  const int hi = __builtin_amdgcn_readfirstlane((int)(v >> 32));
  return ((long long)hi << 32) | (long long)(unsigned int)lo;
}
__device__ __forceinline__ double uniform_f64(double v) {
  return __builtin_bit_cast(double, uniform_i64(__builtin_bit_cast(long long, v)));
}

// Loads through the global address space: a generic pointer read through the kernel-argument struct becomes a FLAT
// load, which also counts in lgkmcnt -- every LDS wait would then wait for it too.
template <typename T>
__device__ __forceinline__ T gld(const T* p) {
  return *(const __attribute__((address_space(1))) T*)p;
}

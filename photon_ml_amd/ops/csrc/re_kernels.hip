// photon_ml_amd — CDNA4 (gfx950 / MI355X) fused per-entity PRIMAL TRON for random effects.
//
// The reference solves every random-effect entity as its own small GLM (photon-api/.../algorithm/
// RandomEffectCoordinate.scala:103-143 -> optimization/SingleNodeOptimizationProblem.scala:85-103 -> photon-lib/
// .../optimization/TRON.scala:80-340). Entities with few rows are solved in their row space (rs_tron in
// glm_kernels.hip); this file handles the others — typically 65 .. thousands of rows over ~1k projected
// coefficients — WITHOUT a pass-per-Hessian-vector launch sequence over the whole block-diagonal problem:
//
// * one workgroup (4 waves) owns one entity for its whole solve: the coefficient-space vectors (w, g, step, r,
//   d) and one accumulator per wave live in LDS (d_e <= dmax doubles each); the TRON control flow (truncated CG,
//   trust-region radius, accept / reject, Photon convergence tests) runs on workgroup-uniform scalars;
// * every Hessian-vector product X^T (D (X d)) is ONE read of the entity's CSR rows (a wave per row, lane k =
//   non-zero k of the row: gather d[c] from LDS, DPP wave sum, scale by the cached D_i = w_i l''(z_i), scatter
//   t x_ik into the wave's private LDS accumulator). The block-diagonal pass path reads the rows twice (CSR
//   forward + CSC transpose copy) per product and launches per pass; here there is no CSC copy at all;
// * deterministic: fixed-order DPP / readlane wave sums, per-wave accumulators combined in wave order, distinct
//   columns inside a row (so one ds_add_f64 never has two lanes on one address within a row);
// * per-row scratch in HBM: D and the margins x_i.w for the current iterate and the trial point (swapped on
//   acceptance), so the final margins come out of the solve (scores without another pass).
//
// Semantics follow batched_tron / rs_tron_kernel: eta = (1e-4, .25, .75), sigma = (.25, .5, 4), delta0 = ||g0||,
// first-iteration delta = min(delta, ||step||), CG tolerance 0.1 ||g||, <= max_cg CG steps, <= max_fail
// consecutive rejections; reason codes 1 max-iter, 2 not-improving, 3 f-converged, 4 g-converged; tolerances
// from the state at zero coefficients (photon-lib/.../optimization/Optimizer.scala:136-196).
//
// Built with: hipcc --offload-arch=gfx950 -O3 -shared -fPIC (photon_ml_amd/ops/build.py). C ABI, ctypes.

#include "tron_core.h"

#define RE_NW 4                 // waves per workgroup (one entity)
#define RE_THREADS (RE_NW * 64)

// Workgroup sums of K values (K <= 8), in every thread. ``red`` holds two [RE_NW][8] slots used alternately,
// so one barrier per call suffices: a slot is rewritten only two calls later, after every thread has passed
// the barrier of the call in between (all threads run the same, workgroup-uniform control flow).
template <int K, int NW = RE_NW>
__device__ __forceinline__ void block_sums(double (&v)[K], double* __restrict__ red, int& parity) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = wave_total(v[k]);
  double* slot = red + parity * (NW * 8);
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) slot[w * 8 + k] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) {
    double s = 0.0;
#pragma unroll
    for (int q = 0; q < NW; ++q) s += slot[q * 8 + k];
    v[k] = uniform_f64(s);      // identical in every thread
  }
  parity ^= 1;
}

struct ReTronArgs {
  const int* order;          // launch slot -> entity (largest entities first)
  int n_launch;
  const long long* row_ptr;  // [E + 1] entity row ranges
  const long long* col_ptr;  // [E + 1] entity coefficient ranges (packed W)
  const long long* nip;      // [N + 1] row -> non-zero range
  const uint16_t* lcol;      // entity-local column of every non-zero (< d_e, distinct inside a row)
  const double* val;         // value of every non-zero
  const double* y;           // per-row label / offset / weight
  const double* off;
  const double* wt;
  double* scr;               // per-row scratch [4][n_rows]: D (2 buffers), margins x.w (2 buffers)
  long long n_rows;
  double* W;                 // packed coefficients: in = warm start, out = solution
  double* f;                 // per entity: final objective, iterations, reason code
  int* iters;
  int* reason;
  double* zout;              // per row: x_i . w of the solution (no offset)
  int* npass;                // optional, per entity: row passes run (function evaluations + Hessian-vector)
  int loss;
  double l2, tol;
  int max_iter, max_fail, max_cg, dmax;
  double* gsc;               // lean kernel: gradient at W, per coefficient (packed like W)
  const double* xf2;         // lean kernel, optional: ||X_e||_F^2 per entity (lazy zero-point gradient norm)
  const double* nc;          // re_tron_csr_kernel<LOSS, true>: shift c = f s per coefficient (packed like W)
  const int* ni0;            // re_tron_csr_kernel<LOSS, true>: entity-local intercept column per entity (c[i0] = 0)
};

#define RE_G 16                      // lanes per row (one DPP row)
#define RE_RPI (64 / RE_G)           // rows per wave instruction
#define RE_U 4                       // row groups in flight per wave batch (re_tron_csr_kernel; 3: +2.4 %)
#define RE_K 4                       // entries per lane kept in registers (rows of <= 64 entries in one go)
#ifndef RE_ABL
#define RE_ABL 0                     // profiling-only ablation mask (see row_pass); 0 in production
#endif

// One pass over the entity's rows [r0, r1): a wave takes BATCH = 4 U consecutive rows at a time, RE_G lanes per
// row (lane k of the row: entries k, k + 16, ...). The next batch's row pointers are fetched while the current
// batch computes, and all BATCH rows' entries are loaded before the first gather, so a batch costs about one
// dependent global-memory latency.
// MODE 0: Hessian-vector data term: acc_w += X^T (Dc * (X vec)).
// MODE 1: value + gradient at vec: acc_w += X^T (wt * l'), fpart += wt * l, Dn = wt * l'', Zn = x.vec.
// MODE 2: value + gradient at zero (no gathers, no scratch writes).
template <int MODE, int LOSS, int U = RE_U, int NW = RE_NW>
__device__ __forceinline__ void row_pass(const ReTronArgs& a, long long r0, long long r1,
                                         const double* __restrict__ vec, double* __restrict__ acc,
                                         const double* __restrict__ Dc, double* __restrict__ Dn,
                                         double* __restrict__ Zn, double& fpart) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int grp = lane / RE_G, gl = lane % RE_G;
  // entity-local 32-bit row / entry offsets from per-entity bases: one VGPR per address instead of 64-bit math
  const int nrows = (int)(r1 - r0);
  const long long e0 = a.nip[r0];
  const long long* __restrict__ nip = a.nip + r0;
  const uint16_t* __restrict__ lcol = a.lcol + e0;
  const double* __restrict__ val = a.val + e0;
  const double* __restrict__ wt = a.wt + r0;
  const double* __restrict__ off = a.off + r0;
  const double* __restrict__ yv = a.y + r0;
  if (MODE == 0) Dc += r0;
  if (MODE == 1) { Dn += r0; Zn += r0; }
  constexpr int BATCH = RE_RPI * U;
  const int step = NW * BATCH;
  int base = w * BATCH;
  // row pointers of a batch, prefetched one batch ahead: lane j <= BATCH holds nip[base + j] (clamped to the
  // entity's end). The load is unconditional and its raw value is only converted at its use in the next batch, so
  // the prefetch never waits (a conditional load / immediate conversion put a full memory round trip per batch)
  auto fetch_raw = [&](int b) -> long long {
    const int i = b + (lane <= BATCH ? lane : BATCH);
    return gld(nip + (i < nrows ? i : nrows));
  };
  long long npr = fetch_raw(base);
  for (; base < nrows; base += step) {
    const int np = (int)(npr - e0);
    const long long npr_next = fetch_raw(base + step);
    int lo[U], hi[U];
    int c[U][RE_K];
    double v[U][RE_K], dot[U], rs[U][3];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int q = u * RE_RPI + grp;
      lo[u] = __shfl(np, q, 64);
      hi[u] = __shfl(np, q + 1, 64);
      const int i = base + q;
      const bool valid = i < nrows;
      const int ic = valid ? i : 0;
      if (MODE == 0) {
        rs[u][0] = valid ? gld(Dc + ic) : 0.0;
      } else {
        rs[u][0] = valid ? gld(wt + ic) : 0.0;
        rs[u][1] = valid ? gld(off + ic) : 0.0;
        rs[u][2] = valid ? gld(yv + ic) : 0.0;
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
#pragma unroll
      for (int k = 0; k < RE_K; ++k) {
        const int p = lo[u] + gl + RE_G * k;
        const bool in = p < hi[u];
        c[u][k] = in ? (int)lcol[p] : 0;
        v[u][k] = in ? val[p] : 0.0;
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      double s = 0.0;
      if (MODE != 2) {
#pragma unroll
        for (int k = 0; k < RE_K; ++k) s = fma(v[u][k], vec[c[u][k]], s);
        for (int p = lo[u] + gl + RE_G * RE_K; p < hi[u]; p += RE_G) s = fma(val[p], vec[lcol[p]], s);
#if RE_ABL
        // profiling ablations (scripts/gpu_r5_s5.sh): the same math plus one extra LDS gather (2) or one extra
        // value load (4) per entry, scaled by a runtime zero -- their marginal cost, at identical iterates
        const double zero = a.l2 - a.l2;
#pragma unroll
        for (int k = 0; k < RE_K; ++k) {
          if (RE_ABL & 2) s = fma(zero, vec[c[u][k] >> 1], s);
          if (RE_ABL & 4) {
            const int p = lo[u] + gl + RE_G * k;
            s = fma(zero, p < hi[u] ? ((volatile const double*)val)[p] : 0.0, s);
          }
        }
#endif
      }
      dot[u] = s;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (MODE != 2) dot[u] = row16_total(dot[u]);
      const int i = base + u * RE_RPI + grp;
      const bool valid = i < nrows;
      double t;
      if (MODE == 0) {
        t = rs[u][0] * dot[u];
      } else {
        double l = 0.0, dl = 0.0, d2 = 0.0;
        if (valid) {
          loss_t<LOSS>(dot[u] + rs[u][1], rs[u][2], l, dl, d2);
          if (gl == 0) {
            fpart += wx(rs[u][0], l);
            if (MODE == 1) { Dn[i] = wx(rs[u][0], d2); Zn[i] = dot[u]; }
          }
        }
        t = wx(rs[u][0], dl);
      }
#pragma unroll
      for (int k = 0; k < RE_K; ++k)
        if (lo[u] + gl + RE_G * k < hi[u]) {
          atomicAdd(&acc[c[u][k]], t * v[u][k]);
#if RE_ABL & 1
          atomicAdd(&acc[c[u][k]], (a.l2 - a.l2) * v[u][k]);   // profiling: one extra LDS atomic per entry
#endif
        }
      for (int p = lo[u] + gl + RE_G * RE_K; p < hi[u]; p += RE_G) atomicAdd(&acc[lcol[p]], t * val[p]);
    }
    npr = npr_next;
  }
}

// ------------------------------------------------------------------------------------------------------------
// Quad row pass (lean kernel, rows padded to whole quads of 4 entries: EntityTronBatch pads with column 0 / value
// 0.0, which add exactly nothing). Lane gl of a row's 16 lanes owns the quad gl (+ 16 per extra chunk): its 4
// columns arrive in ONE 8-byte load and its 4 values in TWO 16-byte loads, where row_pass issues 4 + 4 narrow
// loads. The kernel is bound by the texture path's per-instruction work (profiles/re_lean_ablation_r5.md: one
// extra value load per entry costs +67 %, one extra LDS atomic +8 %), so 3 instead of 8 loads per 4 entries.
// Only a quad past the row end is masked (no per-entry masks).
typedef double re_d2 __attribute__((ext_vector_type(2)));
typedef unsigned re_u2 __attribute__((ext_vector_type(2)));

// Four LDS gathers in flight together (one wait for all four): left to itself the compiler issues each gather,
// waits for it and consumes it before the next (register pressure), which serialises four LDS round trips per
// lane per row group. ``vec`` is a __shared__ array; the byte offsets are its LDS addresses.
__device__ __forceinline__ void lds_gather4(const double* vec, int c0, int c1, int c2, int c3, double& g0, double& g1,
                                            double& g2, double& g3) {
  const unsigned b = (unsigned)(uintptr_t)(const __attribute__((address_space(3))) double*)vec;
  const unsigned a0 = b + 8u * (unsigned)c0, a1 = b + 8u * (unsigned)c1, a2 = b + 8u * (unsigned)c2,
                 a3 = b + 8u * (unsigned)c3;
  asm volatile(
      "ds_read_b64 %0, %4\n\t"
      "ds_read_b64 %1, %5\n\t"
      "ds_read_b64 %2, %6\n\t"
      "ds_read_b64 %3, %7\n\t"
      "s_waitcnt lgkmcnt(0)"
      : "=&v"(g0), "=&v"(g1), "=&v"(g2), "=&v"(g3)
      : "v"(a0), "v"(a1), "v"(a2), "v"(a3)
      : "memory");
}

template <int MODE, int LOSS, int U, int NW = RE_NW>
__device__ __forceinline__ void row_pass_q(const ReTronArgs& a, long long r0, long long r1,
                                           const double* __restrict__ vec, double* __restrict__ acc,
                                           const double* __restrict__ Dc, double* __restrict__ Dn,
                                           double* __restrict__ Zn, double& fpart) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int grp = lane / RE_G, gl = lane % RE_G;
  const int nrows = (int)(r1 - r0);
  const long long e0 = a.nip[r0];                           // a multiple of 4 (padded rows)
  const long long* __restrict__ nip = a.nip + r0;
  const re_u2* __restrict__ cq = (const re_u2*)(a.lcol + e0);   // quad q: 4 columns
  const re_d2* __restrict__ vq = (const re_d2*)(a.val + e0);    // quad q: values at 2q, 2q + 1
  const double* __restrict__ wt = a.wt + r0;
  const double* __restrict__ off = a.off + r0;
  const double* __restrict__ yv = a.y + r0;
  if (MODE == 0) Dc += r0;
  if (MODE == 1) { Dn += r0; Zn += r0; }
  constexpr int BATCH = RE_RPI * U;
  const int step = NW * BATCH;
  int base = w * BATCH;
  // row pointers of a batch, in quads: lane j <= BATCH holds nip[base + j] / 4 (prefetched as in row_pass)
  auto fetch_raw = [&](int b) -> long long {
    const int i = b + (lane <= BATCH ? lane : BATCH);
    return gld(nip + (i < nrows ? i : nrows));
  };
  auto cols = [](re_u2 c, int (&k)[4]) {
    k[0] = (int)(c.x & 0xFFFFu); k[1] = (int)(c.x >> 16); k[2] = (int)(c.y & 0xFFFFu); k[3] = (int)(c.y >> 16);
  };
  long long npr = fetch_raw(base);
  for (; base < nrows; base += step) {
    const int np = (int)((npr - e0) >> 2);
    const long long npr_next = fetch_raw(base + step);
    int qa[U], qb[U];
    re_u2 c[U];
    re_d2 v0[U], v1[U];
    double dot[U], rs[U][3];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int q = u * RE_RPI + grp;
      qa[u] = __shfl(np, q, 64) + gl;                         // this lane's quad
      qb[u] = __shfl(np, q + 1, 64);                          // the row's end (quads)
      const int i = base + q;
      const bool valid = i < nrows;
      const int ic = valid ? i : 0;
      if (MODE == 0) {
        rs[u][0] = valid ? gld(Dc + ic) : 0.0;
      } else {
        rs[u][0] = valid ? gld(wt + ic) : 0.0;
        rs[u][1] = valid ? gld(off + ic) : 0.0;
        rs[u][2] = valid ? gld(yv + ic) : 0.0;
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const bool in = qa[u] < qb[u];
      const int qq = in ? qa[u] : 0;
      c[u] = gld(cq + qq);
      v0[u] = gld(vq + 2 * qq);
      v1[u] = gld(vq + 2 * qq + 1);
      if (!in) { c[u] = re_u2{0u, 0u}; v0[u] = re_d2{0.0, 0.0}; v1[u] = re_d2{0.0, 0.0}; }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      double s = 0.0;
      if (MODE != 2) {
        int k[4];
        cols(c[u], k);
        double g[4];
        lds_gather4(vec, k[0], k[1], k[2], k[3], g[0], g[1], g[2], g[3]);
        s = fma(v0[u].x, g[0], s);
        s = fma(v0[u].y, g[1], s);
        s = fma(v1[u].x, g[2], s);
        s = fma(v1[u].y, g[3], s);
        for (int qq = qa[u] + RE_G; qq < qb[u]; qq += RE_G) {     // rows longer than 64 entries
          int kt[4];
          cols(cq[qq], kt);
          const re_d2 a0 = vq[2 * qq], a1 = vq[2 * qq + 1];
          s = fma(a0.x, vec[kt[0]], s);
          s = fma(a0.y, vec[kt[1]], s);
          s = fma(a1.x, vec[kt[2]], s);
          s = fma(a1.y, vec[kt[3]], s);
        }
      }
      dot[u] = s;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (MODE != 2) dot[u] = row16_total(dot[u]);
      const int i = base + u * RE_RPI + grp;
      const bool valid = i < nrows;
      double t;
      if (MODE == 0) {
        t = rs[u][0] * dot[u];
      } else {
        double l = 0.0, dl = 0.0, d2 = 0.0;
        if (valid) {
          loss_t<LOSS>(dot[u] + rs[u][1], rs[u][2], l, dl, d2);
          if (gl == 0) {
            fpart += wx(rs[u][0], l);
            if (MODE == 1) { Dn[i] = wx(rs[u][0], d2); Zn[i] = dot[u]; }
          }
        }
        t = wx(rs[u][0], dl);
      }
      if (qa[u] < qb[u]) {
        int k[4];
        cols(c[u], k);
        atomicAdd(&acc[k[0]], t * v0[u].x);
        atomicAdd(&acc[k[1]], t * v0[u].y);
        atomicAdd(&acc[k[2]], t * v1[u].x);
        atomicAdd(&acc[k[3]], t * v1[u].y);
      }
      for (int qq = qa[u] + RE_G; qq < qb[u]; qq += RE_G) {
        int kt[4];
        cols(cq[qq], kt);
        const re_d2 a0 = vq[2 * qq], a1 = vq[2 * qq + 1];
        atomicAdd(&acc[kt[0]], t * a0.x);
        atomicAdd(&acc[kt[1]], t * a0.y);
        atomicAdd(&acc[kt[2]], t * a1.x);
        atomicAdd(&acc[kt[3]], t * a1.y);
      }
    }
    npr = npr_next;
  }
}

// SHIFT: the entity's design matrix is X' = X (I - e_i0 c^T) (the shift of a STANDARDIZATION context over the
// factor-scaled rows; column i0 of X is the all-ones intercept, c[i0] = 0). Both hooks are coefficient-side: before a
// row pass over vec the intercept slot holds vec[i0] - c.vec (one more workgroup sum, two more barriers per pass) and
// is restored in the combine sweep; the sweep forms g_j - c_j g0 with g0 = the fixed-order sum of the wave
// accumulators at i0. Thread i0 % RE_THREADS owns slot i0 everywhere outside the row pass, and it writes acc[i0] only
// after the sweep's workgroup sum, so the other threads' g0 reads need no barrier of their own. c is read from
// global memory (at dmax = 2048 the LDS is taken). The MODE 1 pass thus writes the true margins.
template <int LOSS, bool SHIFT = false>
__global__ __launch_bounds__(RE_THREADS) void re_tron_csr_kernel(ReTronArgs a) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int e = a.order[blockIdx.x];
  const long long r0 = a.row_ptr[e], r1 = a.row_ptr[e + 1];
  const long long c0 = a.col_ptr[e];
  const int d = (int)(a.col_ptr[e + 1] - c0);
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const int dm = a.dmax;
  double* sW = smem;
  double* sG = sW + dm;
  double* sS = sG + dm;     // CG step
  double* sR = sS + dm;     // CG residual
  double* sD = sR + dm;     // CG direction; trial point during the function evaluation
  double* acc = sD + dm;    // RE_NW accumulators; acc[0 .. d) = combined Hd (with l2 d) / trial gradient
  double* red = acc + RE_NW * dm;
  double* myacc = acc + w * dm;
  double* D[2] = {a.scr, a.scr + a.n_rows};
  double* Z[2] = {a.scr + 2 * a.n_rows, a.scr + 3 * a.n_rows};
  int cur = 0, parity = 0, npass = 0;
  double* Wg = a.W + c0;
  // SHIFT only: the entity's c segment, its intercept slot (clamped into the segment) and that slot's owner thread
  const double* cs = nullptr;
  int i0 = 0;
  bool own0 = false;
  if constexpr (SHIFT) {
    cs = a.nc + c0;
    const int i = a.ni0[e];
    i0 = i < 0 ? 0 : (i < d ? i : d - 1);
    own0 = tid == i0 % RE_THREADS;
  }

  auto zero_own = [&]() {
    for (int j = lane; j < d; j += 64) myacc[j] = 0.0;
  };
  // SHIFT: vec[i0] -= c . vec ahead of a row pass over vec (every thread's writes of vec are behind a barrier);
  // returns the saved vec[i0] in the owner thread. Ends with the barrier that publishes the slot to the row pass.
  auto shift_in = [&](double* vec) -> double {
    double s1[1] = {0.0};
    for (int j = tid; j < d; j += RE_THREADS) s1[0] += gld(cs + j) * vec[j];
    block_sums<1>(s1, red, parity);
    double saved = 0.0;
    if (own0) {
      saved = vec[i0];
      vec[i0] = saved - s1[0];
    }
    __syncthreads();
    return saved;
  };
  // SHIFT: g0 = the combined accumulator at i0 (the same fixed wave order as the sweeps; broadcast LDS reads)
  auto acc_i0 = [&]() -> double {
    double g0 = acc[i0];
#pragma unroll
    for (int q = 1; q < RE_NW; ++q) g0 += acc[q * dm + i0];
    return g0;
  };
  // value + gradient at vec (MODE 1: writes D / Z buffer ``nb``); the gradient lands in acc[0 .. d). One sweep
  // combines the wave accumulators (fixed wave order) and forms ||vec||^2 and ||g||^2; three barriers in all.
  auto value_grad = [&](double* vec, int nb, bool at_zero, double& gg) -> double {
    ++npass;
    __syncthreads();
    zero_own();
    double saved = 0.0;
    if constexpr (SHIFT) {
      if (!at_zero) saved = shift_in(vec);        // P 0 = 0 at the zero point
    }
    double fp = 0.0;
    if (at_zero) row_pass<2, LOSS>(a, r0, r1, vec, myacc, nullptr, nullptr, nullptr, fp);
    else row_pass<1, LOSS>(a, r0, r1, vec, myacc, nullptr, D[nb], Z[nb], fp);
    __syncthreads();
    double s3[3] = {fp, 0.0, 0.0};
    double g0 = 0.0, gi0 = 0.0;
    if constexpr (SHIFT) g0 = acc_i0();
    for (int j = tid; j < d; j += RE_THREADS) {
      double g = acc[j];
#pragma unroll
      for (int q = 1; q < RE_NW; ++q) g += acc[q * dm + j];
      double v = vec[j];
      if constexpr (SHIFT) {
        g -= gld(cs + j) * g0;
        if (j == i0 && !at_zero) {                // the unmodified vec for the L2 term and ||vec||^2
          v = saved;
          vec[j] = saved;
        }
      }
      g += a.l2 * v;
      if (SHIFT && j == i0) gi0 = g;              // written after the workgroup sum (others still read acc[i0])
      else acc[j] = g;
      s3[1] += v * v;
      s3[2] += g * g;
    }
    block_sums<3>(s3, red, parity);
    if constexpr (SHIFT) {
      if (own0) acc[i0] = gi0;
    }
    gg = s3[2];
    return s3[0] + 0.5 * a.l2 * s3[1];
  };

  for (int j = tid; j < d; j += RE_THREADS) sW[j] = Wg[j];
  double gnorm2;
  double f = value_grad(sW, cur, false, gnorm2);
  double nz[1] = {0.0};
  for (int j = tid; j < d; j += RE_THREADS) {
    sG[j] = acc[j];
    nz[0] += sW[j] != 0.0 ? 1.0 : 0.0;
  }
  block_sums<1>(nz, red, parity);
  double f0z = f, g0n = sqrt(gnorm2);
  if (nz[0] != 0.0) {
    for (int j = tid; j < d; j += RE_THREADS) sS[j] = 0.0;   // zero vector for the state at zero
    double g0;
    f0z = value_grad(sS, 0, true, g0);
    g0n = sqrt(g0);
  }
  const double loss_tol = f0z * a.tol, grad_tol = g0n * a.tol;
  double delta = sqrt(gnorm2);
  int it = 0, fails = 0, reason = 0;
  bool active = true;
  if (delta == 0.0) { reason = 4; active = false; }
  const int guard_max = a.max_iter * (a.max_fail + 1) + 5;
  for (int guard = 0; active && guard < guard_max; ++guard) {
    // ---- truncated CG at W (Hessian weights D[cur]). Per CG step: the Hessian-vector pass, ONE sweep that
    // combines the accumulators and forms d.Hd, step.d, d.d, r.Hd, Hd.Hd, one workgroup sum, and one update
    // sweep; ||step + a d||^2 and ||r - a Hd||^2 follow by algebra (clamped at 0).
    for (int j = tid; j < d; j += RE_THREADS) {
      sS[j] = 0.0;
      sR[j] = -sG[j];
      sD[j] = -sG[j];
    }
    double rtr = gnorm2, sts = 0.0;
    const double cg_tol2 = 0.01 * gnorm2;        // (0.1 ||g||)^2
    for (int k = 0; k < a.max_cg; ++k) {
      if (!(rtr > cg_tol2)) break;
      ++npass;
      __syncthreads();
      zero_own();
      double saved = 0.0;
      if constexpr (SHIFT) saved = shift_in(sD);
      double fp = 0.0;
      row_pass<0, LOSS>(a, r0, r1, sD, myacc, D[cur], nullptr, nullptr, fp);
      __syncthreads();
      double s5[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
      double h0 = 0.0, hi0 = 0.0;
      if constexpr (SHIFT) h0 = acc_i0();
      for (int j = tid; j < d; j += RE_THREADS) {
        double h = acc[j];
#pragma unroll
        for (int q = 1; q < RE_NW; ++q) h += acc[q * dm + j];
        double dj = sD[j];
        if constexpr (SHIFT) {
          h -= gld(cs + j) * h0;
          if (j == i0) {
            dj = saved;
            sD[j] = saved;
          }
        }
        h += a.l2 * dj;
        if (SHIFT && j == i0) hi0 = h;
        else acc[j] = h;
        s5[0] += dj * h;
        s5[1] += sS[j] * dj;
        s5[2] += dj * dj;
        s5[3] += sR[j] * h;
        s5[4] += h * h;
      }
      block_sums<5>(s5, red, parity);
      if constexpr (SHIFT) {
        if (own0) acc[i0] = hi0;
      }
      const TronCgStep c = tron_cg_step(rtr, sts, delta, s5[0], s5[1], s5[2], s5[3], s5[4]);
      for (int j = tid; j < d; j += RE_THREADS) {
        const double dj = sD[j];
        sS[j] += c.al * dj;
        const double r = sR[j] - c.al * acc[j];
        sR[j] = r;
        if (!c.hit) sD[j] = r + c.beta * dj;
      }
      if (c.hit) break;
      rtr = c.rn;
      sts = c.tn;
    }
    // ---- trial point W + step (in the direction slot), trust-region update, acceptance
    double s3[3] = {0.0, 0.0, 0.0};
    for (int j = tid; j < d; j += RE_THREADS) {
      const double sj = sS[j];
      s3[0] += sG[j] * sj;
      s3[1] += sj * sR[j];
      s3[2] += sj * sj;
      sD[j] = sW[j] + sj;
    }
    block_sums<3>(s3, red, parity);
    const double gs = s3[0], pred = -0.5 * (gs - s3[1]), snorm = sqrt(s3[2]);
    double gn2;
    const double fn = value_grad(sD, cur ^ 1, false, gn2);   // trial gradient in acc[0 .. d)
    delta = tron_radius(delta, snorm, gs, f, fn, pred, it == 0);
    const bool accept = tron_accept(f, fn, pred);
    const double f_prev = f;
    if (accept) {
      for (int j = tid; j < d; j += RE_THREADS) {
        sW[j] = sD[j];
        sG[j] = acc[j];
      }
      gnorm2 = gn2;
      f = fn;
      cur ^= 1;
      ++it;
      fails = 0;
    } else {
      ++fails;
    }
    const bool not_impr = !accept && fails >= a.max_fail;
    const int rc = tron_reason(accept, not_impr, gnorm2, grad_tol, f, f_prev, loss_tol, it, a.max_iter);
    if (rc > 0) { reason = rc; active = false; }
  }
  __syncthreads();
  for (int j = tid; j < d; j += RE_THREADS) Wg[j] = sW[j];
  if (a.zout != nullptr) {
    const double* zc = Z[cur];
    for (long long i = r0 + tid; i < r1; i += RE_THREADS) a.zout[i] = zc[i];
  }
  if (tid == 0) {
    a.f[e] = f; a.iters[e] = it; a.reason[e] = reason;
    if (a.npass != nullptr) a.npass[e] = npass;
  }
}

// ------------------------------------------------------------------------------------------------------------
// Fused per-entity L-BFGS / OWL-QN (L1 and elastic-net random effects): a transcription of batched_lbfgs
// (optimization/batched.py) for ONE entity per workgroup -- two-loop recursion over a ring of m (S, Y) pairs,
// OWL-QN pseudo-gradient / direction alignment / orthant projection when OWL, backtracking Armijo line search,
// Photon's convergence rules. Every function evaluation is one row_pass<1> over the entity's CSR rows; w, the smooth
// gradient at w, the two-loop vector (then the direction) and the trial point live in LDS. The (S, Y) history is
// too large for LDS (2 m dmax doubles) and lives in a global workspace PER RESIDENT WORKGROUP: the grid is
// persistent and a workgroup takes its next entity from a ticket counter (largest entities first). A thread
// reads and writes only its own coefficients j = tid + 256 q of the history, so the workspace needs no fences.
// Floating-point contraction is off in the kernel body: products and sums round as the torch ops of
// batched_lbfgs do (W + t d, q - a Y, f + 1e-4 t g.d are a multiply and an add there), which keeps the two
// within summation-order rounding of each other.
#define RE_LB_MMAX 10                // history pairs at most (the two-loop coefficients stay in registers)

struct ReLbfgsArgs {
  ReTronArgs a;              // data, outputs, l2, tol, max_iter, dmax (max_fail / max_cg / gsc / xf2 unused)
  double l1;
  int m, max_ls;             // history pairs (<= RE_LB_MMAX), line-search trials
  double* hist;              // [grid][2][m][dmax] S then Y of each resident workgroup
  int* ticket;               // dequeue counter (zero before the launch)
};

template <int LOSS, bool OWL>
__global__ __launch_bounds__(RE_THREADS) void re_lbfgs_csr_kernel(ReLbfgsArgs p) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) double smem[];
  __shared__ int sTicket;
  const ReTronArgs& a = p.a;
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const int dm = a.dmax, m = p.m;
  const double l1 = p.l1;
  double* sW = smem;
  double* sGs = sW + dm;    // smooth gradient at W (the pseudo-gradient is formed from sW, sGs, l1 on the fly)
  double* sQ = sGs + dm;    // two-loop vector, then the search direction
  double* sT = sQ + dm;     // trial point
  double* acc = sT + dm;    // RE_NW accumulators; acc[0 .. d) = smooth gradient of the last evaluation
  double* red = acc + RE_NW * dm;
  double* rho = red + 2 * RE_NW * 8;
  double* myacc = acc + w * dm;
  double* hS = p.hist + (size_t)blockIdx.x * 2 * m * dm;
  double* hY = hS + (size_t)m * dm;
  double* D[2] = {a.scr, a.scr + a.n_rows};
  double* Z[2] = {a.scr + 2 * a.n_rows, a.scr + 3 * a.n_rows};

  // OWL-QN pseudo-gradient component (the smooth gradient itself without L1)
  auto pgrad = [&](double wj, double gj) -> double {
    if (!OWL) return gj;
    if (wj != 0.0) return gj + (wj > 0.0 ? l1 : -l1);
    const double dminus = gj - l1, dplus = gj + l1;
    return dminus > 0.0 ? dminus : (dplus < 0.0 ? dplus : 0.0);
  };

  for (;;) {
    __syncthreads();
    if (tid == 0) sTicket = atomicAdd(p.ticket, 1);
    __syncthreads();
    const int tk = sTicket;
    if (tk >= a.n_launch) break;
    const int e = a.order[tk];
    const long long r0 = a.row_ptr[e], r1 = a.row_ptr[e + 1];
    const long long c0 = a.col_ptr[e];
    const int d = (int)(a.col_ptr[e + 1] - c0);
    int cur = 0, parity = 0, npass = 0;
    double* Wg = a.W + c0;

    auto zero_own = [&]() {
      for (int j = lane; j < d; j += 64) myacc[j] = 0.0;
    };
    // smooth value + gradient at vec (MODE 1: writes D / Z buffer ``nb``); the gradient lands in acc[0 .. d) after
    // the fixed-order wave combine; gg = ||g||^2, an = ||vec||_1
    auto value_grad = [&](const double* vec, int nb, bool at_zero, double& gg, double& an) -> double {
      ++npass;
      __syncthreads();
      zero_own();
      double fp = 0.0;
      if (at_zero) row_pass<2, LOSS>(a, r0, r1, vec, myacc, nullptr, nullptr, nullptr, fp);
      else row_pass<1, LOSS>(a, r0, r1, vec, myacc, nullptr, D[nb], Z[nb], fp);
      __syncthreads();
      double s4[4] = {fp, 0.0, 0.0, 0.0};
      for (int j = tid; j < d; j += RE_THREADS) {
        double g = acc[j];
#pragma unroll
        for (int q = 1; q < RE_NW; ++q) g += acc[q * dm + j];
        const double v = vec[j];
        g += a.l2 * v;
        acc[j] = g;
        s4[1] += v * v;
        s4[2] += g * g;
        s4[3] += fabs(v);
      }
      block_sums<4>(s4, red, parity);
      gg = s4[2];
      an = s4[3];
      return s4[0] + 0.5 * a.l2 * s4[1];
    };

    for (int j = tid; j < d; j += RE_THREADS) sW[j] = Wg[j];
    double gs2, an;
    double f = value_grad(sW, cur, false, gs2, an);
    double s2[2] = {0.0, 0.0};
    for (int j = tid; j < d; j += RE_THREADS) {
      const double wj = sW[j], gj = acc[j];
      sGs[j] = gj;
      s2[0] += wj != 0.0 ? 1.0 : 0.0;
      const double pj = pgrad(wj, gj);
      s2[1] += pj * pj;
    }
    block_sums<2>(s2, red, parity);
    double pg2 = s2[1];                        // ||pseudo-gradient||^2 at W
    double f0z = f, g0n = sqrt(gs2);           // tolerances from the SMOOTH state at zero (as _Convergence)
    if (s2[0] != 0.0) {
      for (int j = tid; j < d; j += RE_THREADS) sT[j] = 0.0;
      double g0, a0;
      f0z = value_grad(sT, 0, true, g0, a0);
      g0n = sqrt(g0);
    }
    const double loss_tol = f0z * a.tol, grad_tol = g0n * a.tol;
    if (OWL) f = f + l1 * an;
    int it = 0, reason = 0, nh = 0, head = m - 1;
    bool active = true;
    if (!(pg2 > 0.0)) { reason = 4; active = false; }

    for (int guard = 0; active && guard < a.max_iter + 2; ++guard) {
      // ---- two-loop recursion on the pseudo-gradient; recency k lives in ring slot (head - k) mod m
      for (int j = tid; j < d; j += RE_THREADS) sQ[j] = pgrad(sW[j], sGs[j]);
      double alpha[RE_LB_MMAX] = {};
      double yy = 0.0;
#pragma unroll
      for (int k = 0; k < RE_LB_MMAX; ++k) {
        if (k < nh) {
          const int slot = (head - k + m) % m;
          const double* S = hS + (size_t)slot * dm;
          const double* Y = hY + (size_t)slot * dm;
          double s[2] = {0.0, 0.0};
          for (int j = tid; j < d; j += RE_THREADS) {
            s[0] += S[j] * sQ[j];
            if (k == 0) s[1] += Y[j] * Y[j];
          }
          block_sums<2>(s, red, parity);
          if (k == 0) yy = s[1];
          const double ak = rho[slot] * s[0];
          alpha[k] = ak;
          for (int j = tid; j < d; j += RE_THREADS) sQ[j] = sQ[j] - ak * Y[j];
        }
      }
      if (nh > 0) {
        const double den = rho[head] * yy;
        const double scale = 1.0 / (den > 1e-300 ? den : 1e-300);
        for (int j = tid; j < d; j += RE_THREADS) sQ[j] = sQ[j] * scale;
      }
#pragma unroll
      for (int k = RE_LB_MMAX - 1; k >= 0; --k) {
        if (k < nh) {
          const int slot = (head - k + m) % m;
          const double* S = hS + (size_t)slot * dm;
          const double* Y = hY + (size_t)slot * dm;
          double s[1] = {0.0};
          for (int j = tid; j < d; j += RE_THREADS) s[0] += Y[j] * sQ[j];
          block_sums<1>(s, red, parity);
          const double c = alpha[k] - rho[slot] * s[0];
          for (int j = tid; j < d; j += RE_THREADS) sQ[j] = sQ[j] + c * S[j];
        }
      }
      // ---- direction -q (OWL: components that do not descend along the pseudo-gradient are dropped)
      double s3[3] = {0.0, 0.0, 0.0};
      for (int j = tid; j < d; j += RE_THREADS) {
        const double pj = pgrad(sW[j], sGs[j]);
        double dj = -sQ[j];
        if (OWL) dj = dj * pj < 0.0 ? dj : 0.0;
        sQ[j] = dj;
        s3[0] += pj * dj;
        s3[1] += dj * dj;
        s3[2] += pj * (-pj);
      }
      block_sums<3>(s3, red, parity);
      double gd = s3[0], dd = s3[1];
      if (gd >= 0.0) {             // not a descent direction: steepest descent, history dropped
        for (int j = tid; j < d; j += RE_THREADS) sQ[j] = -pgrad(sW[j], sGs[j]);
        nh = 0;
        gd = s3[2];
        dd = -s3[2];
      }
      // ---- backtracking Armijo line search over orthant-projected trial points
      const double dn = sqrt(dd > 0.0 ? dd : 0.0);
      double t = it == 0 ? 1.0 / (dn > 1e-300 ? dn : 1e-300) : 1.0;
      const double shrink = it == 0 ? (OWL ? 0.1 : 0.5) : 0.5;
      bool found = false;
      double ft = f, gt2 = 0.0;
      for (int ls = 0; ls < p.max_ls && !found; ++ls) {
        for (int j = tid; j < d; j += RE_THREADS) {
          const double wj = sW[j];
          double x = wj + t * sQ[j];
          if (OWL) {
            const double o = wj != 0.0 ? wj : -pgrad(wj, sGs[j]);     // the orthant's sign
            x = ((x > 0.0 && o > 0.0) || (x < 0.0 && o < 0.0)) ? x : 0.0;
          }
          sT[j] = x;
        }
        double at;
        ft = value_grad(sT, cur ^ 1, false, gt2, at);
        if (OWL) ft = ft + l1 * at;
        found = isfinite(ft) && ft <= f + 1e-4 * t * gd;
        if (!found) t = t * shrink;
      }
      // ---- accepted point: history pair (s, y of the SMOOTH gradients), new state
      const double f_prev = f;
      if (found) {
        double u2[2] = {0.0, 0.0};
        for (int j = tid; j < d; j += RE_THREADS) {
          const double x = sT[j], gj = acc[j];
          u2[0] += (x - sW[j]) * (gj - sGs[j]);
          const double pj = pgrad(x, gj);
          u2[1] += pj * pj;
        }
        block_sums<2>(u2, red, parity);
        const double sy = u2[0];
        pg2 = u2[1];
        const bool upd = sy > 1e-300;
        if (upd) {
          head = (head + 1) % m;
          nh = nh < m ? nh + 1 : m;
          if (tid == 0) rho[head] = 1.0 / sy;
        }
        double* S = hS + (size_t)head * dm;
        double* Y = hY + (size_t)head * dm;
        for (int j = tid; j < d; j += RE_THREADS) {
          const double x = sT[j], gj = acc[j];
          if (upd) { S[j] = x - sW[j]; Y[j] = gj - sGs[j]; }
          sW[j] = x;
          sGs[j] = gj;
        }
        f = ft;
        cur ^= 1;
        ++it;
      }
      int rc = 0;
      if (found && sqrt(pg2 > 0.0 ? pg2 : 0.0) <= grad_tol) rc = 4;
      if (found && fabs(f - f_prev) <= loss_tol) rc = 3;
      if (!found) rc = 2;
      if (it >= a.max_iter) rc = 1;
      if (rc > 0) { reason = rc; active = false; }
    }
    __syncthreads();
    for (int j = tid; j < d; j += RE_THREADS) Wg[j] = sW[j];
    if (a.zout != nullptr) {
      const double* zc = Z[cur];
      for (long long i = r0 + tid; i < r1; i += RE_THREADS) a.zout[i] = zc[i];
    }
    if (tid == 0) {
      a.f[e] = f; a.iters[e] = it; a.reason[e] = reason;
      if (a.npass != nullptr) a.npass[e] = npass;
    }
  }
}

// Lean streaming TRON (d_e <= 1024): the same solve as re_tron_csr_kernel with only the GATHERED vector and the
// per-wave accumulators in LDS ((1 + RE_NW) x dmax doubles: 40 KB at dmax 1024, so four workgroups = 16 waves per
// CU instead of two). A thread owns coefficients j = tid + 256 q (q < J) for the whole solve: their CG step and
// residual live in its registers, the gradient at W in global scratch (a.gsc) and W itself is updated in place
// in a.W (both are touched once per TRON iteration by their owner thread only). Held to <= 168 VGPRs (3 waves
// per SIMD): small and mid entities are latency-bound (a pass is a few dependent batches), so more entities in
// flight per CU is more streaming throughput.
// Measured on 43K game5pl-like entities (scripts/re_fused_bench.py, profiles/re_lean_ab_r4.md): 3 waves per SIMD
// (<= 168 VGPRs, 12 waves per CU) with two row groups per batch in function evaluations (one: same total, the 64
// largest entities 33.6 instead of 28.1 ms) and three in Hessian-vector passes (four: +15 %); 4 waves per SIMD
// spills in the row loop (80 ms vs 61 ms for re_tron_csr_kernel)
// waves per lean workgroup (one entity): an A/B switch of the profiling builds (production: RE_NW)
#ifndef LEAN_NW
#define LEAN_NW RE_NW
#endif
#define LEAN_THREADS (LEAN_NW * 64)
// row pass of the lean kernel: quads over padded rows (Q) or the strided row_pass
template <bool Q, int MODE, int LOSS, int U>
__device__ __forceinline__ void lean_pass(const ReTronArgs& a, long long r0, long long r1, const double* vec,
                                          double* acc, const double* Dc, double* Dn, double* Zn, double& fpart) {
  if constexpr (Q) row_pass_q<MODE, LOSS, U, LEAN_NW>(a, r0, r1, vec, acc, Dc, Dn, Zn, fpart);
  else row_pass<MODE, LOSS, U, LEAN_NW>(a, r0, r1, vec, acc, Dc, Dn, Zn, fpart);
}
#ifndef LEAN_WPE
#define LEAN_WPE 3
#endif
#ifndef LEAN_UF
#define LEAN_UF 1
#endif
#ifndef LEAN_UH
#define LEAN_UH 3
#endif
template <int LOSS, int J, bool Q>
__global__ __launch_bounds__(LEAN_THREADS) __attribute__((amdgpu_waves_per_eu(LEAN_WPE, LEAN_WPE)))
void re_tron_lean_kernel(ReTronArgs a) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int e = __builtin_amdgcn_readfirstlane(a.order[blockIdx.x]);
  const long long r0 = uniform_i64(a.row_ptr[e]), r1 = uniform_i64(a.row_ptr[e + 1]);
  const long long c0 = uniform_i64(a.col_ptr[e]);
  const int d = (int)(uniform_i64(a.col_ptr[e + 1]) - c0);
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const int dm = a.dmax;
  double* sD = smem;        // CG direction; W / the trial point during a function evaluation
  double* acc = sD + dm;    // LEAN_NW accumulators; acc[0 .. d) = combined gradient after a function evaluation
  double* red = acc + LEAN_NW * dm;
  double* myacc = acc + w * dm;
  double* D[2] = {a.scr, a.scr + a.n_rows};
  double* Z[2] = {a.scr + 2 * a.n_rows, a.scr + 3 * a.n_rows};
  double* Wg = a.W + c0;
  double* Gg = a.gsc + c0;
  int cur = 0, parity = 0, npass = 0;
  double S[J], R[J];

  auto combined = [&](int j) -> double {
    double g = acc[j];
#pragma unroll
    for (int q = 1; q < LEAN_NW; ++q) g += acc[q * dm + j];
    return g;
  };
  // value + gradient at sD (or at zero); gradient -> acc[0 .. d)
  auto value_grad = [&](bool at_zero, int nb, double& gg) -> double {
    ++npass;
    __syncthreads();
    for (int j = lane; j < d; j += 64) myacc[j] = 0.0;
    double fp = 0.0;
    if (at_zero) lean_pass<Q, 2, LOSS, LEAN_UF>(a, r0, r1, sD, myacc, nullptr, nullptr, nullptr, fp);
    else lean_pass<Q, 1, LOSS, LEAN_UF>(a, r0, r1, sD, myacc, nullptr, D[nb], Z[nb], fp);
    __syncthreads();
    double s3[3] = {fp, 0.0, 0.0};
#pragma unroll
    for (int q = 0; q < J; ++q) {
      const int j = tid + LEAN_THREADS * q;
      if (j < d) {
        const double v = at_zero ? 0.0 : sD[j];
        const double g = combined(j) + a.l2 * v;
        acc[j] = g;
        s3[1] += v * v;
        s3[2] += g * g;
      }
    }
    block_sums<3, LEAN_NW>(s3, red, parity);
    gg = s3[2];
    return s3[0] + 0.5 * a.l2 * s3[1];
  };

#pragma unroll
  for (int q = 0; q < J; ++q) {
    const int j = tid + LEAN_THREADS * q;
    if (j < d) sD[j] = Wg[j];
  }
  double gnorm2;
  double f = value_grad(false, cur, gnorm2);
  double nz[1] = {0.0};
#pragma unroll
  for (int q = 0; q < J; ++q) {
    const int j = tid + LEAN_THREADS * q;
    if (j < d) {
      Gg[j] = acc[j];
      nz[0] += sD[j] != 0.0 ? 1.0 : 0.0;
    }
  }
  block_sums<1, LEAN_NW>(nz, red, parity);
  double f0z = f, g0n = sqrt(gnorm2);
  bool g0_lazy = false;
  if (nz[0] != 0.0) {
    if (a.xf2 != nullptr) {
      // warm start: the tolerances scale with the zero point's f(0) and ||g(0)|| (Optimizer.scala). f(0) needs only
      // the rows' offsets; ||g(0)|| = ||X_e^T c|| <= ||X_e||_F ||c|| (c_i = w_i l'(o_i)) stands in until a gradient
      // norm comes below the bound's tolerance -- then the exact pass at zero runs (convergence decisions are
      // those of the exact norm). No pass over the entity's entries for the common case.
      double s2[2] = {0.0, 0.0};
      for (long long i = r0 + tid; i < r1; i += LEAN_THREADS) {
        double l, dl, d2;
        loss_t<LOSS>(gld(a.off + i), gld(a.y + i), l, dl, d2);
        const double wi = gld(a.wt + i);
        s2[0] += wx(wi, l);
        s2[1] += wx(wi, dl) * wx(wi, dl);
      }
      block_sums<2, LEAN_NW>(s2, red, parity);
      f0z = s2[0];
      g0n = sqrt(gld(a.xf2 + e) * s2[1]) * (1.0 + 1e-6) + 1e-300;
      g0_lazy = true;
    } else {
      double g0;
      f0z = value_grad(true, 0, g0);
      g0n = sqrt(g0);
    }
  }
  const double loss_tol = f0z * a.tol;
  double grad_tol = g0n * a.tol;
  double delta = sqrt(gnorm2);
  int it = 0, fails = 0, reason = 0;
  bool active = true;
  if (delta == 0.0) { reason = 4; active = false; }
  const int guard_max = a.max_iter * (a.max_fail + 1) + 5;
  for (int guard = 0; active && guard < guard_max; ++guard) {
    // truncated CG at W: one Hessian-vector pass, one combine sweep with the five dot products, one update sweep
#pragma unroll
    for (int q = 0; q < J; ++q) {
      const int j = tid + LEAN_THREADS * q;
      const double g = j < d ? Gg[j] : 0.0;
      S[q] = 0.0;
      R[q] = -g;
      if (j < d) sD[j] = -g;
    }
    double rtr = gnorm2, sts = 0.0;
    const double cg_tol2 = 0.01 * gnorm2;        // (0.1 ||g||)^2
    for (int k = 0; k < a.max_cg; ++k) {
      if (!(rtr > cg_tol2)) break;
      ++npass;
      __syncthreads();
      for (int j = lane; j < d; j += 64) myacc[j] = 0.0;
      double fp = 0.0;
      lean_pass<Q, 0, LOSS, LEAN_UH>(a, r0, r1, sD, myacc, D[cur], nullptr, nullptr, fp);
      __syncthreads();
      double s5[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
      double H[J];
#pragma unroll
      for (int q = 0; q < J; ++q) {
        const int j = tid + LEAN_THREADS * q;
        H[q] = 0.0;
        if (j < d) {
          const double dj = sD[j];
          const double h = combined(j) + a.l2 * dj;
          H[q] = h;
          s5[0] += dj * h;
          s5[1] += S[q] * dj;
          s5[2] += dj * dj;
          s5[3] += R[q] * h;
          s5[4] += h * h;
        }
      }
      block_sums<5, LEAN_NW>(s5, red, parity);
      const TronCgStep c = tron_cg_step(rtr, sts, delta, s5[0], s5[1], s5[2], s5[3], s5[4]);
#pragma unroll
      for (int q = 0; q < J; ++q) {
        const int j = tid + LEAN_THREADS * q;
        if (j < d) {
          const double dj = sD[j];
          S[q] += c.al * dj;
          const double r = R[q] - c.al * H[q];
          R[q] = r;
          if (!c.hit) sD[j] = r + c.beta * dj;
        }
      }
      if (c.hit) break;
      rtr = uniform_f64(c.rn);
      sts = uniform_f64(c.tn);
    }
    // trial point W + step (in sD), trust-region update, acceptance
    double s3[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int q = 0; q < J; ++q) {
      const int j = tid + LEAN_THREADS * q;
      if (j < d) {
        const double sj = S[q];
        s3[0] += Gg[j] * sj;
        s3[1] += sj * R[q];
        s3[2] += sj * sj;
        sD[j] = Wg[j] + sj;
      }
    }
    block_sums<3, LEAN_NW>(s3, red, parity);
    const double gs = s3[0], pred = -0.5 * (gs - s3[1]), snorm = sqrt(s3[2]);
    double gn2;
    const double fn = value_grad(false, cur ^ 1, gn2);   // trial gradient in acc[0 .. d)
    delta = uniform_f64(tron_radius(delta, snorm, gs, f, fn, pred, it == 0));
    const bool accept = tron_accept(f, fn, pred);
    const double f_prev = f;
    if (accept) {
#pragma unroll
      for (int q = 0; q < J; ++q) {
        const int j = tid + LEAN_THREADS * q;
        if (j < d) {
          Wg[j] = sD[j];
          Gg[j] = acc[j];
        }
      }
      gnorm2 = gn2;
      f = fn;
      cur ^= 1;
      ++it;
      fails = 0;
    } else {
      ++fails;
    }
    const bool not_impr = !accept && fails >= a.max_fail;
    if (accept && g0_lazy && sqrt(gnorm2) <= grad_tol) {
      // the bound no longer decides: the exact ||g(0)|| (a pass at zero; acc is free, Gg holds the gradient)
      double g0;
      (void)value_grad(true, 0, g0);
      grad_tol = sqrt(g0) * a.tol;
      g0_lazy = false;
    }
    const int rc = tron_reason(accept, not_impr, gnorm2, grad_tol, f, f_prev, loss_tol, it, a.max_iter);
    if (rc > 0) { reason = rc; active = false; }
  }
  __syncthreads();
  if (a.zout != nullptr) {
    const double* zc = Z[cur];
    for (long long i = r0 + tid; i < r1; i += LEAN_THREADS) a.zout[i] = zc[i];
  }
  if (tid == 0) {
    a.f[e] = f; a.iters[e] = it; a.reason[e] = reason;
    if (a.npass != nullptr) a.npass[e] = npass;
  }
}

// ============================================================================================================
// Tall-narrow entities (d_e <= 64 coefficients, typically more rows than coefficients): ONE WAVE PER ENTITY, the
// whole TRON with the EXACT per-entity Hessian in LDS -- tron_dense_wave (tron_core.h), which mf_tron_kernel runs
// too. This file supplies the row source: the entity's CSR rows, 16 at a time, their entries scattered from
// registers into the dense LDS block (zero at the start) and zeroed again after use; the NEXT block's entries (and
// the row pointers two blocks ahead) are already in flight while a block computes. For d_e <= 32 (FH) the Hessian
// at the trial point is formed inside the trial point's function evaluation; wider entities keep the Hessian
// weights D per row and run a separate Hessian pass.
// ============================================================================================================
template <int T>
struct TallRows {
  static constexpr bool FH = T <= 2;
  static constexpr int XS = TronDenseCfg<T, FH>::XS, KE = T;     // KE entries per lane and row: rows of <= 16 T
  struct Blk {
    int c[TRON_RB / 4][KE];
    double v[TRON_RB / 4][KE];
    double rs[3];
  };
  const ReTronArgs& a;
  const int lane = threadIdx.x, grp = lane >> 4, gl = lane & 15;
  const long long r0;
  const int nrows, nc;
  double* const Wg;
  double* const D0;
  double* const D1;
  double* const Z0;
  double* const Z1;
  // entity-local 32-bit offsets from per-entity bases (one VGPR per address)
  const long long e0;
  const uint16_t* const lcol;
  const double* const val;

  __device__ __forceinline__ TallRows(const ReTronArgs& a_, int e)
      : a(a_), r0(a_.row_ptr[e]), nrows((int)(a_.row_ptr[e + 1] - r0)),
        nc((int)(a_.col_ptr[e + 1] - a_.col_ptr[e])), Wg(a_.W + a_.col_ptr[e]), D0(a_.scr), D1(a_.scr + a_.n_rows),
        Z0(a_.scr + 2 * a_.n_rows), Z1(a_.scr + 3 * a_.n_rows), e0(a_.nip[r0]), lcol(a_.lcol + e0),
        val(a_.val + e0) {}

  // row pointers of block b (lane q <= TRON_RB: entity-local offset of row b + q)
  __device__ __forceinline__ int fetch(int b) const {
    const int ip = b + (lane <= TRON_RB ? lane : TRON_RB);
    return b < nrows ? (int)(a.nip[r0 + (ip < nrows ? ip : nrows)] - e0) : 0;
  }
  // issue the loads of block b (entries + per-row scalars: mode 0 = D[cur] in rs[0], else wt / off / y)
  __device__ __forceinline__ void issue(Blk& B, int b, int np, int mode, int cur) const {
    B.rs[0] = B.rs[1] = B.rs[2] = 0.0;
    if (lane < TRON_RB && b + lane < nrows) {
      const long long i = r0 + b + lane;
      if (mode == 0) B.rs[0] = (cur ? D1 : D0)[i];
      else { B.rs[0] = a.wt[i]; B.rs[1] = a.off[i]; B.rs[2] = a.y[i]; }
    }
#pragma unroll
    for (int u = 0; u < TRON_RB / 4; ++u) {
      const int q = u * 4 + grp;
      const int lo = __shfl(np, q, 64), hi = __shfl(np, q + 1, 64);
#pragma unroll
      for (int k = 0; k < KE; ++k) {
        const int p = lo + gl + 16 * k;
        const bool in = p < hi;
        B.c[u][k] = in ? (int)lcol[p] : -1;
        B.v[u][k] = in ? val[p] : 0.0;
      }
    }
  }
  template <bool ZERO>
  __device__ __forceinline__ void scatter(const Blk& B, double* Xs) const {
#pragma unroll
    for (int u = 0; u < TRON_RB / 4; ++u)
#pragma unroll
      for (int k = 0; k < KE; ++k)
        if (B.c[u][k] >= 0) Xs[(u * 4 + grp) * XS + B.c[u][k]] = ZERO ? 0.0 : B.v[u][k];
  }
  __device__ __forceinline__ void stage(const Blk& B, double* Xs) const { scatter<false>(B, Xs); }
  __device__ __forceinline__ void unstage(const Blk& B, double* Xs) const { scatter<true>(B, Xs); }
};

template <int T, int LOSS>
__global__ __launch_bounds__(64) void re_tron_tall_kernel(ReTronArgs a) {
  using C = TronDenseCfg<T, TallRows<T>::FH>;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int e = a.order[blockIdx.x];
  for (int i = threadIdx.x; i < TRON_RB * C::XS; i += 64) smem[C::XOFF + i] = 0.0;    // the staged block starts empty
  tron_dense_wave<T, LOSS>(a, e, TallRows<T>(a, e), smem);
}

// ============================================================================================================
// Row-space TRON for WIDE entities of 64 < n_e <= 192 rows (optimization/row_space.py: the entity's problem is the
// dense GLM with the n x n lower-triangular design matrix L_e, K_e = X_e X_e^T = L_e L_e^T). The n <= 64 classes
// run rs_tron_kernel / rs_tron_dpp_kernel (glm_kernels.hip); here ONE WAVE owns one problem with E = ceil(n / 64)
// vector entries per lane (lane l: entries l, l + 64, ...), L's packed lower triangle is staged once into the
// wave's LDS, every sum is a DPP / readlane wave sum (no workgroup barriers) and the whole TRON runs in the kernel.
// Against the primal fused kernel on such an entity (d_e ~ 1000 coefficients, ~50 non-zeros per row) every CG
// step is two LDS-resident triangular mat-vecs over n-length vectors instead of a pass over the rows' non-zeros
// plus d-length vector work. Same TRON semantics as rs_tron_kernel (photon-lib/.../optimization/TRON.scala).
// ============================================================================================================
template <int E, int LOSS>
__global__ __launch_bounds__(64) void rs_tron_big_kernel(int B, int n, const double* __restrict__ Lm,
                                                         const double* __restrict__ Y, const double* __restrict__ O,
                                                         const double* __restrict__ WT, double* __restrict__ Beta,
                                                         double* __restrict__ Fout, int* __restrict__ Iters,
                                                         int* __restrict__ Reason, double* __restrict__ Zout,
                                                         double l2, double tol, int max_iter, int max_fail,
                                                         int max_cg) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int lane = threadIdx.x;
  const long long b = blockIdx.x;
  if (b >= B) return;
  const int np = n * (n + 1) / 2;
  double* Lp = smem;              // packed lower triangle: L[r][c] (c <= r) at r (r + 1) / 2 + c
  double* sv = smem + np;         // [n] vector broadcast to the lanes
  const double* Lb = Lm + b * (long long)n * n;
  for (int r = 0; r < n; ++r)
    for (int c = lane; c <= r; c += 64) Lp[r * (r + 1) / 2 + c] = Lb[(long long)r * n + c];
  bool on[E];
  double y[E], off[E], wt[E], W[E];
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const int i = lane + 64 * e;
    on[e] = i < n;
    const long long o = b * n + (on[e] ? i : 0);
    y[e] = on[e] ? Y[o] : 0.0;
    off[e] = on[e] ? O[o] : 0.0;
    wt[e] = on[e] ? WT[o] : 0.0;
    W[e] = on[e] ? Beta[o] : 0.0;
  }
  wave_sync();
  auto gsum = [&](const double (&v)[E]) -> double {
    double s = 0.0;
#pragma unroll
    for (int e = 0; e < E; ++e) s += v[e];
    return wave_total(s);
  };
  auto gsum2 = [&](const double (&u)[E], const double (&v)[E]) -> double {
    double s = 0.0;
#pragma unroll
    for (int e = 0; e < E; ++e) s = fma(u[e], v[e], s);
    return wave_total(s);
  };
  auto put = [&](const double (&v)[E]) {
#pragma unroll
    for (int e = 0; e < E; ++e)
      if (on[e]) sv[lane + 64 * e] = v[e];
    wave_sync();
  };
  auto mv = [&](const double (&v)[E], double (&out)[E]) {     // (L v)_i
    put(v);
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const int i = on[e] ? lane + 64 * e : 0;
      const double* Lr = Lp + i * (i + 1) / 2;
      double a0 = 0.0, a1 = 0.0;
      int j = 0;
      for (; j + 1 <= i; j += 2) {
        a0 = fma(Lr[j], sv[j], a0);
        a1 = fma(Lr[j + 1], sv[j + 1], a1);
      }
      if (j <= i) a0 = fma(Lr[j], sv[j], a0);
      out[e] = on[e] ? a0 + a1 : 0.0;
    }
    wave_sync();                       // sv reads done before the next put
  };
  auto mvt = [&](const double (&u)[E], double (&out)[E]) {    // (L^T u)_i
    put(u);
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const int i = on[e] ? lane + 64 * e : 0;
      double a0 = 0.0, a1 = 0.0;
      int r = i;
      for (; r + 1 < n; r += 2) {
        a0 = fma(Lp[r * (r + 1) / 2 + i], sv[r], a0);
        a1 = fma(Lp[(r + 1) * (r + 2) / 2 + i], sv[r + 1], a1);
      }
      if (r < n) a0 = fma(Lp[r * (r + 1) / 2 + i], sv[r], a0);
      out[e] = on[e] ? a0 + a1 : 0.0;
    }
    wave_sync();
  };
  // value, gradient and Hessian weights at v; z (margins L v, no offset) kept for the output
  auto vg = [&](const double (&v)[E], double& f, double (&gr)[E], double (&Dw)[E], double (&z)[E]) {
    mv(v, z);
    double t[E], fl[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
      double l = 0.0, dl = 0.0, d2 = 0.0;
      if (on[e]) loss_t<LOSS>(z[e] + off[e], y[e], l, dl, d2);
      fl[e] = wx(wt[e], l) + 0.5 * l2 * v[e] * v[e];
      t[e] = wx(wt[e], dl);
      Dw[e] = wx(wt[e], d2);
    }
    f = gsum(fl);
    mvt(t, gr);
#pragma unroll
    for (int e = 0; e < E; ++e) gr[e] = on[e] ? gr[e] + l2 * v[e] : 0.0;
  };
  double f, gr[E], Dw[E], Z[E];
  vg(W, f, gr, Dw, Z);
  double f0z, g0n;
  double nzv[E];
#pragma unroll
  for (int e = 0; e < E; ++e) nzv[e] = W[e] != 0.0 ? 1.0 : 0.0;
  if (gsum(nzv) == 0.0) {
    f0z = f;
    g0n = sqrt(gsum2(gr, gr));
  } else {
    double zero[E], g0[E], D0[E], z0[E];
#pragma unroll
    for (int e = 0; e < E; ++e) zero[e] = 0.0;
    vg(zero, f0z, g0, D0, z0);
    g0n = sqrt(gsum2(g0, g0));
  }
  const double loss_tol = f0z * tol, grad_tol = g0n * tol;
  double delta = sqrt(gsum2(gr, gr));
  int it = 0, fails = 0, reason = 0;
  bool active = true;
  if (delta == 0.0) { reason = 4; active = false; }
  const int guard_max = max_iter * (max_fail + 1) + 5;
  for (int guard = 0; active && guard < guard_max; ++guard) {
    // ---- truncated CG at W (Hessian weights Dw of the current iterate)
    double step[E], r[E], d[E];
#pragma unroll
    for (int e = 0; e < E; ++e) { step[e] = 0.0; r[e] = -gr[e]; d[e] = r[e]; }
    double rtr = gsum2(r, r);
    const double cg_tol = 0.1 * sqrt(gsum2(gr, gr));
    for (int k = 0; k < max_cg; ++k) {
      if (!(sqrt(rtr > 0.0 ? rtr : 0.0) > cg_tol)) break;
      double Ld[E], Hd[E], Hl[E];
      mv(d, Ld);
#pragma unroll
      for (int e = 0; e < E; ++e) Ld[e] *= Dw[e];
      mvt(Ld, Hd);
#pragma unroll
      for (int e = 0; e < E; ++e) Hl[e] = Hd[e] + l2 * d[e];
      const double dhd = gsum2(d, Hl), std_ = gsum2(step, d), sts = gsum2(step, step), dtd = gsum2(d, d);
      const double alpha = rtr / (dhd == 0.0 ? 1.0 : dhd);
      double tr[E];
#pragma unroll
      for (int e = 0; e < E; ++e) tr[e] = step[e] + alpha * d[e];
      const double tn = gsum2(tr, tr);
      const bool hit = sqrt(tn > 0.0 ? tn : 0.0) > delta;
      double a = alpha;
      if (hit) {
        const double dsq = delta * delta;
        const double q = std_ * std_ + dtd * (dsq - sts);
        const double rad = sqrt(q > 0.0 ? q : 0.0);
        const double den1 = std_ + rad;
        a = std_ >= 0.0 ? (dsq - sts) / (den1 > 1e-300 ? den1 : 1e-300) : (rad - std_) / (dtd > 1e-300 ? dtd : 1e-300);
      }
      double rn_v[E];
#pragma unroll
      for (int e = 0; e < E; ++e) {
        step[e] = step[e] + a * d[e];
        rn_v[e] = r[e] - a * Hl[e];
      }
      const double rn = gsum2(rn_v, rn_v);
      const double beta = rn / (rtr == 0.0 ? 1.0 : rtr);
#pragma unroll
      for (int e = 0; e < E; ++e) {
        r[e] = rn_v[e];
        if (!hit) d[e] = rn_v[e] + beta * d[e];
      }
      if (hit) break;
      rtr = rn;
    }
    // ---- trial point, trust-region update, acceptance
    double Wn[E];
#pragma unroll
    for (int e = 0; e < E; ++e) Wn[e] = W[e] + step[e];
    const double gs = gsum2(gr, step);
    const double pred = -0.5 * (gs - gsum2(step, r));
    double fn, gn[E], Dn[E], Zn[E];
    vg(Wn, fn, gn, Dn, Zn);
    const double snorm = sqrt(gsum2(step, step));
    delta = tron_radius(delta, snorm, gs, f, fn, pred, it == 0);
    const bool accept = tron_accept(f, fn, pred);
    const double f_prev = f;
    if (accept) {
#pragma unroll
      for (int e = 0; e < E; ++e) { W[e] = Wn[e]; gr[e] = gn[e]; Dw[e] = Dn[e]; Z[e] = Zn[e]; }
      f = fn;
      ++it;
      fails = 0;
    } else {
      ++fails;
    }
    const bool not_impr = !accept && fails >= max_fail;
    const int rc = tron_reason(accept, not_impr, gsum2(gr, gr), grad_tol, f, f_prev, loss_tol, it, max_iter);
    if (rc > 0) { reason = rc; active = false; }
  }
#pragma unroll
  for (int e = 0; e < E; ++e) {
    if (!on[e]) continue;
    const long long o = b * n + lane + 64 * e;
    Beta[o] = W[e];
    if (Zout != nullptr) Zout[o] = Z[e];
  }
  if (lane == 0) { Fout[b] = f; Iters[b] = it; Reason[b] = reason; }
}

// ============================================================================================================
// REGISTER-RESIDENT fused primal TRON (wide entities: d_e <= 1024, rows of <= 64 non-zeros).
// The fused kernel above streams an entity's CSR rows from memory for every Hessian-vector product (~36 row
// passes per solve at ~3.6 TB/s). Here the rows are loaded ONCE into VGPRs and every later pass runs on-chip:
// * a workgroup of RS_NW = 8 waves holds up to RS_CAP = 8 x 4 x S rows: row r -> slot group sg = r / 4, wave
//   sg % 8, register slot sg / 8; 16 lanes per row, lane k of the row keeps entries k, k + 16, k + 32, k + 48
//   (fp64 value + packed u16 column). Per-row D (current / trial), margins (current / trial), weight, offset and
//   label sit in LDS; the coefficient vectors and one accumulator per wave in LDS as in the streaming kernel.
// * entities longer than RS_CAP rows are split over a CLUSTER of k workgroups (member m holds rows
//   [m RS_CAP, (m + 1) RS_CAP)): after every row pass each member publishes its partial sum (d doubles + the
//   loss), the members meet at a cluster barrier (agent-scope release / acquire on a per-task counter), and
//   every member sums the k partials in member order. All control flow then derives from identical sums, so the
//   k replicas of the TRON state stay bitwise identical and no other exchange is needed.
// * ONE persistent launch (one workgroup per CU, grid = resident capacity) serves every task: a workgroup
//   dequeues a ticket (one atomic), a task with k members owns k consecutive tickets (largest tasks first).
//   Tickets are taken in order by running workgroups only, so the earliest incomplete cluster is always filled
//   by workgroups finishing earlier tasks: deadlock-free while k <= the resident workgroups. Every wait is
//   bounded anyway (~1 s, then a global error flag releases every waiter and the host raises).
// Deterministic: fixed-order DPP row sums, per-wave LDS accumulators combined in wave order, member partials
// combined in member order (same LDS ds_add_f64 lane-order assumption as the streaming kernel inside a wave).
// ============================================================================================================
#define RS_NW 8
#define RS_THREADS (RS_NW * 64)
#define RS_DMAX 1024
#define RES_S 12              // register slots per wave (rows per workgroup = 8 x 4 x RES_S)

template <int K>
__device__ __forceinline__ void block_sums8(double (&v)[K], double* __restrict__ red, int& parity) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = wave_total(v[k]);
  double* slot = red + parity * (RS_NW * 8);
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) slot[w * 8 + k] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) {
    double s = 0.0;
#pragma unroll
    for (int q = 0; q < RS_NW; ++q) s += slot[q * 8 + k];
    v[k] = s;
    __builtin_amdgcn_sched_barrier(0);    // one value at a time (8 LDS reads), not 8 x K reads in flight
  }
  parity ^= 1;
}

struct ResTasks {
  int* ticket;               // dequeue counter (zero before the launch)
  const int* task_ent;       // [n_tasks] entity
  const int* task_t0;        // [n_tasks + 1] first ticket of each task (task j has task_t0[j+1] - task_t0[j] members)
  int n_tasks;
  unsigned* bar;             // [n_tasks] cluster barrier counters (zero before the launch)
  double* ws;                // [n_tickets][2][RS_DMAX + 8] member partials (double-buffered by pass parity)
  int* err;                  // set when a cluster wait timed out (the results are then invalid)
};

// Cluster barrier of the k members of one task (k > 1). Producer: every wave drains its stores, workgroup barrier,
// one lane releases at agent scope and adds to the task's counter; consumer: relaxed polls of the counter, one
// agent-scope acquire, workgroup barrier (MI355X_MICROARCH.md, valid hand-off forms). Bounded: ~1 s, then err.
__device__ __forceinline__ void cluster_barrier(unsigned* bar, unsigned target, int* err) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __hip_atomic_fetch_add(bar, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    while (__hip_atomic_load(bar, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
      if (__hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) break;
      if (__builtin_amdgcn_s_memrealtime() - t0 > 100000000ull) {      // 1 s at the 100 MHz constant clock
        __hip_atomic_store(err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        break;
      }
      __builtin_amdgcn_s_sleep(2);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  __syncthreads();
}

template <int S, int LOSS>
__global__ __launch_bounds__(RS_THREADS) void re_tron_res_kernel(ReTronArgs a, ResTasks tk) {
  constexpr int CAP = RS_NW * 4 * S;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const int grp = lane >> 4, gl = lane & 15;
  constexpr int DM = RS_DMAX, DMS = RS_DMAX + 8;   // + a dummy slot (index DM) for the empty register entries
  double* sV = smem;                  // [DMS] gathered vector: CG direction / trial point (sV[DM] == 0)
  double* sH = sV + DMS;              // combined Hessian-vector product / trial gradient
  double* sW = sH + DM;
  double* sG = sW + DM;
  double* sS = sG + DM;              // CG step
  double* sR = sS + DM;              // CG residual
  double* acc = sR + DM;             // [RS_NW][DMS] per-wave accumulators (zero between passes)
  double* rD = acc + RS_NW * DMS;    // [2][CAP] per local row: Hessian weight D (current / trial)
  double* rZ = rD + 2 * CAP;         // [2][CAP] margins x.w (current / trial)
  double* rW = rZ + 2 * CAP;         // [CAP] weight
  double* rO = rW + CAP;             // [CAP] offset
  double* rY = rO + CAP;             // [CAP] label
  double* red = rY + CAP;            // [2][RS_NW][8], then [16] TRON scalars
  double* myacc = acc + w * DMS;
  __shared__ int sTicket;
  for (int i = tid; i < RS_NW * DMS; i += RS_THREADS) acc[i] = 0.0;
  if (tid < 8) sV[DM + tid] = 0.0;

  for (;;) {
    __syncthreads();
    if (tid == 0) sTicket = atomicAdd(tk.ticket, 1);
    __syncthreads();
    const int t = sTicket;
    if (t >= tk.task_t0[tk.n_tasks]) break;
    // task of ticket t: the last j with task_t0[j] <= t
    int lo = 0, hi = tk.n_tasks - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (tk.task_t0[mid] <= t) lo = mid; else hi = mid - 1;
    }
    const int j = lo, m = t - tk.task_t0[j], k = tk.task_t0[j + 1] - tk.task_t0[j];
    const int e = tk.task_ent[j];
    unsigned* bar = tk.bar + j;
    unsigned epoch = 0;
    double* wsm = tk.ws + (size_t)tk.task_t0[j] * 2 * (DM + 8);   // member 0's partials; member q at + q * 2 (DM + 8)
    const long long r0 = a.row_ptr[e];
    const long long rb = r0 + (long long)m * CAP;                  // this member's first row
    const int nloc = (int)min((long long)CAP, a.row_ptr[e + 1] - rb);
    const long long c0 = a.col_ptr[e];
    const int d = (int)(a.col_ptr[e + 1] - c0);
    int cur = 0, parity = 0, npass = 0, wpar = 0;
    double* Wg = a.W + c0;

    // ---- load this member's rows into registers, its row scalars into LDS
    double xv[S][4];
    uint32_t xc[S][2];
    // number of register slots of this wave holding rows: sg = s * RS_NW + w < ceil(nloc / 4)
    const int nsg = (nloc + 3) >> 2;
    const int ns = nsg > w ? (nsg - w + RS_NW - 1) / RS_NW : 0;
    {
      // member-local 32-bit entry offsets (one VGPR per address); loads issued 4 slots at a time
      const long long eb = a.nip[rb];
      const uint16_t* __restrict__ lc = a.lcol + eb;
      const double* __restrict__ vl = a.val + eb;
#pragma unroll
      for (int s = 0; s < S; ++s) {
        const int r = ((s * RS_NW + w) << 2) + grp;
        int p0 = 0, p1 = 0;
        if (s < ns && r < nloc) { p0 = (int)(a.nip[rb + r] - eb); p1 = (int)(a.nip[rb + r + 1] - eb); }
        uint32_t cc[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int p = p0 + gl + 16 * q;
          const bool in = p < p1;
          xv[s][q] = in ? vl[p] : 0.0;
          cc[q] = in ? (uint32_t)lc[p] : (uint32_t)DM;
        }
        xc[s][0] = cc[0] | (cc[1] << 16);
        xc[s][1] = cc[2] | (cc[3] << 16);
        if ((s & 3) == 3) __builtin_amdgcn_sched_barrier(0);
      }
    }
    for (int r = tid; r < nloc; r += RS_THREADS) {
      rW[r] = a.wt[rb + r];
      rO[r] = a.off[rb + r];
      rY[r] = a.y[rb + r];
    }
    for (int jj = tid; jj < d; jj += RS_THREADS) sW[jj] = Wg[jj];

    // One pass over the resident rows. MODE 0: myacc += X^T (D_cur * (X sV)); MODE 1: value + gradient at sV
    // (myacc += X^T (w l'), fpart, trial D / margins -> rD / rZ slot nb); MODE 2: value + gradient at zero.
    auto pass = [&](int mode, int nb, double& fpart) __attribute__((always_inline)) {
      const double* Dc = rD + cur * CAP;
#pragma unroll
      for (int s = 0; s < S; ++s) {
        if (s < ns) {
          int r = ((s * RS_NW + w) << 2) + grp;
          uint32_t p0 = xc[s][0], p1 = xc[s][1];
          // opaque per pass: keeps the compiler from hoisting the decoded LDS addresses of every entry and row
          // out of the solve loops (that doubled the registers of the resident rows)
          asm volatile("" : "+v"(p0), "+v"(p1), "+v"(r));
          const bool valid = r < nloc;
          const uint32_t c[4] = {p0 & 0xFFFFu, p0 >> 16, p1 & 0xFFFFu, p1 >> 16};
          double dot = 0.0;
          if (mode != 2) {
#pragma unroll
            for (int q = 0; q < 4; ++q) dot = fma(xv[s][q], sV[c[q]], dot);
            dot = row16_total(dot);
          }
          double tt = 0.0;
          if (valid) {
            if (mode == 0) {
              tt = Dc[r] * dot;
            } else {
              const double wt = rW[r];
              double l, dl, d2;
              loss_t<LOSS>(dot + rO[r], rY[r], l, dl, d2);
              tt = wx(wt, dl);
              if (gl == 0) {
                fpart += wx(wt, l);
                if (mode == 1) { rD[nb * CAP + r] = wx(wt, d2); rZ[nb * CAP + r] = dot; }
              }
            }
          }
#pragma unroll
          for (int q = 0; q < 4; ++q) atomicAdd(&myacc[c[q]], tt * xv[s][q]);
        }
        __builtin_amdgcn_sched_barrier(0);   // one slot at a time: no hoisting of later slots' gathers
      }
    };
    // Combine the wave accumulators of this member (and zero them), then the members' partials: out[jj] =
    // sum, for jj < d, in every member identically. ``fp`` (this workgroup's loss part, already block-summed)
    // is combined the same way and returned.
    auto combine = [&](double* out, double fp) __attribute__((always_inline)) -> double {
      __syncthreads();
      if (k == 1) {
        for (int jj = tid; jj < d; jj += RS_THREADS) {
          double h = 0.0;
#pragma unroll
          for (int q = 0; q < RS_NW; ++q) { h += acc[q * DMS + jj]; acc[q * DMS + jj] = 0.0; }
          out[jj] = h;
        }
        __syncthreads();
        return fp;
      }
      double* mine = wsm + (size_t)(m * 2 + wpar) * (DM + 8);
      for (int jj = tid; jj < d; jj += RS_THREADS) {
        double h = 0.0;
#pragma unroll
        for (int q = 0; q < RS_NW; ++q) { h += acc[q * DMS + jj]; acc[q * DMS + jj] = 0.0; }
        mine[jj] = h;
      }
      if (tid == 0) mine[DM] = fp;
      ++epoch;
      cluster_barrier(bar, epoch * (unsigned)k, tk.err);
      for (int jj = tid; jj < d; jj += RS_THREADS) {
        double h = 0.0;
        for (int q = 0; q < k; ++q) h += wsm[(size_t)(q * 2 + wpar) * (DM + 8) + jj];
        out[jj] = h;
      }
      double f = 0.0;
      for (int q = 0; q < k; ++q) f += wsm[(size_t)(q * 2 + wpar) * (DM + 8) + DM];
      wpar ^= 1;
      __syncthreads();
      return f;
    };
    // value + gradient at vec (LDS, written to sV first): gradient (l2 included) -> sH; returns f, gg = ||g||^2.
    auto value_grad = [&](const double* vec, int mode, int nb, double& gg) __attribute__((always_inline)) -> double {
      ++npass;
      __syncthreads();
      if (vec != sV)
        for (int jj = tid; jj < d; jj += RS_THREADS) sV[jj] = mode == 2 ? 0.0 : vec[jj];
      __syncthreads();
      double fp[1] = {0.0};
      pass(mode, nb, fp[0]);
      block_sums8<1>(fp, red, parity);
      const double f = combine(sH, fp[0]);
      double s2[2] = {0.0, 0.0};
      for (int jj = tid; jj < d; jj += RS_THREADS) {
        const double v = sV[jj];
        const double g = sH[jj] + a.l2 * v;
        sH[jj] = g;
        s2[0] += v * v;
        s2[1] += g * g;
      }
      block_sums8<2>(s2, red, parity);
      gg = s2[1];
      return f + 0.5 * a.l2 * s2[0];
    };

    // The TRON scalars live in LDS (every thread writes the same value, so no extra barriers): across the row
    // passes nothing but the resident rows and a few indices stays in VGPRs (no spills into the pass loop).
    double* T = red + 2 * RS_NW * 8;      // [16] scalar state
    int* TI = (int*)(T + 12);             // it, fails, reason, active
    enum { F = 0, GN2 = 1, DELTA = 2, LTOL = 3, GTOL = 4, RTR = 5, STS = 6, CGTOL = 7 };
    {
      double gnorm2;
      const double f = value_grad(sW, 1, cur, gnorm2);
      T[F] = f;
      T[GN2] = gnorm2;
    }
    double nz[1] = {0.0};
    for (int jj = tid; jj < d; jj += RS_THREADS) {
      sG[jj] = sH[jj];
      nz[0] += sW[jj] != 0.0 ? 1.0 : 0.0;
    }
    block_sums8<1>(nz, red, parity);
    {
      double f0z = T[F], g0n = sqrt(T[GN2]);
      if (nz[0] != 0.0) {
        double g0;
        f0z = value_grad(sS, 2, 0, g0);
        g0n = sqrt(g0);
      }
      T[LTOL] = f0z * a.tol;
      T[GTOL] = g0n * a.tol;
      T[DELTA] = sqrt(T[GN2]);
      TI[0] = 0; TI[1] = 0; TI[2] = T[DELTA] == 0.0 ? 4 : 0; TI[3] = T[DELTA] == 0.0 ? 0 : 1;
    }
    const int guard_max = a.max_iter * (a.max_fail + 1) + 5;
    for (int guard = 0; TI[3] && guard < guard_max; ++guard) {
      for (int jj = tid; jj < d; jj += RS_THREADS) {
        sS[jj] = 0.0;
        sR[jj] = -sG[jj];
        sV[jj] = -sG[jj];
      }
      T[RTR] = T[GN2];
      T[STS] = 0.0;
      T[CGTOL] = 0.01 * T[GN2];
      for (int kk = 0; kk < a.max_cg; ++kk) {
        // state read BEFORE this step's barriers: a faster thread overwrites RTR / STS after the block sum
        const double rtr = T[RTR], sts = T[STS], delta = T[DELTA];
        if (!(rtr > T[CGTOL])) break;
        ++npass;
        __syncthreads();
        double fpz = 0.0;
        pass(0, 0, fpz);
        combine(sH, 0.0);
        double s5[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
        for (int jj = tid; jj < d; jj += RS_THREADS) {
          const double dj = sV[jj];
          const double h = sH[jj] + a.l2 * dj;
          sH[jj] = h;
          s5[0] += dj * h;
          s5[1] += sS[jj] * dj;
          s5[2] += dj * dj;
          s5[3] += sR[jj] * h;
          s5[4] += h * h;
        }
        block_sums8<5>(s5, red, parity);
        const TronCgStep c = tron_cg_step(rtr, sts, delta, s5[0], s5[1], s5[2], s5[3], s5[4]);
        for (int jj = tid; jj < d; jj += RS_THREADS) {
          const double dj = sV[jj];
          sS[jj] += c.al * dj;
          const double r = sR[jj] - c.al * sH[jj];
          sR[jj] = r;
          if (!c.hit) sV[jj] = r + c.beta * dj;
        }
        if (c.hit) break;
        T[RTR] = c.rn;
        T[STS] = c.tn;
      }
      // ---- trial point W + step (into sV), trust-region update, acceptance
      __syncthreads();
      double s3[3] = {0.0, 0.0, 0.0};
      for (int jj = tid; jj < d; jj += RS_THREADS) {
        const double sj = sS[jj];
        s3[0] += sG[jj] * sj;
        s3[1] += sj * sR[jj];
        s3[2] += sj * sj;
        sV[jj] = sW[jj] + sj;
      }
      block_sums8<3>(s3, red, parity);
      const double gs = s3[0], pred = -0.5 * (gs - s3[1]), snorm = sqrt(s3[2]);
      // state read BEFORE the trial evaluation's barriers (a faster thread rewrites it after them)
      const double f = T[F], gn2_old = T[GN2], delta = T[DELTA];
      int it = TI[0], fails = TI[1];
      double gn2;
      const double fn = value_grad(sV, 1, cur ^ 1, gn2);     // trial gradient in sH
      T[DELTA] = tron_radius(delta, snorm, gs, f, fn, pred, it == 0);
      const bool accept = tron_accept(f, fn, pred);
      double fc = f, gnc = gn2_old;
      if (accept) {
        for (int jj = tid; jj < d; jj += RS_THREADS) {
          sW[jj] = sV[jj];
          sG[jj] = sH[jj];
        }
        gnc = gn2;
        fc = fn;
        cur ^= 1;
        ++it;
        fails = 0;
      } else {
        ++fails;
      }
      T[GN2] = gnc;
      T[F] = fc;
      const bool not_impr = !accept && fails >= a.max_fail;
      const int rc = tron_reason(accept, not_impr, gnc, T[GTOL], fc, f, T[LTOL], it, a.max_iter);
      TI[0] = it;
      TI[1] = fails;
      if (rc > 0) { TI[2] = rc; TI[3] = 0; }
    }
    __syncthreads();
    if (m == 0)
      for (int jj = tid; jj < d; jj += RS_THREADS) Wg[jj] = sW[jj];
    if (a.zout != nullptr)
      for (int r = tid; r < nloc; r += RS_THREADS) a.zout[rb + r] = rZ[cur * CAP + r];
    if (tid == 0 && m == 0) {
      a.f[e] = T[F]; a.iters[e] = TI[0]; a.reason[e] = TI[2];
      if (a.npass != nullptr) a.npass[e] = npass;
    }
  }
}

template <int LOSS, bool Q>
static void lean_launch(const ReTronArgs& a, int n_launch, size_t smem, hipStream_t st) {
  // J coefficients per thread: the smallest of 1 / 2 / 4 with J x LEAN_THREADS >= dmax (dmax <= 1024)
  if (a.dmax <= LEAN_THREADS)
    hipLaunchKernelGGL((re_tron_lean_kernel<LOSS, 1, Q>), dim3(n_launch), dim3(LEAN_THREADS), smem, st, a);
  else if (a.dmax <= 2 * LEAN_THREADS)
    hipLaunchKernelGGL((re_tron_lean_kernel<LOSS, 2, Q>), dim3(n_launch), dim3(LEAN_THREADS), smem, st, a);
  else hipLaunchKernelGGL((re_tron_lean_kernel<LOSS, 4, Q>), dim3(n_launch), dim3(LEAN_THREADS), smem, st, a);
}

extern "C" {

const char* pml_build_id() { return pml_build_stamp + 13; }

// Shared memory of one workgroup for entities of at most ``dmax`` coefficients.
size_t pml_re_tron_smem(int dmax) { return ((size_t)(5 + RE_NW) * dmax + 2 * RE_NW * 8) * sizeof(double); }

int pml_re_tron_csr(const int* order, int n_launch, const long long* row_ptr, const long long* col_ptr,
                    const long long* nip, const uint16_t* lcol, const double* val, const double* y,
                    const double* off, const double* wt, double* scr, long long n_rows, double* W, double* f,
                    int* iters, int* reason, double* zout, int* npass, int loss, double l2, double tol,
                    int max_iter, int max_fail, int max_cg, int dmax, hipStream_t st) {
  if (n_launch <= 0) return 0;
  if (dmax <= 0 || loss < 0 || loss > 2) return -22;
  const size_t smem = pml_re_tron_smem(dmax);
  if (smem > 160 * 1024) return -22;
  ReTronArgs a{order, n_launch, row_ptr, col_ptr, nip, lcol, val, y, off, wt, scr, n_rows, W, f, iters, reason,
               zout, npass, loss, l2, tol, max_iter, max_fail, max_cg, dmax};
  with_loss(loss, [&](auto L) {
    hipLaunchKernelGGL((re_tron_csr_kernel<L()>), dim3(n_launch), dim3(RE_THREADS), smem, st, a);
  });
  LAUNCH_CHECK();
  return 0;
}

// pml_re_tron_csr with a normalization shift (re_tron_csr_kernel<LOSS, true>): ``nc`` = c per coefficient (packed
// like W), ``ni0`` = entity-local intercept column per entity (0 <= i0 < d_e, c[i0] = 0).
int pml_re_tron_csr_shift(const int* order, int n_launch, const long long* row_ptr, const long long* col_ptr,
                          const long long* nip, const uint16_t* lcol, const double* val, const double* y,
                          const double* off, const double* wt, double* scr, long long n_rows, double* W, double* f,
                          int* iters, int* reason, double* zout, int* npass, int loss, double l2, double tol,
                          int max_iter, int max_fail, int max_cg, int dmax, const double* nc, const int* ni0,
                          hipStream_t st) {
  if (n_launch <= 0) return 0;
  if (dmax <= 0 || loss < 0 || loss > 2 || nc == nullptr || ni0 == nullptr) return -22;
  const size_t smem = pml_re_tron_smem(dmax);
  if (smem > 160 * 1024) return -22;
  ReTronArgs a{order, n_launch, row_ptr, col_ptr, nip, lcol, val, y, off, wt, scr, n_rows, W, f, iters, reason,
               zout, npass, loss, l2, tol, max_iter, max_fail, max_cg, dmax};
  a.nc = nc;
  a.ni0 = ni0;
  with_loss(loss, [&](auto L) {
    hipLaunchKernelGGL((re_tron_csr_kernel<L(), true>), dim3(n_launch), dim3(RE_THREADS), smem, st, a);
  });
  LAUNCH_CHECK();
  return 0;
}

// Fused per-entity L-BFGS / OWL-QN (re_lbfgs_csr_kernel): LDS of one workgroup for entities of at most ``dmax``
// coefficients (w, smooth gradient, direction, trial point, RE_NW accumulators, reduction slots, rho[m]).
size_t pml_re_lbfgs_smem(int dmax) {
  return ((size_t)(4 + RE_NW) * dmax + 2 * RE_NW * 8 + RE_LB_MMAX) * sizeof(double);
}

// Workgroups of the L-BFGS kernel resident on the device at once for ``dmax`` (occupancy API x CUs; 0 on error):
// the persistent grid, and the number of history workspaces (2 m dmax doubles each) a launch needs.
int pml_re_lbfgs_grid(int dmax) {
  int dev = 0, cus = 0, per = 0;
  if (dmax <= 0 || pml_re_lbfgs_smem(dmax) > 160 * 1024) return 0;
  if (hipGetDevice(&dev) != hipSuccess) return 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, (const void*)re_lbfgs_csr_kernel<0, true>, RE_THREADS,
                                                   pml_re_lbfgs_smem(dmax)) != hipSuccess) return 0;
  return cus * per;
}

// Persistent launch of min(n_launch, grid) workgroups over the entities ``order`` (largest first). The data and
// output arguments are pml_re_tron_csr's; ``l1`` > 0 selects OWL-QN; ``hist``: grid x 2 x m x dmax doubles;
// ``ticket`` (1 int) is zeroed here on the stream.
int pml_re_lbfgs_csr(const int* order, int n_launch, const long long* row_ptr, const long long* col_ptr,
                     const long long* nip, const uint16_t* lcol, const double* val, const double* y,
                     const double* off, const double* wt, double* scr, long long n_rows, double* W, double* f,
                     int* iters, int* reason, double* zout, int* npass, int loss, double l2, double tol,
                     int max_iter, int dmax, double l1, int m, int max_ls, double* hist, int* ticket, int grid,
                     hipStream_t st) {
  if (n_launch <= 0) return 0;
  if (dmax <= 0 || loss < 0 || loss > 3 || m < 1 || m > RE_LB_MMAX || max_ls < 1 || max_iter < 0 || grid <= 0 ||
      !(l1 >= 0.0) || hist == nullptr || ticket == nullptr)
    return -22;
  const size_t smem = pml_re_lbfgs_smem(dmax);
  if (smem > 160 * 1024) return -22;
  if (hipMemsetAsync(ticket, 0, sizeof(int), st) != hipSuccess) return -5;
  ReLbfgsArgs p{{order, n_launch, row_ptr, col_ptr, nip, lcol, val, y, off, wt, scr, n_rows, W, f, iters, reason,
                 zout, npass, loss, l2, tol, max_iter, 0, 0, dmax},
                l1, m, max_ls, hist, ticket};
  const dim3 g(n_launch < grid ? n_launch : grid), b(RE_THREADS);
  with_loss<4>(loss, [&](auto L) {
    if (l1 > 0.0) hipLaunchKernelGGL((re_lbfgs_csr_kernel<L(), true>), g, b, smem, st, p);
    else hipLaunchKernelGGL((re_lbfgs_csr_kernel<L(), false>), g, b, smem, st, p);
  });
  LAUNCH_CHECK();
  return 0;
}

// Lean streaming kernel (dmax <= 1024): LDS (1 + RE_NW) x dmax doubles; ``gsc`` scratch of one double per
// coefficient (packed like W); W is updated in place.
size_t pml_re_tron_lean_smem(int dmax) { return ((size_t)(1 + LEAN_NW) * dmax + 2 * LEAN_NW * 8) * sizeof(double); }

int pml_re_tron_lean(const int* order, int n_launch, const long long* row_ptr, const long long* col_ptr,
                     const long long* nip, const uint16_t* lcol, const double* val, const double* y,
                     const double* off, const double* wt, double* scr, long long n_rows, double* W, double* f,
                     int* iters, int* reason, double* zout, int* npass, int loss, double l2, double tol,
                     int max_iter, int max_fail, int max_cg, int dmax, double* gsc, int quad, const double* xf2,
                     hipStream_t st) {
  if (n_launch <= 0) return 0;
  if (dmax <= 0 || dmax > 1024 || loss < 0 || loss > 2 || gsc == nullptr) return -22;
  const size_t smem = pml_re_tron_lean_smem(dmax);
  ReTronArgs a{order, n_launch, row_ptr, col_ptr, nip, lcol, val, y, off, wt, scr, n_rows, W, f, iters, reason,
               zout, npass, loss, l2, tol, max_iter, max_fail, max_cg, dmax, gsc, xf2};
  // quad: every row padded to a multiple of 4 entries (row_pass_q), else the strided row_pass
  with_loss(loss, [&](auto L) {
    if (quad) lean_launch<L(), true>(a, n_launch, smem, st);
    else lean_launch<L(), false>(a, n_launch, smem, st);
  });
  LAUNCH_CHECK();
  return 0;
}

// Tall-narrow entities (d_e <= 64): one wave (= one workgroup) per entity; LDS per workgroup.
size_t pml_re_tron_hess_smem(int dp) {
  switch (dp / 16) {
    case 1: return (size_t)TronDenseCfg<1, TallRows<1>::FH>::WORDS * sizeof(double);
    case 2: return (size_t)TronDenseCfg<2, TallRows<2>::FH>::WORDS * sizeof(double);
    case 3: return (size_t)TronDenseCfg<3, TallRows<3>::FH>::WORDS * sizeof(double);
    default: return (size_t)TronDenseCfg<4, TallRows<4>::FH>::WORDS * sizeof(double);
  }
}

int pml_re_tron_hess(const int* order, int n_launch, const long long* row_ptr, const long long* col_ptr,
                     const long long* nip, const uint16_t* lcol, const double* val, const double* y,
                     const double* off, const double* wt, double* scr, long long n_rows, double* W, double* f,
                     int* iters, int* reason, double* zout, int* npass, int loss, double l2, double tol,
                     int max_iter, int max_fail, int max_cg, int dp, hipStream_t st) {
  if (n_launch <= 0) return 0;
  if (dp < 16 || dp > 64 || dp % 16 || loss < 0 || loss > 2) return -22;
  const size_t smem = pml_re_tron_hess_smem(dp);
  ReTronArgs a{order, n_launch, row_ptr, col_ptr, nip, lcol, val, y, off, wt, scr, n_rows, W, f, iters, reason,
               zout, npass, loss, l2, tol, max_iter, max_fail, max_cg, dp};
  with_loss(loss, [&](auto L) {
    switch (dp / 16) {
      case 1: hipLaunchKernelGGL((re_tron_tall_kernel<1, L()>), dim3(n_launch), dim3(64), smem, st, a); break;
      case 2: hipLaunchKernelGGL((re_tron_tall_kernel<2, L()>), dim3(n_launch), dim3(64), smem, st, a); break;
      case 3: hipLaunchKernelGGL((re_tron_tall_kernel<3, L()>), dim3(n_launch), dim3(64), smem, st, a); break;
      default: hipLaunchKernelGGL((re_tron_tall_kernel<4, L()>), dim3(n_launch), dim3(64), smem, st, a); break;
    }
  });
  LAUNCH_CHECK();
  return 0;
}

// Register-resident kernel: LDS per workgroup, rows per workgroup.
static size_t res_smem(int S) {
  const size_t cap = (size_t)RS_NW * 4 * S;
  return ((size_t)(6 + RS_NW) * (RS_DMAX + 8) + 7 * cap + 2 * RS_NW * 8 + 16) * sizeof(double);
}
int pml_re_res_cap() { return RS_NW * 4 * RES_S; }
int pml_re_res_dmax() { return RS_DMAX; }
size_t pml_re_res_ws_doubles(int n_tickets) { return (size_t)n_tickets * 2 * (RS_DMAX + 8); }

// Persistent launch over ``n_tasks`` tasks (task_ent / task_t0 as in ResTasks); ``ticket`` (1 int), ``bar``
// (n_tasks unsigned) and ``err`` (1 int) are zeroed here on the stream; ``ws``: pml_re_res_ws_doubles(n_tickets).
int pml_re_tron_res(const int* task_ent, const int* task_t0, int n_tasks, int* ticket, unsigned* bar, double* ws,
                    int* err, int grid, const long long* row_ptr, const long long* col_ptr, const long long* nip,
                    const uint16_t* lcol, const double* val, const double* y, const double* off, const double* wt,
                    double* W, double* f, int* iters, int* reason, double* zout, int* npass, int loss, double l2,
                    double tol, int max_iter, int max_fail, int max_cg, hipStream_t st) {
  if (n_tasks <= 0) return 0;
  if (loss < 0 || loss > 2 || grid <= 0) return -22;
  const size_t smem = res_smem(RES_S);
  if (smem > 160 * 1024) return -22;
  if (hipMemsetAsync(ticket, 0, sizeof(int), st) != hipSuccess) return -5;
  if (hipMemsetAsync(bar, 0, sizeof(unsigned) * n_tasks, st) != hipSuccess) return -5;
  if (hipMemsetAsync(err, 0, sizeof(int), st) != hipSuccess) return -5;
  ReTronArgs a{nullptr, 0, row_ptr, col_ptr, nip, lcol, val, y, off, wt, nullptr, 0, W, f, iters, reason,
               zout, npass, loss, l2, tol, max_iter, max_fail, max_cg, RS_DMAX};
  ResTasks tk{ticket, task_ent, task_t0, n_tasks, bar, ws, err};
  with_loss(loss, [&](auto L) {
    hipLaunchKernelGGL((re_tron_res_kernel<RES_S, L()>), dim3(grid), dim3(RS_THREADS), smem, st, a, tk);
  });
  LAUNCH_CHECK();
  return 0;
}

// Workgroups of the resident kernel that fit on the device at once (occupancy API x CUs; 0 on error).
int pml_re_res_grid() {
  int dev = 0, cus = 0, per = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, (const void*)re_tron_res_kernel<RES_S, 0>, RS_THREADS,
                                                   res_smem(RES_S)) != hipSuccess) return 0;
  return cus * per;
}


// Row-space TRON for 64 < n <= 192 (one wave per problem, packed L in LDS).
int pml_rs_tron_big(int B, int n, const double* L, const double* y, const double* off, const double* wt,
                    double* beta, double* f, int* iters, int* reason, double* zout, int loss, double l2, double tol,
                    int max_iter, int max_fail, int max_cg, hipStream_t st) {
  if (B <= 0) return 0;
  if (n < 1 || n > 192 || loss < 0 || loss > 2) return -22;
  const size_t smem = ((size_t)n * (n + 1) / 2 + n) * sizeof(double);
  if (smem > 160 * 1024) return -22;
  with_loss(loss, [&](auto LS) {
    auto go = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, dim3(B), dim3(64), smem, st, B, n, L, y, off, wt, beta, f, iters, reason, zout, l2,
                         tol, max_iter, max_fail, max_cg);
    };
    if (n <= 64) go(rs_tron_big_kernel<1, LS()>);
    else if (n <= 128) go(rs_tron_big_kernel<2, LS()>);
    else go(rs_tron_big_kernel<3, LS()>);
  });
  LAUNCH_CHECK();
  return 0;
}

}  // extern "C"

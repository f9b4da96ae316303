// Matrix-factorization coordinate (algorithm/matrix_factorization.py): fused per-entity TRON whose feature rows
// are GATHERED from the other side's factor table, and the u.v row scorer.
//
// With one side's factors fixed, the other side's update is a batch of independent K-coefficient GLMs (K <= 32),
// one per entity, over the entity's rows; the feature vector of row r is the K-vector Other[oid[r]] of the row's
// entity on the other side. mf_tron_kernel solves one entity per wave in one launch, after the model of
// re_tron_tall_kernel (re_kernels.hip): coefficient-space vectors in registers, the exact K x K Hessian in LDS
// (fp64 matrix cores), wave-level reductions in a fixed order, no atomics -- results are bitwise repeatable. The
// TRON control flow is optimization/tron.py decision for decision (tolerances from the state at zero, 20 CG
// steps, 5 failures by default). The small helpers (DPP sums, loss derivatives) are copies of those in
// re_kernels.hip, which this file does not touch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#ifndef PML_BUILD_ID
#define PML_BUILD_ID "unstamped-build!"
#endif
__attribute__((used)) static const char pml_build_stamp[] = "PML_BUILD_ID=" PML_BUILD_ID;

#define LAUNCH_CHECK()                                         \
  do {                                                         \
    hipError_t e_ = hipGetLastError();                         \
    if (e_ != hipSuccess) return (int)e_;                      \
  } while (0)

enum { LOSS_LOGISTIC = 0, LOSS_POISSON = 1, LOSS_SQUARED = 2 };

template <int LOSS>
__device__ __forceinline__ void loss_t(double z, double y, double& l, double& dl, double& d2) {
  if constexpr (LOSS == LOSS_LOGISTIC) {
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
  } else {
    const double d = z - y;
    l = 0.5 * d * d; dl = d; d2 = 1.0;
  }
}

// weight x per-row term with an exact 0 for zero-weight rows whatever the term (0 x inf must not become NaN)
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

// Sum over the 64 lanes of a wave, bitwise identical in every lane: DPP butterflies inside each 16-lane row, then
// the four row sums in a fixed order.
__device__ __forceinline__ double wave_total(double v) {
  v += dpp_f64<0xB1>(v);    // quad_perm [1,0,3,2]
  v += dpp_f64<0x4E>(v);    // quad_perm [2,3,0,1]
  v += dpp_f64<0x141>(v);   // row_half_mirror
  v += dpp_f64<0x140>(v);   // row_mirror
  return (readlane_f64(v, 0) + readlane_f64(v, 16)) + (readlane_f64(v, 32) + readlane_f64(v, 48));
}

// Sum over the 4 lanes of a quad, in every lane of the quad (fixed order).
__device__ __forceinline__ double quad_total(double v) {
  v += dpp_f64<0xB1>(v);
  v += dpp_f64<0x4E>(v);
  return v;
}

// LDS hand-off between the lanes of one wave: in-order LDS per wave + a compiler fence.
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

struct MfTronArgs {
  const int* order;          // launch slot -> entity
  int n_launch;
  const long long* row_ptr;  // [E + 1] entity row ranges (rows sorted by entity)
  const int* oid;            // [N] per sorted row: the other side's entity code (row of ``other``)
  const double* other;       // [J][K] the other side's factors
  const double* y;           // per sorted row: label / offset / weight
  const double* off;
  const double* wt;
  double* scr;               // per-row scratch [2][n_rows]: margins at the current / the trial point
  long long n_rows;
  double* W;                 // [E][K] this side's factors: in = warm start, out = solution
  double* f;                 // per entity: final objective, iterations, reason code
  int* iters;
  int* reason;
  double* zout;              // per sorted row: u . v of the solution (no offset)
  int* npass;                // optional, per entity: row passes run
  int K;
  double l2, tol;
  int max_iter, max_fail, max_cg;
};

typedef double v4d __attribute__((ext_vector_type(4)));
#define MF_RB 16             // rows per staged block

template <int T>
struct MfCfg {
  static constexpr int DP = 16 * T;                  // padded K
  static constexpr int XS = DP + 4;                  // staged row stride (quad-per-row margin reads: conflict-free)
  static constexpr int WORDS = 2 * DP * DP + MF_RB * XS + DP + 2 * MF_RB;   // LDS doubles per wave
};

// One wave per entity. Row pass: a block of 16 rows is staged as a dense [16][XS] LDS tile by gathering one
// contiguous K-double run Other[oid[r] * K ..] per row with the 16 lanes of a DPP row (lane gl loads columns gl
// and, for T = 2, gl + 16); columns K .. DP - 1 and rows past the entity's end are written as zeros, so the tile
// never holds stale data. The NEXT block's gathers and row scalars (and the ids two blocks ahead) are in flight
// while a block computes. The Hessian at a trial point is formed inside the trial point's function evaluation
// into the second LDS buffer (adopted when the step is accepted): one row pass per TRON iteration.
template <int T, int LOSS>
__global__ __launch_bounds__(64) void mf_tron_kernel(MfTronArgs a) {
  using C = MfCfg<T>;
  constexpr int DP = C::DP, XS = C::XS, NT = T * (T + 1) / 2;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int lane = threadIdx.x;
  const int e = a.order[blockIdx.x];
  double* const H0 = smem;                              // [DP][DP] Hessian buffers, exactly symmetric
  double* const H1 = smem + DP * DP;
  double* Xs = smem + 2 * DP * DP;                      // [MF_RB][XS] staged rows
  double* sV = Xs + MF_RB * XS;                         // [DP] vector broadcast to the lanes (margins / CG)
  double* sT = sV + DP;                                 // [MF_RB] per staged row: gradient weight t_r
  double* sD = sT + MF_RB;                              // [MF_RB] per staged row: Hessian weight D_r
  int hc = 0;                                           // (hc ? H1 : H0) = Hessian at the current point
  const long long r0 = a.row_ptr[e], r1 = a.row_ptr[e + 1];
  const int K = a.K;
  const bool own = lane < K;                            // lane j owns coefficient j
  double* Z[2] = {a.scr, a.scr + a.n_rows};
  int cur = 0, npass = 0;
  double* Wg = a.W + (long long)e * K;
  const int grp = lane >> 4, gl = lane & 15;
  const int* __restrict__ oid = a.oid + r0;
  const double* __restrict__ other = a.other;
  const int nrows = (int)(r1 - r0);

  struct Blk {
    double v[MF_RB / 4][T];
    double rs[3];
  };
  // ids of block b (lane q < MF_RB: the other side's code of row b + q; -1 past the entity's end)
  auto fetch_id = [&](int b) -> int {
    return (lane < MF_RB && b + lane < nrows) ? oid[b + lane] : -1;
  };
  // issue the loads of block b: the gathered factor runs and the per-row scalars wt / off / y
  auto issue = [&](Blk& B, int b, int ids) {
    B.rs[0] = B.rs[1] = B.rs[2] = 0.0;
    if (lane < MF_RB && b + lane < nrows) {
      const long long i = r0 + b + lane;
      B.rs[0] = a.wt[i]; B.rs[1] = a.off[i]; B.rs[2] = a.y[i];
    }
#pragma unroll
    for (int u = 0; u < MF_RB / 4; ++u) {
      const int id = __shfl(ids, u * 4 + grp, 64);
      const double* src = other + (long long)(id < 0 ? 0 : id) * K;
#pragma unroll
      for (int k = 0; k < T; ++k) {
        const int c = gl + 16 * k;
        B.v[u][k] = (id >= 0 && c < K) ? src[c] : 0.0;
      }
    }
  };
  auto stage = [&](const Blk& B) {
#pragma unroll
    for (int u = 0; u < MF_RB / 4; ++u)
#pragma unroll
      for (int k = 0; k < T; ++k) Xs[(u * 4 + grp) * XS + gl + 16 * k] = B.v[u][k];
  };
  // Pipelined pass over the entity's blocks: body(b, B) runs with block b staged in Xs (and its scalars in B.rs).
  auto pass = [&](auto&& body) {
    Blk A, B2;
    int ids = fetch_id(0);
    issue(A, 0, ids);
    ids = fetch_id(MF_RB);
    for (int b = 0; b < nrows; b += 2 * MF_RB) {
      const bool hasB = b + MF_RB < nrows;
      if (hasB) issue(B2, b + MF_RB, ids);
      ids = fetch_id(b + 2 * MF_RB);
      stage(A);
      wave_sync();
      body(b, A);
      wave_sync();
      if (!hasB) break;
      const bool hasA = b + 2 * MF_RB < nrows;
      if (hasA) issue(A, b + 2 * MF_RB, ids);
      ids = fetch_id(b + 3 * MF_RB);
      stage(B2);
      wave_sync();
      body(b + MF_RB, B2);
      wave_sync();
      if (!hasA) break;
    }
  };
  // MFMA accumulation of X_blk^T diag(w) X_blk for the staged block (w in LDS ``sw``)
  auto hess_block = [&](v4d (&cacc)[NT], const double* sw) {
    const int rr = lane & 15, kk = lane >> 4;
#pragma unroll 1
    for (int kg = 0; kg < MF_RB / 4; ++kg) {
      const int k = kg * 4 + kk;
      const double dk = sw[k];
      const double* xk = Xs + k * XS;
      int t = 0;
#pragma unroll
      for (int ti = 0; ti < T; ++ti)
#pragma unroll
        for (int tj = ti; tj < T; ++tj, ++t)
          cacc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(xk[ti * 16 + rr], dk * xk[tj * 16 + rr], cacc[t], 0, 0, 0);
    }
  };
  auto store_hess = [&](v4d (&cacc)[NT], double* H) {
    int t = 0;
#pragma unroll
    for (int ti = 0; ti < T; ++ti)
#pragma unroll
      for (int tj = ti; tj < T; ++tj, ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          // accumulator i of lane l holds C[(l >> 4) + 4 i][l & 15] of the tile
          const int lr = (lane >> 4) + 4 * i, lc = lane & 15;
          const int row = ti * 16 + lr, col = tj * 16 + lc;
          if (ti != tj || lr <= lc) {
            H[row * DP + col] = cacc[t][i];
            H[col * DP + row] = cacc[t][i];
          }
        }
    wave_sync();
    if (lane < DP) H[lane * DP + lane] += a.l2;
    wave_sync();
  };

  // value + gradient at the lane-held vector ``vj``. mode 1: writes the margins to Z buffer ``nb``; mode 2 (the
  // state at zero): no scratch writes. ``Hout`` != nullptr: the Hessian at vj is formed in the same pass.
  // Returns f; gj = this lane's gradient component (l2 included).
  auto value_grad = [&](double vj, int mode, int nb, double& gj, double* Hout) -> double {
    ++npass;
    if (lane < DP) sV[lane] = own ? vj : 0.0;
    const int r = lane >> 2, q = lane & 3;
    double fp = 0.0, g = 0.0;
    v4d cacc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) cacc[t] = v4d{0.0, 0.0, 0.0, 0.0};
    pass([&](int b, const Blk& B) {
      double s = 0.0;
#pragma unroll 4
      for (int cc = 0; cc < DP / 4; ++cc) s = fma(Xs[r * XS + q + 4 * cc], sV[q + 4 * cc], s);
      s = quad_total(s);
      const double wt = __shfl(B.rs[0], r, 64), of = __shfl(B.rs[1], r, 64), yy = __shfl(B.rs[2], r, 64);
      double t = 0.0, h = 0.0;
      if (b + r < nrows) {
        const long long i = r0 + b + r;
        double l, dl, d2;
        loss_t<LOSS>(s + of, yy, l, dl, d2);
        t = wx(wt, dl);
        h = wx(wt, d2);
        if (q == 0) {
          fp += wx(wt, l);
          if (mode == 1) Z[nb][i] = s;
        }
      }
      if (q == 0) { sT[r] = t; sD[r] = h; }
      wave_sync();
      if (lane < DP) {
#pragma unroll 4
        for (int rr = 0; rr < MF_RB; ++rr) g = fma(Xs[rr * XS + lane], sT[rr], g);
      }
      if (Hout != nullptr) hess_block(cacc, sD);
    });
    if (Hout != nullptr) store_hess(cacc, Hout);
    gj = own ? g + a.l2 * vj : 0.0;
    return wave_total(fp) + 0.5 * a.l2 * wave_total(own ? vj * vj : 0.0);
  };

  double Wj = own ? Wg[lane] : 0.0, Gj;
  double f = value_grad(Wj, 1, cur, Gj, H0);
  double gnorm2 = wave_total(Gj * Gj);
  const double nz = wave_total(own && Wj != 0.0 ? 1.0 : 0.0);
  double f0z = f, g0n = sqrt(gnorm2);
  if (nz != 0.0) {
    double g0j;
    f0z = value_grad(0.0, 2, 0, g0j, nullptr);
    g0n = sqrt(wave_total(g0j * g0j));
  }
  const double loss_tol = f0z * a.tol, grad_tol = g0n * a.tol;
  double delta = sqrt(gnorm2);
  int it = 0, fails = 0, reason = 0;
  bool active = true;
  if (delta == 0.0) { reason = 4; active = false; }
  const double eta0 = 1e-4, eta1 = 0.25, eta2 = 0.75, sg1 = 0.25, sg2 = 0.5, sg3 = 4.0;
  const int guard_max = a.max_iter * (a.max_fail + 1) + 5;
  for (int guard = 0; active && guard < guard_max; ++guard) {
    const double* H = (hc ? H1 : H0);
    // ---- truncated CG on the LDS Hessian: per step one column-read mat-vec and five wave sums
    double Sj = 0.0, Rj = -Gj, Dj = -Gj;
    double rtr = gnorm2, sts = 0.0;
    const double cg_tol2 = 0.01 * gnorm2;
    for (int k = 0; k < a.max_cg; ++k) {
      if (!(rtr > cg_tol2)) break;
      if (lane < DP) sV[lane] = Dj;
      wave_sync();
      double h0 = 0.0, h1 = 0.0;
      if (lane < DP) {
#pragma unroll 2
        for (int cc = 0; cc < DP; cc += 2) {
          h0 = fma(H[cc * DP + lane], sV[cc], h0);
          h1 = fma(H[(cc + 1) * DP + lane], sV[cc + 1], h1);
        }
      }
      wave_sync();
      const double hj = own ? h0 + h1 : 0.0;
      const double dhd = wave_total(Dj * hj), std_ = wave_total(Sj * Dj), dtd = wave_total(Dj * Dj);
      const double rh = wave_total(Rj * hj), hh = wave_total(hj * hj);
      const double alpha = rtr / (dhd == 0.0 ? 1.0 : dhd);
      double tn = sts + 2.0 * alpha * std_ + alpha * alpha * dtd;
      tn = tn > 0.0 ? tn : 0.0;
      const double dsq = delta * delta;
      const bool hit = tn > dsq;
      double al = alpha;
      if (hit) {
        const double qq = std_ * std_ + dtd * (dsq - sts);
        const double rad = sqrt(qq > 0.0 ? qq : 0.0);
        const double den1 = std_ + rad;
        al = std_ >= 0.0 ? (dsq - sts) / (den1 > 1e-300 ? den1 : 1e-300) : (rad - std_) / (dtd > 1e-300 ? dtd : 1e-300);
      }
      double rn = rtr - 2.0 * al * rh + al * al * hh;
      rn = rn > 0.0 ? rn : 0.0;
      const double beta = rn / (rtr == 0.0 ? 1.0 : rtr);
      Sj += al * Dj;
      Rj -= al * hj;
      if (hit) break;
      Dj = Rj + beta * Dj;
      rtr = rn;
      sts = tn;
    }
    // ---- trial point (its Hessian formed in the same pass), trust-region update, acceptance
    const double gs = wave_total(Gj * Sj), pred = -0.5 * (gs - wave_total(Sj * Rj)), snorm = sqrt(wave_total(Sj * Sj));
    const double Tj = own ? Wj + Sj : 0.0;
    double Gn;
    const double fn = value_grad(Tj, 1, cur ^ 1, Gn, hc ? H0 : H1);
    const double gn2 = wave_total(Gn * Gn);
    const double actual = f - fn;
    if (it == 0) delta = fmin(delta, snorm);
    const double den = fn - f - gs;
    const double alr = den <= 0.0 ? sg3 : fmax(sg1, -0.5 * gs / (den == 0.0 ? 1.0 : den));
    double nd;
    if (actual < eta0 * pred) nd = fmin(fmax(alr, sg1) * snorm, sg2 * delta);
    else if (actual < eta1 * pred) nd = fmax(sg1 * delta, fmin(alr * snorm, sg2 * delta));
    else if (actual < eta2 * pred) nd = fmax(sg1 * delta, fmin(alr * snorm, sg3 * delta));
    else nd = fmax(delta, fmin(alr * snorm, sg3 * delta));
    delta = nd;
    const bool accept = actual > eta0 * pred;
    const double f_prev = f;
    if (accept) {
      Wj = Tj;
      Gj = Gn;
      gnorm2 = gn2;
      f = fn;
      cur ^= 1;
      ++it;
      fails = 0;
      hc ^= 1;
    } else {
      ++fails;
    }
    const bool not_impr = !accept && fails >= a.max_fail;
    int rc = 0;
    if (accept && sqrt(gnorm2) <= grad_tol) rc = 4;
    if (accept && fabs(f - f_prev) <= loss_tol) rc = 3;
    if (not_impr) rc = 2;
    if ((accept || not_impr) && it >= a.max_iter) rc = 1;
    if (rc > 0) { reason = rc; active = false; }
  }
  if (own) Wg[lane] = Wj;
  if (a.zout != nullptr) {
    const double* zc = Z[cur];
    for (long long i = r0 + lane; i < r1; i += 64) a.zout[i] = zc[i];
  }
  if (lane == 0) {
    a.f[e] = f; a.iters[e] = it; a.reason[e] = reason;
    if (a.npass != nullptr) a.npass[e] = npass;
  }
}

// s_r = U[a_r] . V[b_r] per row, 0 where either code is -1. One thread per row; the K products are summed in
// index order with the rounding error of every product and addition carried along (two-sum), so the result is
// the correctly rounded dot product up to one final rounding whatever the cancellation between the terms.
__global__ __launch_bounds__(256) void mf_score_kernel(long long n, int K, const int* __restrict__ ra,
                                                       const int* __restrict__ cb, const double* __restrict__ U,
                                                       const double* __restrict__ V, double* __restrict__ out) {
  // the error terms below are exact only if every product and sum is rounded on its own (no fused contraction)
#pragma clang fp contract(off)
  const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  const int ia = ra[r], ib = cb[r];
  if (ia < 0 || ib < 0) { out[r] = 0.0; return; }
  const double* u = U + (long long)ia * K;
  const double* v = V + (long long)ib * K;
  double s = 0.0, c = 0.0;
  for (int k = 0; k < K; ++k) {
    const double x = u[k], y = v[k];
    const double p = x * y;
    const double pe = fma(x, y, -p);
    const double t = s + p;
    const double bb = t - s;
    c += ((s - (t - bb)) + (p - bb)) + pe;
    s = t;
  }
  out[r] = s + c;
}

extern "C" {

const char* pml_build_id() { return pml_build_stamp + 13; }

// LDS of one wave (= one workgroup) for the padded factor count ``dp`` (16 or 32).
size_t pml_mf_tron_smem(int dp) {
  return (size_t)(dp <= 16 ? MfCfg<1>::WORDS : MfCfg<2>::WORDS) * sizeof(double);
}

int pml_mf_tron(const int* order, int n_launch, const long long* row_ptr, const int* oid, const double* other,
                const double* y, const double* off, const double* wt, double* scr, long long n_rows, double* W,
                double* f, int* iters, int* reason, double* zout, int* npass, int K, int loss, double l2, double tol,
                int max_iter, int max_fail, int max_cg, hipStream_t st) {
  if (n_launch <= 0) return 0;
  if (K < 1 || K > 32 || loss < 0 || loss > 2) return -22;
  const int T = K <= 16 ? 1 : 2;
  const size_t smem = pml_mf_tron_smem(16 * T);
  MfTronArgs a{order, n_launch, row_ptr, oid, other, y, off, wt, scr, n_rows, W, f, iters, reason, zout, npass,
               K, l2, tol, max_iter, max_fail, max_cg};
#define MF_LAUNCH_L(T, L) hipLaunchKernelGGL((mf_tron_kernel<T, L>), dim3(n_launch), dim3(64), smem, st, a)
#define MF_LAUNCH(T)                                  \
  do {                                                \
    if (loss == LOSS_LOGISTIC) MF_LAUNCH_L(T, 0);     \
    else if (loss == LOSS_POISSON) MF_LAUNCH_L(T, 1); \
    else MF_LAUNCH_L(T, 2);                           \
  } while (0)
  if (T == 1) MF_LAUNCH(1);
  else MF_LAUNCH(2);
#undef MF_LAUNCH
#undef MF_LAUNCH_L
  LAUNCH_CHECK();
  return 0;
}

int pml_mf_score(long long n, int K, const int* ra, const int* cb, const double* U, const double* V, double* out,
                 hipStream_t st) {
  if (n <= 0) return 0;
  if (K < 1) return -22;
  const long long blocks = (n + 255) / 256;
  if (blocks > 0x7fffffffLL) return -22;
  hipLaunchKernelGGL(mf_score_kernel, dim3((unsigned)blocks), dim3(256), 0, st, n, K, ra, cb, U, V, out);
  LAUNCH_CHECK();
  return 0;
}

}  // extern "C"

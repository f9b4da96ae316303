// The TRON that every fused per-entity solver of re_kernels.hip and mf_kernels.hip runs, defined once:
// * the scalar decisions (truncated-CG step, trust-region radius, acceptance, stop reason) as functions of sums
//   the calling kernel has already reduced -- workgroup sums, wave sums or LDS state, that is the caller's business;
// * tron_dense_wave, the whole wave-per-entity solve over dense 16-row blocks with the exact Hessian in LDS, which
//   re_tron_tall_kernel (CSR rows scattered into the block) and mf_tron_kernel (rows gathered from the other side's
//   factor table) instantiate with a row-source policy each.
// Semantics follow batched_tron / rs_tron_kernel (photon-lib/.../optimization/TRON.scala:80-340): eta = (1e-4, .25,
// .75), sigma = (.25, .5, 4), first-iteration delta = min(delta, ||step||); reason codes 1 max-iter, 2
// not-improving, 3 f-converged, 4 g-converged. A change to these rules is made here and nowhere else.
#pragma once
#include "pml_device.h"

struct TronCgStep {
  double al;     // step length along the direction (to the trust-region boundary when ``hit``)
  double tn;     // ||step + al_unclipped d||^2 by the recurrence, clamped at 0
  double rn;     // ||r - al H d||^2 by the recurrence, clamped at 0
  double beta;   // rn / rtr
  bool hit;      // the step leaves the trust region: CG ends after this update
};

// One truncated-CG step from the five sums d.Hd, step.d, d.d, r.Hd, Hd.Hd (and r.r, step.step carried along).
__device__ __forceinline__ TronCgStep tron_cg_step(double rtr, double sts, double delta, double dhd, double std_,
                                                   double dtd, double rh, double hh) {
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
  return {al, tn, rn, beta, hit};
}

constexpr double TRON_ETA0 = 1e-4;

// The step from f to fn is taken when the actual reduction exceeds eta0 x the predicted one.
__device__ __forceinline__ bool tron_accept(double f, double fn, double pred) { return f - fn > TRON_ETA0 * pred; }

// New trust-region radius after the trial point's evaluation (``first``: no step accepted yet).
__device__ __forceinline__ double tron_radius(double delta, double snorm, double gs, double f, double fn, double pred,
                                              bool first) {
  const double eta0 = TRON_ETA0, eta1 = 0.25, eta2 = 0.75, sg1 = 0.25, sg2 = 0.5, sg3 = 4.0;
  const double actual = f - fn;
  if (first) delta = fmin(delta, snorm);
  const double den = fn - f - gs;
  const double alr = den <= 0.0 ? sg3 : fmax(sg1, -0.5 * gs / (den == 0.0 ? 1.0 : den));
  double nd;
  if (actual < eta0 * pred) nd = fmin(fmax(alr, sg1) * snorm, sg2 * delta);
  else if (actual < eta1 * pred) nd = fmax(sg1 * delta, fmin(alr * snorm, sg2 * delta));
  else if (actual < eta2 * pred) nd = fmax(sg1 * delta, fmin(alr * snorm, sg3 * delta));
  else nd = fmax(delta, fmin(alr * snorm, sg3 * delta));
  return nd;
}

// Stop reason after the accept / reject bookkeeping (f, gnorm2, it: the state after it); 0 = go on.
__device__ __forceinline__ int tron_reason(bool accept, bool not_impr, double gnorm2, double grad_tol, double f,
                                           double f_prev, double loss_tol, int it, int max_iter) {
  int rc = 0;
  if (accept && sqrt(gnorm2) <= grad_tol) rc = 4;
  if (accept && fabs(f - f_prev) <= loss_tol) rc = 3;
  if (not_impr) rc = 2;
  if ((accept || not_impr) && it >= max_iter) rc = 1;
  return rc;
}

// ============================================================================================================
// ONE WAVE PER ENTITY over dense row blocks, the whole TRON with the EXACT per-entity Hessian H_e = X_e^T D X_e +
// l2 I (at most 64 coefficients). No workgroup barriers: every reduction is a DPP / readlane wave sum, LDS hand-offs
// between the lanes of the wave are ordered by wave_sync; no atomics, so results are bitwise repeatable.
// * Coefficient-space vectors live in registers: lane j holds w_j, g_j, step_j, r_j, dir_j.
// * Row passes stage TRON_RB = 16 rows at a time as a dense [16][DP + 4] LDS block (row stride DP + 4: the
//   quad-per-row margin reads are bank-conflict free). The NEXT block's loads (and its look-ahead metadata two
//   blocks ahead) are in flight while a block computes, so a pass costs about one global-memory latency.
// * Margins: a lane quad per row; gradient: lane j sums X[r][j] t_r over the 16 rows in a fixed order.
// * Hessian: per 4 staged rows one v_mfma_f64_16x16x4f64 per upper-triangle 16 x 16 tile (fixed k order), written
//   to LDS EXACTLY symmetric (diagonal tiles mirrored from their upper half), so a CG step reads column j of H
//   (consecutive lanes: conflict-free) for (H d)_j. With FH the Hessian at the trial point is formed INSIDE the
//   trial point's function evaluation into a second LDS buffer (adopted when the step is accepted): one row pass
//   per TRON iteration. Without it a separate pass forms it from the Hessian weights D kept per row.
//
// The row source ``Src`` says where the rows come from:
//   Src::FH                             Hessian fused into the function evaluation (two H buffers)
//   Src::Blk                            registers of one block in flight; Blk::rs[3] = per-row scalars of lane < 16
//   r0, nrows, nc, Wg                   the entity's first row, row count, coefficient count, coefficients
//   Z0, Z1 (and D0, D1 unless FH)       per-row scratch: margins (Hessian weights), one buffer each for the current
//                                       and the trial point (no arrays: the object must stay in registers)
//   fetch(b)                            look-ahead metadata of block b (row pointers / gather ids)
//   issue(B, b, meta, mode, cur)        start block b's loads: mode 0 rs[0] = D[cur], else rs = wt / off / y
//   stage(B, Xs) / unstage(B, Xs)       write the block into Xs; restore what Xs must hold between blocks
// ``a`` supplies l2, tol, max_iter, max_fail, max_cg and the per-entity outputs f, iters, reason, zout, npass.
// ============================================================================================================
typedef double v4d __attribute__((ext_vector_type(4)));
#define TRON_RB 16             // rows per staged block

template <int T, bool FH_>
struct TronDenseCfg {
  static constexpr int DP = 16 * T;                  // padded coefficient count
  static constexpr int XS = DP + 4;                  // staged row stride (doubles)
  static constexpr bool FH = FH_;
  static constexpr int XOFF = (FH ? 2 : 1) * DP * DP;                        // Hessian buffers come first
  static constexpr int WORDS = XOFF + TRON_RB * XS + DP + 2 * TRON_RB;       // LDS doubles per wave
};

template <int T, int LOSS, class Src, class Args>
__device__ __forceinline__ void tron_dense_wave(const Args& a, int e, const Src& src, double* smem) {
  using C = TronDenseCfg<T, Src::FH>;
  using Blk = typename Src::Blk;
  constexpr int DP = C::DP, XS = C::XS, NT = T * (T + 1) / 2;
  constexpr bool FH = C::FH;
  const int lane = threadIdx.x;
  double* const H0 = smem;                              // [DP][DP] Hessian buffers, exactly symmetric
  double* const H1 = smem + (FH ? DP * DP : 0);
  double* Xs = smem + C::XOFF;                          // [TRON_RB][XS] staged rows
  double* sV = Xs + TRON_RB * XS;                       // [DP] vector broadcast to the lanes (margins / CG)
  double* sT = sV + DP;                                 // [TRON_RB] per staged row: gradient weight t_r
  double* sD = sT + TRON_RB;                            // [TRON_RB] per staged row: Hessian weight D_r
  int hc = 0;                                           // (hc ? H1 : H0) = Hessian at the current point
  const long long r0 = src.r0;
  const int nrows = src.nrows;
  const bool own = lane < src.nc;                       // lane j owns coefficient j
  int cur = 0, npass = 0;

  // Pipelined pass over the entity's blocks: body(b, B) runs with block b staged in Xs (and its loads in B.rs).
  auto pass = [&](int mode, auto&& body) {
    Blk A, B2;
    auto np = src.fetch(0);
    src.issue(A, 0, np, mode, cur);
    np = src.fetch(TRON_RB);
    for (int b = 0; b < nrows; b += 2 * TRON_RB) {
      const bool hasB = b + TRON_RB < nrows;
      if (hasB) src.issue(B2, b + TRON_RB, np, mode, cur);
      np = src.fetch(b + 2 * TRON_RB);
      src.stage(A, Xs);
      wave_sync();
      body(b, A);
      wave_sync();
      src.unstage(A, Xs);
      if (!hasB) break;
      const bool hasA = b + 2 * TRON_RB < nrows;
      if (hasA) src.issue(A, b + 2 * TRON_RB, np, mode, cur);
      np = src.fetch(b + 3 * TRON_RB);
      src.stage(B2, Xs);
      wave_sync();
      body(b + TRON_RB, B2);
      wave_sync();
      src.unstage(B2, Xs);
      if (!hasA) break;
    }
  };
  // MFMA accumulation of X_blk^T diag(w) X_blk for the staged block (w in LDS ``sw``)
  auto hess_block = [&](v4d (&cacc)[NT], const double* sw) {
    const int rr = lane & 15, kk = lane >> 4;
#pragma unroll 1
    for (int kg = 0; kg < TRON_RB / 4; ++kg) {
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

  // value + gradient at the lane-held vector ``vj`` (written to sV here). mode 1: writes Z buffer ``nb`` (and D
  // when the Hessian has its own pass); mode 2 (the state at zero): no scratch writes. ``Hout`` (FH only): the
  // Hessian at vj is formed in the same pass. Returns f; gj = this lane's gradient component (l2 included).
  auto value_grad = [&](double vj, int mode, int nb, double& gj, double* Hout) -> double {
    ++npass;
    if (lane < DP) sV[lane] = own ? vj : 0.0;
    const int r = lane >> 2, q = lane & 3;
    double fp = 0.0, g = 0.0;
    v4d cacc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) cacc[t] = v4d{0.0, 0.0, 0.0, 0.0};
    pass(1, [&](int b, const Blk& B) {
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
          if (mode == 1) {
            (nb ? src.Z1 : src.Z0)[i] = s;
            if constexpr (!FH) (nb ? src.D1 : src.D0)[i] = h;
          }
        }
      }
      if (q == 0) { sT[r] = t; sD[r] = h; }
      wave_sync();
      if (lane < DP) {
#pragma unroll 4
        for (int rr = 0; rr < TRON_RB; ++rr) g = fma(Xs[rr * XS + lane], sT[rr], g);
      }
      if (FH && Hout != nullptr) hess_block(cacc, sD);
    });
    if (FH && Hout != nullptr) store_hess(cacc, Hout);
    gj = own ? g + a.l2 * vj : 0.0;
    return wave_total(fp) + 0.5 * a.l2 * wave_total(own ? vj * vj : 0.0);
  };
  // separate Hessian pass at the current point (not FH): H = X^T diag(D[cur]) X + l2 I
  auto form_hessian = [&]() {
    ++npass;
    v4d cacc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) cacc[t] = v4d{0.0, 0.0, 0.0, 0.0};
    pass(0, [&](int b, const Blk& B) {
      if (lane < TRON_RB) sD[lane] = B.rs[0];
      wave_sync();
      hess_block(cacc, sD);
    });
    store_hess(cacc, (hc ? H1 : H0));
  };

  double Wj = own ? src.Wg[lane] : 0.0, Gj;
  double f = value_grad(Wj, 1, cur, Gj, FH ? (hc ? H1 : H0) : nullptr);
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
  bool active = true, need_h = !FH;
  if (delta == 0.0) { reason = 4; active = false; }
  const int guard_max = a.max_iter * (a.max_fail + 1) + 5;
  for (int guard = 0; active && guard < guard_max; ++guard) {
    if (need_h) { form_hessian(); need_h = false; }
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
      const TronCgStep c = tron_cg_step(rtr, sts, delta, dhd, std_, dtd, rh, hh);
      Sj += c.al * Dj;
      Rj -= c.al * hj;
      if (c.hit) break;
      Dj = Rj + c.beta * Dj;
      rtr = c.rn;
      sts = c.tn;
    }
    // ---- trial point (its Hessian formed in the same pass when FH), trust-region update, acceptance
    const double gs = wave_total(Gj * Sj), pred = -0.5 * (gs - wave_total(Sj * Rj)), snorm = sqrt(wave_total(Sj * Sj));
    const double Tj = own ? Wj + Sj : 0.0;
    double Gn;
    const double fn = value_grad(Tj, 1, cur ^ 1, Gn, FH ? (hc ? H0 : H1) : nullptr);
    const double gn2 = wave_total(Gn * Gn);
    delta = tron_radius(delta, snorm, gs, f, fn, pred, it == 0);
    const bool accept = tron_accept(f, fn, pred);
    const double f_prev = f;
    if (accept) {
      Wj = Tj;
      Gj = Gn;
      gnorm2 = gn2;
      f = fn;
      cur ^= 1;
      ++it;
      fails = 0;
      if (FH) hc ^= 1;
      else need_h = true;
    } else {
      ++fails;
    }
    const bool not_impr = !accept && fails >= a.max_fail;
    const int rc = tron_reason(accept, not_impr, gnorm2, grad_tol, f, f_prev, loss_tol, it, a.max_iter);
    if (rc > 0) { reason = rc; active = false; }
  }
  if (own) src.Wg[lane] = Wj;
  if (a.zout != nullptr) {
    const double* zc = cur ? src.Z1 : src.Z0;
    for (long long i = r0 + lane; i < r0 + nrows; i += 64) a.zout[i] = zc[i];
  }
  if (lane == 0) {
    a.f[e] = f; a.iters[e] = it; a.reason[e] = reason;
    if (a.npass != nullptr) a.npass[e] = npass;
  }
}

// Matrix-factorization coordinate (algorithm/matrix_factorization.py): fused per-entity TRON whose feature rows
// are GATHERED from the other side's factor table, and the u.v row scorer.
//
// With one side's factors fixed, the other side's update is a batch of independent K-coefficient GLMs (K <= 32),
// one per entity, over the entity's rows; the feature vector of row r is the K-vector Other[oid[r]] of the row's
// entity on the other side. mf_tron_kernel solves one entity per wave in one launch. The solve itself is
// tron_dense_wave (tron_core.h), the same code re_tron_tall_kernel runs: coefficient-space vectors in registers,
// the exact K x K Hessian in LDS (fp64 matrix cores), wave-level reductions in a fixed order, no atomics -- results
// are bitwise repeatable; the TRON control flow is optimization/tron.py decision for decision (tolerances from the
// state at zero, 20 CG steps, 5 failures by default). This file supplies only the row source (MfRows: the gather)
// and the scorer; the losses and the DPP sums come from pml_device.h.
#include "tron_core.h"

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

// Row source of tron_dense_wave: a block of 16 rows is staged as a dense [16][XS] LDS tile by gathering one
// contiguous K-double run Other[oid[r] * K ..] per row with the 16 lanes of a DPP row (lane gl loads columns gl
// and, for T = 2, gl + 16); columns K .. DP - 1 and rows past the entity's end are written as zeros, so the tile
// never holds stale data and nothing is restored after use. The Hessian at a trial point is always formed inside
// the trial point's function evaluation (FH): one row pass per TRON iteration, no per-row Hessian weights.
template <int T>
struct MfRows {
  static constexpr bool FH = true;
  static constexpr int XS = TronDenseCfg<T, FH>::XS;
  struct Blk {
    double v[TRON_RB / 4][T];
    double rs[3];
  };
  const MfTronArgs& a;
  const int lane = threadIdx.x, grp = lane >> 4, gl = lane & 15;
  const long long r0;
  const int nrows, nc;
  double* const Wg;
  double* const Z0;
  double* const Z1;
  const int* const oid;

  __device__ __forceinline__ MfRows(const MfTronArgs& a_, int e)
      : a(a_), r0(a_.row_ptr[e]), nrows((int)(a_.row_ptr[e + 1] - r0)), nc(a_.K), Wg(a_.W + (long long)e * a_.K),
        Z0(a_.scr), Z1(a_.scr + a_.n_rows), oid(a_.oid + r0) {}

  // ids of block b (lane q < TRON_RB: the other side's code of row b + q; -1 past the entity's end)
  __device__ __forceinline__ int fetch(int b) const {
    return (lane < TRON_RB && b + lane < nrows) ? oid[b + lane] : -1;
  }
  // issue the loads of block b: the gathered factor runs and the per-row scalars wt / off / y
  __device__ __forceinline__ void issue(Blk& B, int b, int ids, int, int) const {
    B.rs[0] = B.rs[1] = B.rs[2] = 0.0;
    if (lane < TRON_RB && b + lane < nrows) {
      const long long i = r0 + b + lane;
      B.rs[0] = a.wt[i]; B.rs[1] = a.off[i]; B.rs[2] = a.y[i];
    }
#pragma unroll
    for (int u = 0; u < TRON_RB / 4; ++u) {
      const int id = __shfl(ids, u * 4 + grp, 64);
      const double* src = a.other + (long long)(id < 0 ? 0 : id) * nc;
#pragma unroll
      for (int k = 0; k < T; ++k) {
        const int c = gl + 16 * k;
        B.v[u][k] = (id >= 0 && c < nc) ? src[c] : 0.0;
      }
    }
  }
  __device__ __forceinline__ void stage(const Blk& B, double* Xs) const {
#pragma unroll
    for (int u = 0; u < TRON_RB / 4; ++u)
#pragma unroll
      for (int k = 0; k < T; ++k) Xs[(u * 4 + grp) * XS + gl + 16 * k] = B.v[u][k];
  }
  __device__ __forceinline__ void unstage(const Blk&, double*) const {}
};

template <int T, int LOSS>
__global__ __launch_bounds__(64) void mf_tron_kernel(MfTronArgs a) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int e = a.order[blockIdx.x];
  tron_dense_wave<T, LOSS>(a, e, MfRows<T>(a, e), smem);
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
  return (size_t)(dp <= 16 ? TronDenseCfg<1, true>::WORDS : TronDenseCfg<2, true>::WORDS) * sizeof(double);
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
  with_loss(loss, [&](auto L) {
    if (T == 1) hipLaunchKernelGGL((mf_tron_kernel<1, L()>), dim3(n_launch), dim3(64), smem, st, a);
    else hipLaunchKernelGGL((mf_tron_kernel<2, L()>), dim3(n_launch), dim3(64), smem, st, a);
  });
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

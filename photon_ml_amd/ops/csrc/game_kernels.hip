// photon_ml_amd — CDNA4 (gfx950 / MI355X) kernels for GAME scoring and the dense random-effect paths
// (row-space Gram of K7).
//
// * score_rows_kernel  — K5 fixed-effect scoring s_i = x_i . w and K6 random-effect scoring s_i = x_i . w_{e(i)}
//   over a CSR shard. 16 lanes per row (4 rows per wave64): lane-strided fp64 partial sums combined by a fixed
//   shuffle tree, so scores are bitwise reproducible. Random-effect models are entity-major CSR (eptr / sorted
//   feature ids / values, models/game.py): each lane binary-searches its feature in the row's entity segment.
//   Reference: photon-api/.../model/FixedEffectModel.scala:132-144, RandomEffectModel.scala:256-297.
// * MFMA kernels (dense GEMM-shaped work on the matrix cores, fp64 v_mfma_f64_16x16x4f64):
//   - gemm_nt_mfma_kernel — C = A B^T: back-projection of projected coefficients W P (and variances) of the
//     random projection (projector/ProjectionMatrix.scala:95-124);
// * spmm_rows_kernel — K15 forward random projection X P^T of sparse rows (ProjectionMatrix.scala:48-63).
// * downsample_kernel — K20 fixed-effect down-sampling as an on-device weight rewrite.
// * seg_rank_wave_kernel / seg_rank_block_kernel — K12 per-group AUC, AUPR and precision@k (AUC:tag, AUPR:tag,
//   PRECISION@k:tag): every group sorted in registers / LDS and evaluated in one pass, one launch per size class.
// * auc_count_kernel / auc_count_combine_kernel -- integer tie-group counts of the global AUC over one sorted score
//   stream (plain AUC under a process group: every rank counts the score bucket it received).
// * var_normal_kernel / var_scale_gram_kernel / chol_colnorm_kernel -- FULL coefficient variances diag(H_e^-1) of the
//   random-effect entities: per-entity normal matrix, then squared column norms of G^-1 R from its Cholesky factor.
// * var_blk_normal_kernel / var_blk_gram_kernel / blocked_chol_kernel / blocked_trinv_kernel /
//   var_blk_colnorm_kernel -- the same for factor orders 129 .. 1024: matrices in a global workspace, one work-group
//   per entity, Cholesky and triangular inverse blocked in 16-column panels on the fp64 matrix cores.
//
// Built with: hipcc --offload-arch=gfx950 -O3 -shared -fPIC (photon_ml_amd/ops/build.py). C ABI, ctypes.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

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

// ------------------------------------------------------------------------------------------------------------
// K5 / K6 scoring
// ------------------------------------------------------------------------------------------------------------
#define SCORE_GROUP 16                       // lanes per row
#define SCORE_THREADS 256
#define SCORE_ROWS_PER_BLOCK (SCORE_THREADS / SCORE_GROUP)

template <bool RE>
__global__ __launch_bounds__(SCORE_THREADS) void score_rows_kernel(
    const long long* __restrict__ indptr, const int* __restrict__ col, const double* __restrict__ val,
    long long n_rows, const double* __restrict__ w, const int* __restrict__ ent,
    const long long* __restrict__ eptr, const int* __restrict__ efeat, double* __restrict__ out) {
  const long long row = (long long)blockIdx.x * SCORE_ROWS_PER_BLOCK + (threadIdx.x / SCORE_GROUP);
  const int g = threadIdx.x % SCORE_GROUP;
  double s = 0.0;
  if (row < n_rows) {
    const long long lo = indptr[row], hi = indptr[row + 1];
    long long e_lo = 0, e_hi = 0;
    bool ok = true;
    if (RE) {
      const int e = ent[row];
      if (e < 0) ok = false;
      else { e_lo = eptr[e]; e_hi = eptr[e + 1]; }
    }
    if (ok) {
      for (long long p = lo + g; p < hi; p += SCORE_GROUP) {
        const int c = col[p];
        double wv;
        if (RE) {
          long long a = e_lo, b = e_hi;         // lower bound of c in the entity's sorted feature ids
          while (a < b) {
            const long long m = (a + b) >> 1;
            if (efeat[m] < c) a = m + 1; else b = m;
          }
          wv = (a < e_hi && efeat[a] == c) ? w[a] : 0.0;
        } else {
          wv = w[c];
        }
        s += val[p] * wv;
      }
    }
  }
#pragma unroll
  for (int o = SCORE_GROUP / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, SCORE_GROUP);
  if (g == 0 && row < n_rows) out[row] = s;
}

// ------------------------------------------------------------------------------------------------------------
// MFMA: fp64 16x16x4 tiles. One wave computes a 16x16 fp64 output tile. v_mfma_f64_16x16x4_f64 fragments on
// gfx950: lane l holds A[row = l & 15][k = l >> 4] and B[k = l >> 4][col = l & 15]; accumulator i (of 4) of lane l
// holds C[row = (l >> 4) + 4 i][col = l & 15] (the f64 C/D map differs from the f32 / bf16 ones).
// ------------------------------------------------------------------------------------------------------------
typedef double v4d __attribute__((ext_vector_type(4)));

__device__ __forceinline__ v4d mfma_f64_16x16x4(double a, double b, v4d c) {
  return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}


// C[M x N] = A[M x K] * B[N x K]^T (all row-major fp64, leading dimensions lda / ldb / ldc). Work-group = 4 waves
// = a 32 x 32 output tile (2 x 2 wave tiles of 16 x 16); K staged through LDS in slices of 32. Grid over output
// tiles; blockIdx.x runs over N tiles fastest so neighbouring work-groups share the A panel in L2.
#define GN_T 32
#define GN_K 32
__global__ __launch_bounds__(256) void gemm_nt_mfma_kernel(int M, int N, int K, const double* __restrict__ A, int lda,
                                                            const double* __restrict__ Bm, int ldb,
                                                            double* __restrict__ C, int ldc) {
  __shared__ double sa[GN_T][GN_K + 1];
  __shared__ double sb[GN_T][GN_K + 1];
  const int tn = blockIdx.x, tm = blockIdx.y;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int wm = wv >> 1, wn = wv & 1;
  v4d acc = {0.0, 0.0, 0.0, 0.0};
  for (int k0 = 0; k0 < K; k0 += GN_K) {
    __syncthreads();
    for (int idx = threadIdx.x; idx < GN_T * GN_K; idx += 256) {
      const int r = idx / GN_K, c = idx % GN_K;
      const int gr = tm * GN_T + r, gc = k0 + c;
      sa[r][c] = (gr < M && gc < K) ? A[(long long)gr * lda + gc] : 0.0;
      const int hr = tn * GN_T + r;
      sb[r][c] = (hr < N && gc < K) ? Bm[(long long)hr * ldb + gc] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < GN_K; kk += 4) {
      const double a = sa[16 * wm + (lane & 15)][kk + (lane >> 4)];
      const double b = sb[16 * wn + (lane & 15)][kk + (lane >> 4)];
      acc = mfma_f64_16x16x4(a, b, acc);
    }
  }
  const int cj = tn * GN_T + 16 * wn + (lane & 15);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int ri = tm * GN_T + 16 * wm + (lane >> 4) + 4 * i;
    if (ri < M && cj < N) C[(long long)ri * ldc + cj] = acc[i];
  }
}

// K15 forward projection: Y[row][j] = sum_p val[p] * PT[col[p]][j] for a CSR X (rows) and a dense row-major
// PT [D x k] (the transposed projection matrix): one wave per row, lanes over the k outputs (strided by 64),
// non-zeros in CSR order -> deterministic. Each non-zero reads one contiguous k-row of PT (coalesced).
__global__ __launch_bounds__(256) void spmm_rows_kernel(const long long* __restrict__ indptr,
                                                         const int* __restrict__ col, const double* __restrict__ val,
                                                         long long n_rows, const double* __restrict__ PT, int k,
                                                         double* __restrict__ Y) {
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= n_rows) return;
  const long long lo = indptr[row], hi = indptr[row + 1];
  for (int j0 = 0; j0 < k; j0 += 64) {
    const int j = j0 + lane;
    double acc = 0.0;
    for (long long p = lo; p < hi; ++p) {
      const double v = val[p];
      const long long c = col[p];
      if (j < k) acc += v * PT[c * k + j];
    }
    if (j < k) Y[row * k + j] = acc;
  }
}

// K20 down-sampling (BinaryClassificationDownSampler.scala:47-68, DefaultDownSampler.scala:27-41) as a weight
// rewrite on the device: row r is kept with probability `rate` (binary tasks: every positive is kept and kept
// negatives get weight / rate), dropped rows get weight 0 — the HBM streams never change. The uniform of row r is a
// counter-based hash of (seed, global row id) (splitmix64 finaliser, top 53 bits), reproduced bit for bit by the
// host sampler (sampling/samplers.py), so CPU and GPU runs and every rank of a data-parallel job draw the same
// sample for the same row.
__device__ __forceinline__ unsigned long long splitmix64(unsigned long long x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

template <typename T>
__global__ __launch_bounds__(256) void downsample_kernel(const T* __restrict__ y, const T* __restrict__ w0,
                                                          const long long* __restrict__ rowid, long long n,
                                                          unsigned long long seed, double rate, int binary,
                                                          T* __restrict__ w) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const unsigned long long id = rowid ? (unsigned long long)rowid[i] : (unsigned long long)i;
  const double u = (double)(splitmix64(seed ^ splitmix64(id)) >> 11) * 0x1.0p-53;
  const double wi = (double)w0[i];
  double out;
  if (binary) {
    const bool pos = (double)y[i] >= 0.5;
    out = pos ? wi : (u < rate ? wi / rate : 0.0);
  } else {
    out = u < rate ? wi : 0.0;
  }
  w[i] = (T)out;
}

// ------------------------------------------------------------------------------------------------------------
// K20 work saving: row-sampled copy of one chunk of the tiled layout (ops/tiled.py, DeviceGLMData.row_sampled).
// A down-sampled row (weight 0) adds nothing to any pass, so a fixed-effect update at rate r only needs the kept
// rows' entries (the reference trains on a physically smaller sampled RDD: DistributedOptimizationProblem.scala
// :145-160). Every work unit (forward row block / transpose item) keeps its table slot; its narrow and wide
// entries are filtered by the row keep flags and rewritten as WIDE lane-interleaved rounds in the unit's logical
// order (a filtered narrow round no longer spans < 64 keys). No sort: the filtered streams stay in unit order.
// Segments of <= CMP_SEG rounds of one unit, one wave each: pass 0 counts the kept entries per segment, the host
// turns the counts into per-unit round-aligned output starts (device cumsums) and pass 1 writes. Inside a round,
// logical entry t = 64 k + lane is placed with a ballot + popcount per k, so the copy is deterministic.
// key_is_row = 1 (transpose copy): an entry's chunk row is its key (pack >> sbits); 0 (forward copy): the unit's
// first row plus its slot (pack & smask). A TALL forward unit (4 sub-blocks of 2^sbits rows, ops/tiled.py) has
// 2^wbits slots: its narrow packs hold the row inside their sub-block and are rewritten as wide packs of the unit.
// ------------------------------------------------------------------------------------------------------------
#define CMP_SEG 8
struct CmpArgs {
  const int* units;             // unit table, 6 ints per unit: ... e_lo at col_e, e_hi at col_e + 1, n_lo, n_hi at 4, 5
  int col_e, row_col;           // row_col: column of the unit's first chunk row (-1: key_is_row)
  const int* seg;               // 3 ints per segment {unit, round_lo, round_hi}; rounds [0, n_hi - n_lo) are narrow
  int nseg, sbits, key_is_row;
  const uint32_t* pack;         // wide stream (interleaved)
  const void* val;
  const uint16_t* npack;        // narrow stream (interleaved 16-bit packs), one int32 base per round
  const void* nval;             // null: npack holds fused 16-B records (bf16 values; glm_kernels.hip TLNarrowSlot)
  const int* nbase;
  const unsigned char* keep;    // per chunk row: 1 = kept
  int* seg_cnt;                 // pass 0 output
  const long long* seg_first;   // pass 1: logical index (within its unit's output) of the segment's first kept entry
  const long long* unit_lo;     // pass 1: physical output start of every unit (round-aligned)
  uint32_t* opack;              // pass 1 outputs
  void* oval;
  int ustride;                  // ints per unit of ``units``: 6, or 10 = tall forward units (ops/tiled.py): columns 6, 7, 8
                                // hold the first narrow round of sub-blocks 1, 2, 3
  int wbits;                    // slot bits of the wide packs (= sbits, tall units: 12); sbits: the narrow packs'
};

template <typename VT, int PASS>
__global__ __launch_bounds__(256) void tl_compact_kernel(CmpArgs a) {
  const int lane = threadIdx.x & 63;
  const int s = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
  if (s >= a.nseg) return;                                   // wave-uniform
  const int* sg = a.seg + 3 * (long long)s;
  const int u = sg[0], r_lo = sg[1], r_hi = sg[2];
  const int* ut = a.units + a.ustride * (long long)u;
  const long long e_lo = ut[a.col_e];
  const int nw = ut[a.col_e + 1] - ut[a.col_e];
  const int n_lo = ut[4], nn = ut[5] - ut[4];
  const uint32_t row0 = a.row_col >= 0 ? (uint32_t)ut[a.row_col] : 0u;
  const uint32_t smask = (1u << a.sbits) - 1u, wmask = (1u << a.wbits) - 1u;
  const bool tall = a.ustride > 6;
  const VT* val = (const VT*)a.val;
  const VT* nval = (const VT*)a.nval;
  long long ob = PASS ? a.seg_first[s] : 0;
  const long long olo = PASS ? a.unit_lo[u] : 0;
  const unsigned long long below = (1ull << lane) - 1ull;
  int cnt = 0;
  for (int r = r_lo; r < r_hi; ++r) {
    uint32_t p[4];
    VT v[4];
    bool ok[4];
    if (r < nn) {
      const long long q = (long long)n_lo + r;
      const int base = a.nbase[q];
      // tall unit: the round's sub-block (its 1024 rows' offset in the unit) from the sub-blocks' first rounds
      const uint32_t sub = tall ? (uint32_t)((q >= ut[6]) + (q >= ut[7]) + (q >= ut[8])) << a.sbits : 0u;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        // fused records (nval null, 2-byte values): lane's 4 packs then its 4 values in one 16-B record
        const long long pe = nval ? q * 256 + 4 * lane + k : q * 512 + 8 * lane + k;
        const uint32_t p16 = a.npack[pe];
        p[k] = ((uint32_t)(base + (int)(p16 >> a.sbits)) << a.wbits) | sub | (p16 & smask);
        v[k] = nval ? nval[pe] : ((const VT*)a.npack)[pe + 4];
        ok[k] = true;
      }
    } else {
      const int w = r - nn;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        ok[k] = 256 * w + 64 * k + lane < nw;
        const long long e = e_lo + 256LL * w + 4 * lane + k;
        p[k] = ok[k] ? a.pack[e] : 0u;
        v[k] = ok[k] ? val[e] : (VT)0;
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint32_t row = a.key_is_row ? (p[k] >> a.wbits) : row0 + (p[k] & wmask);
      const bool kp = ok[k] && a.keep[row];
      const unsigned long long m = __ballot(kp);
      if (PASS) {
        if (kp) {
          const long long o = ob + __popcll(m & below);
          const long long ph = olo + (o & ~255LL) + ((o & 63) << 2) + ((o & 255) >> 6);
          a.opack[ph] = p[k];
          ((VT*)a.oval)[ph] = v[k];
        }
        ob += __popcll(m);
      } else {
        cnt += __popcll(m);
      }
    }
  }
  if (!PASS && lane == 0) a.seg_cnt[s] = cnt;
}


// ------------------------------------------------------------------------------------------------------------
// Per-entity Gram matrices K_e = X_e X_e^T of the row-space batch (optimization/row_space.py setup), straight
// from the block-diagonal CSR: one wave per entity of a size class (n_e <= n <= 192 rows; K zero padded to n x n).
// Row i of the entity is scattered into a dense LDS image of the entity's projected columns [cb, cb + d_e), then
// lane j takes the sparse dot product of row j with the image (row j's entries in stored order: deterministic
// fp64) and the image is cleared entry by entry. Rows must hold distinct columns (canonical CSR; checked on the
// host). Replaces 2 x n full passes of the GLM kernels over the whole coordinate (one indicator column per pass).
// ------------------------------------------------------------------------------------------------------------
// S rows per scatter round (template): rows i0 .. i0 + S - 1 go into S interleaved image slots (img[c S + s]), and
// one walk over row j's entries feeds S accumulators -- S times fewer walks (global reads + dependent chains) than
// one row per round, the same fma sequence per K entry (bitwise equal for every S).
// STAGE: the entity's entries (local column as uint16, value) and row offsets are first copied into LDS with
// coalesced whole-wave loads; the per-lane walks over row j then read LDS instead of issuing one uncoalesced global
// load per entry (64 lanes on 64 different rows) -- the dependent chain of a walk is LDS-latency bound, not
// HBM-latency bound. Same fma sequence, bitwise equal to the unstaged walk.
template <int S, bool STAGE>
__global__ __launch_bounds__(64) void seg_gram_kernel(int B, int n, int dmax, const long long* __restrict__ ents,
                                                      const long long* __restrict__ row_ptr,
                                                      const long long* __restrict__ col_ptr,
                                                      const long long* __restrict__ nip,
                                                      const long long* __restrict__ pos,
                                                      const double* __restrict__ val, double* __restrict__ K) {
  extern __shared__ double img[];
  const int lane = threadIdx.x;
  const long long b = blockIdx.x;
  if (b >= B) return;
  const long long e = ents[b];
  const long long r0 = row_ptr[e];
  const int ne = (int)(row_ptr[e + 1] - r0);
  const long long cb = col_ptr[e];
  const int de = (int)(col_ptr[e + 1] - cb);
  const long long e0 = nip[r0];
  const int enz = (int)(nip[r0 + ne] - e0);
  // staged layout after the image: values [enz] doubles, local columns [enz] uint16, row offsets [ne + 1] int
  double* sval = img + (size_t)dmax * S;
  unsigned short* scol = (unsigned short*)(sval + enz);
  int* sptr = (int*)(scol + ((enz + 3) & ~3));
  for (int c = lane; c < de * S; c += 64) img[c] = 0.0;
  if (STAGE) {
    for (int t = lane; t < enz; t += 64) {
      sval[t] = val[e0 + t];
      scol[t] = (unsigned short)(pos[e0 + t] - cb);
    }
    for (int i = lane; i <= ne; i += 64) sptr[i] = (int)(nip[r0 + i] - e0);
  }
  __syncthreads();
  double* Kb = K + b * (long long)n * n;
  for (int i0 = 0; i0 < ne; i0 += S) {
    const int ns = ne - i0 < S ? ne - i0 : S;
    for (int s = 0; s < ns; ++s) {
      if (STAGE) {
        const int ib = sptr[i0 + s], ie = sptr[i0 + s + 1];
        for (int t = ib + lane; t < ie; t += 64) img[(int)scol[t] * S + s] = sval[t];
      } else {
        const long long ib = nip[r0 + i0 + s], ie = nip[r0 + i0 + s + 1];
        for (long long t = ib + lane; t < ie; t += 64) img[(pos[t] - cb) * S + s] = val[t];
      }
    }
    __syncthreads();
    // lane takes rows j = lane, lane + 64, lane + 128 (n <= 192)
    for (int j = lane; j < n; j += 64) {
      double acc[S];
#pragma unroll
      for (int s = 0; s < S; ++s) acc[s] = 0.0;
      if (j < ne) {
        if (STAGE) {
          const int jb = sptr[j], je = sptr[j + 1];
          for (int t = jb; t < je; ++t) {
            const double v = sval[t];
            const double* im = img + (int)scol[t] * S;
#pragma unroll
            for (int s = 0; s < S; ++s) acc[s] = fma(v, im[s], acc[s]);
          }
        } else {
          const long long jb = nip[r0 + j], je = nip[r0 + j + 1];
          for (long long t = jb; t < je; ++t) {
            const double v = val[t];
            const double* im = img + (pos[t] - cb) * S;
#pragma unroll
            for (int s = 0; s < S; ++s) acc[s] = fma(v, im[s], acc[s]);
          }
        }
      }
#pragma unroll
      for (int s = 0; s < S; ++s)
        if (s < ns) Kb[(long long)j * n + i0 + s] = acc[s];
    }
    __syncthreads();
    for (int s = 0; s < ns; ++s) {
      if (STAGE) {
        const int ib = sptr[i0 + s], ie = sptr[i0 + s + 1];
        for (int t = ib + lane; t < ie; t += 64) img[(int)scol[t] * S + s] = 0.0;
      } else {
        const long long ib = nip[r0 + i0 + s], ie = nip[r0 + i0 + s + 1];
        for (long long t = ib + lane; t < ie; t += 64) img[(pos[t] - cb) * S + s] = 0.0;
      }
    }
    __syncthreads();
  }
  for (int i = ne; i < n; ++i)
    for (int j = lane; j < n; j += 64) Kb[(long long)j * n + i] = 0.0;
}

// Batched Cholesky of the row-space Gram matrices (replaces torch.linalg.cholesky_ex = rocSOLVER dpotf2: 48
// launches per class set and a one-off library initialisation on the cold path). One wave per problem, the lower
// triangle packed in LDS (n (n + 1) / 2 doubles: <= 148 KB at n = 192), left-looking: column j's entries are dot
// products of row prefixes, lanes over rows i >= j. Rows i >= nv[b] (padding slots) are the identity. Writes the
// full n x n factor (upper triangle zero) over K; info[b] = 0, or j + 1 for the first non-positive / non-finite
// pivot (then the factor is not used).
__global__ __launch_bounds__(64) void batched_chol_kernel(int B, int n, const long long* __restrict__ nv,
                                                          double* __restrict__ K, int* __restrict__ info) {
  extern __shared__ double Lp[];
  const int lane = threadIdx.x;
  const long long b = blockIdx.x;
  if (b >= B) return;
  const int m = (int)nv[b];
  double* Kb = K + b * (long long)n * n;
  for (int i = lane; i < n; i += 64)
    for (int k = 0; k <= i; ++k)
      Lp[i * (i + 1) / 2 + k] = (i < m && k < m) ? Kb[(long long)i * n + k] : (i == k ? 1.0 : 0.0);
  __syncthreads();
  int bad = 0;
  for (int j = 0; j < m && !bad; ++j) {
    const int rj = j * (j + 1) / 2;
    double djj = Lp[rj + j];
    for (int k = 0; k < j; ++k) djj = fma(-Lp[rj + k], Lp[rj + k], djj);
    __syncthreads();
    if (!(djj > 0.0) || !isfinite(djj)) { bad = j + 1; break; }
    const double ljj = sqrt(djj);
    for (int i = j + 1 + lane; i < m; i += 64) {
      const int ri = i * (i + 1) / 2;
      double a = Lp[ri + j];
      for (int k = 0; k < j; ++k) a = fma(-Lp[ri + k], Lp[rj + k], a);
      Lp[ri + j] = a / ljj;
    }
    if (lane == 0) Lp[rj + j] = ljj;
    __syncthreads();
  }
  if (lane == 0) info[b] = bad;
  for (int i = lane; i < n; i += 64)
    for (int k = 0; k < n; ++k) Kb[(long long)i * n + k] = k <= i ? Lp[i * (i + 1) / 2 + k] : 0.0;
}

// Row-space back-map w_e = X_e^T r_e for the entities ents[B] (random-effect model materialisation,
// optimization/row_space.py to_primal): one wave per entity, the entity's projected columns accumulated in LDS
// (d_e doubles), rows in order and the entries of one row on distinct lanes with distinct columns, so every LDS
// address is updated in a fixed order (deterministic) and no two lanes of one instruction collide. Reads only the
// handled entities' rows (the shard-wide transpose pass read every entity's).
// PT: int64 or int32 packed positions (int32 when the packed vector has < 2^31 coefficients: 4 bytes less per entry
// of a bandwidth-bound pass)
template <typename PT>
__global__ __launch_bounds__(64) void rs_primal_kernel(const long long* __restrict__ ents,
                                                       const long long* __restrict__ row_ptr,
                                                       const long long* __restrict__ col_ptr,
                                                       const long long* __restrict__ nip,
                                                       const PT* __restrict__ pos,
                                                       const double* __restrict__ val, const double* __restrict__ r,
                                                       double* __restrict__ W) {
  extern __shared__ double acc[];
  const int lane = threadIdx.x;
  const long long e = ents[blockIdx.x];
  const long long r0 = row_ptr[e], r1 = row_ptr[e + 1], c0 = col_ptr[e];
  const int d = (int)(col_ptr[e + 1] - c0);
  for (int j = lane; j < d; j += 64) acc[j] = 0.0;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  for (long long i = r0; i < r1; ++i) {
    const double a = r[i];
    const long long k0 = nip[i], k1 = nip[i + 1];
    for (long long k = k0 + lane; k < k1; k += 64) {
      const int c = (int)((long long)pos[k] - c0);
      acc[c] += a * val[k];
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
  for (int j = lane; j < d; j += 64) W[c0 + j] = acc[j];
}

// ---------------------------------------------------------------------------------------------------------------
// FULL coefficient variances var_j = (H_e^-1)_jj, H_e = X_e^T diag(c) X_e + lam I (optimization/variance.py is the
// definition; algorithm/coordinates.py dispatches). Both routes end in the squared column norms of G^-1 R for a lower
// Cholesky factor G of order m = min(n_e, d_e) <= VAR_MMAX:
//   primal    (d_e <= n_e): A = H_e = G G^T,                      var_j = |G^-1 e_j|^2
//   row space (n_e <  d_e): A = lam I + B B^T, B = diag(sqrt c) X_e, var_j = (1 - |G^-1 b_j|^2) / lam   (Woodbury)
// var_normal_kernel / var_scale_gram_kernel form A, batched_chol_kernel factors it, chol_colnorm_kernel does the rest.
// One wave per entity, launched per size class (n = the class's largest m). No atomics: every LDS address has one
// owner per step and is updated in a fixed order, so the results are bitwise repeatable.
// ---------------------------------------------------------------------------------------------------------------
#define VAR_MMAX 128    // packed factor (66 KB) + one 64-column panel of 128 rows (64 KB) fit the 160 KB of a workgroup

// Primal normal matrix A = lam I + sum_i c_i x_i x_i^T of the entities ents[B] (d_e <= n) as [B, n, n] (symmetric;
// rows / columns >= d_e: identity). Packed lower triangle in LDS; rows in stored order, the r (r + 1) / 2 pairs
// (a >= b) of one row's entries on distinct lanes = distinct LDS addresses (rows hold distinct columns).
__global__ __launch_bounds__(64) void var_normal_kernel(int B, int n, const long long* __restrict__ ents,
                                                        const long long* __restrict__ row_ptr,
                                                        const long long* __restrict__ col_ptr,
                                                        const long long* __restrict__ nip,
                                                        const long long* __restrict__ pos,
                                                        const double* __restrict__ val, const double* __restrict__ c,
                                                        double lam, double* __restrict__ A) {
  extern __shared__ double Ap[];
  const int lane = threadIdx.x;
  const long long b = blockIdx.x;
  if (b >= B) return;
  const long long e = ents[b];
  const long long r0 = row_ptr[e], r1 = row_ptr[e + 1];
  const long long cb = col_ptr[e];
  const long long dl = col_ptr[e + 1] - cb;
  const int de = dl < n ? (int)dl : n;
  const int np = n * (n + 1) / 2;
  double* sv = Ap + np;            // the current row's values [n]
  int* sc = (int*)(sv + n);        // ... and local columns [n] (-1: outside the entity's range, skipped)
  for (int t = lane; t < np; t += 64) Ap[t] = 0.0;
  __syncthreads();
  for (int j = lane; j < de; j += 64) Ap[j * (j + 1) / 2 + j] = lam;
  for (long long i = r0; i < r1; ++i) {
    const double ci = c[i];
    const long long k0 = nip[i];
    const long long rl = nip[i + 1] - k0;
    const int r = rl < de ? (int)rl : de;
    if (ci == 0.0 || r <= 0) continue;          // wave-uniform
    __syncthreads();
    for (int t = lane; t < r; t += 64) {
      const long long col = pos[k0 + t] - cb;
      const bool ok = col >= 0 && col < de;
      sc[t] = ok ? (int)col : -1;
      sv[t] = val[k0 + t];
    }
    __syncthreads();
    const int npair = r * (r + 1) / 2;
    for (int p = lane; p < npair; p += 64) {
      int a = (int)((sqrtf(8.0f * (float)p + 1.0f) - 1.0f) * 0.5f);
      while (a * (a + 1) / 2 > p) --a;
      while ((a + 1) * (a + 2) / 2 <= p) ++a;
      const int bb = p - a * (a + 1) / 2;
      const int ca = sc[a], cq = sc[bb];
      if (ca < 0 || cq < 0) continue;
      const int hi = ca > cq ? ca : cq, lo = ca > cq ? cq : ca;
      const int at = hi * (hi + 1) / 2 + lo;
      Ap[at] = fma(ci * sv[a], sv[bb], Ap[at]);
    }
  }
  __syncthreads();
  double* Ab = A + b * (long long)n * n;
  for (int t = lane; t < n * n; t += 64) {
    const int i = t / n, k = t - i * n;
    const int hi = i > k ? i : k, lo = i > k ? k : i;
    Ab[t] = hi < de ? Ap[hi * (hi + 1) / 2 + lo] : (i == k ? 1.0 : 0.0);
  }
}

// Row-space normal matrix in place: K [B, n, n] (seg_gram: X_e X_e^T, zero padded) becomes
// A = lam I + diag(s) K diag(s), s_i = sqrt(c_i); rows / columns >= n_e: identity.
__global__ __launch_bounds__(256) void var_scale_gram_kernel(int B, int n, const long long* __restrict__ ents,
                                                             const long long* __restrict__ row_ptr,
                                                             const double* __restrict__ c, double lam,
                                                             double* __restrict__ K) {
  const long long b = blockIdx.x;
  if (b >= B) return;
  const long long e = ents[b];
  const long long r0 = row_ptr[e];
  const long long nl = row_ptr[e + 1] - r0;
  const int ne = nl < n ? (int)nl : n;
  double* Kb = K + b * (long long)n * n;
  for (int t = threadIdx.x; t < n * n; t += 256) {
    const int i = t / n, j = t - i * n;
    double v = i == j ? 1.0 : 0.0;
    if (i < ne && j < ne) v = sqrt(c[r0 + i]) * Kb[t] * sqrt(c[r0 + j]) + (i == j ? lam : 0.0);
    Kb[t] = v;
  }
}

// Squared column norms q_j = |G^-1 r_j|^2 for the factors L [B, n, n] (batched_chol_kernel; order nv[b] <= n) of the
// entities ents[B], written as variances into out at col_ptr[e] + j. The packed factor stays in LDS; the right-hand
// side is processed in panels of 64 columns, one lane per column: the lane forward-substitutes down its own panel
// column (LDS, [row][lane]: conflict-free) and accumulates q in fp64 in row order.
// MODE 0: R = I (primal route), out = q_j for j < min(d_e, nv).
// MODE 1: R = diag(s) X_e, s = sqrt(c) (row-space route), out = (1 - q_j) / lam for j < d_e; the panel is scattered
//         from the entity's CSR rows -- the columns inside a row are sorted, so a per-row cursor finds each window.
template <int MODE>
__global__ __launch_bounds__(64) void chol_colnorm_kernel(int B, int n, const double* __restrict__ L,
                                                          const long long* __restrict__ nv,
                                                          const long long* __restrict__ ents,
                                                          const long long* __restrict__ row_ptr,
                                                          const long long* __restrict__ col_ptr,
                                                          const long long* __restrict__ nip,
                                                          const long long* __restrict__ pos,
                                                          const double* __restrict__ val,
                                                          const double* __restrict__ c, double lam,
                                                          double* __restrict__ out) {
  extern __shared__ double Gp[];
  const int lane = threadIdx.x;
  const long long b = blockIdx.x;
  if (b >= B) return;
  const long long e = ents[b];
  const long long ml = nv[b];
  const int m = ml < 0 ? 0 : (ml < n ? (int)ml : n);
  const long long cb = col_ptr[e];
  const long long de = col_ptr[e + 1] - cb;
  const long long ncols = MODE ? de : (de < m ? de : (long long)m);
  double* panel = Gp + n * (n + 1) / 2;         // [n][64]
  double* sr = panel + n * 64;                  // MODE 1: s_i [n]
  int* cur = (int*)(sr + n);                    // MODE 1: next entry of row i (relative to the entity's first) [n]
  int* end = cur + n;                           // MODE 1: end of row i [n]
  const double* Lb = L + b * (long long)n * n;
  for (int t = lane; t < m * n; t += 64) {
    const int i = t / n, k = t - i * n;
    if (k <= i) Gp[i * (i + 1) / 2 + k] = Lb[t];
  }
  long long e0 = 0;
  if (MODE) {
    const long long r0 = row_ptr[e];
    e0 = nip[r0];
    for (int i = lane; i < m; i += 64) {
      sr[i] = sqrt(c[r0 + i]);
      cur[i] = (int)(nip[r0 + i] - e0);
      end[i] = (int)(nip[r0 + i + 1] - e0);
    }
  }
  __syncthreads();
  for (long long j0 = 0; j0 < ncols; j0 += 64) {
    const long long j = j0 + lane;
    if (MODE) {
      for (int i = 0; i < m; ++i) panel[i * 64 + lane] = 0.0;
      __syncthreads();
      for (int i = lane; i < m; i += 64) {
        int k = cur[i];
        const int ke = end[i];
        const double s = sr[i];
        while (k < ke) {
          const long long col = pos[e0 + k] - cb;
          if (col >= j0 + 64) break;
          if (col >= j0) panel[i * 64 + (int)(col - j0)] = s * val[e0 + k];
          ++k;
        }
        cur[i] = k;
      }
      __syncthreads();
    }
    // identity right-hand sides of this panel are zero above row j0
    const int i0 = MODE ? 0 : (int)j0;
    double q = 0.0;
    for (int i = i0; i < m; ++i) {
      const int ri = i * (i + 1) / 2;
      double acc = MODE ? panel[i * 64 + lane] : (i == j ? 1.0 : 0.0);
      for (int k = i0; k < i; ++k) acc = fma(-Gp[ri + k], panel[k * 64 + lane], acc);
      const double y = acc / Gp[ri + i];
      panel[i * 64 + lane] = y;
      q = fma(y, y, q);
    }
    if (j < ncols) out[cb + j] = MODE ? (1.0 - q) / lam : q;
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Blocked FULL-variance route for VAR_MMAX < m <= VAR_BLOCKED_MMAX: the same two routes, the matrices in a global
// workspace A [chunk, n, n] (L2 / MALL resident) and one work-group of VB_WAVES waves per entity:
//   var_blk_normal_kernel / var_blk_gram_kernel   A (lower triangle; strict upper triangle zero; padding identity)
//   blocked_chol_kernel                           A = G G^T in place, 16-column panels, fp64 MFMA
//   blocked_trinv_kernel                          T = G^-1 in place (forward substitution with identity panels, which
//                                                 are zero above their first row: only the lower triangle is formed)
//   var_blk_colnorm_kernel                        primal: q_j = sum_k T[k][j]^2; row space: q_j = |T b_j|^2 with
//                                                 T b = sparse combinations of the CSR rows (no dense Y is formed)
// No atomics; every address has one owning wave (or thread) per step and a fixed summation order.
// ---------------------------------------------------------------------------------------------------------------
#define VAR_BLOCKED_MMAX 1024
#define VAR_BLOCKED_DMAX 2048   // row-space route: widest entity (LDS images of d_e doubles per wave / per row)
#define VB_WAVES 8
#define VB_THREADS (64 * VB_WAVES)
#define VB_T 16                 // panel width = MFMA tile
#define VBN_U 8                 // var_blk_normal_kernel: own entries of a row updated per round (loads in flight)
#define VBC_R 8                 // var_blk_colnorm_kernel<1>: CSR rows per round (loads in flight)

// leading dimension (doubles) of a 16-row LDS operand of up to n columns: = 2 (mod 32), so the 32 lanes of one
// ds_read_b64 half (16 rows x 2 k) fall on 32 distinct 8-byte bank pairs
__host__ __device__ inline int vb_ld(int n) { return ((n + 31) / 32) * 32 + 2; }

__device__ __forceinline__ void vb_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// One wave: in-place Cholesky of the 16 x 16 block sD ([16][17], lower triangle) whose first w rows / columns are
// live (the rest: identity). Returns 0, or j + 1 for the first non-positive / non-finite pivot (wave-uniform).
__device__ int vb_chol16(double* sD, int w, int lane) {
  const int r = lane & 15, q = lane >> 4;
  for (int j = 0; j < VB_T; ++j) {
    vb_wave_sync();
    const double d = sD[j * 17 + j];
    if (j < w && (!(d > 0.0) || !isfinite(d))) return j + 1;
    const double l = sqrt(d);
    const double lrj = sD[r * 17 + j] / l;
    vb_wave_sync();
    if (q == 0) {
      if (r > j) sD[r * 17 + j] = lrj;
      else if (r == j) sD[r * 17 + j] = l;
    }
    vb_wave_sync();
    for (int c = j + 1 + q; c < VB_T; c += 4)
      if (r >= c) sD[r * 17 + c] = fma(-sD[r * 17 + j], sD[c * 17 + j], sD[r * 17 + c]);
  }
  vb_wave_sync();
  return 0;
}

// One wave: sI [16][16] = inverse of the lower-triangular block sD ([16][17]); lane c < 16 solves column c.
__device__ void vb_inv16(const double* sD, double* sI, int lane) {
  if (lane < VB_T) {
    double x[VB_T];
#pragma unroll
    for (int p = 0; p < VB_T; ++p) {
      double s = p == lane ? 1.0 : 0.0;
#pragma unroll
      for (int k = 0; k < p; ++k) s = fma(-sD[p * 17 + k], x[k], s);
      x[p] = s / sD[p * 17 + p];
    }
#pragma unroll
    for (int p = 0; p < VB_T; ++p) sI[p * VB_T + lane] = p >= lane ? x[p] : 0.0;
  }
  vb_wave_sync();
}

// Primal normal matrix A = lam I + sum_i c_i x_i x_i^T (d_e <= n <= VAR_BLOCKED_MMAX) in the workspace slab of the
// entity. Wave w owns the output rows hi = w (mod VB_WAVES): every wave walks all rows of the entity (each stages the
// row in its own LDS slice) and adds the pairs (a, b <= a) of its own entries a -- the columns of a row increase, so
// col_b <= col_a and only the lower triangle is touched. A long entity's rows are thereby shared by all waves without
// a work-group barrier; one output address is only ever updated by one wave, in row order.
__global__ __launch_bounds__(VB_THREADS) void var_blk_normal_kernel(int B, int n, const long long* __restrict__ ents,
                                                                    const long long* __restrict__ row_ptr,
                                                                    const long long* __restrict__ col_ptr,
                                                                    const long long* __restrict__ nip,
                                                                    const long long* __restrict__ pos,
                                                                    const double* __restrict__ val,
                                                                    const double* __restrict__ c, double lam,
                                                                    double* A) {
  extern __shared__ double vbn_lds[];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long long b = blockIdx.x;
  if (b >= B) return;
  const long long e = ents[b];
  const long long r0 = row_ptr[e], r1 = row_ptr[e + 1];
  const long long cb = col_ptr[e];
  const long long dl = col_ptr[e + 1] - cb;
  const int de = dl < n ? (int)(dl < 0 ? 0 : dl) : n;
  const int per = n + (n + 1) / 2;                 // doubles per wave: values [n] + local columns [n] (int)
  double* sv = vbn_lds + (size_t)w * per;
  int* sc = (int*)(sv + n);
  double* Ab = A + b * (long long)n * n;
  for (int hi = w; hi < n; hi += VB_WAVES)
    for (int j = lane; j < n; j += 64) Ab[(long long)hi * n + j] = hi == j ? (hi < de ? lam : 1.0) : 0.0;
  vb_wave_sync();
  // Two rows of look-ahead hide the chain row pointer -> entries -> output: (kA, rA, cA) are the pointers of row
  // i + 1, (kB, rB, cB, colB, valB) row i with its first 64 entries (loaded from an index clamped to the entity's last
  // entry, so the loads need no branch).
  const long long klast = r1 > r0 ? nip[r1] - 1 : -1;
  long long kA = 0, kB = 0, colB = 0;
  int rA = 0, rB = 0;
  double cA = 0.0, cB = 0.0, valB = 0.0;
#define VBN_PTRS(I)                                   \
  do {                                                \
    if ((I) < r1) {                                   \
      kA = nip[(I)];                                  \
      const long long rl_ = nip[(I) + 1] - kA;        \
      rA = rl_ < de ? (int)(rl_ < 0 ? 0 : rl_) : de;  \
      cA = c[(I)];                                    \
    } else {                                          \
      rA = 0;                                         \
    }                                                 \
  } while (0)
#define VBN_ENTRIES()                                           \
  do {                                                          \
    kB = kA; rB = rA; cB = cA;                                  \
    const long long kc_ = kB + lane < klast ? kB + lane : klast; \
    colB = pos[kc_] - cb;                                       \
    valB = val[kc_];                                            \
  } while (0)
  if (klast < 0) return;                          // no entries: A = lam I
  VBN_PTRS(r0);
  VBN_ENTRIES();
  VBN_PTRS(r0 + 1);
  for (long long i = r0; i < r1; ++i) {
    const double ci = cB;
    const long long k0 = kB;
    const int r = rB;
    const long long col0 = colB;
    const double val0 = valB;
    VBN_ENTRIES();
    VBN_PTRS(i + 2);
    if (ci == 0.0 || r <= 0) continue;            // wave-uniform
    vb_wave_sync();
    if (lane < r) {
      sc[lane] = (col0 >= 0 && col0 < de) ? (int)col0 : -1;
      sv[lane] = val0;
    }
    for (int t = 64 + lane; t < r; t += 64) {
      const long long col = pos[k0 + t] - cb;
      sc[t] = (col >= 0 && col < de) ? (int)col : -1;
      sv[t] = val[k0 + t];
    }
    vb_wave_sync();
    const int lo0 = lane < r ? sc[lane] : -1;     // this lane's partner b = lane of every own entry a >= lane
    const double vb0 = lane < r ? sv[lane] : 0.0;
    for (int g0 = 0; g0 < r; g0 += 64) {
      const int t = g0 + lane;
      const int myc = t < r ? sc[t] : -1;
      unsigned long long mine = __ballot(myc >= 0 && (myc % VB_WAVES) == w);
      while (mine) {
        // VBN_U own entries at a time: their rows differ, so all their loads go out before the first store
        int a[VBN_U];
        double* p[VBN_U];
        double old[VBN_U];
        bool on[VBN_U];
#pragma unroll
        for (int u = 0; u < VBN_U; ++u) {
          a[u] = mine ? g0 + __builtin_ctzll(mine) : -1;
          mine &= mine - 1;
          on[u] = a[u] >= 0 && lane <= a[u] && lo0 >= 0;
          // idle lanes read the slab's first element (one hot line): the loads need no branch between them
          p[u] = on[u] ? Ab + (long long)sc[a[u] >= 0 ? a[u] : 0] * n + lo0 : Ab;
          old[u] = *p[u];
        }
#pragma unroll
        for (int u = 0; u < VBN_U; ++u)
          if (on[u]) *p[u] = fma(ci * sv[a[u]], vb0, old[u]);
#pragma unroll
        for (int u = 0; u < VBN_U; ++u) {
          if (a[u] < 64) continue;                // partners beyond the first 64 entries of a long row
          double* row = Ab + (long long)sc[a[u]] * n;
          const double va = ci * sv[a[u]];
          for (int bb = 64 + lane; bb <= a[u]; bb += 64) {
            const int lo = sc[bb];
            if (lo >= 0) row[lo] = fma(va, sv[bb], row[lo]);
          }
        }
      }
    }
  }
#undef VBN_PTRS
#undef VBN_ENTRIES
}

// Row-space normal matrix A = lam I + diag(s) X_e X_e^T diag(s), s = sqrt(c) (n_e <= n <= VAR_BLOCKED_MMAX,
// d_e <= dcap <= VAR_BLOCKED_DMAX): rounds of 8 rows i whose scaled entries are scattered into an LDS image
// [dcap][8]; thread j then walks row j once per round and forms the 8 dot products A[i][j], j <= i, in entry order.
__global__ __launch_bounds__(VB_THREADS) void var_blk_gram_kernel(int B, int n, int dcap,
                                                                  const long long* __restrict__ ents,
                                                                  const long long* __restrict__ row_ptr,
                                                                  const long long* __restrict__ col_ptr,
                                                                  const long long* __restrict__ nip,
                                                                  const long long* __restrict__ pos,
                                                                  const double* __restrict__ val,
                                                                  const double* __restrict__ c, double lam,
                                                                  double* __restrict__ A) {
  extern __shared__ double vbg_img[];              // [dcap][8]
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const long long b = blockIdx.x;
  if (b >= B) return;
  const long long e = ents[b];
  const long long r0 = row_ptr[e];
  const long long nl = row_ptr[e + 1] - r0;
  const int ne = nl < n ? (int)(nl < 0 ? 0 : nl) : n;
  const long long cb = col_ptr[e];
  const long long dl = col_ptr[e + 1] - cb;
  const int de = dl < dcap ? (int)(dl < 0 ? 0 : dl) : dcap;
  double* Ab = A + b * (long long)n * n;
  for (int t = tid; t < dcap * 8; t += VB_THREADS) vbg_img[t] = 0.0;
  __syncthreads();
  for (int i0 = 0; i0 < n; i0 += 8) {
    const bool live = i0 < ne;
    if (live) {
      // wave w scatters (pass 0) row i0 + w
      const int i = i0 + w;
      if (i < ne) {
        const double si = sqrt(c[r0 + i]);
        const long long ka = nip[r0 + i], kb = nip[r0 + i + 1];
        for (long long k = ka + lane; k < kb; k += 64) {
          const long long col = pos[k] - cb;
          if (col >= 0 && col < de) vbg_img[(int)col * 8 + w] = si * val[k];
        }
      }
      __syncthreads();
    }
    for (int j = tid; j < n; j += VB_THREADS) {
      double acc[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
      if (live && j < ne && j <= i0 + 7) {
        const double sj = sqrt(c[r0 + j]);
        const long long ka = nip[r0 + j], kb = nip[r0 + j + 1];
        for (long long k = ka; k < kb; ++k) {
          const long long col = pos[k] - cb;
          if (col < 0 || col >= de) continue;
          const double v = sj * val[k];
          const double* im = vbg_img + (int)col * 8;
#pragma unroll
          for (int s = 0; s < 8; ++s) acc[s] = fma(v, im[s], acc[s]);
        }
      }
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        const int i = i0 + s;
        if (i >= n) continue;
        double v = 0.0;
        if (j <= i) v = i < ne ? acc[s] + (i == j ? lam : 0.0) : (i == j ? 1.0 : 0.0);
        Ab[(long long)i * n + j] = v;
      }
    }
    if (live) {
      __syncthreads();
      const int i = i0 + w;
      if (i < ne) {
        const long long ka = nip[r0 + i], kb = nip[r0 + i + 1];
        for (long long k = ka + lane; k < kb; k += 64) {
          const long long col = pos[k] - cb;
          if (col >= 0 && col < de) vbg_img[(int)col * 8 + w] = 0.0;
        }
      }
      __syncthreads();
    }
  }
}

// Blocked Cholesky of K [B, n, n] in place (n <= VAR_BLOCKED_MMAX), one work-group per problem, left-looking over
// 16-column panels: the 16 rows L[k0 .. k0+16)[0 .. k0) of the panel sit in LDS (the A operand of every tile of the
// panel), the rows below come from the factor in global memory, and the products run on the fp64 matrix cores. The
// diagonal tile's K range is split over the waves and summed in wave order; one wave factors it and inverts the
// factor, and every other tile is P L11^-T = (L11^-1 P^T)^T by one more MFMA round. Only the lower triangle of K is
// read. Rows / columns >= nv[b] are the identity; the strict upper triangle of the result is zero. info[b] as
// batched_chol_kernel (on a bad pivot the kernel stops; every access stays inside the problem's slab).
__global__ __launch_bounds__(VB_THREADS) void blocked_chol_kernel(int B, int n, const long long* __restrict__ nv,
                                                                  double* K, int* __restrict__ info) {
  extern __shared__ double bc_lds[];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int lr = lane & 15, g = lane >> 4;
  const long long b = blockIdx.x;
  if (b >= B) return;
  const long long ml = nv[b];
  const int m = ml < 0 ? 0 : (ml < n ? (int)ml : n);
  const int ld = vb_ld(n);
  double* sB = bc_lds;                        // [16][ld]
  double* sD = sB + VB_T * ld;                // [16][17]
  double* sI = sD + VB_T * 17;                // [16][16]
  double* sP = sI + VB_T * VB_T;              // [VB_WAVES][256] partial diagonal tiles
  int* sflag = (int*)(sP + VB_WAVES * 256);
  double* Kb = K + b * (long long)n * n;
  if (tid == 0) *sflag = 0;
  __syncthreads();
  int bad = 0;
  for (int k0 = 0; k0 < m; k0 += VB_T) {
    for (int t = tid; t < VB_T * k0; t += VB_THREADS) {
      const int cc = t / k0, k = t - cc * k0;
      sB[cc * ld + k] = k0 + cc < m ? Kb[(long long)(k0 + cc) * n + k] : 0.0;
    }
    __syncthreads();
    {
      // diagonal tile: K steps split over the waves
      const int steps = k0 / 4;
      const int s_lo = (int)((long long)steps * w / VB_WAVES), s_hi = (int)((long long)steps * (w + 1) / VB_WAVES);
      v4d acc = {0.0, 0.0, 0.0, 0.0};
      for (int s = s_lo; s < s_hi; ++s) {
        const double a = sB[lr * ld + 4 * s + g];
        acc = mfma_f64_16x16x4(a, a, acc);
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) sP[w * 256 + q * 64 + lane] = acc[q];
    }
    __syncthreads();
    if (w == 0) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int rr = g + 4 * q, cc = lr;
        double s = 0.0;
        for (int ww = 0; ww < VB_WAVES; ++ww) s += sP[ww * 256 + q * 64 + lane];
        const bool ok = k0 + rr < m && k0 + cc < m;
        double v = rr == cc ? 1.0 : 0.0;
        if (ok && cc <= rr) v = Kb[(long long)(k0 + rr) * n + k0 + cc] - s;
        sD[rr * 17 + cc] = v;
      }
      const int wl = m - k0 < VB_T ? m - k0 : VB_T;
      const int f = vb_chol16(sD, wl, lane);
      if (f) {
        if (lane == 0) *sflag = k0 + f;
      } else {
        vb_inv16(sD, sI, lane);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int rr = lr, cc = g + 4 * q;
          if (k0 + rr < m && k0 + cc < m) Kb[(long long)(k0 + rr) * n + k0 + cc] = cc <= rr ? sD[rr * 17 + cc] : 0.0;
        }
      }
    }
    __syncthreads();
    bad = *sflag;
    if (bad) break;
    const int ntile = (m - k0 + VB_T - 1) / VB_T;
    for (int t = 1 + w; t < ntile; t += VB_WAVES) {
      const int row = k0 + VB_T * t + lr;
      const bool rowok = row < m;
      double* Lr = Kb + (long long)(rowok ? row : 0) * n;
      v4d acc = {0.0, 0.0, 0.0, 0.0};
      for (int kk = 0; kk < k0; kk += VB_T) {      // k0 is a multiple of 16: four loads in flight per round
        double bq[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) bq[u] = Lr[kk + 4 * u + g];
#pragma unroll
        for (int u = 0; u < 4; ++u)
          acc = mfma_f64_16x16x4(sB[lr * ld + kk + 4 * u + g], rowok ? bq[u] : 0.0, acc);
      }
      // acc[q] = sum_k L[k0 + c][k] L[row][k], c = g + 4 q: P^T[c][row] = K[row][k0 + c] - acc[q]
      v4d x = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int cc = g + 4 * q;
        const double p = (rowok && k0 + cc < m) ? Lr[k0 + cc] - acc[q] : 0.0;
        x = mfma_f64_16x16x4(sI[lr * VB_T + cc], p, x);
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int cc = g + 4 * q;
        if (rowok && k0 + cc < m) Lr[k0 + cc] = x[q];
      }
    }
    __syncthreads();
  }
  if (tid == 0) info[b] = bad;
  for (int r = w; r < n; r += VB_WAVES)
    for (int cc = lane; cc < n; cc += 64) {
      if (cc > r) Kb[(long long)r * n + cc] = 0.0;
      else if (r >= m) Kb[(long long)r * n + cc] = r == cc ? 1.0 : 0.0;
    }
}

// T = G^-1 in place over the factors L [B, n, n] of blocked_chol_kernel (order nv[b]; padding rows stay the
// identity): block row i of T is -L_ii^-1 (L[i][0 .. i0) T[0 .. i0)][:]) with T_ii = L_ii^-1 -- the forward
// substitution of the identity in 16-column panels, which are zero above their first row, so tile (i, j) sums over
// k in [j0, i0) only. The 16 rows of L sit in LDS (they are overwritten by the result), the solved row blocks of T
// are read from global memory, the products run on the fp64 matrix cores.
__global__ __launch_bounds__(VB_THREADS) void blocked_trinv_kernel(int B, int n, const long long* __restrict__ nv,
                                                                   double* L) {
  extern __shared__ double bt_lds[];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int lr = lane & 15, g = lane >> 4;
  const long long b = blockIdx.x;
  if (b >= B) return;
  const long long ml = nv[b];
  const int m = ml < 0 ? 0 : (ml < n ? (int)ml : n);
  const int ld = vb_ld(n);
  double* sA = bt_lds;                        // [16][ld]
  double* sD = sA + VB_T * ld;                // [16][17]
  double* sI = sD + VB_T * 17;                // [16][16]
  double* Lb = L + b * (long long)n * n;
  for (int i0 = 0; i0 < m; i0 += VB_T) {
    for (int t = tid; t < VB_T * i0; t += VB_THREADS) {
      const int rr = t / i0, k = t - rr * i0;
      sA[rr * ld + k] = i0 + rr < m ? Lb[(long long)(i0 + rr) * n + k] : 0.0;
    }
    if (tid < VB_T * VB_T) {
      const int rr = tid >> 4, cc = tid & 15;
      double v = rr == cc ? 1.0 : 0.0;
      if (i0 + rr < m && i0 + cc < m) v = cc <= rr ? Lb[(long long)(i0 + rr) * n + i0 + cc] : 0.0;
      sD[rr * 17 + cc] = v;
    }
    __syncthreads();
    if (w == 0) vb_inv16(sD, sI, lane);
    __syncthreads();
    if (tid < VB_T * VB_T) {
      const int rr = tid >> 4, cc = tid & 15;
      if (i0 + rr < m && i0 + cc < m) Lb[(long long)(i0 + rr) * n + i0 + cc] = sI[rr * VB_T + cc];
    }
    for (int j = w; j < i0 / VB_T; j += VB_WAVES) {
      const int j0 = VB_T * j;
      v4d acc = {0.0, 0.0, 0.0, 0.0};
      for (int kk = j0; kk < i0; kk += VB_T) {     // i0 - j0 is a multiple of 16: four loads in flight per round
        double bq[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) bq[u] = Lb[(long long)(kk + 4 * u + g) * n + j0 + lr];
#pragma unroll
        for (int u = 0; u < 4; ++u) acc = mfma_f64_16x16x4(sA[lr * ld + kk + 4 * u + g], bq[u], acc);
      }
      v4d x = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int q = 0; q < 4; ++q) x = mfma_f64_16x16x4(-sI[lr * VB_T + g + 4 * q], acc[q], x);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int rr = g + 4 * q;
        if (i0 + rr < m) Lb[(long long)(i0 + rr) * n + j0 + lr] = x[q];
      }
    }
    __syncthreads();
  }
}

// Variances from T = G^-1 [B, n, n] (blocked_trinv_kernel; order nv[b]) into out[col_ptr[e] + j].
// MODE 0 (primal): q_j = sum_{k >= j} T[k][j]^2 for j < min(d_e, nv), one thread per column, rows in order.
// MODE 1 (row space): q_j = |T b_j|^2, B = diag(s) X_e, out = (1 - q_j) / lam for j < d_e <= dcap. Wave w forms the
//   rows k = w (mod VB_WAVES) of T B in its own LDS image [dcap] as the combination sum_{i <= k} T[k][i] s_i x_i of
//   the entity's sparse rows (rows in order, four rows' entries in flight) and adds its squares to per-lane sums q
//   (lane owns the columns = lane mod 64); the waves' sums are added in wave order at the end.
template <int MODE>
__global__ __launch_bounds__(VB_THREADS) void var_blk_colnorm_kernel(int B, int n, int dcap,
                                                                     const double* __restrict__ T,
                                                                     const long long* __restrict__ nv,
                                                                     const long long* __restrict__ ents,
                                                                     const long long* __restrict__ row_ptr,
                                                                     const long long* __restrict__ col_ptr,
                                                                     const long long* __restrict__ nip,
                                                                     const long long* __restrict__ pos,
                                                                     const double* __restrict__ val,
                                                                     const double* __restrict__ c, double lam,
                                                                     double* __restrict__ out) {
  extern __shared__ double vbc_lds[];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const long long b = blockIdx.x;
  if (b >= B) return;
  const long long e = ents[b];
  const long long ml = nv[b];
  const int m = ml < 0 ? 0 : (ml < n ? (int)ml : n);
  const long long cb = col_ptr[e];
  const long long dl = col_ptr[e + 1] - cb;
  const double* Tb = T + b * (long long)n * n;
  if (MODE == 0) {
    const int ncols = dl < m ? (int)(dl < 0 ? 0 : dl) : m;
    for (int j = tid; j < ncols; j += VB_THREADS) {
      double q = 0.0;
      for (int k = j; k < m; ++k) {
        const double t = Tb[(long long)k * n + j];
        q = fma(t, t, q);
      }
      out[cb + j] = q;
    }
    return;
  }
  const int de = dl < dcap ? (int)(dl < 0 ? 0 : dl) : dcap;
  double* img = vbc_lds;                          // [VB_WAVES][dcap]
  double* sr = img + (size_t)VB_WAVES * dcap;     // s_i [n]
  int* sk = (int*)(sr + n);                       // first entry of row i relative to the entity's first [n + 1]
  const long long r0 = row_ptr[e];
  const long long e0 = nip[r0];
  for (int i = tid; i < m; i += VB_THREADS) sr[i] = sqrt(c[r0 + i]);
  for (int i = tid; i <= m; i += VB_THREADS) sk[i] = (int)(nip[r0 + i] - e0);
  for (int t = tid; t < VB_WAVES * dcap; t += VB_THREADS) img[t] = 0.0;
  __syncthreads();
  double* im = img + (size_t)w * dcap;
  double q[VAR_BLOCKED_DMAX / 64];
#pragma unroll
  for (int u = 0; u < VAR_BLOCKED_DMAX / 64; ++u) q[u] = 0.0;
  const int klast = sk[m] - 1;                    // last entry of the entity's rows (< 0: no entries, every q_j = 0)
  for (int k = w; klast >= 0 && k < m; k += VB_WAVES) {
    const double* Tk = Tb + (long long)k * n;
    // rounds of VBC_R rows i; the loads of the next round go out before this round's LDS updates
    double t[2][VBC_R], v[2][VBC_R];
    int col[2][VBC_R], ka[2][VBC_R], kb[2][VBC_R];
#define VBC_LOAD(S, I0)                                              \
  _Pragma("unroll") for (int u = 0; u < VBC_R; ++u) {                \
    /* every load is unconditional on a clamped, valid index (no branch between the loads of a round) */ \
    const bool ok = (I0) + u <= k;                                   \
    const int ii = ok ? (I0) + u : k;                                \
    ka[S][u] = sk[ii];                                               \
    kb[S][u] = ok ? sk[ii + 1] : ka[S][u];                           \
    t[S][u] = Tk[ii] * sr[ii];                                       \
    const int kx = ka[S][u] + lane;                                  \
    const bool has = kx < kb[S][u];                                  \
    const int kc = kx < klast ? kx : klast;                          \
    const long long cl = pos[e0 + kc] - cb;                          \
    col[S][u] = (has && cl >= 0 && cl < de) ? (int)cl : -1;          \
    v[S][u] = val[e0 + kc];                                          \
  }
#define VBC_APPLY(S)                                                                              \
  _Pragma("unroll") for (int u = 0; u < VBC_R; ++u) {                                             \
    if (col[S][u] >= 0) im[col[S][u]] = fma(t[S][u], v[S][u], im[col[S][u]]);                     \
    for (int kx = ka[S][u] + 64 + lane; kx < kb[S][u]; kx += 64) { /* rows of more than 64 entries */ \
      const long long cl = pos[e0 + kx] - cb;                                                     \
      if (cl >= 0 && cl < de) im[(int)cl] = fma(t[S][u], val[e0 + kx], im[(int)cl]);              \
    }                                                                                             \
    vb_wave_sync();                                                                               \
  }
    VBC_LOAD(0, 0)
    for (int i = 0; i <= k; i += 2 * VBC_R) {
      if (i + VBC_R <= k) { VBC_LOAD(1, i + VBC_R) }
      VBC_APPLY(0)
      if (i + VBC_R <= k) {
        if (i + 2 * VBC_R <= k) { VBC_LOAD(0, i + 2 * VBC_R) }
        VBC_APPLY(1)
      }
    }
#undef VBC_LOAD
#undef VBC_APPLY
#pragma unroll
    for (int u = 0; u < VAR_BLOCKED_DMAX / 64; ++u) {
      const int cc = u * 64 + lane;
      if (cc < de) {
        const double y = im[cc];
        q[u] = fma(y, y, q[u]);
        im[cc] = 0.0;
      }
    }
    vb_wave_sync();
  }
#pragma unroll
  for (int u = 0; u < VAR_BLOCKED_DMAX / 64; ++u) {
    const int cc = u * 64 + lane;
    if (cc < de) im[cc] = q[u];
  }
  __syncthreads();
  for (int j = tid; j < de; j += VB_THREADS) {
    double s = 0.0;
    for (int ww = 0; ww < VB_WAVES; ++ww) s += img[(size_t)ww * dcap + j];
    out[cb + j] = (1.0 - s) / lam;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Histogram of integer keys (torch.bincount) for inputs with very hot keys: the fixed-effect relabel counts 775M
// column ids of which one (the intercept) occurs in EVERY row and a Zipf head in most, so plain global atomics
// serialise on a few addresses (torch's kernelHistogram1D: 443 ms at GAME config 5). Each workgroup aggregates its
// slice in an LDS open-addressing table (HIST_SLOTS keys, linear probing, HIST_PROBES tries) and flushes one global
// atomic per distinct key it holds; keys that find no slot go straight to global atomics (they are the rare ones).
// Integer counts: the result does not depend on the order of the atomics.
#define HIST_SLOTS 4096
#define HIST_PROBES 8
#define HIST_THREADS 256
template <typename KT>
__global__ __launch_bounds__(HIST_THREADS) void key_hist_kernel(const KT* __restrict__ keys, long long n,
                                                                long long per_block, long long nbins,
                                                                unsigned long long* __restrict__ counts) {
  __shared__ int s_key[HIST_SLOTS];
  __shared__ unsigned int s_cnt[HIST_SLOTS];
  for (int i = threadIdx.x; i < HIST_SLOTS; i += HIST_THREADS) { s_key[i] = -1; s_cnt[i] = 0; }
  __syncthreads();
  const long long a = (long long)blockIdx.x * per_block;
  const long long b = a + per_block < n ? a + per_block : n;
  for (long long i = a + threadIdx.x; i < b; i += HIST_THREADS) {
    const long long k = (long long)keys[i];
    if (k < 0 || k >= nbins) continue;                       // the wrapper validates; never index out of range
    bool done = false;
    if (k < 0x7fffffffLL) {
      const int ki = (int)k;
      unsigned int h = ((unsigned int)ki * 2654435761u) >> (32 - 12);
      for (int p = 0; p < HIST_PROBES && !done; ++p) {
        const int s = (int)((h + (unsigned int)p) & (HIST_SLOTS - 1));
        int cur = s_key[s];
        if (cur == -1) cur = atomicCAS(&s_key[s], -1, ki) == -1 ? ki : s_key[s];
        if (cur == ki) { atomicAdd(&s_cnt[s], 1u); done = true; }
      }
    }
    if (!done) atomicAdd(&counts[k], 1ULL);
  }
  __syncthreads();
  for (int s = threadIdx.x; s < HIST_SLOTS; s += HIST_THREADS) {
    const int k = s_key[s];
    if (k >= 0 && s_cnt[s]) atomicAdd(&counts[k], (unsigned long long)s_cnt[s]);
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Row gather of a CSR into a new CSR (random-effect solver setup: the fused primal batch's rows, the row-space
// back-map's compact copy). Row r of the output = row rows[r] of the input, starting at optr[r] with
// optr[r + 1] - optr[r] >= its length slots (extra slots zero-filled: the lean kernel's quad padding); columns minus
// cbase[r] (entity-local) when cbase is given, stored as CT (int16 / int64). One wave per row, coalesced copies:
// replaces a chain of torch repeat_interleave / gather / scatter passes over every non-zero.
template <typename CT>
__global__ __launch_bounds__(256) void csr_gather_rows_kernel(const long long* __restrict__ nip,
                                                              const long long* __restrict__ pos,
                                                              const double* __restrict__ val,
                                                              const long long* __restrict__ rows, long long nr,
                                                              const long long* __restrict__ optr,
                                                              const long long* __restrict__ cbase,
                                                              CT* __restrict__ ocol, double* __restrict__ oval) {
  const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (r >= nr) return;
  const long long src = nip[rows[r]], len = nip[rows[r] + 1] - src;
  const long long dst = optr[r], dlen = optr[r + 1] - dst;
  const long long base = cbase != nullptr ? cbase[r] : 0;
  for (long long t = lane; t < dlen; t += 64) {
    if (t < len) {
      ocol[dst + t] = (CT)(pos[src + t] - base);
      oval[dst + t] = val[src + t];
    } else {
      ocol[dst + t] = (CT)0;
      oval[dst + t] = 0.0;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Prior fold (incremental training, data/random_effect.py): a Gaussian prior N(mu_j, sigma_j^2) per packed
// coefficient becomes plain L2 on column-scaled data with shifted offsets (w = mu + sigma v). One pass over the
// entity-sorted CSR (nip, pos, val): m[r] = sum_k val[k] mu[pos[k]] with the ORIGINAL values (the prior model's
// score on row r), then val[k] *= sigma[pos[k]] IN PLACE (every entry is read and written by the same lane; no second
// copy of the values). One 16-lane row per CSR row: lanes stride the row's entries by 16 with one fp64 partial each,
// then a fixed xor butterfly over the 16 lanes. No atomics: every launch gives the same bits. Empty rows write 0.
#define FOLD_GROUP 16
#define FOLD_THREADS 256
#define FOLD_ROWS_PER_BLOCK (FOLD_THREADS / FOLD_GROUP)
__global__ __launch_bounds__(FOLD_THREADS) void prior_fold_kernel(const long long* __restrict__ nip,
                                                                  const long long* __restrict__ pos,
                                                                  double* __restrict__ val, long long n_rows,
                                                                  const double* __restrict__ mu,
                                                                  const double* __restrict__ sigma,
                                                                  double* __restrict__ m) {
  const long long row = (long long)blockIdx.x * FOLD_ROWS_PER_BLOCK + (threadIdx.x / FOLD_GROUP);
  const int g = threadIdx.x % FOLD_GROUP;
  double s = 0.0;
  if (row < n_rows) {
    const long long lo = nip[row], hi = nip[row + 1];
    for (long long p = lo + g; p < hi; p += FOLD_GROUP) {
      const long long c = pos[p];
      const double v = val[p];
      s += v * mu[c];
      val[p] = v * sigma[c];
    }
  }
#pragma unroll
  for (int o = FOLD_GROUP / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, FOLD_GROUP);
  if (g == 0 && row < n_rows) m[row] = s;
}

// ---------------------------------------------------------------------------------------------------------------
// K12 per-group ranking metrics (AUC:tag, PRECISION@k:tag; evaluation/segmented.py): one fp64 value per group of a
// group-ordered row layout (seg_ptr over groups, perm = row position of every group-ordered slot, group-ordered
// weights and positive flags). Groups are bucketed by length on the host and every bucket has its own execution:
//   C16 (1..16 rows)   seg_rank_wave_kernel<16>: four groups per wave, one 16-lane row each, rows in registers
//   C64 (17..64)       seg_rank_wave_kernel<64>: one wave per group, rows in registers
//   CWG (65..4096)     seg_rank_block_kernel<false>: one 256-thread workgroup per group, bitonic sort in LDS
//                      (8 B score + 4 B local index per padded row: 48 KB at 4096)
//   LONG (> wg_max)    seg_rank_block_kernel<true>: rows arrive sorted (two stable torch sorts on the host side of
//                      the wrapper), one workgroup streams its group in chunks of 256 rows
// Order: score descending, ties by position within the group ascending (a total order, so the bitonic network need
// not be stable; the tie test is ==, so -0.0 ties with 0.0). Padding rows: score -inf, weight 0, index past the end.
// AUC is the tie-grouped weighted trapezoid of AreaUnderROCCurveLocalEvaluator.scala:33-70: a tie group with
// positive / negative weight gp / gn that closes at sorted row i adds (P_i - gp) gn + gp gn / 2, P_i the inclusive
// positive prefix; gp, gn are segmented scans (sums of non-negative terms, no differences of prefixes of gn), the
// value is raw / (tp * tn) in exactly that expression (NaN when a class is missing). Precision@k counts positives
// among the first min(k, L) sorted rows, over k. AUPR (METRIC SR_AUPR) is the tie-grouped weighted trapezoid under
// the precision/recall points (diagnostics/evaluation.py::binary_metrics with weights): the group that closes at
// row i adds gp (p + q) / 2, p = P_i / (P_i + N_i) from the inclusive prefixes, q the same ratio of the prefixes
// BEFORE the group's head (p when those are both 0), nothing when gp = 0; the value is sum / tp, NaN when a class
// is missing. It shares the sort, the loads, the padding rows, the NaN flag and every index with AUC. No atomics:
// scans and reductions are fixed shuffle / LDS trees, so every launch gives the same bits. A NaN score sets *nan_flag (all writers store 1) and the wrapper discards the
// result; the compare-exchange evaluates ONE predicate per pair on both sides, so even then the indices stay a
// permutation and nothing is read out of bounds.
// Under a process group every rank runs these kernels over the rows it OWNS: MultiEvaluator routes each row once to
// the owner of its group and hands GroupedRanking the routed rows (n_list = 0 launches nothing: a rank may own no
// group). The global AUC of all rows is not a per-group metric: see auc_count_kernel below.
// ---------------------------------------------------------------------------------------------------------------
struct SegRankArgs {
  const long long* seg_ptr;     // [n_groups + 1] (unused by the pre-sorted kernel)
  const long long* perm;        // [n_rows] row position of every group-ordered slot (unused when pre-sorted)
  const double* scores;         // [n_rows] in row order; pre-sorted: the LONG rows' scores in sorted order
  const double* wts;            // [n_rows] group-ordered; pre-sorted: sorted order
  const unsigned char* flag;    // positive flags, same order as wts
  const long long* list;        // [n_list] group indices of this class
  const long long* lptr;        // pre-sorted only: [n_list + 1] row range of every listed group
  double* out;                  // [n_groups]
  int* nan_flag;
  long long n_list, n_rows, n_groups;
  int k;                        // precision@k position (AUC, AUPR: ignored)
};

#define SR_THREADS 256
#define SR_WG_MAX 4096
#define SR_PREC 0                 // METRIC of the kernels below: precision@k,
#define SR_AUC 1                  // tie-grouped weighted ROC AUC,
#define SR_AUPR 2                 // tie-grouped weighted area under the precision/recall curve

__device__ __forceinline__ bool sr_before(double sa, int ia, double sb, int ib) {
  return sa > sb || (sa == sb && ia < ib);
}

// The head-of-tie-group prefixes of AUPR: eP / eN are a lane's exclusive prefixes (the inclusive ones shifted up a
// lane, 0 in the first lane of the row), heads the ballot of the lanes that open a tie group. Every lane gets the
// pair of the last head at or before it; a lane with no head below it in the wave gets (0, 0) and the caller's
// carry applies.
__device__ __forceinline__ void sr_head_prefix(bool f0, int wl, double eP, double eN, double& hP, double& hN) {
  const unsigned long long m = __ballot(f0) & (~0ull >> (63 - wl));
  const int h = m ? 63 - __clzll((long long)m) : wl;
  hP = __shfl(eP, h, 64);
  hN = __shfl(eN, h, 64);
  if (!m) { hP = 0.0; hN = 0.0; }
}

// One tie group's AUPR term, formed by its closing lane: gp (p + q) / 2 with p the precision after the group
// (P, N: inclusive prefixes) and q the precision before it (hP, hN: prefixes before its head; p when nothing with
// weight precedes it). A group without positive weight makes no recall step and adds nothing.
__device__ __forceinline__ double sr_aupr_term(double gp, double P, double N, double hP, double hN) {
  if (!(gp > 0.0)) return 0.0;
  const double pr = P / (P + N);
  const double den = hP + hN;
  const double q = den > 0.0 ? hP / den : pr;
  return gp * (pr + q) / 2.0;
}

template <int W, int METRIC>
__global__ __launch_bounds__(SR_THREADS) void seg_rank_wave_kernel(SegRankArgs a) {
  const int l = threadIdx.x % W;
  const long long b = (long long)blockIdx.x * (SR_THREADS / W) + threadIdx.x / W;
  // every lane of a W-lane row takes part in the shuffles: an idle or malformed group runs with L = 0
  long long g = -1, r0 = 0;
  int L = 0;
  if (b < a.n_list) {
    g = a.list[b];
    if (g >= 0 && g < a.n_groups) {
      r0 = a.seg_ptr[g];
      const long long len = a.seg_ptr[g + 1] - r0;
      if (len >= 1 && len <= W && r0 >= 0 && r0 + len <= a.n_rows) L = (int)len;
    } else {
      g = -1;
    }
  }
  double s = -INFINITY, w = 0.0;
  bool fl = false;
  if (l < L) {
    const long long pr = a.perm[r0 + l];
    s = (pr >= 0 && pr < a.n_rows) ? a.scores[pr] : (double)NAN;
    w = a.wts[r0 + l];
    fl = a.flag[r0 + l] != 0;
    if (s != s) *a.nan_flag = 1;
  }
  int idx = l;
#pragma unroll
  for (int k = 2; k <= W; k <<= 1) {
#pragma unroll
    for (int j = k >> 1; j > 0; j >>= 1) {
      const double so = __shfl_xor(s, j, W);
      const int io = __shfl_xor(idx, j, W);
      const bool up = (l & k) == 0;
      const bool c = (l & j) == 0 ? sr_before(s, idx, so, io) : sr_before(so, io, s, idx);   // lower before upper?
      if (c != up) { s = so; idx = io; }
    }
  }
  const double p0 = fl ? w : 0.0;
  const double n0 = w - p0;
  double val;
  if (METRIC != SR_PREC) {
    const double p = __shfl(p0, idx, W), n = __shfl(n0, idx, W);
    const double sp = __shfl_up(s, 1, W), sn = __shfl_down(s, 1, W);
    // padding rows (-inf, weight 0) take part as ordinary rows: they add 0 to whatever tie group they join
    bool f = l == 0 || s != sp;
    const bool tail = l == W - 1 || s != sn;
    const bool f0 = f;
    double gp = p, gn = n, P = p, N = n;
#pragma unroll
    for (int d = 1; d < W; d <<= 1) {
      const double tgp = __shfl_up(gp, d, W), tgn = __shfl_up(gn, d, W), tP = __shfl_up(P, d, W);
      const double tN = METRIC == SR_AUPR ? __shfl_up(N, d, W) : 0.0;
      const int tf = __shfl_up((int)f, d, W);
      if (l >= d) {
        P += tP;
        if (METRIC == SR_AUPR) N += tN;
        if (!f) { gp += tgp; gn += tgn; f = tf != 0; }
      }
    }
    if (METRIC == SR_AUC) {
      double raw = tail ? (P - gp) * gn + gp * gn / 2.0 : 0.0;
      double tp = p, tn = n;
#pragma unroll
      for (int o = W / 2; o > 0; o >>= 1) {
        raw += __shfl_xor(raw, o, W);
        tp += __shfl_xor(tp, o, W);
        tn += __shfl_xor(tn, o, W);
      }
      val = raw / (tp * tn);
    } else {
      // lane 0 of every row opens a tie group, so the head found is one of this row's lanes
      double eP = __shfl_up(P, 1, W), eN = __shfl_up(N, 1, W), hP, hN;
      if (l == 0) { eP = 0.0; eN = 0.0; }
      sr_head_prefix(f0, threadIdx.x & 63, eP, eN, hP, hN);
      double sum = tail ? sr_aupr_term(gp, P, N, hP, hN) : 0.0;
#pragma unroll
      for (int o = W / 2; o > 0; o >>= 1) sum += __shfl_xor(sum, o, W);
      const double tp = __shfl(P, W - 1, W), tn = __shfl(N, W - 1, W);
      val = tp > 0.0 && tn > 0.0 ? sum / tp : (double)NAN;
    }
  } else {
    const int fs = __shfl((int)fl, idx, W);
    int hit = (l < a.k && l < L) ? fs : 0;
#pragma unroll
    for (int o = W / 2; o > 0; o >>= 1) hit += __shfl_xor(hit, o, W);
    val = (double)hit / (double)a.k;
  }
  if (l == 0 && g >= 0) a.out[g] = L > 0 ? val : (double)NAN;
}

// CWG (PRE = false): sort the group in LDS, then evaluate the sorted rows in chunks of 256. LONG (PRE = true): the
// rows are already sorted, the same chunk loop reads them from global memory. Carried across chunks (uniform in the
// workgroup): total positive / negative weight, raw, and the open tie group's two sums -- a tie group may span
// chunks; a row's neighbours are read directly, so no previous score is carried. AUPR also scans the negative
// prefix and carries, with the open tie group, the two prefixes before its head (formed as running total + the
// wave's exclusive prefix at the head, never as inclusive prefix - group sum); raw then holds the sum of its terms.
template <bool PRE, int METRIC>
__global__ __launch_bounds__(SR_THREADS) void seg_rank_block_kernel(SegRankArgs a, int npad_max) {
  extern __shared__ double sr_lds[];              // !PRE: keys [npad_max], then local indices [npad_max]
  __shared__ double w_gp[4], w_gn[4], w_P[4], w_N[4], w_raw[4], w_hP[4], w_hN[4];
  __shared__ int w_f[4], w_hit[4];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const long long b = blockIdx.x;
  if (b >= a.n_list) return;
  const long long g = a.list[b];
  if (g < 0 || g >= a.n_groups) return;
  long long r0, L;
  if (PRE) {
    r0 = a.lptr[b];
    L = a.lptr[b + 1] - r0;
  } else {
    r0 = a.seg_ptr[g];
    L = a.seg_ptr[g + 1] - r0;
  }
  if (L < 1 || r0 < 0 || r0 + L > a.n_rows || (!PRE && L > npad_max)) {    // uniform in the workgroup
    if (tid == 0) a.out[g] = (double)NAN;
    return;
  }
  double* key = sr_lds;
  int* ix = (int*)(sr_lds + npad_max);
  if (!PRE) {
    int npad = 64;
    while (npad < L) npad <<= 1;                  // <= npad_max (a power of two >= L)
    for (int i = tid; i < npad; i += SR_THREADS) {
      double s = -INFINITY;
      if (i < L) {
        const long long pr = a.perm[r0 + i];
        s = (pr >= 0 && pr < a.n_rows) ? a.scores[pr] : (double)NAN;
        if (s != s) *a.nan_flag = 1;
      }
      key[i] = s;
      ix[i] = i;
    }
    __syncthreads();
    for (int k = 2; k <= npad; k <<= 1) {
      for (int j = k >> 1; j > 0; j >>= 1) {
        for (int t = tid; t < npad / 2; t += SR_THREADS) {
          const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), q = i | j;
          const bool up = (i & k) == 0;
          const double si = key[i], sq = key[q];
          const int ii = ix[i], iq = ix[q];
          if (sr_before(si, ii, sq, iq) != up) {
            key[i] = sq; key[q] = si;
            ix[i] = iq; ix[q] = ii;
          }
        }
        __syncthreads();
      }
    }
  }
  if (METRIC == SR_PREC) {
    const long long kk = a.k < L ? a.k : L;
    int hit = 0;
    for (long long pos = tid; pos < (PRE ? L : kk); pos += SR_THREADS) {
      if (PRE) {
        const double s = a.scores[r0 + pos];
        if (s != s) *a.nan_flag = 1;
        if (pos < kk) hit += a.flag[r0 + pos] != 0;
      } else {
        const int li = ix[pos];
        if (li < L) hit += a.flag[r0 + li] != 0;  // a padding row can only come this far up after a NaN
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) hit += __shfl_xor(hit, o, 64);
    if (lane == 0) w_hit[wv] = hit;
    __syncthreads();
    if (tid == 0) a.out[g] = (double)(w_hit[0] + w_hit[1] + w_hit[2] + w_hit[3]) / (double)a.k;
    return;
  }
  double TP = 0.0, TN = 0.0, RAW = 0.0, ogp = 0.0, ogn = 0.0, ohP = 0.0, ohN = 0.0;
  for (long long c0 = 0; c0 < L; c0 += SR_THREADS) {
    const long long pos = c0 + tid;
    const bool valid = pos < L;
    double p = 0.0, n = 0.0;
    bool f = false, tail = false;
    if (valid) {
      double s, sp = 0.0, sn = 0.0, w = 0.0;
      bool fl = false;
      if (PRE) {
        s = a.scores[r0 + pos];
        if (s != s) *a.nan_flag = 1;
        if (pos > 0) sp = a.scores[r0 + pos - 1];
        if (pos + 1 < L) sn = a.scores[r0 + pos + 1];
        w = a.wts[r0 + pos];
        fl = a.flag[r0 + pos] != 0;
      } else {
        s = key[pos];
        if (pos > 0) sp = key[pos - 1];
        if (pos + 1 < L) sn = key[pos + 1];
        const int li = ix[pos];
        if (li < L) {
          w = a.wts[r0 + li];
          fl = a.flag[r0 + li] != 0;
        }
      }
      p = fl ? w : 0.0;
      n = w - p;
      f = pos == 0 || s != sp;
      tail = pos == L - 1 || s != sn;
    }
    const bool f0 = f;
    double gp = p, gn = n, P = p, N = n;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const double tgp = __shfl_up(gp, d, 64), tgn = __shfl_up(gn, d, 64), tP = __shfl_up(P, d, 64);
      const double tN = METRIC == SR_AUPR ? __shfl_up(N, d, 64) : 0.0;
      const int tf = __shfl_up((int)f, d, 64);
      if (lane >= d) {
        P += tP;
        if (METRIC == SR_AUPR) N += tN;
        if (!f) { gp += tgp; gn += tgn; f = tf != 0; }
      }
    }
    double hP = 0.0, hN = 0.0;                    // AUPR: the wave-local prefixes before the lane's tie-group head
    if (METRIC == SR_AUPR) {
      double eP = __shfl_up(P, 1, 64), eN = __shfl_up(N, 1, 64);
      if (lane == 0) { eP = 0.0; eN = 0.0; }
      sr_head_prefix(f0, lane, eP, eN, hP, hN);
    } else {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) N += __shfl_xor(N, o, 64);
    }
    if (lane == 63) {                             // N: the wave's total either way (AUPR: its inclusive scan)
      w_f[wv] = f; w_gp[wv] = gp; w_gn[wv] = gn; w_P[wv] = P; w_N[wv] = N;
      if (METRIC == SR_AUPR) { w_hP[wv] = hP; w_hN[wv] = hN; }
    }
    __syncthreads();
    double cp = ogp, cn = ogn, Pb = TP;           // what the waves (and chunks) before this one leave open
    double Nb = TN, chP = ohP, chN = ohN;
    for (int v = 0; v < wv; ++v) {
      if (w_f[v]) {
        cp = w_gp[v]; cn = w_gn[v];
        if (METRIC == SR_AUPR) { chP = Pb + w_hP[v]; chN = Nb + w_hN[v]; }
      } else {
        cp += w_gp[v]; cn += w_gn[v];
      }
      Pb += w_P[v];
      if (METRIC == SR_AUPR) Nb += w_N[v];
    }
    if (!f) { gp += cp; gn += cn; }
    P += Pb;
    double raw;
    if (METRIC == SR_AUPR) {
      if (f) { hP += Pb; hN += Nb; } else { hP = chP; hN = chN; }
      N += Nb;
      raw = tail ? sr_aupr_term(gp, P, N, hP, hN) : 0.0;
    } else {
      raw = tail ? (P - gp) * gn + gp * gn / 2.0 : 0.0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) raw += __shfl_xor(raw, o, 64);
    if (lane == 0) w_raw[wv] = raw;
    __syncthreads();
    for (int v = 0; v < 4; ++v) {
      if (w_f[v]) {
        ogp = w_gp[v]; ogn = w_gn[v];
        if (METRIC == SR_AUPR) { ohP = TP + w_hP[v]; ohN = TN + w_hN[v]; }
      } else {
        ogp += w_gp[v]; ogn += w_gn[v];
      }
      TP += w_P[v];
      TN += w_N[v];
      RAW += w_raw[v];
    }
    __syncthreads();
  }
  if (tid == 0) {
    if (METRIC == SR_AUPR) a.out[g] = TP > 0.0 && TN > 0.0 ? RAW / TP : (double)NAN;
    else a.out[g] = RAW / (TP * TN);
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Global unweighted AUC counts of ONE sorted score stream (plain AUC under a process group: every rank evaluates the
// score bucket it received, evaluation/evaluators.py::auc_distributed). Input: n scores sorted non-increasing and n
// positive flags. Output, all int64: out[0] = sum over negative rows of (positives with a greater score) +
// (positives with a greater or equal score) = 2 * sum_tiegroups (P_before gn + gp gn / 2), out[1] = positives,
// out[2] = negatives. Tie test ==. Every sum is an integer, so the result does not depend on any order: no float
// atomics, no atomics at all.
//   auc_count_kernel: one workgroup per run of AC_ROWS rows, 16 contiguous rows per thread (eight 16-byte score
//     loads and one 16-byte flag load). Rows are sorted, so the rows equal to the run's first / last score are exactly
//     its leading / trailing tie group, which may continue in the neighbouring runs; every other ("interior") tie group
//     closes here. For an interior negative row the two positive counts are the run-local prefix at its tie group's
//     start (exclusive) and end (inclusive); they reach a thread whose rows do not hold that start / end by a
//     last-valid max-scan and a first-valid min-scan over the threads. Summary per run (AC_SUMMARY int64 slots):
//     first and last score, positives / negatives of the leading and the trailing group, totals, the interior sum
//     and the interior negatives.
//   auc_count_combine_kernel: one workgroup, one thread per run: adds 2 * P_before * (interior negatives) per run and
//     closes the tie groups that span runs with prefix sums and running maxima over the runs (see the kernel).
// Range: n < 2^31 keeps P * N < 2^62 and every term in int64.
// ---------------------------------------------------------------------------------------------------------------
#define AC_THREADS 256
#define AC_T 16
#define AC_ROWS (AC_THREADS * AC_T)
#define AC_SUMMARY 10
#define AC_CTHREADS 512               // threads (= runs per round) of the combine workgroup

struct AucCountArgs {
  const double* scores;         // [n] sorted non-increasing, 16-byte aligned
  const unsigned char* flag;    // [n] positive flags, 16-byte aligned
  long long* summ;              // [n_blocks * AC_SUMMARY] workspace
  long long* out;               // [3]
  long long n, n_blocks;
};

__device__ __forceinline__ long long ac_block_sum(long long v, long long* red, int lane, int wv) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if (lane == 0) red[wv] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

__global__ __launch_bounds__(AC_THREADS) void auc_count_kernel(AucCountArgs a) {
  __shared__ double t_first[AC_THREADS], t_last[AC_THREADS];
  __shared__ long long red[4], w_cnt[4], w_s[4], w_e[4];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const long long r0 = (long long)blockIdx.x * AC_ROWS;
  if (r0 >= a.n) return;                                      // uniform: never with the launcher's grid
  const int nb = (int)((a.n - r0) < (long long)AC_ROWS ? (a.n - r0) : (long long)AC_ROWS);
  const int t0 = tid * AC_T;
  const int v = nb - t0 >= AC_T ? AC_T : (nb - t0 > 0 ? nb - t0 : 0);      // valid rows of this thread
  double s[AC_T];
  unsigned f = 0;                                             // bit j: row j is positive
  if (v == AC_T) {
    const double2* ps = reinterpret_cast<const double2*>(a.scores + r0 + t0);
#pragma unroll
    for (int j = 0; j < AC_T / 2; ++j) {
      const double2 d = ps[j];
      s[2 * j] = d.x;
      s[2 * j + 1] = d.y;
    }
    const uint4 q = *reinterpret_cast<const uint4*>(a.flag + r0 + t0);
    const unsigned qw[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int j = 0; j < AC_T; ++j) f |= (((qw[j >> 2] >> (8 * (j & 3))) & 0xffu) != 0u ? 1u : 0u) << j;
  } else {
#pragma unroll
    for (int j = 0; j < AC_T; ++j) {
      s[j] = 0.0;
      if (j < v) {
        s[j] = a.scores[r0 + t0 + j];
        f |= (a.flag[r0 + t0 + j] != 0 ? 1u : 0u) << j;
      }
    }
  }
  double sl = s[0];                                           // this thread's last valid score
#pragma unroll
  for (int j = 1; j < AC_T; ++j) sl = j < v ? s[j] : sl;
  t_first[tid] = s[0];
  t_last[tid] = sl;
  // run-local exclusive prefix of the positives over the threads
  const int pc = __popc(f);
  int inc = pc;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int t = __shfl_up(inc, d, 64);
    if (lane >= d) inc += t;
  }
  if (lane == 63) w_cnt[wv] = inc;
  __syncthreads();
  int base = inc - pc, tot_p = 0;
  for (int w = 0; w < 4; ++w) {
    if (w < wv) base += (int)w_cnt[w];
    tot_p += (int)w_cnt[w];
  }
  const double bfirst = t_first[0], blast = t_last[(nb - 1) / AC_T];
  const double s_prev = t_last[tid > 0 ? tid - 1 : 0], s_next = t_first[tid < AC_THREADS - 1 ? tid + 1 : tid];
  // tie-group starts / ends among this thread's rows: positives before its LAST start, positives through its FIRST end
  unsigned st = 0, en = 0;
#pragma unroll
  for (int j = 0; j < AC_T; ++j) {
    if (j < v) {
      const bool sj = j == 0 ? (tid == 0 || s[0] != s_prev) : s[j] != s[j - 1];
      const double nx = j == v - 1 ? s_next : s[(j + 1) % AC_T];          // j == AC_T - 1 implies j == v - 1
      const bool ej = t0 + j == nb - 1 || s[j] != nx;
      st |= (sj ? 1u : 0u) << j;
      en |= (ej ? 1u : 0u) << j;
    }
  }
  long long ks = 0, ke = 0x7fffffffffffffffLL;
  if (st) {
    const int j = 31 - __clz((int)st);
    ks = ((long long)(tid + 1) << 32) | (long long)(base + __popc(f & ((1u << j) - 1u)));
  }
  if (en) {
    const int j = __ffs((int)en) - 1;
    ke = ((long long)tid << 32) | (long long)(base + __popc(f & ((2u << j) - 1u)));
  }
  long long xs = ks, xe = ke;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const long long ts = __shfl_up(xs, d, 64), te = __shfl_down(xe, d, 64);
    if (lane >= d && ts > xs) xs = ts;
    if (lane + d < 64 && te < xe) xe = te;
  }
  if (lane == 63) w_s[wv] = xs;
  if (lane == 0) w_e[wv] = xe;
  long long cl = __shfl_up(xs, 1, 64), cr = __shfl_down(xe, 1, 64);
  if (lane == 0) cl = 0;
  if (lane == 63) cr = 0x7fffffffffffffffLL;
  __syncthreads();
  for (int w = 0; w < 4; ++w) {
    if (w < wv && w_s[w] > cl) cl = w_s[w];
    if (w > wv && w_e[w] < cr) cr = w_e[w];
  }
  // interior negatives: positives strictly before their tie group (forward) + through its end (backward)
  long long acc = 0;
  int lead_p = 0, lead_n = 0, trail_p = 0, trail_n = 0, int_n = 0;
  int cur = (int)(cl & 0xffffffffLL), cp = base;
#pragma unroll
  for (int j = 0; j < AC_T; ++j) {
    if (j < v) {
      const bool pos = (f >> j) & 1u, lead = s[j] == bfirst, trail = s[j] == blast;
      if ((st >> j) & 1u) cur = cp;
      if (!pos && !lead && !trail) { acc += cur; ++int_n; }
      lead_p += lead && pos;
      lead_n += lead && !pos;
      trail_p += trail && pos;
      trail_n += trail && !pos;
      cp += pos;
    }
  }
  cur = (int)(cr & 0xffffffffLL);                              // cp = inclusive prefix at the last valid row
#pragma unroll
  for (int j = AC_T - 1; j >= 0; --j) {
    if (j < v) {
      const bool pos = (f >> j) & 1u;
      if ((en >> j) & 1u) cur = cp;
      if (!pos && s[j] != bfirst && s[j] != blast) acc += cur;
      cp -= pos;
    }
  }
  const long long edges = ac_block_sum((long long)lead_p | ((long long)lead_n << 16) | ((long long)trail_p << 32)
                                       | ((long long)trail_n << 48), red, lane, wv);
  const long long inner = ac_block_sum(acc | ((long long)int_n << 40), red, lane, wv);
  if (tid == 0) {
    long long* o = a.summ + (long long)blockIdx.x * AC_SUMMARY;
    o[0] = __double_as_longlong(bfirst);
    o[1] = __double_as_longlong(blast);
    o[2] = edges & 0xffff;
    o[3] = (edges >> 16) & 0xffff;
    o[4] = (edges >> 32) & 0xffff;
    o[5] = (edges >> 48) & 0xffff;
    o[6] = tot_p;
    o[7] = nb - tot_p;
    o[8] = inner & ((1LL << 40) - 1);
    o[9] = inner >> 40;
  }
}

// Inclusive and exclusive scan of one int64 per thread over the AC_CTHREADS threads of the combine workgroup (MAX:
// running maximum with identity -1, else running sum); *total = the scan's last value.
template <bool MAX>
__device__ __forceinline__ long long ac_scan(long long v, long long* lds, int lane, int wv, long long* excl,
                                             long long* total) {
  const long long id = MAX ? -1LL : 0LL;
  long long x = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const long long t = __shfl_up(x, d, 64);
    if (lane >= d) x = MAX ? (t > x ? t : x) : x + t;
  }
  long long e = __shfl_up(x, 1, 64);
  if (lane == 0) e = id;
  __syncthreads();
  if (lane == 63) lds[wv] = x;
  __syncthreads();
  long long pre = id, tot = id;
  for (int w = 0; w < AC_CTHREADS / 64; ++w) {
    const long long t = lds[w];
    if (w < wv) pre = MAX ? (t > pre ? t : pre) : pre + t;
    tot = MAX ? (t > tot ? t : tot) : tot + t;
  }
  *excl = MAX ? (pre > e ? pre : e) : pre + e;
  *total = tot;
  return MAX ? (pre > x ? pre : x) : pre + x;
}

// The runs' edge tie groups form a sequence L_0 T_0 L_1 T_1 ... (leading / trailing group of every run; a run that is
// one tie group has only L). Neighbours with equal scores chain into one tie group; a chain with N negatives, P_head
// positives before it and P_tail positives through its end adds N (P_head + P_tail). Both P_head and the negatives
// before the chain are values AT the chain's head, and both are non-decreasing along the sequence, so "the value at
// the latest head" is a running maximum: two prefix sums and two max-scans over the runs, no serial walk. One thread
// per run, AC_CTHREADS runs per round, the scans' totals carried from round to round.
__global__ __launch_bounds__(AC_CTHREADS) void auc_count_combine_kernel(AucCountArgs a) {
  __shared__ long long lds[AC_CTHREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  long long acc = 0;
  long long carryP = 0, carryN = 0, carryHp = -1, carryHn = -1;
  for (long long b0 = 0; b0 < a.n_blocks; b0 += AC_CTHREADS) {
    const long long b = b0 + tid;
    const bool live = b < a.n_blocks;
    double first = 0.0, last = 0.0;
    long long q2 = 0, q3 = 0, q4 = 0, q5 = 0, tp = 0, tn = 0, q8 = 0, q9 = 0;
    bool hL = false, tT = false;
    if (live) {
      const long long* q = a.summ + b * AC_SUMMARY;
      first = __longlong_as_double(q[0]);
      last = __longlong_as_double(q[1]);
      q2 = q[2]; q3 = q[3]; q4 = q[4]; q5 = q[5]; tp = q[6]; tn = q[7]; q8 = q[8]; q9 = q[9];
      hL = b == 0 || first != __longlong_as_double(q[1 - AC_SUMMARY]);             // last score of the run before
      tT = b == a.n_blocks - 1 || last != __longlong_as_double(q[AC_SUMMARY]);       // first score of the next run
    }
    const bool single = first == last;                        // (idle threads: an empty single run, no head, no tail)
    const long long pL = single ? tp : q2, nL = single ? tn : q3, pT = single ? 0 : q4, nT = single ? 0 : q5;
    long long exP, totP, exN, totN;
    ac_scan<false>(tp, lds, lane, wv, &exP, &totP);
    ac_scan<false>(nL + nT, lds, lane, wv, &exN, &totN);
    const long long Pb = carryP + exP, Nb = carryN + exN;     // positives / edge negatives before this run
    // the run's latest head: T when the run has two groups, else L when it starts a chain
    const long long mHp = !live ? -1 : !single ? Pb + tp - pT : hL ? Pb : -1;
    const long long mHn = !live ? -1 : !single ? Nb + nL : hL ? Nb : -1;
    long long exHp, totHp, exHn, totHn;
    ac_scan<true>(mHp, lds, lane, wv, &exHp, &totHp);
    ac_scan<true>(mHn, lds, lane, wv, &exHn, &totHn);
    if (live) {
      const long long inHp = exHp > carryHp ? exHp : carryHp, inHn = exHn > carryHn ? exHn : carryHn;
      const long long HpL = hL ? Pb : inHp, HnL = hL ? Nb : inHn;
      long long HpT = HpL, HnT = HnL;
      if (!single) {
        acc += q8 + 2 * Pb * q9;                              // interior tie groups
        acc += (Nb + nL - HnL) * (HpL + Pb + pL);             // L closes a chain
        HpT = Pb + tp - pT;
        HnT = Nb + nL;
      }
      if (tT) acc += (Nb + nL + nT - HnT) * (HpT + Pb + tp);
    }
    carryP += totP;
    carryN += totN;
    carryHp = totHp > carryHp ? totHp : carryHp;
    carryHn = totHn > carryHn ? totHn : carryHn;
  }
  long long ex, tot;
  ac_scan<false>(acc, lds, lane, wv, &ex, &tot);
  if (tid == 0) {
    a.out[0] = tot;
    a.out[1] = carryP;
    a.out[2] = a.n - carryP;
  }
}

extern "C" {

const char* pml_build_id() { return pml_build_stamp + 13; }

int pml_auc_count_block_rows() { return AC_ROWS; }

// a->out[3] = (2 raw, positives, negatives) of a->n > 0 sorted rows; a->summ: a->n_blocks * AC_SUMMARY int64 of
// workspace, n_blocks = ceil(n / AC_ROWS). Both input streams must be 16-byte aligned.
int pml_auc_counts(const AucCountArgs* a, void* stream) {
  if (a->n <= 0) return -22;
  const long long blocks = (a->n + AC_ROWS - 1) / AC_ROWS;
  if (blocks != a->n_blocks || blocks > 0x7fffffffLL || a->n >= (1LL << 31)) return -22;
  if (((uintptr_t)a->scores & 15) || ((uintptr_t)a->flag & 15)) return -22;
  hipLaunchKernelGGL(auc_count_kernel, dim3((unsigned)blocks), dim3(AC_THREADS), 0, (hipStream_t)stream, *a);
  LAUNCH_CHECK();
  hipLaunchKernelGGL(auc_count_combine_kernel, dim3(1), dim3(AC_CTHREADS), 0, (hipStream_t)stream, *a);
  LAUNCH_CHECK();
  return 0;
}

// Per-group ranking metric of the groups a->list of one size class (cls 0: C16, 1: C64, 2: CWG, 3: LONG / pre-sorted)
// into a->out; metric: SR_PREC (k > 0), SR_AUC or SR_AUPR (k ignored). npad_max (CWG): a power of two >= the
// longest listed group, <= 4096.
int pml_seg_rank_metric(int cls, int metric, int k, const SegRankArgs* a, int npad_max, void* stream) {
  if (a->n_list <= 0) return 0;
  if (cls < 0 || cls > 3 || metric < SR_PREC || metric > SR_AUPR || (metric == SR_PREC ? k <= 0 : k < 0)) return -22;
  hipStream_t st = (hipStream_t)stream;
  SegRankArgs v = *a;
  v.k = k;
  const long long per = cls == 0 ? SR_THREADS / 16 : cls == 1 ? SR_THREADS / 64 : 1;
  const long long blocks = (v.n_list + per - 1) / per;
  if (blocks > 0x7fffffffLL) return -22;
  const dim3 grid((unsigned)blocks), blk(SR_THREADS);
#define SR_LAUNCH(KERNEL, A, LDS, ...)                                                                      \
  do {                                                                                                      \
    if (metric == SR_PREC) hipLaunchKernelGGL((KERNEL<A, SR_PREC>), grid, blk, LDS, st, __VA_ARGS__);       \
    else if (metric == SR_AUC) hipLaunchKernelGGL((KERNEL<A, SR_AUC>), grid, blk, LDS, st, __VA_ARGS__);    \
    else hipLaunchKernelGGL((KERNEL<A, SR_AUPR>), grid, blk, LDS, st, __VA_ARGS__);                         \
  } while (0)
  if (cls == 0) {
    SR_LAUNCH(seg_rank_wave_kernel, 16, 0, v);
  } else if (cls == 1) {
    SR_LAUNCH(seg_rank_wave_kernel, 64, 0, v);
  } else if (cls == 2) {
    if (npad_max < 64 || npad_max > SR_WG_MAX || (npad_max & (npad_max - 1))) return -22;
    const size_t lds = (size_t)npad_max * (sizeof(double) + sizeof(int));
    SR_LAUNCH(seg_rank_block_kernel, false, lds, v, npad_max);
  } else {
    SR_LAUNCH(seg_rank_block_kernel, true, 0, v, 0);
  }
#undef SR_LAUNCH
  LAUNCH_CHECK();
  return 0;
}

// The two metrics this entry point has always served: k = 0: AUC, k > 0: precision@k.
int pml_seg_rank_eval(int cls, int k, const SegRankArgs* a, int npad_max, void* stream) {
  if (k < 0) return -22;
  return pml_seg_rank_metric(cls, k ? SR_PREC : SR_AUC, k, a, npad_max, stream);
}

int pml_downsample(int f64, const void* y, const void* w0, const long long* rowid, long long n,
                   unsigned long long seed, double rate, int binary, void* w, void* stream) {
  if (n <= 0) return 0;
  const long long blocks = (n + 255) / 256;
  if (blocks > 0x7fffffffLL) return -22;
  if (f64)
    hipLaunchKernelGGL(downsample_kernel<double>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                       (const double*)y, (const double*)w0, rowid, n, seed, rate, binary, (double*)w);
  else
    hipLaunchKernelGGL(downsample_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                       (const float*)y, (const float*)w0, rowid, n, seed, rate, binary, (float*)w);
  LAUNCH_CHECK();
  return 0;
}

// pass 0: count, 1: write; vbytes = sizeof(value) (bf16 2, fp32 4, fp64 8)
int pml_tl_compact(int pass, int vbytes, const CmpArgs* a, void* stream) {
  if (a->nseg <= 0) return 0;
  const dim3 grid((unsigned)((a->nseg + 3) / 4)), blk(256);
  hipStream_t st = (hipStream_t)stream;
#define CMP_LAUNCH(VT)                                                              \
  do {                                                                              \
    if (pass) hipLaunchKernelGGL((tl_compact_kernel<VT, 1>), grid, blk, 0, st, *a); \
    else hipLaunchKernelGGL((tl_compact_kernel<VT, 0>), grid, blk, 0, st, *a);      \
  } while (0)
  if (vbytes == 2) CMP_LAUNCH(unsigned short);
  else if (vbytes == 4) CMP_LAUNCH(unsigned int);
  else if (vbytes == 8) CMP_LAUNCH(unsigned long long);
  else return -22;
#undef CMP_LAUNCH
  LAUNCH_CHECK();
  return 0;
}

int pml_spmm_rows(const long long* indptr, const int* col, const double* val, long long n_rows, const double* PT,
                  int k, double* Y, void* stream) {
  if (n_rows <= 0 || k <= 0) return 0;
  const long long blocks = (n_rows + 3) / 4;
  if (blocks > 0x7fffffffLL) return -22;
  hipLaunchKernelGGL(spmm_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, indptr, col, val,
                     n_rows, PT, k, Y);
  LAUNCH_CHECK();
  return 0;
}

int pml_score_rows(const long long* indptr, const int* col, const double* val, long long n_rows, const double* w,
                   const int* ent, const long long* eptr, const int* efeat, double* out, void* stream) {
  if (n_rows <= 0) return 0;
  const long long blocks = (n_rows + SCORE_ROWS_PER_BLOCK - 1) / SCORE_ROWS_PER_BLOCK;
  if (blocks > 0x7fffffffLL) return -22;
  if (ent) {
    hipLaunchKernelGGL(score_rows_kernel<true>, dim3((unsigned)blocks), dim3(SCORE_THREADS), 0, (hipStream_t)stream,
                       indptr, col, val, n_rows, w, ent, eptr, efeat, out);
  } else {
    hipLaunchKernelGGL(score_rows_kernel<false>, dim3((unsigned)blocks), dim3(SCORE_THREADS), 0,
                       (hipStream_t)stream, indptr, col, val, n_rows, w, ent, eptr, efeat, out);
  }
  LAUNCH_CHECK();
  return 0;
}


int pml_gemm_nt(int M, int N, int K, const double* A, int lda, const double* Bm, int ldb, double* C, int ldc,
                void* stream) {
  if (M <= 0 || N <= 0) return 0;
  if (K < 0) return -22;
  dim3 grid((N + GN_T - 1) / GN_T, (M + GN_T - 1) / GN_T);
  hipLaunchKernelGGL(gemm_nt_mfma_kernel, grid, dim3(256), 0, (hipStream_t)stream, M, N, K, A, lda, Bm, ldb, C, ldc);
  LAUNCH_CHECK();
  return 0;
}


static int g_seg_gram_s = 0;   // rows per scatter round of seg_gram_kernel (0: by LDS size; A/B: pml_seg_gram_set_s)
void pml_seg_gram_set_s(int s) { g_seg_gram_s = (s == 1 || s == 2 || s == 4 || s == 8) ? s : 0; }

// K [B, n, n] for the entities ents[B]; dmax = max projected columns of those entities (LDS image size); maxnnz = max
// non-zeros of one of those entities (> 0: stage the entries in LDS when they fit, see seg_gram_kernel STAGE).
int pml_seg_gram(int B, int n, int dmax, long long maxnnz, const long long* ents, const long long* row_ptr,
                 const long long* col_ptr, const long long* nip, const long long* pos, const double* val, double* K,
                 void* stream) {
  if (B <= 0) return 0;
  if (n < 1 || n > 192 || dmax < 0 || (size_t)dmax * sizeof(double) > 160 * 1024) return -22;
  // rows per scatter round: as many as keep the image <= 32 KB (>= 5 one-wave workgroups per CU)
  const size_t d8 = (size_t)std::max(dmax, 1) * sizeof(double);
  const int S = g_seg_gram_s > 0 ? g_seg_gram_s : (d8 * 8 <= 32768 ? 8 : d8 * 4 <= 32768 ? 4 : d8 * 2 <= 32768 ? 2 : 1);
  const size_t img = d8 * (size_t)S;
  const size_t stage = maxnnz > 0 ? (size_t)maxnnz * 10 + 8 + (size_t)(n + 1) * 4 + 16 : 0;
  const bool staged = maxnnz > 0 && img + stage <= 64 * 1024;
  const size_t lds = staged ? img + stage : img;
  if (lds > 160 * 1024) return -22;
  hipStream_t st = (hipStream_t)stream;
#define SEG_GRAM_LAUNCH(SS)                                                                                       \
  do {                                                                                                           \
    if (staged)                                                                                                  \
      hipLaunchKernelGGL((seg_gram_kernel<SS, true>), dim3((unsigned)B), dim3(64), lds, st, B, n, std::max(dmax, 1), \
                         ents, row_ptr, col_ptr, nip, pos, val, K);                                              \
    else                                                                                                         \
      hipLaunchKernelGGL((seg_gram_kernel<SS, false>), dim3((unsigned)B), dim3(64), lds, st, B, n, std::max(dmax, 1), \
                         ents, row_ptr, col_ptr, nip, pos, val, K);                                              \
  } while (0)
  if (S == 8) SEG_GRAM_LAUNCH(8);
  else if (S == 4) SEG_GRAM_LAUNCH(4);
  else if (S == 2) SEG_GRAM_LAUNCH(2);
  else SEG_GRAM_LAUNCH(1);
#undef SEG_GRAM_LAUNCH
  LAUNCH_CHECK();
  return 0;
}

// In-place Cholesky of K [B, n, n] (n <= 192); nv[b] = valid rows of problem b (the rest: identity); info[B].
int pml_batched_chol(int B, int n, const long long* nv, double* K, int* info, void* stream) {
  if (B <= 0) return 0;
  if (n < 1 || n > 192) return -22;
  const size_t lds = (size_t)n * (n + 1) / 2 * sizeof(double);
  hipLaunchKernelGGL(batched_chol_kernel, dim3((unsigned)B), dim3(64), lds, (hipStream_t)stream, B, n, nv, K, info);
  LAUNCH_CHECK();
  return 0;
}

// W (packed projected coefficients) of the entities ents[B] = X_e^T r over their rows; dmax = max projected columns
// of those entities (LDS per wave). Other entities' coefficients are left untouched.
// pos32: positions are int32 (else int64).
int pml_rs_primal(int B, int dmax, const long long* ents, const long long* row_ptr, const long long* col_ptr,
                  const long long* nip, const void* pos, const double* val, const double* r, double* W,
                  void* stream, int pos32) {
  if (B <= 0) return 0;
  if (dmax < 0 || (size_t)dmax * sizeof(double) > 64 * 1024) return -22;
  const size_t lds = (size_t)std::max(dmax, 1) * sizeof(double);
  if (pos32)
    hipLaunchKernelGGL(rs_primal_kernel<int>, dim3((unsigned)B), dim3(64), lds, (hipStream_t)stream, ents, row_ptr,
                       col_ptr, nip, (const int*)pos, val, r, W);
  else
    hipLaunchKernelGGL(rs_primal_kernel<long long>, dim3((unsigned)B), dim3(64), lds, (hipStream_t)stream, ents,
                       row_ptr, col_ptr, nip, (const long long*)pos, val, r, W);
  LAUNCH_CHECK();
  return 0;
}

// ---- FULL coefficient variances (var_normal_kernel, var_scale_gram_kernel, chol_colnorm_kernel) ----
int pml_var_mmax() { return VAR_MMAX; }

// LDS bytes of chol_colnorm_kernel for a class of order n (mode 1 adds the row scales and cursors)
long long pml_chol_colnorm_lds(int mode, int n) {
  return ((long long)n * (n + 1) / 2 + 64LL * n + (mode ? 2LL * n : 0)) * (long long)sizeof(double);
}

// A [B, n, n] = lam I + X_e^T diag(c) X_e for the entities ents[B] (d_e <= n <= VAR_MMAX); c per row of the CSR
int pml_var_normal(int B, int n, const long long* ents, const long long* row_ptr, const long long* col_ptr,
                   const long long* nip, const long long* pos, const double* val, const double* c, double lam,
                   double* A, void* stream) {
  if (B <= 0) return 0;
  if (n < 1 || n > VAR_MMAX) return -22;
  const size_t lds = ((size_t)n * (n + 1) / 2 + n) * sizeof(double) + (size_t)n * sizeof(int) + 8;
  if (lds > 160 * 1024) return -22;
  hipLaunchKernelGGL(var_normal_kernel, dim3((unsigned)B), dim3(64), lds, (hipStream_t)stream, B, n, ents, row_ptr,
                     col_ptr, nip, pos, val, c, lam, A);
  LAUNCH_CHECK();
  return 0;
}

// K [B, n, n] (seg_gram) -> lam I + diag(sqrt c) K diag(sqrt c) in place (n <= 192)
int pml_var_scale_gram(int B, int n, const long long* ents, const long long* row_ptr, const double* c, double lam,
                       double* K, void* stream) {
  if (B <= 0) return 0;
  if (n < 1 || n > 192) return -22;
  hipLaunchKernelGGL(var_scale_gram_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, B, n, ents, row_ptr,
                     c, lam, K);
  LAUNCH_CHECK();
  return 0;
}

// out[col_ptr[e] + j] = |G^-1 e_j|^2 (mode 0) or (1 - |G^-1 b_j|^2) / lam (mode 1) from the factors L [B, n, n]
int pml_chol_colnorm(int mode, int B, int n, const double* L, const long long* nv, const long long* ents,
                     const long long* row_ptr, const long long* col_ptr, const long long* nip, const long long* pos,
                     const double* val, const double* c, double lam, double* out, void* stream) {
  if (B <= 0) return 0;
  if (n < 1 || n > VAR_MMAX || (mode != 0 && mode != 1)) return -22;
  const long long lds = pml_chol_colnorm_lds(mode, n);
  if (lds > 160 * 1024) return -22;
  if (mode) {
    if (!(lam > 0.0)) return -22;
    hipLaunchKernelGGL(chol_colnorm_kernel<1>, dim3((unsigned)B), dim3(64), (size_t)lds, (hipStream_t)stream, B, n, L,
                       nv, ents, row_ptr, col_ptr, nip, pos, val, c, lam, out);
  } else {
    hipLaunchKernelGGL(chol_colnorm_kernel<0>, dim3((unsigned)B), dim3(64), (size_t)lds, (hipStream_t)stream, B, n, L,
                       nv, ents, row_ptr, col_ptr, nip, pos, val, c, lam, out);
  }
  LAUNCH_CHECK();
  return 0;
}

// ---- blocked FULL-variance route (VAR_MMAX < n <= VAR_BLOCKED_MMAX), one work-group per problem ----
int pml_var_blocked_mmax() { return VAR_BLOCKED_MMAX; }
int pml_var_blocked_dmax() { return VAR_BLOCKED_DMAX; }

static_assert(VB_WAVES == 8, "var_blk_gram_kernel scatters one image row per wave");

// A [B, n, n] (lower triangle) for the entities ents[B]: mode 0 primal lam I + X_e^T diag(c) X_e (d_e <= n), mode 1
// row space lam I + diag(s) X_e X_e^T diag(s) (n_e <= n, d_e <= dcap <= VAR_BLOCKED_DMAX)
int pml_var_blocked_assemble(int mode, int B, int n, int dcap, const long long* ents, const long long* row_ptr,
                             const long long* col_ptr, const long long* nip, const long long* pos, const double* val,
                             const double* c, double lam, double* A, void* stream) {
  if (B <= 0) return 0;
  if (n < 1 || n > VAR_BLOCKED_MMAX || (mode != 0 && mode != 1)) return -22;
  if (mode == 0) {
    const size_t lds = (size_t)VB_WAVES * (n + (n + 1) / 2) * sizeof(double);
    hipLaunchKernelGGL(var_blk_normal_kernel, dim3((unsigned)B), dim3(VB_THREADS), lds, (hipStream_t)stream, B, n, ents,
                       row_ptr, col_ptr, nip, pos, val, c, lam, A);
  } else {
    if (dcap < 1 || dcap > VAR_BLOCKED_DMAX) return -22;
    const size_t lds = (size_t)dcap * 8 * sizeof(double);
    hipLaunchKernelGGL(var_blk_gram_kernel, dim3((unsigned)B), dim3(VB_THREADS), lds, (hipStream_t)stream, B, n, dcap,
                       ents, row_ptr, col_ptr, nip, pos, val, c, lam, A);
  }
  LAUNCH_CHECK();
  return 0;
}

// In-place Cholesky of K [B, n, n] (n <= VAR_BLOCKED_MMAX; lower triangle read); nv / info as pml_batched_chol
int pml_blocked_chol(int B, int n, const long long* nv, double* K, int* info, void* stream) {
  if (B <= 0) return 0;
  if (n < 1 || n > VAR_BLOCKED_MMAX) return -22;
  const size_t lds = ((size_t)VB_T * vb_ld(n) + VB_T * 17 + VB_T * VB_T + VB_WAVES * 256) * sizeof(double) + 16;
  if (lds > 160 * 1024) return -22;
  hipLaunchKernelGGL(blocked_chol_kernel, dim3((unsigned)B), dim3(VB_THREADS), lds, (hipStream_t)stream, B, n, nv, K,
                     info);
  LAUNCH_CHECK();
  return 0;
}

// out[col_ptr[e] + j] from the factors L [B, n, n] of pml_blocked_chol: L becomes G^-1 in place, then mode 0
// |G^-1 e_j|^2, mode 1 (1 - |G^-1 b_j|^2) / lam (d_e <= dcap <= VAR_BLOCKED_DMAX)
int pml_var_blocked_colnorm(int mode, int B, int n, int dcap, double* L, const long long* nv, const long long* ents,
                            const long long* row_ptr, const long long* col_ptr, const long long* nip,
                            const long long* pos, const double* val, const double* c, double lam, double* out,
                            void* stream) {
  if (B <= 0) return 0;
  if (n < 1 || n > VAR_BLOCKED_MMAX || (mode != 0 && mode != 1)) return -22;
  if (mode && (!(lam > 0.0) || dcap < 1 || dcap > VAR_BLOCKED_DMAX)) return -22;
  const size_t lds_t = ((size_t)VB_T * vb_ld(n) + VB_T * 17 + VB_T * VB_T) * sizeof(double);
  hipLaunchKernelGGL(blocked_trinv_kernel, dim3((unsigned)B), dim3(VB_THREADS), lds_t, (hipStream_t)stream, B, n, nv, L);
  LAUNCH_CHECK();
  if (mode) {
    const size_t lds = ((size_t)VB_WAVES * dcap + n) * sizeof(double) + (size_t)(n + 2) * sizeof(int);
    if (lds > 160 * 1024) return -22;
    hipLaunchKernelGGL(var_blk_colnorm_kernel<1>, dim3((unsigned)B), dim3(VB_THREADS), lds, (hipStream_t)stream, B, n,
                       dcap, L, nv, ents, row_ptr, col_ptr, nip, pos, val, c, lam, out);
  } else {
    hipLaunchKernelGGL(var_blk_colnorm_kernel<0>, dim3((unsigned)B), dim3(VB_THREADS), 0, (hipStream_t)stream, B, n, 1,
                       L, nv, ents, row_ptr, col_ptr, nip, pos, val, c, lam, out);
  }
  LAUNCH_CHECK();
  return 0;
}

// counts[nbins] += histogram of keys[n] (int32 if k32 else int64); counts must be zeroed by the caller
int pml_key_hist(int k32, const void* keys, long long n, long long nbins, unsigned long long* counts, void* stream) {
  if (n <= 0) return 0;
  const long long per_block = 1 << 16;
  const long long blocks = (n + per_block - 1) / per_block;
  if (blocks > 0x7fffffffLL) return -22;
  if (k32)
    hipLaunchKernelGGL(key_hist_kernel<int>, dim3((unsigned)blocks), dim3(HIST_THREADS), 0, (hipStream_t)stream,
                       (const int*)keys, n, per_block, nbins, counts);
  else
    hipLaunchKernelGGL(key_hist_kernel<long long>, dim3((unsigned)blocks), dim3(HIST_THREADS), 0,
                       (hipStream_t)stream, (const long long*)keys, n, per_block, nbins, counts);
  LAUNCH_CHECK();
  return 0;
}

// out (col as int16 if c16 else int64, val fp64) = rows[nr] of (nip, pos, val) at optr, minus cbase (may be null)
int pml_csr_gather_rows(int c16, const long long* nip, const long long* pos, const double* val, const long long* rows,
                        long long nr, const long long* optr, const long long* cbase, void* ocol, double* oval,
                        void* stream) {
  if (nr <= 0) return 0;
  const long long blocks = (nr + 3) / 4;
  if (blocks > 0x7fffffffLL) return -22;
  if (c16)
    hipLaunchKernelGGL(csr_gather_rows_kernel<short>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, nip,
                       pos, val, rows, nr, optr, cbase, (short*)ocol, oval);
  else
    hipLaunchKernelGGL(csr_gather_rows_kernel<long long>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                       nip, pos, val, rows, nr, optr, cbase, (long long*)ocol, oval);
  LAUNCH_CHECK();
  return 0;
}

// m[r] = sum_k val[k] mu[pos[k]] over row r of (nip, pos, val), then val[k] *= sigma[pos[k]] in place
int pml_prior_fold(const long long* nip, const long long* pos, double* val, long long n_rows, const double* mu,
                   const double* sigma, double* m, void* stream) {
  if (n_rows <= 0) return 0;
  const long long blocks = (n_rows + FOLD_ROWS_PER_BLOCK - 1) / FOLD_ROWS_PER_BLOCK;
  if (blocks > 0x7fffffffLL) return -22;
  hipLaunchKernelGGL(prior_fold_kernel, dim3((unsigned)blocks), dim3(FOLD_THREADS), 0, (hipStream_t)stream, nip, pos,
                     val, n_rows, mu, sigma, m);
  LAUNCH_CHECK();
  return 0;
}

}  // extern "C"

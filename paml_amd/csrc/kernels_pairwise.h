// kernels_pairwise.h — pairwise maximum-likelihood dN / dS (codeml runmode = -2, Goldman & Yang 1994) on the device (gfx950), FP64.
//
// The reference (PairwiseCodon codeml.c:4344-4604) takes the ns (ns - 1) / 2 pairs one after another; each is a 3-parameter search whose
// every function call (lfun2dSdN codeml.c:4219-4264) decomposes a 61 x 61 rate matrix on one core.  Pairs, and the finite-difference and
// line-search points of every pair, are independent: here they are the ELEMENTS (pair, t, kappa, omega) of one batch.
//
//   pair_count_kernel   the table fp[max(za, zb)][min(za, zb)] += w_h of a pair (codeml.c:4407-4413) from the tips resident in the engine,
//                       one workgroup per pair, an n x n FP64 histogram in LDS (61 x 61 x 8 B = 29.8 KB) filled with LDS atomics and written
//                       once; ls_pair = sum of the weights.  The reference accumulates fp in `float`: with integer weights (what pattern
//                       compression produces) every partial sum is an integer, exact in float below 2^24 and exact in double — the two
//                       tables are then equal, in whatever order the atomics land.
//   pair_q_kernel       the rate matrix of a (pair, kappa, omega): the elements a codon matrix can have (positions at and below the diagonal,
//                       each flagged transition / nonsynonymous: the table the host's sparse hand-over uses) times pi of the pair, the diagonal
//                       from the row sums, and the mean rate the roots are divided by (eigenQcodon codeml.c:3229-3316) — in the layout
//                       eigen_qrev_kernel reads (eigen_kernels.h), which then decomposes it into the pair set's arena.
//   pair_lnl_kernel     one workgroup of four waves per element: P = (U o e^{t Root}) V on v_mfma_f64_16x16x4 (64-padded, V staged through
//                       LDS in the instruction's operand order, wave w the rows 16 w .. 16 w + 15 and only the column blocks at or left of
//                       the diagonal), then lnL = sum_{j >= k, fp > 0} fp[j][k] log(pi_j P_jk) with the reference's floor (f <= 0 -> 1e-70,
//                       codeml.c:4256-4260).  Every lane adds its terms in a fixed order, the lanes of a wave are combined by a butterfly,
//                       the four waves in order: an element's lnL has the same bits in whatever batch it is evaluated.
#pragma once
#include <hip/hip_runtime.h>

namespace paml_amd {

enum { PAIR_FLAG_TRANSITION = 1, PAIR_FLAG_NONSYN = 2 };

struct PairCountArgs {
   int n, n_patt, n_pairs;
   const unsigned char *z;      // [n_tips][n_patt] clean data: codes are states
   const double *w;             // [n_patt]
   const int *seq_a, *seq_b;    // [n_pairs]
   double *fp;                  // [n_pairs][n * n]
   double *ls;                  // [n_pairs]
};

__global__ __launch_bounds__(256) void pair_count_kernel(PairCountArgs a)
{
   __shared__ double sH[64 * 64];
   __shared__ double sRed[4];
   const int p = blockIdx.x, tid = threadIdx.x, n = a.n, nn = n * n;
   for (int i = tid; i < nn; i += 256) sH[i] = 0.0;
   __syncthreads();
   const unsigned char *za = a.z + (size_t)a.seq_a[p] * a.n_patt, *zb = a.z + (size_t)a.seq_b[p] * a.n_patt;
   double s = 0;
   for (int h = tid; h < a.n_patt; h += 256) {
      const int x = za[h], y = zb[h];
      const double w = a.w[h];
      if (x < n && y < n) {      // (clean data: always)
         atomicAdd(&sH[(x > y ? x : y) * n + (x > y ? y : x)], w);
         s += w;
      }
   }
   for (int off = 32; off; off >>= 1) s += __shfl_xor(s, off);
   if ((tid & 63) == 0) sRed[tid >> 6] = s;
   __syncthreads();
   for (int i = tid; i < nn; i += 256) a.fp[(size_t)p * nn + i] = sH[i];
   if (tid == 0) a.ls[p] = ((sRed[0] + sRed[1]) + sRed[2]) + sRed[3];
}

struct PairDecomp {      // what crosses PCIe per decomposition
   int pair, pad;
   double kappa, omega;
};
struct PairElem {
   int slot, pair;       // slot: the decomposition (of this chunk) the element uses
   double t;
};

struct PairQArgs {
   int n, nnz;
   const int *rc;                // [nnz][2] row >= col (the diagonal's positions included: their values are the row sums)
   const unsigned char *flags;   // [nnz]
   const double *pi;             // [n_pairs][n]
   const PairDecomp *dec;        // [n_slots]
   double *vals;                 // out [n_slots][nnz]: the elements eigen_qrev_kernel reads
   double *pi_slot;              // out [n_slots][n]
   double *scale;                // out [n_slots]
};

__global__ __launch_bounds__(256) void pair_q_kernel(PairQArgs a)
{
   __shared__ double sPi[64], sRow[64], sVal[1024];
   const int slot = blockIdx.x, tid = threadIdx.x, n = a.n, nnz = a.nnz;
   const PairDecomp d = a.dec[slot];
   if (tid < 64) sPi[tid] = tid < n ? a.pi[(size_t)d.pair * n + tid] : 0.0;
   __syncthreads();
   // the exchangeability of every position (1, kappa, omega, kappa omega); the diagonal's is left at zero
   for (int k = tid; k < nnz; k += 256) {
      const int r = a.rc[2 * k], c = a.rc[2 * k + 1];
      const unsigned f = a.flags[k];
      sVal[k] = r == c ? 0.0 : ((f & PAIR_FLAG_TRANSITION) ? d.kappa : 1.0) * ((f & PAIR_FLAG_NONSYN) ? d.omega : 1.0);
   }
   __syncthreads();
   // row sums over the elements a row has on either side of the diagonal, in the order of the table: sum_j s_ij pi_j
   if (tid < n) {
      double s = 0;
      for (int k = 0; k < nnz; k++) {
         const int r = a.rc[2 * k], c = a.rc[2 * k + 1];
         if (r == c) continue;
         if (r == tid) s += sVal[k] * sPi[c];
         else if (c == tid) s += sVal[k] * sPi[r];
      }
      sRow[tid] = s;
      a.pi_slot[(size_t)slot * n + tid] = sPi[tid];
   }
   __syncthreads();
   for (int k = tid; k < nnz; k += 256) {
      const int r = a.rc[2 * k], c = a.rc[2 * k + 1];
      a.vals[(size_t)slot * nnz + k] = r == c ? -sRow[r] : sVal[k] * sPi[c];      // Q[r][c] = s_rc pi_c
   }
   if (tid == 0) {
      double mr = 0;
      for (int i = 0; i < n; i++) mr += sPi[i] * sRow[i];
      a.scale[slot] = mr;      // one substitution per codon: Root = w / mr
   }
}

struct PairLnlArgs {
   int n;
   const PairElem *elem;         // [n_elem]
   const double *U, *V, *Root;   // the arena: slot s at U + s n n, V + s n n, Root + s n
   const double *pi;             // [n_pairs][n]
   const double *fp;             // [n_pairs][n * n]
   double *lnL;                  // [n_elem]
};

__global__ __launch_bounds__(256) void pair_lnl_kernel(PairLnlArgs a)
{
   typedef double pw_v4d __attribute__((ext_vector_type(4)));
   __shared__ double sV[64 * 64];      // B operands [k-block][column block][lane] = V[4 kb + (lane >> 4)][16 cb + (lane & 15)]
   __shared__ double sE[64], sPi[64], sRed[4];
   const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = a.n;
   const PairElem el = a.elem[blockIdx.x];
   const double *U = a.U + (size_t)el.slot * n * n, *V = a.V + (size_t)el.slot * n * n, *Root = a.Root + (size_t)el.slot * n;
   for (int idx = tid; idx < 4096; idx += 256) {
      const int ln = idx & 63, k = 4 * (idx >> 8) + (ln >> 4), j = 16 * ((idx >> 6) & 3) + (ln & 15);
      sV[idx] = (k < n && j < n) ? V[k * n + j] : 0.0;
   }
   if (tid < 64) {
      sE[tid] = tid < n ? exp(el.t * Root[tid]) : 0.0;
      sPi[tid] = tid < n ? a.pi[(size_t)el.pair * n + tid] : 0.0;
   }
   // this wave's A operands: U[16 wave + (lane & 15)][4 kb + (lane >> 4)], scaled below by e^{t Root_k}
   const int ai = 16 * wave + (lane & 15), kq = lane >> 4;
   double ua[16];
#pragma unroll
   for (int kb = 0; kb < 16; kb++) {
      const int k = 4 * kb + kq;
      ua[kb] = (ai < n && k < n) ? U[ai * n + k] : 0.0;
   }
   __syncthreads();
#pragma unroll
   for (int kb = 0; kb < 16; kb++) ua[kb] *= sE[4 * kb + kq];
   const double *fp = a.fp + (size_t)el.pair * n * n;
   double sum = 0;
   for (int cb = 0; cb <= wave; cb++) {      // (the column blocks right of the diagonal hold no j >= k)
      pw_v4d acc = {0, 0, 0, 0};
#pragma unroll
      for (int kb = 0; kb < 16; kb++) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(ua[kb], sV[(kb * 4 + cb) * 64 + lane], acc, 0, 0, 0);
      // accumulator element r of this lane = P[16 wave + 4 r + (lane >> 4)][16 cb + (lane & 15)]
      const int k = 16 * cb + (lane & 15);
#pragma unroll
      for (int r = 0; r < 4; r++) {
         const int j = 16 * wave + 4 * r + kq;
         if (j < n && k <= j) {
            const double c = fp[j * n + k];
            if (c > 0) {
               double f = sPi[j] * acc[r];
               if (f <= 0) f = 1e-70;
               sum += c * log(f);
            }
         }
      }
   }
   for (int off = 32; off; off >>= 1) sum += __shfl_xor(sum, off);
   if (lane == 0) sRed[wave] = sum;
   __syncthreads();
   if (tid == 0) a.lnL[blockIdx.x] = ((sRed[0] + sRed[1]) + sRed[2]) + sRed[3];
}

}  // namespace paml_amd

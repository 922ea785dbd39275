// The lnL of every nearest-neighbour-interchange (NNI) neighbour of the tree at the present branch lengths, in one call
// (paml_amd_nni_scores; what the reference's search, Perturbation treesub.c:4642 on NeighborNNI treespace.c:283, walks one tree after
// the other).
//
// A swap (v, s, x): v an internal node that is not the root, s a son of v, x a son of f = the father of v other than v.  The subtrees
// below s and x change places; each keeps the branch above it (length and label).  With the down partials L_u and the outer messages
// A_u of kernels_gradient.h (M_u = P_u L_u), per gene, class k and pattern h:
//   L'_v   = M_x prod_{s' son of v, s' != s} M_s'                    the down partial of v in the rearranged tree (not rescaled)
//   H'_v   = A_f M_s prod_{x' son of f, x' != v, x' != x} M_x'       (f the root: A_f = pi; a root that is a tip: pi o its indicator)
//   f_hk   = sum_y H'_v(y) (P_v L'_v)(y)
// with the log factor sigma = SA_f + (SL of every subtree that was multiplied in).  The classes meet as the lnf row of grad_combine:
//   lnf[i][h] = log sum_k freqK_k e^{sigma_k - max_k sigma_k} f_hk + max_k sigma_k;    lnL[i] = sum_h w_h lnf[i][h]  (w_h > 0)
// Nothing outside the four subtrees around the edge (f, v) changes, so L and A of the present tree serve every swap: the down pass is
// the ancestral module's, the outer pass is the gradient's without the derivative (A_v = P_v^T H_v, rescaled by its maximum at every
// internal node of a tree with scaling nodes), and it also leaves f_hk of the present tree at the root's first son (lnL0, as the
// gradient takes it).  The swap pass needs no dP: per swap and class it is the sons' products of an ordinary node plus one with P_v.
//
// Products: 21..64 states (and 20 on a matrix-core engine) are sixteen patterns per wave on v_mfma_f64_16x16x4, a workgroup of four
// waves owning ANC_TILE patterns of one class and looping over the swaps (nni_mfma_kernel, shaped as grad_mfma_kernel); 4 / 5 / 20
// states are one pattern per lane (nni_lane_swap).  P_v^T in the A-operand order comes from nni_pt_kernel.
// Sums: a wave adds its 64 consecutive patterns (one chunk, counted from the gene's first pattern) in a fixed butterfly, then the
// rows' chunks are added in a fixed order (red_total256).  A (swap, pattern) is computed by itself: nothing depends on the batch the
// pattern falls in, on the group or the place of the swap in the list.  Ordinary vector stores only; no atomics.
//
// The per-lane bodies (nni_lane_*, nni_combine) are plain functions of (arguments, class or row, pattern): a host program calls them
// in a loop (NNI_HOST_ONLY: no HIP at all; tools/nni_host_check.cpp), which is how they are run under the host sanitizers.
#pragma once
#ifdef NNI_HOST_ONLY
#ifndef GRAD_HOST_ONLY
#define GRAD_HOST_ONLY
#endif
#include "kernels_gradient.h"
#define NNI_HD inline
#else
#include "kernels_gradient.h"
#define NNI_HD __host__ __device__ __forceinline__
#endif

namespace paml_amd {

struct NniArgs {
   AncMargArgs m;             // the tree, the batch, tips, P(t), pi, freqK; L / SL: the down pass; G / SG: the outer messages A_v and their log factors
   const double *PT;          // matrix cores: P_v^T, [pset][n_nodes][4096] in A-operand order (internal nodes)
   const int *swaps;          // [n_swaps][3] = v, s, x: the whole list
   int swap0, n_group, cap;   // the group of swaps in the workspace: first, count, rows of the workspace (row `cap`: the present tree)
   int n_swaps;               // the list's length
   double *f, *sig;           // [K][cap + 1][stride]: f_hk and its log factor
   const double *weights;     // [n_patt] (engine index)
   double *lnf;               // [cap + 1][stride]
   double *partial;           // [n_swaps + 1][n_chunks]: the chunks' sums of w lnf; row n_swaps: the present tree
   long chunk0, n_chunks;     // the batch's first chunk; chunks of the whole engine
   int ref_node;              // the root's first son: where the present tree's f_hk is taken
};

NNI_HD long nni_out_idx(const NniArgs &a, int k, int row, long p) { return ((long)k * (a.cap + 1) + row) * a.m.stride + p; }

// A_f, or pi (o the indicator of a root that is a tip), and its log factor
template <int N> NNI_HD void nni_lane_father(const AncMargArgs &m, int k, long p, int f, double (&h)[N], double *ls)
{
   const AncTree &t = m.t;
   if (f >= t.n_tips) {
      const int fi = f - t.n_tips;
      for (int c = 0; c < N; c++) h[c] = m.G[anc_idx(m, k, fi, c, p)];
      *ls = m.SG[((long)k * t.n_int + fi) * m.stride + p];
      return;
   }
   const double *pi = m.pi + (long)(m.n_pi > 1 ? m.gene : 0) * N;
   const unsigned long long mask = m.code_mask[m.z[(long)f * m.z_stride + m.h0 + p]];
   for (int c = 0; c < N; c++) h[c] = (mask >> c) & 1ull ? pi[c] : 0.0;
   *ls = 0;
}

// the outer pass of pattern p, class k, without the derivative (grad_lane_root / grad_lane_node): A_v and SA_v of every internal node,
// father first, then f_hk of the present tree at ref_node
template <int N> NNI_HD void nni_lane_outer(const NniArgs &a, int k, long p)
{
   const AncMargArgs &m = a.m;
   const AncTree &t = m.t;
   const long pset = (long)m.gene * m.K + k;
   if (t.root >= t.n_tips) {
      const double *pi = m.pi + (long)(m.n_pi > 1 ? m.gene : 0) * N;
      const int ri = t.root - t.n_tips;
      for (int c = 0; c < N; c++) m.G[anc_idx(m, k, ri, c, p)] = pi[c];
      m.SG[((long)k * t.n_int + ri) * m.stride + p] = 0;
   }
   for (int i = 0; i <= t.n_pre; i++) {
      const int v = i < t.n_pre ? t.pre[i] : a.ref_node;
      if (i == t.n_pre && v >= t.n_tips) break;      // (an internal ref_node was met in the walk)
      const int f = t.father[v];
      double h[N], ls;
      nni_lane_father<N>(m, k, p, f, h, &ls);
      for (int j = t.sons_ptr[f]; j < t.sons_ptr[f + 1]; j++)
         if (t.sons[j] != v) anc_lane_mul_son<N>(m, k, p, t.sons[j], h, &ls);
      const double *Pv = m.P + (pset * t.n_nodes + v) * (N * N);
      if (v == a.ref_node) {
         double x[N], y[N], sl = 0;
         if (v < t.n_tips) {
            const unsigned long long mask = m.code_mask[m.z[(long)v * m.z_stride + m.h0 + p]];
            for (int c = 0; c < N; c++) x[c] = (mask >> c) & 1ull ? 1.0 : 0.0;
         }
         else {
            for (int c = 0; c < N; c++) x[c] = m.L[anc_idx(m, k, v - t.n_tips, c, p)];
            sl = m.SL[((long)k * t.n_int + v - t.n_tips) * m.stride + p];
         }
         anc_lane_matvec<N>(Pv, x, y);
         double den = 0;
         for (int c = 0; c < N; c++) den += h[c] * y[c];
         const long oi = nni_out_idx(a, k, a.cap, p);
         a.f[oi] = den;
         a.sig[oi] = ls + sl;
      }
      if (v < t.n_tips) continue;
      const int vi = v - t.n_tips;
      double g[N];      // A_v = P_v^T H_v
      for (int c = 0; c < N; c++) {
         double s = 0;
         for (int r = 0; r < N; r++) s += h[r] * Pv[r * N + c];
         g[c] = s;
      }
      if (m.scaled) {
         double mx = 0;
         for (int c = 0; c < N; c++) mx = g[c] > mx ? g[c] : mx;
         if (mx > 0) {
            for (int c = 0; c < N; c++) g[c] /= mx;
            ls += log(mx);
         }
      }
      for (int c = 0; c < N; c++) m.G[anc_idx(m, k, vi, c, p)] = g[c];
      m.SG[((long)k * t.n_int + vi) * m.stride + p] = ls;
   }
}

// swap `swap` of the group (row of the workspace) at pattern p, class k: f_hk and its log factor
template <int N> NNI_HD void nni_lane_swap(const NniArgs &a, int k, long p, int swap)
{
   const AncMargArgs &m = a.m;
   const AncTree &t = m.t;
   const long pset = (long)m.gene * m.K + k;
   const int *sw = a.swaps + 3L * (a.swap0 + swap);
   const int v = sw[0], s = sw[1], x = sw[2], f = t.father[v];
   double h[N], ls;
   nni_lane_father<N>(m, k, p, f, h, &ls);
   anc_lane_mul_son<N>(m, k, p, s, h, &ls);
   for (int j = t.sons_ptr[f]; j < t.sons_ptr[f + 1]; j++)
      if (t.sons[j] != v && t.sons[j] != x) anc_lane_mul_son<N>(m, k, p, t.sons[j], h, &ls);
   double l[N], y[N];
   for (int c = 0; c < N; c++) l[c] = 1;
   anc_lane_mul_son<N>(m, k, p, x, l, &ls);
   for (int j = t.sons_ptr[v]; j < t.sons_ptr[v + 1]; j++)
      if (t.sons[j] != s) anc_lane_mul_son<N>(m, k, p, t.sons[j], l, &ls);
   anc_lane_matvec<N>(m.P + (pset * t.n_nodes + v) * (N * N), l, y);
   double fk = 0;
   for (int c = 0; c < N; c++) fk += h[c] * y[c];
   const long oi = nni_out_idx(a, k, swap, p);
   a.f[oi] = fk;
   a.sig[oi] = ls;
}

// the classes of row `row` of the workspace (cap: the present tree) at pattern p, as the lnf row of grad_combine: stores lnf, returns the
// pattern's term of the weighted sum
NNI_HD double nni_combine(const NniArgs &a, int row, long p)
{
   const AncMargArgs &m = a.m;
   const double w = a.weights[m.h0 + p];
   double smax = -1e300;
   for (int k = 0; k < m.K; k++) {
      const double s = a.sig[nni_out_idx(a, k, row, p)];
      smax = s > smax ? s : smax;
   }
   double den = 0;
   for (int k = 0; k < m.K; k++) {
      const long oi = nni_out_idx(a, k, row, p);
      den += m.freqK[k] * exp(a.sig[oi] - smax) * a.f[oi];
   }
   const double lf = log(den) + smax;
   a.lnf[(long)row * m.stride + p] = lf;
   return w > 0 ? w * lf : 0.0;
}

#ifndef NNI_HOST_ONLY
// ---- kernels: defined in engine_nni.hip, launched from any unit of the library ---------------------------------------------------

__global__ void nni_pt_kernel(const double *P, double *PT, int n, int n_nodes, int n_tips, int root);
__global__ void nni_pt_all_kernel(const double *P, double *PT, int n, int n_nodes, int root);
__global__ void nni_mfma_outer_kernel(NniArgs a);
__global__ void nni_mfma_kernel(NniArgs a);
__global__ void nni_combine_kernel(NniArgs a);

// one pattern per lane: grid (patterns / 256, K); pass 0: the down pass, 1: the outer pass (the placement call launches it too)
template <int N> __global__ __launch_bounds__(256) void nni_lane_kernel(NniArgs a, int pass)
{
   const long p = (long)blockIdx.x * 256 + threadIdx.x;
   if (p >= a.m.nb) return;
   if (pass) nni_lane_outer<N>(a, blockIdx.y, p);
   else anc_lane_down<N>(a.m, blockIdx.y, p);
}

// A_f of the pattern's lanes (pi o the indicator under a root that is a tip) and its log factor
__device__ __forceinline__ void nni_mfma_father(const AncMargArgs &m, int k, long g16, long pc, int lane, int q, int f, double (&h)[16], double *ls)
{
   const AncTree &t = m.t;
   if (f >= t.n_tips) {
      const int fi = f - t.n_tips;
      part_load(m.G + (((long)k * t.n_int + fi) * (m.stride >> 4) + g16) * 1024, lane, h);
      *ls = m.SG[((long)k * t.n_int + fi) * m.stride + pc];
      return;
   }
   const double *pi = m.pi + (long)(m.n_pi > 1 ? m.gene : 0) * m.n;
   const unsigned long long mask = m.code_mask[m.z[(long)f * m.z_stride + m.h0 + pc]];
#pragma unroll
   for (int j = 0; j < 16; j++) h[j] = (4 * j + q < m.n && ((mask >> (4 * j + q)) & 1ull)) ? pi[4 * j + q] : 0.0;
   *ls = 0;
}

// where a lane of the matrix-core row kernels stands (grid (stride / ANC_TILE, K), four waves): lane = q * 16 + pattern; k: the class;
// g16: the wave's group of sixteen patterns; p: the pattern in the batch; pc: the pattern read (lanes past the batch's end read the last
// pattern and write into the padding: p < stride); pset: the class's parameter set
struct ScoreTile {
   int lane, wave, q, k;
   long g16, p, pc, pset;
};
__device__ __forceinline__ ScoreTile score_tile(const AncMargArgs &m)
{
   ScoreTile c;
   c.lane = threadIdx.x & 63;
   c.wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
   c.q = c.lane >> 4;
   c.k = blockIdx.y;
   c.g16 = (long)blockIdx.x * 4 + c.wave;
   c.p = c.g16 * 16 + (c.lane & 15);
   c.pc = c.p < m.nb ? c.p : m.nb - 1;
   c.pset = (long)m.gene * m.K + c.k;
   return c;
}

// H_v = A_f prod_{sons of f other than v} M, f the father of v, and its log factor
__device__ __forceinline__ void score_mfma_hv(const AncMargArgs &m, const AncMfma &w, const ScoreTile &c, int v, double (&h)[16], double *ls)
{
   const AncTree &t = m.t;
   const int f = t.father[v];
   nni_mfma_father(m, c.k, c.g16, c.pc, c.lane, c.q, f, h, ls);
   for (int j = t.sons_ptr[f]; j < t.sons_ptr[f + 1]; j++)
      if (t.sons[j] != v) anc_mfma_mul_son(m, w, c.k, c.g16, c.pc, t.sons[j], h, ls);
}

// L_v of an internal node v, its log factor added to *ls
__device__ __forceinline__ void score_mfma_lv(const AncMargArgs &m, const ScoreTile &c, int v, double (&l)[16], double *ls)
{
   const long vi = (long)c.k * m.t.n_int + v - m.t.n_tips;
   part_load(m.L + (vi * (m.stride >> 4) + c.g16) * 1024, c.lane, l);
   *ls += m.SL[vi * m.stride + c.pc];
}

// The end of a combining kernel (grid (stride / 256, rows); a wave = one chunk of GRAD_CHUNK patterns): the wave's 64 terms added in a
// fixed butterfly, and whether this lane stores the sum (lane 0 of a wave that starts inside the batch) with the chunk's index
__device__ __forceinline__ double score_wave_sum(double acc)
{
#pragma unroll
   for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off);
   return acc;
}
__device__ __forceinline__ bool score_chunk_lane(const NniArgs &o, long p, long *chunk)
{
   *chunk = o.chunk0 + (p >> 6);
   return (threadIdx.x & 63) == 0 && (p & ~63L) < o.m.nb;
}

#endif

}  // namespace paml_amd

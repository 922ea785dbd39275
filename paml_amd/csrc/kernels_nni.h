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
// kernels_ancestral.h and kernels_gradient.h define their plain kernels wherever they are included and a __global__ function has one
// home: the copies of this translation unit get names of their own (as at the top of kernels_gradient.h)
#define anc_log_kernel nni_unit_anc_log_kernel
#define anc_posterior_kernel nni_unit_anc_posterior_kernel
#define anc_mfma_kernel nni_unit_anc_mfma_kernel
#define anc_joint_kernel nni_unit_anc_joint_kernel
#include "kernels_ancestral.h"
#undef anc_log_kernel
#undef anc_posterior_kernel
#undef anc_mfma_kernel
#undef anc_joint_kernel
#define grad_pmat_kernel nni_unit_grad_pmat_kernel
#define grad_mfma_kernel nni_unit_grad_mfma_kernel
#define grad_combine_kernel nni_unit_grad_combine_kernel
#define grad_total_kernel nni_unit_grad_total_kernel
#include "kernels_gradient.h"
#undef grad_pmat_kernel
#undef grad_mfma_kernel
#undef grad_combine_kernel
#undef grad_total_kernel
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
// ---- kernels ------------------------------------------------------------------------------------------------------------------------

// P_v^T of every (parameter set, internal node) in the A-operand order (the index formula of grad_pmat_kernel): grid (n_nodes, gene x class)
__global__ __launch_bounds__(256) void nni_pt_kernel(const double *P, double *PT, int n, int n_nodes, int n_tips, int root)
{
   const int node = blockIdx.x;
   if (node == root || node < n_tips) return;
   const long slot = (long)blockIdx.y * n_nodes + node;
   const double *Pv = P + slot * n * n;
   double *tf = PT + slot * 4096;
   for (int idx = threadIdx.x; idx < 4096; idx += 256) {
      const int e = idx & 1, lane = (idx >> 1) & 63, jb = (idx >> 7) & 3, kb2 = idx >> 9;
      const int r = jb * 16 + (lane & 15), c = 4 * (2 * kb2 + e) + (lane >> 4);
      tf[idx] = r < n && c < n ? Pv[c * n + r] : 0.0;
   }
}

// one pattern per lane: grid (patterns / 256, K); pass 0: the down pass, 1: the outer pass
template <int N> __global__ __launch_bounds__(256) void nni_lane_kernel(NniArgs a, int pass)
{
   const long p = (long)blockIdx.x * 256 + threadIdx.x;
   if (p >= a.m.nb) return;
   if (pass) nni_lane_outer<N>(a, blockIdx.y, p);
   else anc_lane_down<N>(a.m, blockIdx.y, p);
}

// one pattern per lane, the swap pass: grid (patterns / 256, K, swaps of the group)
template <int N> __global__ __launch_bounds__(256) void nni_lane_swap_kernel(NniArgs a)
{
   const long p = (long)blockIdx.x * 256 + threadIdx.x;
   if (p >= a.m.nb) return;
   nni_lane_swap<N>(a, blockIdx.y, p, blockIdx.z);
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

// Matrix cores, the outer pass without the derivative (grad_mfma_kernel's walk over the internal nodes, then ref_node when it is a tip):
// lane = q * 16 + pattern, register m = state 4 m + q.  Grid (stride / ANC_TILE, K).
__global__ __launch_bounds__(256) void nni_mfma_outer_kernel(NniArgs a)
{
   __shared__ __attribute__((aligned(16))) double sP[4096];
   const AncMargArgs &m = a.m;
   const AncTree &t = m.t;
   const int tid = threadIdx.x, lane = tid & 63, n = m.n;
   const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
   const int q = lane >> 4, k = blockIdx.y;
   const AncMfma w{sP, lane, wave, q};
   const long g16 = (long)blockIdx.x * 4 + wave, p = g16 * 16 + (lane & 15);
   const long pc = p < m.nb ? p : m.nb - 1;      // (lanes past the batch's end read the last pattern and write into the padding: p < stride)
   const long pset = (long)m.gene * m.K + k;
   if (t.root >= t.n_tips) {
      const double *pi = m.pi + (long)(m.n_pi > 1 ? m.gene : 0) * n;
      const int ri = t.root - t.n_tips;
      double x[16];
#pragma unroll
      for (int i = 0; i < 16; i++) x[i] = 4 * i + q < n ? pi[4 * i + q] : 0.0;
      part_store(m.G + (((long)k * t.n_int + ri) * (m.stride >> 4) + g16) * 1024, lane, x);
      if (q == 0) m.SG[((long)k * t.n_int + ri) * m.stride + p] = 0;
   }
   const int n_walk = t.n_pre + (a.ref_node < t.n_tips ? 1 : 0);
   for (int i = 0; i < n_walk; i++) {
      const int v = i < t.n_pre ? t.pre[i] : a.ref_node;
      const int f = t.father[v];
      double h[16], ls;
      __syncthreads();      // (SG of the father was stored by the pattern's q = 0 lane: a workgroup-scope fence before the other lanes read it)
      nni_mfma_father(m, k, g16, pc, lane, q, f, h, &ls);
      for (int j = t.sons_ptr[f]; j < t.sons_ptr[f + 1]; j++)
         if (t.sons[j] != v) anc_mfma_mul_son(m, w, k, g16, pc, t.sons[j], h, &ls);
      const long oi = nni_out_idx(a, k, a.cap, p);
      double x[16], y[16];
      if (v < t.n_tips) {      // ref_node, a tip: P_v L_v from the tip's column table
         double2 tv[8];
         tip_gather(m.ptip + pset * t.n_nodes * m.tip_words, m.tip_words, v, (int)m.z[(long)v * m.z_stride + m.h0 + pc], q, tv);
#pragma unroll
         for (int j = 0; j < 8; j++) { y[2 * j] = tv[j].x; y[2 * j + 1] = tv[j].y; }
         const double den = grad_mfma_dot(h, y);
         if (q == 0) { a.f[oi] = den; a.sig[oi] = ls; }
         continue;
      }
      const int vi = v - t.n_tips;
      v4d acc[4];
      w.product(a.PT + (pset * t.n_nodes + v) * 4096, h, acc);      // A_v = P_v^T H_v
#pragma unroll
      for (int j = 0; j < 16; j++) y[j] = acc[j >> 2][j & 3];
      if (v == a.ref_node) {      // (uniform over the workgroup) sum_x A_v(x) L_v(x) before A_v is rescaled, as grad_mfma_kernel
         part_load(m.L + (((long)k * t.n_int + vi) * (m.stride >> 4) + g16) * 1024, lane, x);
         const double den = grad_mfma_dot(y, x);
         if (q == 0) { a.f[oi] = den; a.sig[oi] = ls + m.SL[((long)k * t.n_int + vi) * m.stride + pc]; }
      }
      if (m.scaled) {
         const double mx = anc_mfma_max(y);
         if (mx > 0) {
#pragma unroll
            for (int j = 0; j < 16; j++) y[j] /= mx;
            ls += log(mx);
         }
      }
      part_store(m.G + (((long)k * t.n_int + vi) * (m.stride >> 4) + g16) * 1024, lane, y);
      if (q == 0) m.SG[((long)k * t.n_int + vi) * m.stride + p] = ls;
   }
}

// Matrix cores, the swap pass: four waves own ANC_TILE patterns of one class and loop over the group's swaps.  Grid (stride / ANC_TILE, K).
__global__ __launch_bounds__(256) void nni_mfma_kernel(NniArgs a)
{
   __shared__ __attribute__((aligned(16))) double sP[4096];
   const AncMargArgs &m = a.m;
   const AncTree &t = m.t;
   const int tid = threadIdx.x, lane = tid & 63, n = m.n;
   const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
   const int q = lane >> 4, k = blockIdx.y;
   const AncMfma w{sP, lane, wave, q};
   const long g16 = (long)blockIdx.x * 4 + wave, p = g16 * 16 + (lane & 15);
   const long pc = p < m.nb ? p : m.nb - 1;      // (lanes past the batch's end read the last pattern and write into the padding: p < stride)
   const long pset = (long)m.gene * m.K + k;
   for (int i = 0; i < a.n_group; i++) {
      const int *sw = a.swaps + 3L * (a.swap0 + i);
      const int v = sw[0], s = sw[1], x = sw[2], f = t.father[v];
      double h[16], l[16], ls;
      nni_mfma_father(m, k, g16, pc, lane, q, f, h, &ls);
      anc_mfma_mul_son(m, w, k, g16, pc, s, h, &ls);
      for (int j = t.sons_ptr[f]; j < t.sons_ptr[f + 1]; j++)
         if (t.sons[j] != v && t.sons[j] != x) anc_mfma_mul_son(m, w, k, g16, pc, t.sons[j], h, &ls);
#pragma unroll
      for (int j = 0; j < 16; j++) l[j] = 4 * j + q < n ? 1.0 : 0.0;
      anc_mfma_mul_son(m, w, k, g16, pc, x, l, &ls);
      for (int j = t.sons_ptr[v]; j < t.sons_ptr[v + 1]; j++)
         if (t.sons[j] != s) anc_mfma_mul_son(m, w, k, g16, pc, t.sons[j], l, &ls);
      v4d acc[4];
      w.product(m.pint + (pset * t.n_nodes + v) * 4096, l, acc);
      double y[16];
#pragma unroll
      for (int j = 0; j < 16; j++) y[j] = acc[j >> 2][j & 3];
      const double fk = grad_mfma_dot(h, y);
      const long oi = nni_out_idx(a, k, i, p);
      if (q == 0) { a.f[oi] = fk; a.sig[oi] = ls; }
   }
}

// the classes of every (row, pattern) and the chunks' sums: grid (stride / 256, rows); a wave = one chunk of GRAD_CHUNK patterns
__global__ __launch_bounds__(256) void nni_combine_kernel(NniArgs a)
{
   const long p = (long)blockIdx.x * 256 + threadIdx.x;
   const bool present = (int)blockIdx.y == a.n_group;      // (a batch's first group is launched with a row more: the present tree)
   const int row = present ? a.cap : (int)blockIdx.y;
   double acc = p < a.m.nb ? nni_combine(a, row, p) : 0.0;
#pragma unroll
   for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off);
   const long chunk = a.chunk0 + (p >> 6);
   const long out_row = present ? a.n_swaps : a.swap0 + row;
   if ((threadIdx.x & 63) == 0 && (p & ~63L) < a.m.nb) a.partial[out_row * a.n_chunks + chunk] = acc;
}
#endif

}  // namespace paml_amd

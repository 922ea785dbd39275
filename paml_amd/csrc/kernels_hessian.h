// The Hessian of lnL over all branch lengths, with lnL and the gradient, in one call (paml_amd_hessian): the cross second derivatives
// beside the diagonal of paml_amd_curvature.
//
// The definition extends those of kernels_gradient.h and kernels_curvature.h: the same down pass, the same outer pass with H_v, L_v, A_v
// at every node, f_k, d_vk, e_vk and their log factor sigma_vk.  Per gene, class k and pattern h, for a source branch u (not the root),
// D_u = dP_u L_u:
//   up the path      a_1 = father(u), a_2 = father(a_1), ... to the root:
//                    L'_{a_1} = D_u o prod_{siblings s of u} M_s;   L'_{a_{i+1}} = (P_{a_i} L'_{a_i}) o prod_{other sons s of a_{i+1}} M_s
//                    m_{u,a,k} = H_a . (dP_a L'_a)  for every path node a that is not the root; H_a and A_a of a path node are the
//                    present tree's (the subtree below u lies under every one of them)
//   outwards         w off the path and not below u, its father a on the path, c the son of a on the path (c = u when a = a_1):
//                    H'_w = A_a o M'_c o prod_{other siblings s of w} M_s,   M'_c = P_c L'_c (c = u: D_u)
//                    below such a w: A'_w = P_w^T H'_w;  H'_x = A'_w o prod_{siblings of x} M_s for the sons x of w
//                    m_{u,w,k} = H'_w . (dP_w L_w)  for every node w reached
//   entries          a pair with v below u is the pair (v, u) of the first step; of an unrelated pair the node with the smaller number is
//                    the source (hess_source_of, hessian_plan.h)
//                    Hess[u][v] = sum_h w_h ( sum_k freqK_k e^{sigma'_uvk} m_uvk / f_h - s_u(h) s_v(h) ),   f_h = e^{lnf[h]}
//                    Hess[v][v] = curv[v];  the root's row and column are 0;  a pattern with w_h = 0 contributes nothing
// Nothing is re-rooted and no reversibility is assumed.  The factors of a product are multiplied in son-list order.
// On a tree with scaling nodes L' and A' are divided by their largest magnitude where they are stored (their entries have either sign
// and may all be 0: then nothing is divided); sigma'_uvk = (the factor of the head A or A') + (SL of every subtree multiplied in) + (the
// logarithms L' and A' were divided by) is the term's own log factor, and the classes meet relative to the largest of them:
//   sum_k freqK_k e^{sigma'_k - max sigma'} m_k  x  e^{max sigma' - lnf[h]}
//
// The kernels walk, per source u, a list of steps the host made (hessian_plan.h): the products up the path, the outward chain over the
// nodes that lead to requested targets only, then per target one product and one dot product.  L' and A' of a source live in the call's
// workspace next to L and A, indexed as they are, and are written again by the next source.  D_v is formed again where it is used.
// Products: 21..64 states (and 20 on a matrix-core engine) are sixteen patterns per wave on v_mfma_f64_16x16x4, a workgroup of four
// waves owning ANC_TILE patterns of one class and looping over the group's sources (hess_mfma_kernel, shaped as spr_mfma_kernel); 4 / 5 /
// 20 states are one (pattern, class) per lane looping over the sources (hess_lane_source).
// Sums: hess_combine per (pair, pattern); a wave adds its 64 consecutive patterns (one chunk, counted from the gene's first pattern) in
// the gradient's fixed butterfly; hess_total_kernel adds a pair's chunks to its total one after the other in the order of the patterns,
// one lane per pair — the same additions for any batch size, any grouping of the sources and any list.  Ordinary vector stores only; no
// atomics.
//
// The per-lane bodies (hess_lane_source, hess_score, hess_combine) are plain functions of (arguments, class or row, pattern): a host
// program calls them in a loop (HESS_HOST_ONLY: no HIP at all; tools/hessian_host_check.cpp), which is how they are run under the host
// sanitizers.
#pragma once
#ifdef HESS_HOST_ONLY
#ifndef SPR_HOST_ONLY
#define SPR_HOST_ONLY
#endif
#include "kernels_spr.h"
#define HESS_HD inline
#else
#include "kernels_spr.h"
#define HESS_HD __host__ __device__ __forceinline__
#endif
#include "hessian_plan.h"

namespace paml_amd {

struct HessArgs {
   GradArgs g;                // the curvature's passes: g.m the tree, the batch, tips, P(t), L / SL, G / SG; dP, d2P, PT, num, den, cur, sig, lnf;
                              // g.scores [n_nodes][stride]: s_v(h), written by hess_score
   const int *sources;        // [n_sources][HESS_SOURCE_INTS], steps [n_steps][HESS_STEP_INTS], factors [n_factors][2], pairs [n_pairs][2] (hessian_plan.h)
   const int *steps, *factors, *pairs;
   int source0, n_sources;    // the group's sources
   int row0, n_group, cap;    // the group's first pair, its pairs, rows of the workspace
   double *Lp, *Ap;           // this source's L' and A', laid out as L and G
   double *SLp, *SAp;         // and their log factors, as SL and SG
   double *mm, *msig;         // [K][cap][stride]: m_uvk and its log factor
   double *part;              // [chunks of the batch][cap]: the chunks' sums of the group's pairs
   double *total;             // [n_pairs]
};

// bytes of the batch workspace per pattern: the curvature's, L' and A' with their log factors, the scores; and per row of the group
inline double hess_bytes_per_pattern(int K, int n_int, int n_nodes, int n_s) { return 4.0 * K * n_int * (n_s + 1) * 8 + 4.0 * K * n_nodes * 8 + 8.0 + 8.0 * n_nodes; }
inline double hess_bytes_per_row(int K) { return 2.0 * K * 8 + 8.0 / GRAD_CHUNK; }

HESS_HD long hess_out_idx(const HessArgs &a, int k, int row, long p) { return ((long)k * a.cap + row) * a.g.m.stride + p; }

// a message of either sign divided by its largest magnitude
template <int N> HESS_HD void hess_lane_rescale(const AncMargArgs &m, double (&x)[N], double *ls)
{
   if (!m.scaled) return;
   double mx = 0;
   for (int c = 0; c < N; c++) mx = fabs(x[c]) > mx ? fabs(x[c]) : mx;
   if (mx > 0) {
      for (int c = 0; c < N; c++) x[c] /= mx;
      *ls += log(mx);
   }
}

// source `is` of the list at pattern p, class k: its steps; m_uvk and its log factor of every target
template <int N> HESS_HD void hess_lane_source(const HessArgs &a, int k, long p, int is)
{
   const AncMargArgs &m = a.g.m;
   const AncTree &t = m.t;
   const long pset = (long)m.gene * m.K + k;
   const int *sr = a.sources + (long)HESS_SOURCE_INTS * is;
   for (int i = sr[1]; i < sr[1] + sr[2]; i++) {
      const int *st = a.steps + (long)HESS_STEP_INTS * i;
      const int op = st[0], node = st[1];
      double h[N], ls = 0;
      if (st[2] == HESS_HEAD_ONES)
         for (int c = 0; c < N; c++) h[c] = 1;
      else if (st[2] == HESS_HEAD_PRESENT) nni_lane_father<N>(m, k, p, st[3], h, &ls);
      else {
         const int fi = st[3] - t.n_tips;
         for (int c = 0; c < N; c++) h[c] = a.Ap[anc_idx(m, k, fi, c, p)];
         ls = a.SAp[((long)k * t.n_int + fi) * m.stride + p];
      }
      for (int j = st[4]; j < st[4] + st[5]; j++) {
         const int kind = a.factors[2 * j], s = a.factors[2 * j + 1];
         if (kind == HESS_FAC_PRESENT) spr_lane_mul<N>(m, m.P, m.L, m.SL, k, p, s, h, &ls);
         else if (kind == HESS_FAC_SOURCE) spr_lane_mul<N>(m, a.g.dP, m.L, m.SL, k, p, s, h, &ls);
         else spr_lane_mul<N>(m, m.P, a.Lp, a.SLp, k, p, s, h, &ls);
      }
      if (op == HESS_UP) {
         const int vi = node - t.n_tips;
         hess_lane_rescale<N>(m, h, &ls);
         for (int c = 0; c < N; c++) a.Lp[anc_idx(m, k, vi, c, p)] = h[c];
         a.SLp[((long)k * t.n_int + vi) * m.stride + p] = ls;
         continue;
      }
      if (op == HESS_OUT) {
         const int vi = node - t.n_tips;
         const double *Pt = m.P + (pset * t.n_nodes + node) * (N * N);
         double x[N];      // P^T H'
         for (int y = 0; y < N; y++) {
            double s = 0;
            for (int r = 0; r < N; r++) s += h[r] * Pt[r * N + y];
            x[y] = s;
         }
         hess_lane_rescale<N>(m, x, &ls);
         for (int c = 0; c < N; c++) a.Ap[anc_idx(m, k, vi, c, p)] = x[c];
         a.SAp[((long)k * t.n_int + vi) * m.stride + p] = ls;
         continue;
      }
      spr_lane_mul<N>(m, a.g.dP, st[6] ? a.Lp : m.L, st[6] ? a.SLp : m.SL, k, p, node, h, &ls);      // H' o (dP L)
      double mk = 0;
      for (int y = 0; y < N; y++) mk += h[y];
      const long oi = hess_out_idx(a, k, st[7] - a.row0, p);
      a.mm[oi] = mk;
      a.msig[oi] = ls;
   }
}

// s_v(h) of node v at pattern p by grad_combine's statements; stored (the root, a pattern of weight 0: 0)
HESS_HD void hess_score(const HessArgs &a, int v, long p)
{
   const GradArgs &g = a.g;
   const AncMargArgs &m = g.m;
   double s = 0;
   if (v != m.t.root && g.weights[m.h0 + p] > 0) {
      double smax = -1e300;
      for (int k = 0; k < m.K; k++) {
         const double x = g.sig[grad_out_idx(g, k, v, p)];
         smax = x > smax ? x : smax;
      }
      double num = 0, den = 0;
      for (int k = 0; k < m.K; k++) {
         const long oi = grad_out_idx(g, k, v, p);
         const double c = m.freqK[k] * exp(g.sig[oi] - smax);
         num += c * g.num[oi];
         den += c * g.den[oi];
      }
      s = num / den;
   }
   g.scores[(long)v * m.stride + p] = s;
}

// the classes of row `row` of the group at pattern p: the pattern's term of the pair's weighted sum
HESS_HD double hess_combine(const HessArgs &a, int row, long p)
{
   const AncMargArgs &m = a.g.m;
   const double w = a.g.weights[m.h0 + p];
   if (!(w > 0)) return 0;
   const int u = a.pairs[2 * (a.row0 + row)], v = a.pairs[2 * (a.row0 + row) + 1];
   double smax = -1e300;
   for (int k = 0; k < m.K; k++) {
      const double s = a.msig[hess_out_idx(a, k, row, p)];
      smax = s > smax ? s : smax;
   }
   double num = 0;
   for (int k = 0; k < m.K; k++) {
      const long oi = hess_out_idx(a, k, row, p);
      num += m.freqK[k] * exp(a.msig[oi] - smax) * a.mm[oi];
   }
   return w * (num * exp(smax - a.g.lnf[p]) - a.g.scores[(long)u * m.stride + p] * a.g.scores[(long)v * m.stride + p]);
}

#ifndef HESS_HOST_ONLY
// ---- kernels: defined in engine_hessian.hip ------------------------------------------------------------------------------------------

__global__ void hess_mfma_kernel(HessArgs a);
__global__ void hess_score_kernel(HessArgs a);
__global__ void hess_combine_kernel(HessArgs a);
__global__ void hess_total_kernel(HessArgs a, int n_chunks_batch);

// x *= dP_node X_node (a tip: the indicator of its code's set through the dP product; the tips have no column table of dP)
__device__ __forceinline__ void hess_mfma_mul_d(const AncMargArgs &m, const AncMfma &w, const double *dP, const double *Lb, const double *SLb, int k, long g16, long pc,
                                                int node, double (&x)[16], double *ls)
{
   const long pset = (long)m.gene * m.K + k;
   double xs[16];
   if (node < m.t.n_tips) {
      const unsigned long long mask = m.code_mask[m.z[(long)node * m.z_stride + m.h0 + pc]];
#pragma unroll
      for (int j = 0; j < 16; j++) xs[j] = (mask >> (4 * j + w.q)) & 1ull ? 1.0 : 0.0;
   }
   else {
      const int vi = node - m.t.n_tips;
      part_load(Lb + (((long)k * m.t.n_int + vi) * (m.stride >> 4) + g16) * 1024, w.lane, xs);
      *ls += SLb[((long)k * m.t.n_int + vi) * m.stride + pc];
   }
   v4d acc[4];
   w.product(dP + (pset * m.t.n_nodes + node) * 4096, xs, acc);
#pragma unroll
   for (int j = 0; j < 16; j++) x[j] *= acc[j >> 2][j & 3];
}

__device__ __forceinline__ void hess_mfma_rescale(const AncMargArgs &m, double (&x)[16], double *ls)
{
   if (!m.scaled) return;
   double mx = 0;
#pragma unroll
   for (int j = 0; j < 16; j++) mx = fabs(x[j]) > mx ? fabs(x[j]) : mx;
   double o = __shfl_xor(mx, 16);
   mx = o > mx ? o : mx;
   o = __shfl_xor(mx, 32);
   mx = o > mx ? o : mx;
   if (mx > 0) {
#pragma unroll
      for (int j = 0; j < 16; j++) x[j] /= mx;
      *ls += log(mx);
   }
}

#endif

}  // namespace paml_amd

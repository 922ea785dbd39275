// The lnL of every requested subtree-prune-and-regraft (SPR) neighbour of the tree at the present branch lengths, in one call
// (paml_amd_spr_scores).  paml_amd_placement_scores is the regraft half with a tip code hung on the branch; here the thing hung is a
// whole subtree and the rest of the tree is re-evaluated without it.
//
// A move is (s, x) with a split phi in [0, 1].  f = father(s), g = father(f), c = the other son of f.  It is valid when s is not the
// root; f is not the root and has exactly two sons; x is not the root, not f, not c (the same topology) and does not lie in the subtree
// below s (s included).
// The rearranged tree (Tree.spr(s, x, phi) in paml_amd/problem.py; node ids, n_nodes and the root stay):
//   1. c takes f's place in the son list of g; t'_c = t_c + t_f; c keeps its label.
//   2. f takes x's place in the son list of x's father; sons[f] = [x, s]; t'_f = (1 - phi) t_x, t'_x = phi t_x; label[f] = label[x];
//      s keeps t_s and its label.
// The tree's length is unchanged and node f travels with s.
// The scores.  T' is the tree after step 1; L_u, A_u, M_u = P_u L_u are the present tree's (kernels_gradient.h / kernels_nni.h); the
// path is g, father(g), ..., root.  Per gene, class k and pattern h:
//   merged branch    M'_c = P_{lambda_c}(t_c + t_f) L_c
//   up the path      L'_a = prod_{sons of a in T'} M'   (a son on the path: P_a' L'_a'; c: M'_c; every other son: its present M),
//                    for a = g and then upwards (L' of the root is not needed: no branch above it)
//   A_a of a path node is the present tree's (the subtree below s lies under every one of them), and so is H_a, the message arriving
//   at the top of a's branch
//   outwards         for every other node u of T':  H'_u = A'_{father'(u)} o prod_{siblings of u in T'} M'  (in son-list order);
//                    A'_u = P'_u^T H'_u for internal u (P'_c: the merged matrix)
//   target x         W = (P_{lambda_x}((1 - phi) t_x)^T H'_x) o (P_{lambda_x}(phi t_x) L'_x)
//                    f_hk = sum_y W(y) (P_s L_s)(y)
// with the log factor sigma = (that of the head A') + (SL of every subtree multiplied in) + (the factors L' and A' were rescaled by).
// The classes meet as in nni_combine:  lnf[i][h] = log sum_k freqK_k e^{sigma_k - max_k sigma_k} f_hk + max_k sigma_k;  lnL[i] = sum_h
// w_h lnf[i][h]  (w_h > 0).  Nothing is re-rooted and no reversibility is assumed: lnL[i] and lnf[i][h] are what paml_amd_eval returns for
// Tree.spr(s, x, phi) as rooted, to rounding (not to the bit, and without regard to where that tree's own scaling marks would sit).
// Only P(t) is used, so sets of every kind are served.
// Out of scope: a prune of the side of a branch that holds the root (it would reverse branches), and a prune whose father is the root or
// a polytomy.  The list of all valid moves therefore reaches a part of the 2 (n - 3)(2 n - 7) SPR neighbours of an unrooted binary
// tree of n tips, not all of them.
//
// L' of the path and the A' chain are rescaled by their maximum on a tree with scaling nodes, as the outer pass rescales A.
// The kernels walk, per pruned s, a list of steps the host made (spr_plan.h): the products up the path, the outward chain over the nodes
// that lead to requested targets only, then per target two products and one dot product; P_s L_s is formed once per s.  L' and A' of
// a prune live in the call's workspace next to L and A, indexed as they are, and are written again by the next s.
// Products: 21..64 states (and 20 on a matrix-core engine) are sixteen patterns per wave on v_mfma_f64_16x16x4, a workgroup of four
// waves owning ANC_TILE patterns of one class and looping over the group's prunes (spr_mfma_kernel, shaped as nni_mfma_kernel and
// place_mfma_kernel); 4 / 5 / 20 states are one (pattern, class) per lane looping over the prunes (spr_lane_prune).
// Sums: nni_combine and the chunks of kernels_nni.h.  A (move, pattern) is computed by the same sequence of operations whatever else is
// in the list: nothing depends on the batch, the group or the place of the move.  Ordinary vector stores only; no atomics.
//
// The per-lane bodies (spr_lane_prune, and nni_combine for the rows) are plain functions of (arguments, class or row, pattern): a host
// program calls them in a loop (SPR_HOST_ONLY: no HIP at all; tools/spr_host_check.cpp), which is how they are run under the host sanitizers.
#pragma once
#ifdef SPR_HOST_ONLY
#ifndef NNI_HOST_ONLY
#define NNI_HOST_ONLY
#endif
#include "kernels_nni.h"
#define SPR_HD inline
#else
#include "kernels_nni.h"
#define SPR_HD __host__ __device__ __forceinline__
#endif
#include "spr_plan.h"

namespace paml_amd {

struct SprArgs {
   NniArgs o;                 // the outer pass and the rows (swap0 / n_group / cap: the group's first row, rows, rows of the workspace; row `cap`:
                              // the present tree); o.m: the tree, the batch, tips, P(t) of the tree, L / SL, G / SG
   const double *Pup, *Pdn, *Pm;   // lanes: row-major [pset][n_nodes][n * n]: P_v((1 - phi) t_v), P_v(phi t_v), P_v(t_v + t_father(v))
   const double *PTup;        // matrix cores: P_v((1 - phi) t_v)^T, [pset][n_nodes][4096] in A-operand order (every node but the root)
   const double *pint_dn, *ptip_dn;   // matrix cores: P_v(phi t_v): [pset][n_nodes][4096] (internal nodes) and the tips' column tables
   const double *pint_m, *ptip_m;     // matrix cores: the merged matrices, likewise
   const double *PTm;         // matrix cores: the merged matrices transposed, as PTup
   const int *prunes;         // [n_prunes][SPR_PRUNE_INTS], steps [n_steps][SPR_STEP_INTS], factors [n_factors][2] (spr_plan.h)
   const int *steps, *factors;
   int prune0, n_prunes;      // the group's prunes
   double *Lp, *Ap;           // this prune's L' and A', laid out as L and G
   double *SLp, *SAp;         // and their log factors, as SL and SG
};

// x *= P L of `node` with the given matrices and partials (a tip: the indicator of its code's set); the subtree's log factors are added
// to *ls (anc_lane_mul_son with the operands named)
template <int N> SPR_HD void spr_lane_mul(const AncMargArgs &m, const double *P, const double *Lb, const double *SLb, int k, long p, int node, double (&x)[N], double *ls)
{
   const long pset = (long)m.gene * m.K + k;
   const double *Ps = P + (pset * m.t.n_nodes + node) * (N * N);
   double y[N];
   if (node < m.t.n_tips) anc_lane_tip_msg<N>(Ps, m.code_mask[m.z[(long)node * m.z_stride + m.h0 + p]], y);
   else {
      double xs[N];
      const int vi = node - m.t.n_tips;
      for (int c = 0; c < N; c++) xs[c] = Lb[anc_idx(m, k, vi, c, p)];
      anc_lane_matvec<N>(Ps, xs, y);
      *ls += SLb[((long)k * m.t.n_int + vi) * m.stride + p];
   }
   for (int c = 0; c < N; c++) x[c] *= y[c];
}

// the outer pass's rescaling of a message
template <int N> SPR_HD void spr_lane_rescale(const AncMargArgs &m, double (&x)[N], double *ls)
{
   if (!m.scaled) return;
   double mx = 0;
   for (int c = 0; c < N; c++) mx = x[c] > mx ? x[c] : mx;
   if (mx > 0) {
      for (int c = 0; c < N; c++) x[c] /= mx;
      *ls += log(mx);
   }
}

// prune ip of the list at pattern p, class k: its steps; f_hk and its log factor of every target
template <int N> SPR_HD void spr_lane_prune(const SprArgs &a, int k, long p, int ip)
{
   const AncMargArgs &m = a.o.m;
   const AncTree &t = m.t;
   const long pset = (long)m.gene * m.K + k;
   const int *pr = a.prunes + (long)SPR_PRUNE_INTS * ip;
   double ms[N], ls_s = 0;      // P_s L_s, once per s
   for (int c = 0; c < N; c++) ms[c] = 1;
   spr_lane_mul<N>(m, m.P, m.L, m.SL, k, p, pr[0], ms, &ls_s);
   for (int is = pr[1]; is < pr[1] + pr[2]; is++) {
      const int *st = a.steps + (long)SPR_STEP_INTS * is;
      const int op = st[0], node = st[1];
      double h[N], ls = 0;
      if (st[2] == SPR_HEAD_ONES)
         for (int c = 0; c < N; c++) h[c] = 1;
      else if (st[2] == SPR_HEAD_PRESENT) nni_lane_father<N>(m, k, p, st[3], h, &ls);
      else {
         const int fi = st[3] - t.n_tips;
         for (int c = 0; c < N; c++) h[c] = a.Ap[anc_idx(m, k, fi, c, p)];
         ls = a.SAp[((long)k * t.n_int + fi) * m.stride + p];
      }
      for (int j = st[4]; j < st[4] + st[5]; j++) {
         const int kind = a.factors[2 * j], u = a.factors[2 * j + 1];
         if (kind == SPR_FAC_PRESENT) spr_lane_mul<N>(m, m.P, m.L, m.SL, k, p, u, h, &ls);
         else if (kind == SPR_FAC_MERGED) spr_lane_mul<N>(m, a.Pm, m.L, m.SL, k, p, u, h, &ls);
         else spr_lane_mul<N>(m, m.P, a.Lp, a.SLp, k, p, u, h, &ls);
      }
      const long slot = pset * t.n_nodes + node;
      if (op == SPR_UP) {
         const int vi = node - t.n_tips;
         spr_lane_rescale<N>(m, h, &ls);
         for (int c = 0; c < N; c++) a.Lp[anc_idx(m, k, vi, c, p)] = h[c];
         a.SLp[((long)k * t.n_int + vi) * m.stride + p] = ls;
         continue;
      }
      const double *Pt = (op == SPR_OUT ? (st[6] ? a.Pm : m.P) : a.Pup) + slot * (N * N);
      double u[N];      // P^T H'
      for (int y = 0; y < N; y++) {
         double s = 0;
         for (int x = 0; x < N; x++) s += h[x] * Pt[x * N + y];
         u[y] = s;
      }
      if (op == SPR_OUT) {
         const int vi = node - t.n_tips;
         spr_lane_rescale<N>(m, u, &ls);
         for (int c = 0; c < N; c++) a.Ap[anc_idx(m, k, vi, c, p)] = u[c];
         a.SAp[((long)k * t.n_int + vi) * m.stride + p] = ls;
         continue;
      }
      spr_lane_mul<N>(m, a.Pdn, st[6] ? a.Lp : m.L, st[6] ? a.SLp : m.SL, k, p, node, u, &ls);      // W
      double fk = 0;
      for (int y = 0; y < N; y++) fk += u[y] * ms[y];
      const long oi = nni_out_idx(a.o, k, st[7] - a.o.swap0, p);
      a.o.f[oi] = fk;
      a.o.sig[oi] = ls + ls_s;
   }
}

#ifndef SPR_HOST_ONLY
// ---- kernels: defined in engine_spr.hip --------------------------------------------------------------------------------------------

__global__ void spr_mfma_kernel(SprArgs a);

// x *= P L of `node` with the given matrices (A-operand blocks of internal nodes, column tables of tips) and partials
__device__ __forceinline__ void spr_mfma_mul(const AncMargArgs &m, const AncMfma &w, const double *pint, const double *ptip, const double *Lb, const double *SLb, int k,
                                             long g16, long pc, int node, double (&x)[16], double *ls)
{
   const long pset = (long)m.gene * m.K + k;
   if (node < m.t.n_tips) {
      double2 v[8];
      tip_gather(ptip + pset * m.t.n_nodes * m.tip_words, m.tip_words, node, (int)m.z[(long)node * m.z_stride + m.h0 + pc], w.q, v);
#pragma unroll
      for (int i = 0; i < 8; i++) { x[2 * i] *= v[i].x; x[2 * i + 1] *= v[i].y; }
   }
   else {
      const int vi = node - m.t.n_tips;
      double xs[16];
      part_load(Lb + (((long)k * m.t.n_int + vi) * (m.stride >> 4) + g16) * 1024, w.lane, xs);
      v4d acc[4];
      w.product(pint + (pset * m.t.n_nodes + node) * 4096, xs, acc);
#pragma unroll
      for (int j = 0; j < 16; j++) x[j] *= acc[j >> 2][j & 3];
      *ls += SLb[((long)k * m.t.n_int + vi) * m.stride + pc];
   }
}

__device__ __forceinline__ void spr_mfma_rescale(const AncMargArgs &m, double (&x)[16], double *ls)
{
   if (!m.scaled) return;
   const double mx = anc_mfma_max(x);
   if (mx > 0) {
#pragma unroll
      for (int j = 0; j < 16; j++) x[j] /= mx;
      *ls += log(mx);
   }
}

#endif

}  // namespace paml_amd

// The lnL of the tree with one more tip hung on branch e, for every query sequence, every branch e and every pendant length, in one call
// (paml_amd_placement_scores; the primitive under the reference's stepwise addition, StepwiseAddition treesub.c:4866 on AddSpecies
// treesub.c:4592, which sets and evaluates one enlarged tree after the other; also the regraft half of an SPR move and the placement of new
// sequences on a fitted tree).
//
// An edge is a node v != root: the branch above v, of length t_v and label lambda_v; f is its father.  Placing a query on edge v with
// split phi in [0, 1] and pendant length tau >= 0 makes a new internal node u between f and v: the branch above u has length (1 - phi) t_v,
// the branch above v has length phi t_v, both with label lambda_v, and u's second son is the query tip on a branch of length tau with
// label pendant_label.  With the down partials L_u and the outer messages A_u of kernels_gradient.h / kernels_nni.h (M_c = P_c L_c), per
// gene, class k and pattern h:
//   H_v  = A_f o prod_{c son of f, c != v} M_c            (f the root: A_f = pi; a root that is a tip: pi o its indicator)
//   U_v  = P_v((1 - phi) t_v)^T H_v
//   D_v  = P_v(phi t_v) L_v                               (a tip v: L_v is the indicator of its code's set)
//   W_v  = U_v o D_v
//   f_hk(q, v, tau) = sum_y W_v(y) T_tau[code_q(h)][y],   T_tau[c][y] = sum_{x in set(c)} P_{pendant_label}(tau)[y][x]
// with the log factor sigma = SA_f + (SL of every subtree that was multiplied in: the siblings' and v's own).  The classes meet as in
// nni_combine:  lnf[q][v][tau][h] = log sum_k freqK_k e^{sigma_k - max_k sigma_k} f_hk + max_k sigma_k;  lnL = sum_h w_h lnf  (w_h > 0).
// W_v does not depend on the query: every query and every pendant length is one table gather and one dot product with it.  Nothing is
// re-rooted and no reversibility is assumed; only P(t) is used, so sets of every kind are served.
// The down pass is the ancestral module's, the outer pass is nni_lane_outer / nni_mfma_outer_kernel (it also leaves f_hk of the present
// tree: lnL0).  The three extra families of matrices, P_v((1 - phi) t_v), P_v(phi t_v) and P_{pendant_label}(tau), come from the
// evaluation's own builder run on other branch vectors (engine_place.hip).
//
// Products: 21..64 states (and 20 on a matrix-core engine) are sixteen patterns per wave on v_mfma_f64_16x16x4, a workgroup of four waves
// owning ANC_TILE patterns of one class and looping over the group's edges (place_mfma_kernel, shaped as nni_mfma_kernel); 4 / 5 / 20
// states are one (pattern, class, edge) per lane (place_lane_edge).
// Rows: a row of the workspace is one (edge of the group, query, pendant).  Sums: a wave adds its 64 consecutive patterns (one chunk,
// counted from the gene's first pattern) in a fixed butterfly, then a row's chunks are added in a fixed order (red_total256).  A (query,
// edge, pendant, pattern) is computed by itself: nothing depends on the batch, the group or the place in the lists.  Ordinary vector stores
// only; no atomics.
//
// The per-lane bodies (place_lane_edge, place_combine) are plain functions of (arguments, class or row, pattern): a host program calls them
// in a loop (PLACE_HOST_ONLY: no HIP at all; tools/placement_host_check.cpp), which is how they are run under the host sanitizers.
#pragma once
#ifdef PLACE_HOST_ONLY
#ifndef NNI_HOST_ONLY
#define NNI_HOST_ONLY
#endif
#include "kernels_nni.h"
#define PLACE_HD inline
#else
#include "kernels_nni.h"
#define PLACE_HD __host__ __device__ __forceinline__
#endif

namespace paml_amd {

struct PlaceArgs {
   NniArgs o;                 // the outer pass (cap = 0: its one row is the present tree); o.m: the tree, the batch, tips, P(t) of the tree, L / SL, G / SG
   const double *Pup, *Pdn;   // lanes: row-major [pset][n_nodes][n * n], P_v((1 - phi) t_v) and P_v(phi t_v)
   const double *PTup;        // matrix cores: P_v((1 - phi) t_v)^T, [pset][n_nodes][4096] in A-operand order (every node but the root)
   const double *pint_dn;     // matrix cores: P_v(phi t_v), [pset][n_nodes][4096] in A-operand order (internal nodes)
   const double *ptip_dn;     // matrix cores: the tips' column tables of P_v(phi t_v), [pset][n_nodes][tip_words]
   const double *Ppend;       // lanes: row-major [pset][n_pend][n * n]
   const double *ptip_pend;   // matrix cores: the column tables of P_{pendant_label}(tau), [pset][n_pend][tip_words]
   const unsigned char *qz;   // [n_q][z_stride]: the queries' character codes
   const int *edges;          // [n_edges]: the whole list
   int n_q, n_pend, n_edges;
   int edge0, n_group, cap;   // the group of edges in the workspace: first, count, edges the workspace has rows for
   double *f, *sig;           // [K][cap * n_q * n_pend][stride]: f_hk and its log factor
   double *lnf;               // [cap * n_q * n_pend][stride]
   double *partial;           // [n_q * n_edges * n_pend + 1][n_chunks]: the chunks' sums of w lnf; the last row: the present tree
};

PLACE_HD long place_rows(const PlaceArgs &a) { return (long)a.cap * a.n_q * a.n_pend; }
PLACE_HD long place_out_idx(const PlaceArgs &a, int k, long row, long p) { return ((long)k * place_rows(a) + row) * a.o.m.stride + p; }
// the workspace row of (edge i of the group, query qi, pendant j) and the row of the caller's [n_q][n_edges][n_pend]
PLACE_HD long place_row(const PlaceArgs &a, int i, int qi, int j) { return ((long)i * a.n_q + qi) * a.n_pend + j; }
PLACE_HD long place_out_row(const PlaceArgs &a, long row)
{
   const int j = (int)(row % a.n_pend), qi = (int)(row / a.n_pend % a.n_q), i = (int)(row / ((long)a.n_pend * a.n_q));
   return ((long)qi * a.n_edges + a.edge0 + i) * a.n_pend + j;
}

// edge i of the group at pattern p, class k: W_v, then f_hk and its log factor of every (query, pendant)
template <int N> PLACE_HD void place_lane_edge(const PlaceArgs &a, int k, long p, int i)
{
   const AncMargArgs &m = a.o.m;
   const AncTree &t = m.t;
   const long pset = (long)m.gene * m.K + k;
   const int v = a.edges[a.edge0 + i], f = t.father[v];
   double h[N], w[N], ls;
   nni_lane_father<N>(m, k, p, f, h, &ls);
   for (int j = t.sons_ptr[f]; j < t.sons_ptr[f + 1]; j++)
      if (t.sons[j] != v) anc_lane_mul_son<N>(m, k, p, t.sons[j], h, &ls);
   const double *Pu = a.Pup + (pset * t.n_nodes + v) * (N * N), *Pd = a.Pdn + (pset * t.n_nodes + v) * (N * N);
   for (int y = 0; y < N; y++) {      // U_v = P_v((1 - phi) t)^T H_v
      double s = 0;
      for (int x = 0; x < N; x++) s += h[x] * Pu[x * N + y];
      w[y] = s;
   }
   {
      double d[N];
      if (v < t.n_tips) anc_lane_tip_msg<N>(Pd, m.code_mask[m.z[(long)v * m.z_stride + m.h0 + p]], d);
      else {
         double x[N];
         const int vi = v - t.n_tips;
         for (int c = 0; c < N; c++) x[c] = m.L[anc_idx(m, k, vi, c, p)];
         anc_lane_matvec<N>(Pd, x, d);
         ls += m.SL[((long)k * t.n_int + vi) * m.stride + p];
      }
      for (int y = 0; y < N; y++) w[y] *= d[y];
   }
   for (int qi = 0; qi < a.n_q; qi++) {
      const unsigned long long mask = m.code_mask[a.qz[(long)qi * m.z_stride + m.h0 + p]];
      for (int j = 0; j < a.n_pend; j++) {
         double tq[N], fk = 0;
         anc_lane_tip_msg<N>(a.Ppend + (pset * a.n_pend + j) * (N * N), mask, tq);
         for (int y = 0; y < N; y++) fk += w[y] * tq[y];
         const long oi = place_out_idx(a, k, place_row(a, i, qi, j), p);
         a.f[oi] = fk;
         a.sig[oi] = ls;
      }
   }
}

// the classes of workspace row `row` at pattern p, as nni_combine: stores lnf, returns the pattern's term of the weighted sum
PLACE_HD double place_combine(const PlaceArgs &a, long row, long p)
{
   const AncMargArgs &m = a.o.m;
   const double w = a.o.weights[m.h0 + p];
   double smax = -1e300;
   for (int k = 0; k < m.K; k++) {
      const double s = a.sig[place_out_idx(a, k, row, p)];
      smax = s > smax ? s : smax;
   }
   double den = 0;
   for (int k = 0; k < m.K; k++) {
      const long oi = place_out_idx(a, k, row, p);
      den += m.freqK[k] * exp(a.sig[oi] - smax) * a.f[oi];
   }
   const double lf = log(den) + smax;
   a.lnf[row * m.stride + p] = lf;
   return w > 0 ? w * lf : 0.0;
}

#ifndef PLACE_HOST_ONLY
// ---- kernels: defined in engine_place.hip ------------------------------------------------------------------------------------------

__global__ void place_mfma_kernel(PlaceArgs a);
__global__ void place_combine_kernel(PlaceArgs a, long row0);
__global__ void place_present_kernel(PlaceArgs a);
#endif

}  // namespace paml_amd

// The lnL of the tree with the label of one branch changed, for many (branch, label) rows in one call (paml_amd_relabel_scores; what
// the branch-site test costs a tree file, a set_tree, a model set-up and a search for when every branch is tried as the foreground in
// turn).  No tree is set and no kernel is built: the down partials L_v and the outer messages A_v of the present tree
// (kernels_gradient.h, kernels_nni.h) serve every row.
//
// A row (v, l): the present tree (its labels, or the call's base labels) with the label of the branch above v set to l; v any node
// other than the root, tips included; f = the father of v.  Per gene g, class k and pattern h:
//   H_v    = A_f prod_{b son of f, b != v} M_b            (the gradient's H_v; f the root: A_f = pi, a tip root: pi o its indicator)
//   P'_v   = P(set eigen_of[g][k][l], t_v qfactor[k][l] x class rate x gene rate)       (edge_pmat_fill, kernels_edge.h)
//   f_hk   = sum_y H_v(y) (P'_v L_v)(y)                   (a tip v: L_v = the indicator of its character set)
// with the log factor sigma_k = SA_f + SL of everything multiplied in.  The classes meet as nni_combine, so lnf has the NNI call's
// floors; lnfk[k][h] = log f_hk + sigma_k is the log of the class-conditional likelihood without freqK (-inf where f_hk <= 0).
// A class whose eigen set and Qfactor are the same under l as under the branch's present label, for the pattern's gene, is UNCHANGED:
// no matrix is built and no product formed for it, its f_hk and sigma_k are the present tree's (taken where the NNI call takes lnL0),
// so its lnfk has the bytes of the present tree's, and a row in which no class changes has the present tree's lnf and lnL.
//
// The rows are sorted by node on the host.  Products: 21..64 states (and 20 on a matrix-core engine) are sixteen patterns per wave on
// v_mfma_f64_16x16x4, a workgroup of four waves owning ANC_TILE patterns of one class (relabel_mfma_kernel, shaped as nni_mfma_kernel;
// the override matrices in the A-operand order): H_v and L_v are formed once per node and stay in registers over that node's rows,
// each of which is one product with P' and one dot product.  4 / 5 / 20 states are one pattern per lane (relabel_lane_node), the same
// loop.  A (row, class, pattern) is computed by itself: nothing depends on the batch, the group or the place of the row in the list.
// Ordinary vector stores only; no atomics.
//
// The per-lane bodies (relabel_lane_node, relabel_combine) are plain functions of (arguments, class or row, pattern): a host program
// calls them in a loop (RELABEL_HOST_ONLY: no HIP at all; tools/relabel_host_check.cpp), which is how they are run under the host
// sanitizers.
#pragma once
#ifdef RELABEL_HOST_ONLY
#ifndef NNI_HOST_ONLY
#define NNI_HOST_ONLY
#endif
#endif
#include "kernels_nni.h"

namespace paml_amd {

struct RelabelArgs {
   NniArgs o;                      // the tree, the batch, the present tree's passes; f / sig / lnf: f_hk, sigma and lnf of the rows (row `cap`: the
                                   // present tree); swap0 / n_group / cap: the group of rows; n_swaps: the list's length
   const int *rows;                // [n_rows][3] = v, matrix slot, the caller's index: the whole list, sorted by v
   const unsigned char *changed;   // [n_slots][psets]: 1 where the slot's label changes the class of the gene
   const double *OM;               // [n_slots][psets][n * n row-major (lanes) or 4096 in A-operand order (matrix cores)]
   int psets;
   double *lk;                     // [K][cap + 1][stride]: lnfk; null: not asked for
};

// does row `row` of the group start a node's run of rows?
NNI_HD bool relabel_run_start(const RelabelArgs &a, int row)
{
   return row == 0 || a.rows[3L * (a.o.swap0 + row)] != a.rows[3L * (a.o.swap0 + row - 1)];
}

// the run of rows of one node that starts at row `row` of the group, at pattern p, class k: H_v and L_v once, then f_hk and its log
// factor of every row
template <int N> NNI_HD void relabel_lane_node(const RelabelArgs &a, int k, long p, int row)
{
   const AncMargArgs &m = a.o.m;
   const AncTree &t = m.t;
   const long pset = (long)m.gene * m.K + k;
   const int v = a.rows[3L * (a.o.swap0 + row)], f = t.father[v];
   double h[N], l[N], y[N], ls;
   nni_lane_father<N>(m, k, p, f, h, &ls);
   for (int j = t.sons_ptr[f]; j < t.sons_ptr[f + 1]; j++)
      if (t.sons[j] != v) anc_lane_mul_son<N>(m, k, p, t.sons[j], h, &ls);
   if (v < t.n_tips) {
      const unsigned long long mask = m.code_mask[m.z[(long)v * m.z_stride + m.h0 + p]];
      for (int c = 0; c < N; c++) l[c] = (mask >> c) & 1ull ? 1.0 : 0.0;
   }
   else {
      for (int c = 0; c < N; c++) l[c] = m.L[anc_idx(m, k, v - t.n_tips, c, p)];
      ls += m.SL[((long)k * t.n_int + v - t.n_tips) * m.stride + p];
   }
   const long o0 = nni_out_idx(a.o, k, a.o.cap, p);
   for (int i = row; i < a.o.n_group && a.rows[3L * (a.o.swap0 + i)] == v; i++) {
      const int slot = a.rows[3L * (a.o.swap0 + i) + 1];
      const long oi = nni_out_idx(a.o, k, i, p);
      if (!a.changed[(long)slot * a.psets + pset]) {
         a.o.f[oi] = a.o.f[o0];
         a.o.sig[oi] = a.o.sig[o0];
         continue;
      }
      anc_lane_matvec<N>(a.OM + ((long)slot * a.psets + pset) * (N * N), l, y);
      double fk = 0;
      for (int c = 0; c < N; c++) fk += h[c] * y[c];
      a.o.f[oi] = fk;
      a.o.sig[oi] = ls;
   }
}

// the classes of row `row` of the workspace (cap: the present tree) at pattern p: nni_combine, and lnfk where it is asked for
NNI_HD double relabel_combine(const RelabelArgs &a, int row, long p)
{
   if (a.lk)
      for (int k = 0; k < a.o.m.K; k++) {
         const long oi = nni_out_idx(a.o, k, row, p);
         const double fk = a.o.f[oi];
         a.lk[oi] = fk > 0 ? log(fk) + a.o.sig[oi] : -INFINITY;
      }
   return nni_combine(a.o, row, p);
}

#ifndef RELABEL_HOST_ONLY
// ---- kernels: defined in engine_relabel.hip ---------------------------------------------------------------------------------------

struct RelabelPmatArgs {
   GradPmatArgs g;            // the model (grad_pmat_args with no label: a slot names its own; P unread); branch: the tree's lengths
   const int *slots;          // [n_slots][2] = v, label
   const unsigned char *changed;
   double *OM;                // RelabelArgs::OM
   long msz;
   int psets;
};

__global__ void relabel_pmat_kernel(RelabelPmatArgs a);
__global__ void relabel_mfma_kernel(RelabelArgs a);
__global__ void relabel_combine_kernel(RelabelArgs a);

#endif

}  // namespace paml_amd

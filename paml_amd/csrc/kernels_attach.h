// The lnL of the tree with one more tip hung on a branch at free lengths of the three branches that meet at the new node, with the first
// and second derivative along one of them, for many (query, branch, role, lengths) rows in one call (paml_amd_attach_scores; what a
// maximum-likelihood placement, EPA / pplacer, maximises per branch, and where the reference's AddSpecies treesub.c:4592 ends once the
// enlarged tree is optimised).  paml_amd_placement_scores is the same tree on a grid: one split for the whole call, pendants from a list.
//
// A row (q, v, role) with lengths (t_up, t_dn, t_pend): v != root, f = father(v); the new node u sits between f and v; the branch above u
// has length t_up, the branch above v has length t_dn, both with v's label lambda_v; u's second son is the tip of query q on a branch of
// length t_pend and label pendant_label.  t_up + t_dn need not be t_v.  role: -1 (no derivative), 0 (up), 1 (dn), 2 (pendant).  With
// H_v and L_v of kernels_place.h (H_v = A_f o prod_{c son of f, c != v} M_c, f the root: A_f = pi, a root that is a tip: pi o its
// indicator; L_v the down partial, a tip v: the indicator of its code's set), per gene, class k and pattern h:
//   U      = P_v(t_up)^T H_v
//   D      = P_v(t_dn) L_v
//   T      = T_{t_pend}[code_q(h)],        T_t[c][y] = sum_{x in set(c)} P_{pendant_label}(t)[y][x]
//   f_hk   = sum_y U(y) D(y) T(y)
//   f'_hk, f''_hk: the same expression with the one factor of `role` formed from dP/dt, d^2P/dt^2 in place of P     (role -1: both 0)
// with the log factor sigma = SA_f + SL of every subtree that was multiplied in (the siblings' and v's own).  The classes meet as
// edge_combine (kernels_edge.h): with W_k = freqK_k e^{sigma_k - max sigma},
//   lnf = log sum_k W_k f_k + max sigma;   g1 = sum W_k f'_k / sum W_k f_k;   g2 = sum W_k f''_k / sum W_k f_k - g1^2
// and lnL, d1, d2 are the sums of w_h lnf, w_h g1, w_h g2 over the patterns of weight > 0 (chunks and order: edge_combine_kernel's).  The
// present tree's lnL0 is taken as the NNI call takes it.  No reversibility is assumed and nothing is re-rooted.
// P, dP, d^2P of a row's own lengths by edge_pmat_fill (kernels_edge.h): UVROOT, CIJK, K80 and JC69-like sets.
//
// The rows are sorted by v on the host.  Products: 21..64 states (and 20 on a matrix-core engine) are sixteen patterns per wave on
// v_mfma_f64_16x16x4, a workgroup of four waves owning ANC_TILE patterns of one class (attach_mfma_kernel, shaped as relabel_mfma_kernel):
// H_v and L_v are formed once per node and stay in registers over that node's rows; a row is one product with P(t_up)^T, one product with
// P(t_dn) (a tip v: a gather from its column table), one gather from the pendant's column table and the dot product, and for a role two
// more of the role's own.  4 / 5 / 20 states are one pattern per lane (attach_lane_node), the same loop.  A (row, class, pattern) is
// computed by itself: nothing depends on the batch, the group or the place of the row in the list.  Ordinary vector stores only; no atomics.
//
// The per-lane bodies (attach_lane_node; the classes: edge_combine) are plain functions of (arguments, class or row, pattern): a host
// program calls them in a loop (ATTACH_HOST_ONLY: no HIP at all; tools/attach_host_check.cpp), which is how they are run under the host
// sanitizers.
#pragma once
#ifdef ATTACH_HOST_ONLY
#ifndef EDGE_HOST_ONLY
#define EDGE_HOST_ONLY
#endif
#endif
#include "kernels_edge.h"

namespace paml_amd {

#define ATTACH_MATS 5      // matrices of a (row, parameter set): P(t_up), P(t_dn), P(t_pend), then dP and d^2P of the role's branch
#define ATTACH_TABS 4      // column tables of a (row, parameter set), matrix cores: of P(t_dn) (a tip v), of P(t_pend), of dP and d^2P (role 2, or 1 at a tip)

struct AttachArgs {
   EdgeArgs e;                // e.o: the tree, the batch, the present tree's passes; f / sig / lnf: f_hk, sigma and lnf of the rows (row `cap`: the
                              // present tree); swap0 / n_group / cap: the group of rows; n_swaps: the list's length; e.f1 / f2 / g1 / g2 as
                              // the edge call's; e.rows / ovr_node / OM unused
   const int *rows;           // [n_rows][4] = v, q, role, the caller's index: the whole list, sorted by v
   const double *AM;          // [n_rows][psets][ATTACH_MATS][n * n row-major (lanes) or 4096 in A-operand order, the up branch's transposed (matrix cores)]
   const double *AT;          // matrix cores: [n_rows][psets][ATTACH_TABS][tip_words]
   const unsigned char *qz;   // [n_q][z_stride]: the queries' character codes
   int psets;
};

// does row `row` of the group start a node's run of rows?
NNI_HD bool attach_run_start(const AttachArgs &a, int row)
{
   return row == 0 || a.rows[4L * (a.e.o.swap0 + row)] != a.rows[4L * (a.e.o.swap0 + row - 1)];
}

// the run of rows of one node that starts at row `row` of the group, at pattern p, class k: H_v and L_v once, then f_hk, f'_hk, f''_hk
// and their log factor of every row
template <int N> NNI_HD void attach_lane_node(const AttachArgs &a, int k, long p, int row)
{
   const NniArgs &o = a.e.o;
   const AncMargArgs &m = o.m;
   const AncTree &t = m.t;
   const long pset = (long)m.gene * m.K + k;
   const int v = a.rows[4L * (o.swap0 + row)], f = t.father[v];
   double h[N], l[N], ls;
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
   for (int i = row; i < o.n_group && a.rows[4L * (o.swap0 + i)] == v; i++) {
      const int *rw = a.rows + 4L * (o.swap0 + i);
      const int role = rw[2];
      const unsigned long long qmask = m.code_mask[a.qz[(long)rw[1] * m.z_stride + m.h0 + p]];
      const double *am = a.AM + ((long)(o.swap0 + i) * a.psets + pset) * ATTACH_MATS * (N * N);
      auto up = [&](const double *M, double (&u)[N]) {      // M^T H_v
         for (int y = 0; y < N; y++) {
            double s = 0;
            for (int x = 0; x < N; x++) s += h[x] * M[x * N + y];
            u[y] = s;
         }
      };
      double u[N], d[N], tq[N], x[N], fd[3] = {0, 0, 0};
      up(am, u);
      anc_lane_matvec<N>(am + N * N, l, d);
      anc_lane_tip_msg<N>(am + 2 * N * N, qmask, tq);
      for (int y = 0; y < N; y++) fd[0] += (u[y] * d[y]) * tq[y];
      for (int dd = 1; dd <= 2 && role >= 0; dd++) {
         const double *dm = am + (2 + dd) * (N * N);
         double fk = 0;
         if (role == 0) {
            up(dm, x);
            for (int y = 0; y < N; y++) fk += (x[y] * d[y]) * tq[y];
         }
         else if (role == 1) {
            anc_lane_matvec<N>(dm, l, x);
            for (int y = 0; y < N; y++) fk += (u[y] * x[y]) * tq[y];
         }
         else {
            anc_lane_tip_msg<N>(dm, qmask, x);
            for (int y = 0; y < N; y++) fk += (u[y] * d[y]) * x[y];
         }
         fd[dd] = fk;
      }
      const long oi = nni_out_idx(o, k, i, p);
      o.f[oi] = fd[0];
      a.e.f1[oi] = fd[1];
      a.e.f2[oi] = fd[2];
      o.sig[oi] = ls;
   }
}

#ifndef ATTACH_HOST_ONLY
// ---- kernels: defined in engine_attach.hip ----------------------------------------------------------------------------------------

struct AttachPmatArgs {
   GradPmatArgs g;                        // the model (grad_pmat_args; branch and P unread: the lengths are the rows')
   const int *rows;                       // AttachArgs::rows
   const double *t3;                      // [n_rows][3] = t_up, t_dn, t_pend, in the sorted order
   const unsigned long long *code_mask;   // [n_codes]
   double *AM, *AT;                       // AttachArgs::AM, AttachArgs::AT
   long msz, tip_words;
   int psets, n_codes, pendant_label;
};

__global__ void attach_pmat_kernel(AttachPmatArgs a);
__global__ void attach_mfma_kernel(AttachArgs a);
__global__ void attach_combine_kernel(AttachArgs a);

#endif

}  // namespace paml_amd

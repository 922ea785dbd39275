// Posterior expected numbers of labelled substitutions, and expected dwell times, on every branch and at every pattern in one call
// (paml_amd_subst_counts): what substitution mapping, an EM step on a rate matrix and per-branch, per-site dN/dS summaries start from.
//
// Notation of kernels_gradient.h and kernels_modelgrad.h.  P_v = exp(A tau): A the rate matrix of the branch's eigen set for (gene g,
// class k, label of v), tau = tau_gkv the effective length, Pi_r the spectral projectors of A, Psi_rs the divided difference of exp
// (tau e^{lambda tau} on coinciding eigenvalues), evaluated exactly as mg_pull_kernel does (mg_psi: from the larger eigenvalue, so that no
// difference of nearly equal exponentials is divided).  A LABEL l is an n x n matrix of real weights M_l: off the diagonal M_l[a][b]
// weights every jump a -> b; on it M_l[a][a] rewards the time spent in a, measured in units of branch[v].
//   B_l        = A o M_l off the diagonal;  (B_l)_aa = M_l[a][a] branch[v] / tau                     (tau = 0: I = 0)
//   I_lkv      = int_0^tau e^{Au} B_l e^{A(tau - u)} du = sum_{r,s} Psi_rs Pi_r B_l Pi_s              (row = the father's state, as P_v)
//              = U (Psi o (V B_l U)) V for a UVROOT set                                               (counts_label_kernel)
//   c_lvk(h)   = sum_y H_v(y) (I_lkv L_v)(y)                                                          (the same log factor sigma_vk as f_vk)
//   n_lv(h)    = sum_k rho_k c_lvk / sum_k rho_k f_vk,   rho_k = freqK_k e^{sigma_vk - max_k sigma_vk} (grad_combine's class weights)
//   counts[l][v] = sum_h w_h n_lv(h)
// n_lv(h) is the posterior expectation, given pattern h, of the labelled jumps plus rewards on the branch above v; the rate classes are
// weighted by their posterior automatically.  The root's entries are 0; a pattern with w_h = 0 contributes nothing and its per-pattern
// values are 0.  Nothing is re-rooted and no reversibility is assumed: the quantity belongs to exactly the likelihood paml_amd_eval
// returns.  I_lkv is the forward form of the operator whose adjoint mg_pull_kernel applies to W: <W_gkv, I_lkv> summed over (g, k) is
// counts[l][v].
//
// Kernel choice.  The passes are paml_amd_model_gradient's: the ancestral module's down pass and the outer pass that stores H_v, f_vk and
// sigma_vk of every non-root node; lnL and lnf are that call's statements (mg_coef at the root's first son, mg_rows_kernel, the chunks
// added as grad_total_kernel adds them).  A product kernel follows; the products are NOT folded into the outer pass as CURV folds d2P:
// the label count is a run-time number, a workgroup of the outer pass owns one class only (the classes meet in another kernel), and the
// product kernel loads H_v and L_v of a (tile, node, class) once for all labels.  A workgroup owns (pattern tile, queried node), walks
// the classes in ascending order and, inside a class, the labels; on the matrix cores (21..64 states, 20 on a matrix-core engine) the four
// waves hold sixteen patterns each with H_v and L_v in registers and stream the label matrices (A-operand order, 32 KB) through LDS
// (stage_p + mfma_matvec, as every product of this family); 4 / 5 / 20 states are one pattern per lane with the label matrices read
// row-major at wave-uniform addresses.  The per-pattern values go to the batch workspace [label][query][pattern].
// Sums: a wave adds w_h n_lv(h) of its 64 consecutive patterns (one chunk, counted from the gene's first pattern) in the fixed butterfly;
// grad_total_kernel adds a row's chunks in its fixed order.  Every (label, node, pattern) is computed by itself: nothing depends on the
// batch a pattern falls in, on which other labels or nodes are asked for, or on their order.  Ordinary vector stores only; no atomics.
//
// The per-lane bodies (counts_lane, counts_row_term) are plain functions of (arguments, query, pattern): a host program calls them in a
// loop (COUNTS_HOST_ONLY: no HIP at all; tools/counts_host_check.cpp) under the host sanitizers.
#pragma once
#ifdef COUNTS_HOST_ONLY
#ifndef MODELGRAD_HOST_ONLY
#define MODELGRAD_HOST_ONLY
#endif
#endif
#include "kernels_modelgrad.h"

namespace paml_amd {

#define COUNTS_MAX_LABELS 16      // labels of one call

struct CountsArgs {
   ModelGradArgs g;           // the passes' arguments: H, den, sig, lnf, rows as paml_amd_model_gradient fills them
   const double *I;           // I_lkv, [pset][n_query][n_lab][n * n row-major (lanes) or 4096 in A-operand order (matrix cores)]
   const int *nodes;          // [n_query] the queried nodes (none is the root)
   int n_query, n_lab;
   double *site;              // [n_lab][n_query][stride]: n_lv(h)
};

// bytes of batch workspace per pattern: L and G with their log factors, H of every node, f_vk and sigma_vk, a tip root's partial and
// log factor and coefficient, the scalar rows and lnf, the per-pattern values (ns: the states of a stored partial, 64 on the matrix cores)
GRAD_HD double counts_bytes_per_pattern(int K, int n_int, int n_nodes, int ns, int n_lab, int n_query)
{
   return 8.0 * (2.0 * K * n_int * (ns + 1) + (double)K * n_nodes * ns + 2.0 * K * n_nodes + (double)K * (ns + 2) + (2.0 + K) + (double)n_lab * n_query);
}

GRAD_HD long counts_site_idx(const CountsArgs &a, int l, int qi, long p) { return ((long)l * a.n_query + qi) * a.g.m.stride + p; }

// query qi at pattern p, one pattern per lane: n_lv(h) of every label, classes ascending, labels inside
template <int N> GRAD_HD void counts_lane(const CountsArgs &a, int qi, long p)
{
   const ModelGradArgs &g = a.g;
   const AncMargArgs &m = g.m;
   const int v = a.nodes[qi], K = m.K;
   const double w = g.weights[m.h0 + p];
   if (!(w > 0)) {
      for (int l = 0; l < a.n_lab; l++) a.site[counts_site_idx(a, l, qi, p)] = 0;
      return;
   }
   double smax = -1e300;
   for (int k = 0; k < K; k++) {
      const double s = g.sig[mg_out_idx(g, k, v, p)];
      smax = s > smax ? s : smax;
   }
   double den = 0, num[COUNTS_MAX_LABELS];
   for (int l = 0; l < COUNTS_MAX_LABELS; l++) num[l] = 0;
   for (int k = 0; k < K; k++) {
      const long oi = mg_out_idx(g, k, v, p);
      const double rho = m.freqK[k] * exp(g.sig[oi] - smax);
      den += rho * g.den[oi];
      double h[N], x[N], y[N];
      for (int c = 0; c < N; c++) {
         h[c] = g.H[mg_h_idx(g, k, v, c, p)];
         x[c] = mg_node_L(g, k, v, c, p);
      }
      const double *Ik = a.I + (((long)m.gene * K + k) * a.n_query + qi) * a.n_lab * (N * N);
#ifndef COUNTS_HOST_ONLY
#pragma unroll
#endif
      for (int l = 0; l < COUNTS_MAX_LABELS; l++)
         if (l < a.n_lab) {
            anc_lane_matvec<N>(Ik + (long)l * (N * N), x, y);
            double c = 0;
            for (int s = 0; s < N; s++) c += h[s] * y[s];
            num[l] += rho * c;
         }
   }
#ifndef COUNTS_HOST_ONLY
#pragma unroll
#endif
   for (int l = 0; l < COUNTS_MAX_LABELS; l++)
      if (l < a.n_lab) a.site[counts_site_idx(a, l, qi, p)] = num[l] / den;
}

// pattern p's term of row (label x n_query + query) of the sums
GRAD_HD double counts_row_term(const CountsArgs &a, int row, long p)
{
   const double w = a.g.weights[a.g.m.h0 + p];
   return w > 0 ? w * a.site[(long)row * a.g.m.stride + p] : 0.0;
}

#ifndef COUNTS_HOST_ONLY
// ---- kernels: defined in engine_counts.hip -------------------------------------------------------------------------------------------

struct CountsLabelArgs {
   int n, K, n_labels, rate_gs, mfma, n_query, n_lab;
   const int *nodes, *label, *eigen_of;
   const EigenDev *eigen;
   const double *branch, *rate, *gene_rate, *qfactor;
   const double *M;           // [n_lab][n * n] the labels' weights
   double *I;                 // CountsArgs::I
};

#endif

}  // namespace paml_amd

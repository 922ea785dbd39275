// The derivative of lnL with respect to every INPUT of the engine — the rate matrix of each eigen set, the effective length of every
// (gene, class, branch), freqK and the root frequencies — in one call (paml_amd_model_gradient): what a chain rule on the host needs to
// give d lnL / d (any model parameter) without an evaluation or a decomposition per parameter.
//
// With the down partials L_v and the outer messages H_v of kernels_gradient.h, f_hk = sum_{y,x} H_v(y) P_v(y, x) L_v(x) at every non-root
// node v, class k and pattern h; f_h = sum_k freqK_k f_hk.  H_v and L_v do not depend on P_v, so per gene g, class k and node v
//   W_gkv[y][x] = sum_{h in g} w_h rho_hk H_v(y) L_v(x) / f_h      = d lnL / d P_v(y, x) of that (gene, class)
// with rho_hk = freqK_k e^{sigma_vk - max_k sigma_vk} the class weight grad_combine forms and f_h the denominator it forms (both carry
// the node's log factors; their quotient does not).  In the kernels c_vk(h) = w_h rho_hk / f_h is the `coef` of (k, v, h) (mg_coef).
//
// P_v = exp(A tau), A the matrix of the branch's eigen set (U diag(Root) V; sum_r Root_r Cijk[.][.][r]; the closed forms of K80 and
// JC69-like), tau_gkv = branch[v] x gene rate x class rate x Qfactor (Qfactor: UVROOT sets only) the effective length.  With the
// spectral projectors Pi_r of A (Pi_r = U[:, r] V[r, :]; Cijk[.][.][r]; the two or three of the closed forms),
//   exp(A tau) = sum_r e^{lambda_r tau} Pi_r,     d exp(A tau)[E] = sum_{r,s} Psi_rs Pi_r E Pi_s,
//   Psi_rs = (e^{lambda_r tau} - e^{lambda_s tau}) / (lambda_r - lambda_s),   tau e^{lambda_r tau} where the two coincide
// (differentiate the resolvent integral, or check on a diagonal A: both sides are the divided difference of exp).  Hence
//   g_A[set] += sum_{r,s} Psi_rs Pi_r^T W Pi_s^T   = V^T (Psi o (U^T W V^T)) U^T for a UVROOT set      (mg_pull_kernel)
//   g_eff[g][k][v] = <W, A exp(A tau)> = sum_r lambda_r e^{lambda_r tau} <W, Pi_r>  = sum_i lambda_i e^{lambda_i tau} (U^T W V^T)_ii
// Psi is evaluated from the larger of the two eigenvalues as tau e^{lambda tau} phi(d), d = (smaller - larger) tau <= 0, phi(d) =
// expm1(d) / d, by its series 1 + d/2 + d^2/6 + d^3/24 below |d| = MODELGRAD_PSI_SERIES (error d^4 / 120 < 1e-18): no difference of
// nearly equal exponentials is ever divided and nothing overflows.
//   g_freqK[k] = sum_h w_h f_hk / f_h     (at the root's first son, where gradient takes lnf)
//   g_pi[.][x] = sum_h w_h sum_k freqK_k L_root,k(x) / f_h      (a root that is a tip: L_root = its indicator x the sons' messages)
//
// Sums over the patterns.  W: segments of MODELGRAD_SEG patterns counted from the gene's first pattern.  Inside a segment the patterns
// are added in ascending order, sixteen (matrix cores: four v_mfma_f64_16x16x4 steps, the patterns are the k dimension) or sixty-four
// (lanes: one fixed butterfly over the wave) at a time, into one accumulator; a segment that a batch border cuts is carried to the next
// batch in that accumulator (`carry`), so the operations are the same whatever the batch.  Finished segments are added to the running
// sum W in segment order after every batch: the partials of one batch only ever exist.  The scalar rows (lnL, g_freqK, g_pi) take
// gradient's route: 64-pattern chunks in a butterfly, a row's chunks in a fixed order.  Ordinary vector stores only; no atomics.
//
// Kernel choice.  The outer pass stores H_v of every non-root node to the batch workspace and a (segment, class, node)-major product
// kernel forms W from it; the product is NOT folded into the outer pass.  A workgroup of the outer pass owns 64 patterns of one class
// and walks all nodes: folded, it would hold a 64 x 64 accumulator per node (or write one per node and tile, n^2 doubles for 64 patterns:
// more bytes than H itself), and it cannot scale by rho / f_h, which needs every class of the pattern — other workgroups — first.  The
// product kernel's workgroup owns one (segment, class, node): its four waves hold the 64 x 64 accumulator as sixteen 16 x 16 tiles,
// 16 registers a lane (not 128), and stage sixteen patterns of coef x H_v and L_v (16 KB) in LDS per step.
//
// The per-lane bodies (mg_lane_*, mg_coef, mg_row_term, mg_w_term) are plain functions of (arguments, class or node, pattern): a host
// program calls them in a loop (MODELGRAD_HOST_ONLY: no HIP at all; tools/modelgrad_host_check.cpp) under the host sanitizers.
#pragma once
#ifdef MODELGRAD_HOST_ONLY
#ifndef GRAD_HOST_ONLY
#define GRAD_HOST_ONLY
#endif
#endif
#include "kernels_gradient.h"

namespace paml_amd {

#define MODELGRAD_SEG 1024            // patterns per summation segment of W (a multiple of ANC_TILE)
#define MODELGRAD_PSI_SERIES 1e-4     // |(lambda_r - lambda_s) tau| below which phi is its series

struct ModelGradArgs {
   AncMargArgs m;             // the tree, the batch, tips, P(t), pi, freqK; L / SL: the down pass; G / SG: the outer messages A_v
   const double *PT;          // matrix cores: P_v^T, [pset][n_nodes][4096] in A-operand order (internal nodes)
   double *H;                 // H_v of every node (the root's row unused): lanes [K][n_nodes][n][stride]; matrix cores [K][n_nodes][stride / 16][1024]
   double *den, *sig;         // [K][n_nodes][stride]: f_vk and its log factor
   double *coef;              // [K][n_nodes][stride]: c_vk(h)
   double *R, *SR;            // a root that is a tip: its partial, [K][n][stride] / [K][stride / 16][1024], and log factor [K][stride]
   double *croot;             // [K][stride]: w_h freqK_k e^{SR_k - smax} / den, the coefficient of L_root,k
   double *rows;              // [1 + K][stride]: w_h lnf_h; w_h f_hk / f_h
   double *lnf;               // [stride]
   const double *weights;     // [n_patt] (engine index)
   double *partial;           // [1 + K + n][n_chunks]: the chunks' sums of rows, then of g_pi's terms
   long chunk0, n_chunks;
   int ref_node;              // the root's first son
   // W
   long off0, gene_len;       // the batch's first pattern counted from the gene's first; the gene's patterns
   int ld, wn;                // row stride and doubles of one W matrix: lanes n, n * n; matrix cores 64, 4096
   const double *carry_in;    // [K][n_nodes][wn]: the segment the last batch left unfinished
   double *carry_out, *Wpart; // the one this batch leaves; [segments of the batch][K][n_nodes][wn]
};

GRAD_HD long mg_out_idx(const ModelGradArgs &a, int k, int v, long p) { return ((long)k * a.m.t.n_nodes + v) * a.m.stride + p; }
// anc_idx with a row per node
GRAD_HD long mg_h_idx(const ModelGradArgs &a, int k, int v, int x, long p)
{
   const AncMargArgs &m = a.m;
   if (!m.mfma) return (((long)k * m.t.n_nodes + v) * m.n + x) * m.stride + p;
   const int r = x >> 2, lane = (x & 3) * 16 + (int)(p & 15);
   return (((long)k * m.t.n_nodes + v) * (m.stride >> 4) + (p >> 4)) * 1024 + ((((r >> 1) * 64 + lane) << 1) | (r & 1));
}
GRAD_HD long mg_r_idx(const ModelGradArgs &a, int k, int x, long p)
{
   const AncMargArgs &m = a.m;
   if (!m.mfma) return ((long)k * m.n + x) * m.stride + p;
   const int r = x >> 2, lane = (x & 3) * 16 + (int)(p & 15);
   return ((long)k * (m.stride >> 4) + (p >> 4)) * 1024 + ((((r >> 1) * 64 + lane) << 1) | (r & 1));
}
// L_root,k(x) of pattern p and its log factor
GRAD_HD double mg_root_L(const ModelGradArgs &a, int k, int x, long p)
{
   const AncTree &t = a.m.t;
   return t.root >= t.n_tips ? a.m.L[anc_idx(a.m, k, t.root - t.n_tips, x, p)] : a.R[mg_r_idx(a, k, x, p)];
}
GRAD_HD double mg_root_S(const ModelGradArgs &a, int k, long p)
{
   const AncTree &t = a.m.t;
   return t.root >= t.n_tips ? a.m.SL[((long)k * t.n_int + (t.root - t.n_tips)) * a.m.stride + p] : a.SR[(long)k * a.m.stride + p];
}

// the outer message of the root: A_root = pi; a root that is a tip: its partial R = its indicator x the sons' messages
template <int N> GRAD_HD void mg_lane_root(const ModelGradArgs &a, int k, long p)
{
   const AncMargArgs &m = a.m;
   const AncTree &t = m.t;
   if (t.root >= t.n_tips) {
      const double *pi = m.pi + (long)(m.n_pi > 1 ? m.gene : 0) * N;
      const int ri = t.root - t.n_tips;
      for (int c = 0; c < N; c++) m.G[anc_idx(m, k, ri, c, p)] = pi[c];
      m.SG[((long)k * t.n_int + ri) * m.stride + p] = 0;
      return;
   }
   const unsigned long long mask = m.code_mask[m.z[(long)t.root * m.z_stride + m.h0 + p]];
   double x[N], ls = 0;
   for (int c = 0; c < N; c++) x[c] = (mask >> c) & 1ull ? 1.0 : 0.0;
   for (int j = t.sons_ptr[t.root]; j < t.sons_ptr[t.root + 1]; j++) anc_lane_mul_son<N>(m, k, p, t.sons[j], x, &ls);
   for (int c = 0; c < N; c++) a.R[mg_r_idx(a, k, c, p)] = x[c];
   a.SR[(long)k * m.stride + p] = ls;
}

// node v (not the root) of pattern p, class k: H_v (stored), f_vk, and A_v of an internal v — grad_lane_node without the derivative
template <int N> GRAD_HD void mg_lane_node(const ModelGradArgs &a, int k, long p, int v)
{
   const AncMargArgs &m = a.m;
   const AncTree &t = m.t;
   const long pset = (long)m.gene * m.K + k;
   const int f = t.father[v];
   double h[N], ls = 0;
   if (f >= t.n_tips) {
      const int fi = f - t.n_tips;
      for (int c = 0; c < N; c++) h[c] = m.G[anc_idx(m, k, fi, c, p)];
      ls = m.SG[((long)k * t.n_int + fi) * m.stride + p];
   }
   else {      // the root is a tip
      const double *pi = m.pi + (long)(m.n_pi > 1 ? m.gene : 0) * N;
      const unsigned long long mask = m.code_mask[m.z[(long)f * m.z_stride + m.h0 + p]];
      for (int c = 0; c < N; c++) h[c] = (mask >> c) & 1ull ? pi[c] : 0.0;
   }
   for (int j = t.sons_ptr[f]; j < t.sons_ptr[f + 1]; j++)
      if (t.sons[j] != v) anc_lane_mul_son<N>(m, k, p, t.sons[j], h, &ls);
   for (int c = 0; c < N; c++) a.H[mg_h_idx(a, k, v, c, p)] = h[c];
   const double *Pv = m.P + (pset * t.n_nodes + v) * (N * N);
   double x[N], y[N];
   if (v < t.n_tips) {
      const unsigned long long mask = m.code_mask[m.z[(long)v * m.z_stride + m.h0 + p]];
      for (int c = 0; c < N; c++) x[c] = (mask >> c) & 1ull ? 1.0 : 0.0;
   }
   else {
      const int vi = v - t.n_tips;
      for (int c = 0; c < N; c++) x[c] = m.L[anc_idx(m, k, vi, c, p)];
   }
   double den = 0;
   anc_lane_matvec<N>(Pv, x, y);
   for (int c = 0; c < N; c++) den += h[c] * y[c];
   const long oi = mg_out_idx(a, k, v, p);
   a.den[oi] = den;
   if (v < t.n_tips) {
      a.sig[oi] = ls;
      return;
   }
   const int vi = v - t.n_tips;
   a.sig[oi] = ls + m.SL[((long)k * t.n_int + vi) * m.stride + p];
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

template <int N> GRAD_HD void mg_lane_outer(const ModelGradArgs &a, int k, long p)
{
   const AncTree &t = a.m.t;
   mg_lane_root<N>(a, k, p);
   for (int i = 0; i < t.n_pre; i++) mg_lane_node<N>(a, k, p, t.pre[i]);
   for (int v = 0; v < t.n_tips; v++)
      if (v != t.root) mg_lane_node<N>(a, k, p, v);
}

// node v of pattern p: the coefficients c_vk(h) of its classes (the root's row and a pattern of weight 0: 0).  v = n_nodes: the
// pattern's scalar rows and the root's coefficients, at ref_node
GRAD_HD void mg_coef(const ModelGradArgs &a, int v, long p)
{
   const AncMargArgs &m = a.m;
   const int K = m.K;
   const bool scalars = v == m.t.n_nodes;
   const double w = a.weights[m.h0 + p];
   const bool live = w > 0;
   if (!scalars && (v == m.t.root || !live)) {
      for (int k = 0; k < K; k++) a.coef[mg_out_idx(a, k, v, p)] = 0;
      return;
   }
   const int node = scalars ? a.ref_node : v;
   double smax = -1e300;
   for (int k = 0; k < K; k++) {
      const double s = a.sig[mg_out_idx(a, k, node, p)];
      smax = s > smax ? s : smax;
   }
   double den = 0;
   for (int k = 0; k < K; k++) {
      const long oi = mg_out_idx(a, k, node, p);
      den += m.freqK[k] * exp(a.sig[oi] - smax) * a.den[oi];
   }
   if (!scalars) {
      for (int k = 0; k < K; k++) {
         const long oi = mg_out_idx(a, k, v, p);
         a.coef[oi] = w * (m.freqK[k] * exp(a.sig[oi] - smax)) / den;
      }
      return;
   }
   const double lf = log(den) + smax;
   a.lnf[p] = lf;
   a.rows[p] = live ? w * lf : 0.0;
   for (int k = 0; k < K; k++) {
      const long oi = mg_out_idx(a, k, node, p);
      a.rows[(long)(1 + k) * m.stride + p] = live ? w * (exp(a.sig[oi] - smax) * a.den[oi]) / den : 0.0;
      a.croot[(long)k * m.stride + p] = live ? w * (m.freqK[k] * exp(mg_root_S(a, k, p) - smax)) / den : 0.0;
   }
}

// pattern p's term of scalar row r: r = 0: w lnf; 1 + k: g_freqK[k]; 1 + K + x: g_pi[.][x]
GRAD_HD double mg_row_term(const ModelGradArgs &a, int r, long p)
{
   const AncMargArgs &m = a.m;
   if (r <= m.K) return a.rows[(long)r * m.stride + p];
   const int x = r - 1 - m.K;
   double s = 0;
   for (int k = 0; k < m.K; k++) {
      const double c = a.croot[(long)k * m.stride + p];
      if (c != 0) s += c * mg_root_L(a, k, x, p);
   }
   return s;
}

// L_v(x) of pattern p (a tip: the indicator of its code)
GRAD_HD double mg_node_L(const ModelGradArgs &a, int k, int v, int x, long p)
{
   const AncMargArgs &m = a.m;
   if (v < m.t.n_tips) return (m.code_mask[m.z[(long)v * m.z_stride + m.h0 + p]] >> x) & 1ull ? 1.0 : 0.0;
   return m.L[anc_idx(m, k, v - m.t.n_tips, x, p)];
}

// pattern p's term of W_kv[y][x]
GRAD_HD double mg_w_term(const ModelGradArgs &a, int k, int v, long p, int y, int x)
{
   const double c = a.coef[mg_out_idx(a, k, v, p)];
   return c != 0 ? (c * a.H[mg_h_idx(a, k, v, y, p)]) * mg_node_L(a, k, v, x, p) : 0.0;
}

// the patterns [lo, hi) of the batch that segment si of the batch covers, whether an earlier batch began it and whether it ends here
struct ModelGradSeg {
   long lo, hi;
   bool continued, finished;
};
GRAD_HD ModelGradSeg mg_segment(const ModelGradArgs &a, int si)
{
   const long s = a.off0 / MODELGRAD_SEG + si, b = s * MODELGRAD_SEG, e = b + MODELGRAD_SEG, end = a.off0 + a.m.nb;
   ModelGradSeg r;
   r.lo = (b > a.off0 ? b : a.off0) - a.off0;
   r.hi = (e < end ? e : end) - a.off0;
   r.continued = b < a.off0;
   r.finished = e <= end || end >= a.gene_len;
   return r;
}

// phi(d) = expm1(d) / d
GRAD_HD double mg_phi(double d)
{
   if (fabs(d) < MODELGRAD_PSI_SERIES) return 1 + d * (0.5 + d * (1.0 / 6 + d * (1.0 / 24)));
   return expm1(d) / d;
}
// Psi of two eigenvalues at tau (symmetric: written from the larger one, so that phi's argument is never positive and nothing overflows)
GRAD_HD double mg_psi(double lr, double ls, double tau)
{
   const double hi = lr > ls ? lr : ls, lo = lr > ls ? ls : lr;
   return tau * exp(hi * tau) * mg_phi((lo - hi) * tau);
}

#ifndef MODELGRAD_HOST_ONLY
// ---- kernels: defined in engine_modelgrad.hip ----------------------------------------------------------------------------------------

struct ModelGradPullArgs {
   int n, K, n_nodes, root, n_labels, rate_gs, ld, wn, n_eigen;
   const int *label, *eigen_of;
   const EigenDev *eigen;
   const double *branch, *rate, *gene_rate, *qfactor;
   const double *W;           // [pset][n_nodes][wn]
   double *GA;                // [pset][n_nodes][n * n]: the slot's term of its set's g_A
   double *g_eff;             // [pset][n_nodes]
   double *g_A;               // [n_eigen][n * n]
};

__global__ void mg_mfma_outer_kernel(ModelGradArgs a);
__global__ void mg_rows_kernel(ModelGradArgs a);

// the spectral projector r of a CIJK / K80 / JC69-like set and its eigenvalue (mg_pull_kernel; counts_label_kernel, engine_counts.hip)
__device__ __forceinline__ double mg_proj(const EigenDev &es, int n, int r, int i, int j)
{
   if (es.kind == PAML_AMD_EIGEN_CIJK) return es.Cijk[((long)i * n + j) * es.nR + r];
   if (es.kind == PAML_AMD_EIGEN_K80) {
      if (r == 0) return 0.25;
      if (r == 1) return (i == j || (i ^ j) == 1) ? 0.25 : -0.25;
      return i == j ? 0.5 : ((i ^ j) == 1 ? -0.5 : 0.0);
   }
   return r == 0 ? 1.0 / n : (i == j ? 1 - 1.0 / n : -1.0 / n);
}
__device__ __forceinline__ double mg_lambda(const EigenDev &es, int n, int r)
{
   if (es.kind == PAML_AMD_EIGEN_CIJK || es.kind == PAML_AMD_EIGEN_UVROOT) return es.Root[r];
   if (r == 0) return 0.0;
   if (es.kind == PAML_AMD_EIGEN_K80) return r == 1 ? -4 / (es.kappa + 2) : -2 * (es.kappa + 1) / (es.kappa + 2);
   return -(double)n / (n - 1);
}

#endif

}  // namespace paml_amd

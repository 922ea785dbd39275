// The derivative of lnL with respect to every branch length, and the per-pattern scores d log f_h / d t_v, in one call (paml_amd_gradient;
// what gradientB / HessianSKT2004, treesub.c:7241, take 2 np evaluations for).
//
// grad[v] is the derivative, with respect to branch[v], of exactly the number paml_amd_eval returns — for any rooting and any mix of
// eigen systems: nothing is re-rooted and no reversibility is assumed (the outer message of kernels_ancestral.h, G = pi g, is the
// reversible shortcut and is NOT used here).  Per gene, class k and pattern h, with P_v = P(t) of the branch above v (row = the father's
// state), L_v the down partial (a tip: the indicator of its code's state set) and M_s = P_s L_s:
//   down   (post-order)  L_v(x) = prod_{s son of v} M_s(x)                  (anc_lane_down / anc_mfma_kernel of kernels_ancestral.h: NodeScale at
//                                                                            the marked nodes, SL_v = the log factors of v's subtree)
//   outer  (pre-order)   A_root = pi_g            (a root that is a tip: pi_g o the indicator of its code)
//                        H_v(y) = A_f(y) prod_{s sibling of v} M_s(y)       f = the father of v; the siblings' M_s are formed again here
//                        A_v(x) = sum_y H_v(y) P_v(y, x) = (P_v^T H_v)(x)   internal v only; rescaled by its maximum at every internal node
//                                                                            of a tree with scaling nodes, SA_v carries the logarithms
//   identity             f_hk   = sum_y H_v(y) (P_v L_v)(y)                 at every non-root v
//   derivative           d_vk   = sum_y H_v(y) (dP_v L_v)(y)
// Both sums of a node carry the same log factor sigma_vk = SL_v + (the factor of H_v), so the classes meet as anc_posterior's do:
//   score                s_v(h) = sum_k freqK_k e^{sigma_vk - max_k sigma_vk} d_vk / sum_k freqK_k e^{sigma_vk - max_k sigma_vk} f_vk
//   results              grad[v] = sum_h w_h s_v(h);   lnf[h] = log(the denominator at the root's first son) + max_k sigma;   lnL = sum_h w_h lnf[h]
// grad[root] = 0 and the root's scores are 0; a pattern with w_h = 0 contributes nothing and its scores are 0.
// dP_v = d P_v / d branch[v] by the formulas of pmat_deriv_kernel (kernels_branch.h): mu_k = gene rate x class rate x Qfactor x Root_k,
// dP = sum_{k >= 1} U[:, k] mu_k e^{t mu_k} V[k, :] (Cijk, K80 and JC69-like as there) — grad_pmat_kernel, which also writes P_v^T for the
// matrix-core kernel, both in the A-operand order mfma_matvec reads (the index formula of pmat_mfma_kernel, kernels_pmat.h).
//
// Products: 21..64 states (and 20 on a matrix-core engine) are sixteen patterns per wave on v_mfma_f64_16x16x4 (stage_p + mfma_matvec, as
// anc_mfma_kernel); there an internal v takes its denominator as sum_x A_v(x) L_v(x) before A_v is rescaled — the same number, H^T P L,
// without a product of its own — and a tip v feeds its code's indicator through the dP product and reads P_v L_v from the tip's column
// table.  4 / 5 / 20 states are one pattern per lane.
// Sums: a wave adds its 64 consecutive patterns (one chunk, counted from the gene's first pattern, so a chunk never spans two batches or
// two genes) in a fixed butterfly; grad_total_kernel adds a row's chunks in a fixed order (red_total256).  Nothing depends on the batch a
// pattern falls in.  Ordinary vector stores only; no atomics.
//
// The bodies take a compile-time switch, CURV: false is this call; true adds the second derivative along every branch (paml_amd_curvature,
// kernels_curvature.h) — one more product and one more dot product per non-root node, and a row of the combination per node.  Everything
// the switch adds stands inside `if constexpr (CURV)`: the arithmetic of lnL and grad is the same statements in both.
//
// The per-lane bodies (grad_lane_*, grad_combine) are plain functions of (arguments, class or node, pattern): a host program calls them in
// a loop (GRAD_HOST_ONLY: no HIP at all; tools/gradient_host_check.cpp), which is how they are run under the host sanitizers.
#pragma once
#ifdef GRAD_HOST_ONLY
#ifndef ANC_HOST_ONLY
#define ANC_HOST_ONLY
#endif
#include "kernels_ancestral.h"
#define GRAD_HD inline
#else
#include "kernels_ancestral.h"
#include "kernel_args.h"
#define GRAD_HD __host__ __device__ __forceinline__
#endif

namespace paml_amd {

#define GRAD_CHUNK 64      // patterns per partial sum: one wave of the combining kernel

struct GradArgs {
   AncMargArgs m;             // the tree, the batch, tips, P(t), pi, freqK; L / SL: the down pass; G / SG: the outer messages A_v and their log factors
   const double *dP;          // lanes: row-major [pset][n_nodes][n * n]; matrix cores: [pset][n_nodes][4096] in A-operand order
   const double *PT;          // matrix cores: P_v^T, [pset][n_nodes][4096] in A-operand order (internal nodes)
   double *num, *den, *sig;   // [K][n_nodes][stride]: d_vk, f_vk and their common log factor
   const double *weights;     // [n_patt] (engine index)
   double *scores;            // [n_nodes][stride]
   double *lnf;               // [stride]
   double *partial;           // [n_nodes + 1][n_chunks]: the chunks' sums of w s_v; row n_nodes: of w lnf
   long chunk0, n_chunks;     // the batch's first chunk; chunks of the whole engine
   int ref_node;              // the root's first son: where lnf is taken
   // CURV only (kernels_curvature.h); partial is then [2 n_nodes + 1][n_chunks]: w s_v, w c_v, w lnf, and scores is not written
   const double *d2P;         // as dP
   double *cur;               // [K][n_nodes][stride]: e_vk
};

GRAD_HD long grad_out_idx(const GradArgs &a, int k, int v, long p) { return ((long)k * a.m.t.n_nodes + v) * a.m.stride + p; }

// the outer message of the root (when it is not a tip): A_root = pi
template <int N> GRAD_HD void grad_lane_root(const GradArgs &a, int k, long p)
{
   const AncMargArgs &m = a.m;
   const AncTree &t = m.t;
   if (t.root < t.n_tips) return;
   const double *pi = m.pi + (long)(m.n_pi > 1 ? m.gene : 0) * N;
   const int ri = t.root - t.n_tips;
   for (int c = 0; c < N; c++) m.G[anc_idx(m, k, ri, c, p)] = pi[c];
   m.SG[((long)k * t.n_int + ri) * m.stride + p] = 0;
}

// node v (not the root) of pattern p, class k: H_v, the two sums, and A_v of an internal v.  The father's A is there already.
template <int N, bool CURV = false> GRAD_HD void grad_lane_node(const GradArgs &a, int k, long p, int v)
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
   const double *Pv = m.P + (pset * t.n_nodes + v) * (N * N), *dPv = a.dP + (pset * t.n_nodes + v) * (N * N);
   double x[N], y[N];
   if (v < t.n_tips) {
      const unsigned long long mask = m.code_mask[m.z[(long)v * m.z_stride + m.h0 + p]];
      for (int c = 0; c < N; c++) x[c] = (mask >> c) & 1ull ? 1.0 : 0.0;
   }
   else {
      const int vi = v - t.n_tips;
      for (int c = 0; c < N; c++) x[c] = m.L[anc_idx(m, k, vi, c, p)];
   }
   double den = 0, num = 0;
   anc_lane_matvec<N>(Pv, x, y);
   for (int c = 0; c < N; c++) den += h[c] * y[c];
   anc_lane_matvec<N>(dPv, x, y);
   for (int c = 0; c < N; c++) num += h[c] * y[c];
   const long oi = grad_out_idx(a, k, v, p);
   a.num[oi] = num;
   a.den[oi] = den;
   if constexpr (CURV) {
      double cur = 0;
      anc_lane_matvec<N>(a.d2P + (pset * t.n_nodes + v) * (N * N), x, y);
      for (int c = 0; c < N; c++) cur += h[c] * y[c];
      a.cur[oi] = cur;
   }
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

// the outer + derivative pass of pattern p, class k: the internal nodes father first, then the tips
template <int N, bool CURV = false> GRAD_HD void grad_lane_outer(const GradArgs &a, int k, long p)
{
   const AncTree &t = a.m.t;
   grad_lane_root<N>(a, k, p);
   for (int i = 0; i < t.n_pre; i++) grad_lane_node<N, CURV>(a, k, p, t.pre[i]);
   for (int v = 0; v < t.n_tips; v++)
      if (v != t.root) grad_lane_node<N, CURV>(a, k, p, v);
}

// the classes of node v (v = n_nodes: ln f_h, at ref_node) at pattern p: stores the score (the root, a pattern of weight 0: 0) or lnf;
// returns the pattern's term of the weighted sum.  CURV: the rows are 0 .. n_nodes - 1 the scores (not stored), n_nodes .. 2 n_nodes - 1
// the curvatures c_v(h) = sum_k rho_k e_vk / sum_k rho_k f_vk - s_v(h)^2, 2 n_nodes ln f_h
template <bool CURV = false> GRAD_HD double grad_combine(const GradArgs &a, int row, long p)
{
   const AncMargArgs &m = a.m;
   const int nn = m.t.n_nodes;
   const bool want_lnf = row == (CURV ? 2 * nn : nn), want_cur = CURV && !want_lnf && row >= nn;
   const int v = want_cur ? row - nn : row;
   const double w = a.weights[m.h0 + p];
   if (!want_lnf && (v == m.t.root || !(w > 0))) {
      if constexpr (!CURV) a.scores[(long)v * m.stride + p] = 0;
      return 0;
   }
   const int node = want_lnf ? a.ref_node : v;
   double smax = -1e300;
   for (int k = 0; k < m.K; k++) {
      const double s = a.sig[grad_out_idx(a, k, node, p)];
      smax = s > smax ? s : smax;
   }
   double num = 0, den = 0, cur = 0;
   for (int k = 0; k < m.K; k++) {
      const long oi = grad_out_idx(a, k, node, p);
      const double c = m.freqK[k] * exp(a.sig[oi] - smax);
      num += c * a.num[oi];
      den += c * a.den[oi];
      if constexpr (CURV)
         if (want_cur) cur += c * a.cur[oi];
   }
   if (want_lnf) {
      const double lf = log(den) + smax;
      a.lnf[p] = lf;
      return w > 0 ? w * lf : 0.0;
   }
   const double s = num / den;
   if constexpr (CURV) {
      if (want_cur) return w * (cur / den - s * s);
   }
   else a.scores[(long)v * m.stride + p] = s;
   return w * s;
}

#ifndef GRAD_HOST_ONLY
// ---- kernels: defined in engine_gradient.hip, launched from any unit of the library; their bodies here, for the CURV instantiations of
// ---- engine_curvature.hip ------------------------------------------------------------------------------------------------------------

struct GradPmatArgs {
   int n, K, n_nodes, n_tips, root, n_labels, rate_gs, mfma;
   const int *label, *eigen_of;
   const EigenDev *eigen;
   const double *branch, *rate, *gene_rate, *qfactor;
   const double *P;           // the evaluation's P(t), row-major [pset][n_nodes][n * n]
   double *dP, *PT;           // GradArgs::dP, GradArgs::PT
   double *d2P;               // CURV only: GradArgs::d2P
};

__global__ void grad_pmat_kernel(GradPmatArgs a);
__global__ void grad_mfma_kernel(GradArgs a);
__global__ void grad_combine_kernel(GradArgs a);
__global__ void grad_total_kernel(const double *partial, long n_chunks, double *out);

__device__ __forceinline__ double grad_mfma_dot(const double (&u)[16], const double (&v)[16])      // over the pattern's states: 16 registers x lane bits 4-5
{
   double s = 0;
#pragma unroll
   for (int i = 0; i < 16; i++) s += u[i] * v[i];
   s += __shfl_xor(s, 16);
   s += __shfl_xor(s, 32);
   return s;
}

// dP (CURV: and d^2P) of every (parameter set, node): grid (n_nodes, gene x class), 256 threads; sE, sM: 64 doubles of LDS each.  The
// formulas are pmat_deriv_kernel's, term for term.
template <bool CURV> __device__ __forceinline__ void grad_pmat_body(const GradPmatArgs &a, double *sE, double *sM)
{
   const int node = blockIdx.x, pset = blockIdx.y, n = a.n;
   if (node == a.root) return;
   const int gene = pset / a.K, iclass = pset % a.K, lab = a.label[node];
   const EigenDev es = a.eigen[a.eigen_of[(gene * a.K + iclass) * a.n_labels + lab]];
   const double t = a.branch[node];
   const double qf = es.kind == PAML_AMD_EIGEN_UVROOT ? a.qfactor[iclass * a.n_labels + lab] : 1.0;
   const double base = a.gene_rate[gene] * a.rate[gene * a.rate_gs + iclass] * qf;
   const int nroot = es.kind == PAML_AMD_EIGEN_CIJK ? es.nR : n;
   const bool closed = es.kind == PAML_AMD_EIGEN_K80 || es.kind == PAML_AMD_EIGEN_JC69LIKE, k80 = es.kind == PAML_AMD_EIGEN_K80;
   double m1 = 0, m2 = 0, e1 = 0, e2 = 0;
   if (closed) {
      m1 = base * (k80 ? -4 / (es.kappa + 2) : -(double)n / (n - 1));
      m2 = base * (k80 ? -2 * (es.kappa + 1) / (es.kappa + 2) : 0.0);
      e1 = exp(t * m1);
      e2 = k80 ? exp(t * m2) : 0.0;
   }
   else {
      for (int k = threadIdx.x; k < nroot; k += 256) {
         const double mu = base * es.Root[k];
         sM[k] = mu;
         sE[k] = k ? exp(t * mu) : 1.0;
      }
      __syncthreads();
   }
   auto entry = [&](int i, int j) -> double {
      if (closed) {
         double c1, c2;
         if (k80) { c1 = (i == j || (i ^ j) == 1) ? 0.25 : -0.25; c2 = i == j ? 0.5 : ((i ^ j) == 1 ? -0.5 : 0.0); }
         else { c1 = i == j ? 1 - 1.0 / n : -1.0 / n; c2 = 0; }
         return c1 * e1 * m1 + c2 * e2 * m2;
      }
      double dp = 0;
      for (int k = 1; k < nroot; k++) {
         const double c0 = es.kind == PAML_AMD_EIGEN_CIJK ? es.Cijk[((long)i * n + j) * nroot + k] * sE[k] : (es.U[i * n + k] * sE[k]) * es.V[k * n + j];
         dp += c0 * sM[k];
      }
      return dp;
   };
   // (CURV: d2P in loops of its own after dP's, so that dP's statements are compiled as they are without it — the same bytes of dP, and
   //  with them of grad, in both instantiations)
   auto entry2 = [&](int i, int j) -> double {
      if (closed) {
         double c1, c2;
         if (k80) { c1 = (i == j || (i ^ j) == 1) ? 0.25 : -0.25; c2 = i == j ? 0.5 : ((i ^ j) == 1 ? -0.5 : 0.0); }
         else { c1 = i == j ? 1 - 1.0 / n : -1.0 / n; c2 = 0; }
         return c1 * e1 * m1 * m1 + c2 * e2 * m2 * m2;
      }
      double ddp = 0;
      for (int k = 1; k < nroot; k++) {
         const double c0 = es.kind == PAML_AMD_EIGEN_CIJK ? es.Cijk[((long)i * n + j) * nroot + k] * sE[k] : (es.U[i * n + k] * sE[k]) * es.V[k * n + j];
         ddp += c0 * sM[k] * sM[k];
      }
      return ddp;
   };
   const long slot = (long)pset * a.n_nodes + node;
   if (!a.mfma) {
      double *dP = a.dP + slot * n * n;
      for (int idx = threadIdx.x; idx < n * n; idx += 256) dP[idx] = entry(idx / n, idx % n);
      if constexpr (CURV)
         for (int idx = threadIdx.x; idx < n * n; idx += 256) a.d2P[slot * n * n + idx] = entry2(idx / n, idx % n);
      return;
   }
   // A-operand order: element ((kb2*4 + jb)*64 + lane)*2 + e  =  M[jb*16 + (lane&15)][4*(2*kb2+e) + (lane>>4)], zero padded
   const double *P = a.P + slot * n * n;
   double *df = a.dP + slot * 4096, *tf = a.PT + slot * 4096;
   for (int idx = threadIdx.x; idx < 4096; idx += 256) {
      const int e = idx & 1, lane = (idx >> 1) & 63, jb = (idx >> 7) & 3, kb2 = idx >> 9;
      const int r = jb * 16 + (lane & 15), c = 4 * (2 * kb2 + e) + (lane >> 4);
      const bool in = r < n && c < n;
      df[idx] = in ? entry(r, c) : 0.0;
      if (node >= a.n_tips) tf[idx] = in ? P[c * n + r] : 0.0;
   }
   if constexpr (CURV)
      for (int idx = threadIdx.x; idx < 4096; idx += 256) {
         const int e = idx & 1, lane = (idx >> 1) & 63, jb = (idx >> 7) & 3, kb2 = idx >> 9;
         const int r = jb * 16 + (lane & 15), c = 4 * (2 * kb2 + e) + (lane >> 4);
         a.d2P[slot * 4096 + idx] = r < n && c < n ? entry2(r, c) : 0.0;
      }
}

// Matrix cores, the outer + derivative pass: a workgroup of four waves owns ANC_TILE patterns of one class, as anc_mfma_kernel (whose
// down pass runs first): lane = q * 16 + pattern, register m = state 4 m + q.  Grid (stride / ANC_TILE, K); sP: 4096 doubles of LDS.
// CURV: the d^2P product goes through the same x -> acc -> y as the dP product did, after its dot product is taken.
template <bool CURV> __device__ __forceinline__ void grad_mfma_body(const GradArgs &a, double *sP)
{
   const AncMargArgs &m = a.m;
   const AncTree &t = m.t;
   const int tid = threadIdx.x, lane = tid & 63, n = m.n;
   const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
   const int q = lane >> 4, k = blockIdx.y;
   const AncMfma w{sP, lane, wave, q};
   const long g16 = (long)blockIdx.x * 4 + wave, p = g16 * 16 + (lane & 15);
   const long pc = p < m.nb ? p : m.nb - 1;      // (lanes past the batch's end read the last pattern and write into the padding: p < stride)
   const long pset = (long)m.gene * m.K + k;
   const double *pi = m.pi + (long)(m.n_pi > 1 ? m.gene : 0) * n;
   if (t.root >= t.n_tips) {
      const int ri = t.root - t.n_tips;
      double x[16];
#pragma unroll
      for (int i = 0; i < 16; i++) x[i] = 4 * i + q < n ? pi[4 * i + q] : 0.0;
      part_store(m.G + (((long)k * t.n_int + ri) * (m.stride >> 4) + g16) * 1024, lane, x);
      if (q == 0) m.SG[((long)k * t.n_int + ri) * m.stride + p] = 0;
   }
   const int n_walk = t.n_pre + t.n_tips;
   for (int i = 0; i < n_walk; i++) {
      const int v = i < t.n_pre ? t.pre[i] : i - t.n_pre;      // the internal nodes father first, then the tips
      if (v == t.root) continue;
      const int f = t.father[v];
      double h[16], ls = 0;
      __syncthreads();      // (SG of the father was stored by the pattern's q = 0 lane: a workgroup-scope fence before the other lanes read it)
      if (f >= t.n_tips) {
         const int fi = f - t.n_tips;
         part_load(m.G + (((long)k * t.n_int + fi) * (m.stride >> 4) + g16) * 1024, lane, h);      // (this lane's own stores)
         ls = m.SG[((long)k * t.n_int + fi) * m.stride + pc];
      }
      else {
         const unsigned long long mask = m.code_mask[m.z[(long)f * m.z_stride + m.h0 + pc]];
#pragma unroll
         for (int j = 0; j < 16; j++) h[j] = (4 * j + q < n && ((mask >> (4 * j + q)) & 1ull)) ? pi[4 * j + q] : 0.0;
      }
      for (int j = t.sons_ptr[f]; j < t.sons_ptr[f + 1]; j++)
         if (t.sons[j] != v) anc_mfma_mul_son(m, w, k, g16, pc, t.sons[j], h, &ls);
      const long slot = pset * t.n_nodes + v;
      const long oi = grad_out_idx(a, k, v, p);
      double x[16], y[16];
      v4d acc[4];
      if (v < t.n_tips) {
         const int code = (int)m.z[(long)v * m.z_stride + m.h0 + pc];
         const unsigned long long mask = m.code_mask[code];
#pragma unroll
         for (int j = 0; j < 16; j++) x[j] = (mask >> (4 * j + q)) & 1ull ? 1.0 : 0.0;
         w.product(a.dP + slot * 4096, x, acc);
#pragma unroll
         for (int j = 0; j < 16; j++) y[j] = acc[j >> 2][j & 3];
         const double num = grad_mfma_dot(h, y);
         if constexpr (CURV) {
            w.product(a.d2P + slot * 4096, x, acc);
#pragma unroll
            for (int j = 0; j < 16; j++) y[j] = acc[j >> 2][j & 3];
            const double cur = grad_mfma_dot(h, y);
            if (q == 0) a.cur[oi] = cur;
         }
         double2 tv[8];
         tip_gather(m.ptip + pset * t.n_nodes * m.tip_words, m.tip_words, v, code, q, tv);
#pragma unroll
         for (int j = 0; j < 8; j++) { y[2 * j] = tv[j].x; y[2 * j + 1] = tv[j].y; }
         const double den = grad_mfma_dot(h, y);
         if (q == 0) { a.num[oi] = num; a.den[oi] = den; a.sig[oi] = ls; }
         continue;
      }
      const int vi = v - t.n_tips;
      part_load(m.L + (((long)k * t.n_int + vi) * (m.stride >> 4) + g16) * 1024, lane, x);
      w.product(a.dP + slot * 4096, x, acc);
#pragma unroll
      for (int j = 0; j < 16; j++) y[j] = acc[j >> 2][j & 3];
      const double num = grad_mfma_dot(h, y);
      if constexpr (CURV) {
         w.product(a.d2P + slot * 4096, x, acc);
#pragma unroll
         for (int j = 0; j < 16; j++) y[j] = acc[j >> 2][j & 3];
         const double cur = grad_mfma_dot(h, y);
         if (q == 0) a.cur[oi] = cur;
      }
      w.product(a.PT + slot * 4096, h, acc);      // A_v = P_v^T H_v
#pragma unroll
      for (int j = 0; j < 16; j++) y[j] = acc[j >> 2][j & 3];
      const double den = grad_mfma_dot(y, x);
      if (q == 0) { a.num[oi] = num; a.den[oi] = den; a.sig[oi] = ls + m.SL[((long)k * t.n_int + vi) * m.stride + pc]; }
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

// the classes of every (row, pattern) and the chunks' sums: grid (stride / 256, rows), rows = n_nodes + 1 (CURV: 2 n_nodes + 1); a wave =
// one chunk of GRAD_CHUNK patterns
template <bool CURV> __device__ __forceinline__ void grad_combine_body(const GradArgs &a)
{
   const long p = (long)blockIdx.x * 256 + threadIdx.x;
   const int v = blockIdx.y;
   double acc = p < a.m.nb ? grad_combine<CURV>(a, v, p) : 0.0;
#pragma unroll
   for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off);
   const long chunk = a.chunk0 + (p >> 6);
   if ((threadIdx.x & 63) == 0 && (p & ~63L) < a.m.nb) a.partial[(long)v * a.n_chunks + chunk] = acc;
}

#endif

}  // namespace paml_amd

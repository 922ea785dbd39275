// The lnL of a configuration of an internal edge at trial lengths of the five branches around it, with the first and second derivative
// along one of them, for many (edge, configuration, lengths) rows in one call (paml_amd_edge_scores; what the approximate likelihood-ratio
// test of a branch, Anisimova & Gascuel 2006 / Guindon et al. 2010, maximises per edge).  No tree is set and no kernel is built: the
// down partials L_c and the outer messages A_c of the present tree (kernels_gradient.h, kernels_nni.h) serve every row.
//
// A row (v, s, x, u) with override nodes o_1..o_5 (-1: unused) and lengths t_1..t_5: (v, s, x) is the swap of kernels_nni.h (s = x = -1:
// the present configuration of the edge above v); f = the father of v; a branch is named by the node below it and keeps its length and
// label through the swap; S'_v and S'_f are the son sets after the swap; P_c(.) is at the override length where c is listed, otherwise
// at branch[c].  The override nodes are among v, f (not the root), the sons of v and the sons of f other than v.  Per gene, class k and
// pattern h:
//   A^_f  = A_f                                            f not overridden (f the root: pi, a tip root: pi o its indicator)
//         = P_f(t_f)^T [ A_ff prod_{sibling b of f} M_b ]  f overridden (ff = father(f); its message as nni_lane_father gives it); not rescaled
//   Y     = A^_f prod_{c in S'_f, c != v} P_c(t_c) L_c
//   X     =      prod_{c in S'_v}         P_c(t_c) L_c
//   f_hk  = sum_y Y(y) (P_v(t_v) X)(y)
//   f'_hk, f''_hk: the same expression with P_u replaced by dP_u/dt, d^2P_u/dt^2      (exactly one factor carries u; u = -1: both 0)
// with the log factor sigma = SG of f (of ff when f is overridden) + SL of every subtree that was multiplied in.  The classes meet as
// nni_combine: with W_k = freqK_k e^{sigma_k - max sigma},
//   lnf = log sum_k W_k f_k + max sigma;   g1 = sum W_k f'_k / sum W_k f_k;   g2 = sum W_k f''_k / sum W_k f_k - g1^2
// and lnL, d1, d2 are the sums of w_h lnf, w_h g1, w_h g2 over the patterns of weight > 0 (chunks and order: nni_combine_kernel's).  The
// present tree's lnL0 is taken as the NNI call takes it.  No reversibility is assumed and nothing is re-rooted.
// P, dP, d^2P of the override slots by the formulas of pmat_deriv_kernel (kernels_branch.h), as grad_pmat_kernel restates them for dP:
// mu_k = gene rate x class rate x Qfactor x Root_k (edge_pmat_kernel; UVROOT, CIJK, K80 and JC69-like sets).
//
// Products: 21..64 states (and 20 on a matrix-core engine) are sixteen patterns per wave on v_mfma_f64_16x16x4, a workgroup of four waves
// owning ANC_TILE patterns of one class and looping over the group's rows (edge_mfma_kernel, shaped as nni_mfma_kernel; the override
// matrices in the A-operand order, the slot of f transposed; an overridden tip feeds its code's indicator through a product, a tip that is
// not overridden keeps its column table); 4 / 5 / 20 states are one pattern per lane (edge_lane_row).  A (row, pattern) is computed by
// itself: nothing depends on the batch, the group or the place of the row in the list.  Ordinary vector stores only; no atomics.
//
// The per-lane bodies (edge_lane_row, edge_combine) are plain functions of (arguments, class or row, pattern): a host program calls them
// in a loop (EDGE_HOST_ONLY: no HIP at all; tools/edge_host_check.cpp), which is how they are run under the host sanitizers.
#pragma once
#ifdef EDGE_HOST_ONLY
#ifndef NNI_HOST_ONLY
#define NNI_HOST_ONLY
#endif
#endif
#include "kernels_nni.h"

namespace paml_amd {

#define EDGE_SLOTS 5      // override slots of a row
#define EDGE_MATS 7       // matrices of a (row, parameter set): P of the five slots, then dP and d^2P of the slot of u

struct EdgeArgs {
   NniArgs o;                 // the tree, the batch, the present tree's passes; f / sig / lnf: f_hk, sigma and lnf of the rows (row `cap`: the
                              // present tree); swap0 / n_group / cap: the group of rows; n_swaps: the list's length
   const int *rows;           // [n_rows][4] = v, s, x, u: the whole list
   const int *ovr_node;       // [n_rows][5]
   const double *OM;          // [n_rows][psets][EDGE_MATS][n * n row-major (lanes) or 4096 in A-operand order, f's transposed (matrix cores)]
   int psets;
   double *f1, *f2;           // [K][cap + 1][stride]: f'_hk, f''_hk
   double *g1, *g2;           // [cap + 1][stride]
};

NNI_HD int edge_slot_of(const int *on, int c)
{
   for (int j = 0; j < EDGE_SLOTS; j++)
      if (on[j] == c) return j;
   return -1;
}

// (M L_c)(y) of node c below a branch with matrix M (row-major)
template <int N> NNI_HD void edge_lane_msg(const AncMargArgs &m, int k, long p, int c, const double *M, double (&msg)[N])
{
   if (c < m.t.n_tips) anc_lane_tip_msg<N>(M, m.code_mask[m.z[(long)c * m.z_stride + m.h0 + p]], msg);
   else {
      double xs[N];
      for (int y = 0; y < N; y++) xs[y] = m.L[anc_idx(m, k, c - m.t.n_tips, y, p)];
      anc_lane_matvec<N>(M, xs, msg);
   }
}
NNI_HD double edge_sl(const AncMargArgs &m, int k, long p, int c) { return c < m.t.n_tips ? 0.0 : m.SL[((long)k * m.t.n_int + c - m.t.n_tips) * m.stride + p]; }

// row `row` of the group at pattern p, class k: f_hk, f'_hk, f''_hk and their log factor
template <int N> NNI_HD void edge_lane_row(const EdgeArgs &a, int k, long p, int row)
{
   const AncMargArgs &m = a.o.m;
   const AncTree &t = m.t;
   const long pset = (long)m.gene * m.K + k;
   const int gi = a.o.swap0 + row;
   const int *rw = a.rows + 4L * gi, *on = a.ovr_node + (long)EDGE_SLOTS * gi;
   const int v = rw[0], s = rw[1], x = rw[2], u = rw[3], f = t.father[v];
   const double *om = a.OM + ((long)gi * a.psets + pset) * EDGE_MATS * (N * N);
   auto mat = [&](int c, int d) -> const double * {      // d > 0: c = u
      if (d) return om + (long)(EDGE_SLOTS - 1 + d) * (N * N);
      const int j = edge_slot_of(on, c);
      return j >= 0 ? om + (long)j * (N * N) : m.P + (pset * t.n_nodes + c) * (N * N);
   };
   const int nd = u >= 0 ? 3 : 1;
   double h[N], l[N], hff[N], msg[N], ls = 0;
   const bool f_ovr = edge_slot_of(on, f) >= 0;
   int side = u < 0 ? 0 : u == v ? 1 : u == f ? 4 : 2;      // (2: a son; 3 below if it hangs on f)
   if (!f_ovr) nni_lane_father<N>(m, k, p, f, h, &ls);
   else {
      const int ff = t.father[f];
      nni_lane_father<N>(m, k, p, ff, hff, &ls);
      for (int j = t.sons_ptr[ff]; j < t.sons_ptr[ff + 1]; j++)
         if (t.sons[j] != f) anc_lane_mul_son<N>(m, k, p, t.sons[j], hff, &ls);
      if (u == f)
         for (int c = 0; c < N; c++) h[c] = 1;
      else {
         const double *Pf = mat(f, 0);
         for (int c = 0; c < N; c++) {
            double sum = 0;
            for (int r = 0; r < N; r++) sum += hff[r] * Pf[r * N + c];
            h[c] = sum;
         }
      }
   }
   for (int j = t.sons_ptr[f]; j < t.sons_ptr[f + 1]; j++) {
      int c = t.sons[j];
      if (c == v) continue;
      if (c == x) c = s;
      ls += edge_sl(m, k, p, c);
      if (c == u) { side = 3; continue; }
      edge_lane_msg<N>(m, k, p, c, mat(c, 0), msg);
      for (int y = 0; y < N; y++) h[y] *= msg[y];
   }
   for (int c = 0; c < N; c++) l[c] = 1;
   for (int j = t.sons_ptr[v]; j < t.sons_ptr[v + 1]; j++) {
      int c = t.sons[j];
      if (c == s) c = x;
      ls += edge_sl(m, k, p, c);
      if (c == u) continue;
      edge_lane_msg<N>(m, k, p, c, mat(c, 0), msg);
      for (int y = 0; y < N; y++) l[y] *= msg[y];
   }
   double z[N], fd[3] = {0, 0, 0};
   if (side >= 3) anc_lane_matvec<N>(mat(v, 0), l, z);
   for (int d = 0; d < nd; d++) {
      double fk = 0;
      if (side <= 2) {
         double ld[N];
         for (int y = 0; y < N; y++) ld[y] = l[y];
         if (side == 2) {
            edge_lane_msg<N>(m, k, p, u, mat(u, d), msg);
            for (int y = 0; y < N; y++) ld[y] *= msg[y];
         }
         anc_lane_matvec<N>(side == 1 ? mat(v, d) : mat(v, 0), ld, z);
         for (int y = 0; y < N; y++) fk += h[y] * z[y];
      }
      else {
         if (side == 3) edge_lane_msg<N>(m, k, p, u, mat(u, d), msg);
         else {
            const double *Pf = mat(f, d);
            for (int c = 0; c < N; c++) {
               double sum = 0;
               for (int r = 0; r < N; r++) sum += hff[r] * Pf[r * N + c];
               msg[c] = sum;
            }
         }
         for (int y = 0; y < N; y++) fk += (h[y] * msg[y]) * z[y];
      }
      fd[d] = fk;
   }
   const long oi = nni_out_idx(a.o, k, row, p);
   a.o.f[oi] = fd[0];
   a.f1[oi] = fd[1];
   a.f2[oi] = fd[2];
   a.o.sig[oi] = ls;
}

// the classes of row `row` of the workspace at pattern p: stores lnf, g1 and g2; out[3] = the pattern's terms of the weighted sums
NNI_HD void edge_combine(const EdgeArgs &a, int row, long p, double (&out)[3])
{
   const AncMargArgs &m = a.o.m;
   const double w = a.o.weights[m.h0 + p];
   double smax = -1e300;
   for (int k = 0; k < m.K; k++) {
      const double s = a.o.sig[nni_out_idx(a.o, k, row, p)];
      smax = s > smax ? s : smax;
   }
   double den = 0, n1 = 0, n2 = 0;
   for (int k = 0; k < m.K; k++) {
      const long oi = nni_out_idx(a.o, k, row, p);
      const double c = m.freqK[k] * exp(a.o.sig[oi] - smax);
      den += c * a.o.f[oi];
      n1 += c * a.f1[oi];
      n2 += c * a.f2[oi];
   }
   const double lf = log(den) + smax, g1 = n1 / den, g2 = n2 / den - g1 * g1;
   const long ri = (long)row * m.stride + p;
   a.o.lnf[ri] = lf;
   a.g1[ri] = g1;
   a.g2[ri] = g2;
   const bool live = w > 0;
   out[0] = live ? w * lf : 0.0;
   out[1] = live ? w * g1 : 0.0;
   out[2] = live ? w * g2 : 0.0;
}

#ifndef EDGE_HOST_ONLY
// ---- kernels: defined in engine_edge.hip ------------------------------------------------------------------------------------------

struct EdgePmatArgs {
   GradPmatArgs g;            // the model (grad_pmat_args; branch and P unread: the lengths are the rows')
   const int *father;         // [n_nodes]
   const int *rows, *ovr_node;
   const double *ovr_t;       // [n_rows][5]
   double *OM;                // EdgeArgs::OM
   long msz;
   int psets;
};

// P(t) of parameter set `pset` under branch label `lab` at length t, and with D its first and second derivative (stored when with_d),
// by a workgroup of 256: n x n row-major, or 4096 doubles in the A-operand order (the index formula of grad_pmat_kernel; `transposed`:
// of P^T).  mu_k = gene rate x class rate x Qfactor x Root_k; UVROOT, CIJK, K80 and JC69-like sets.  sE, sM: 64 doubles of LDS each.
// Shared by edge_pmat_kernel and relabel_pmat_kernel (D = false: no derivative term is formed).
template <bool D>
__device__ __forceinline__ void edge_pmat_fill(const GradPmatArgs &g, int pset, int lab, double t, bool with_d, bool transposed, double *sE, double *sM, double *P,
                                               double *dP, double *ddP)
{
   const int n = g.n, gene = pset / g.K, iclass = pset % g.K;
   const EigenDev es = g.eigen[g.eigen_of[(gene * g.K + iclass) * g.n_labels + lab]];
   const double qf = es.kind == PAML_AMD_EIGEN_UVROOT ? g.qfactor[iclass * g.n_labels + lab] : 1.0;
   const double base = g.gene_rate[gene] * g.rate[gene * g.rate_gs + iclass] * qf;
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
   auto entry = [&](int i, int j, double (&out)[3]) {
      if (closed) {
         double c1, c2;      // P = 1/n + c1 e1 + c2 e2
         if (k80) { c1 = (i == j || (i ^ j) == 1) ? 0.25 : -0.25; c2 = i == j ? 0.5 : ((i ^ j) == 1 ? -0.5 : 0.0); }
         else { c1 = i == j ? 1 - 1.0 / n : -1.0 / n; c2 = 0; }
         out[0] = 1.0 / n + c1 * e1 + c2 * e2;
         if constexpr (D) {
            out[1] = c1 * e1 * m1 + c2 * e2 * m2;
            out[2] = c1 * e1 * m1 * m1 + c2 * e2 * m2 * m2;
         }
         return;
      }
      double p = 0, dp = 0, ddp = 0;
      for (int k = 0; k < nroot; k++) {
         const double c0 = es.kind == PAML_AMD_EIGEN_CIJK ? es.Cijk[((long)i * n + j) * nroot + k] * sE[k] : (es.U[i * n + k] * sE[k]) * es.V[k * n + j];
         p += c0;
         if constexpr (D)
            if (k) {
               dp += c0 * sM[k];
               ddp += c0 * sM[k] * sM[k];
            }
      }
      out[0] = p; out[1] = dp; out[2] = ddp;
   };
   const int total = g.mfma ? 4096 : n * n;
   for (int idx = threadIdx.x; idx < total; idx += 256) {
      int r, c;
      if (g.mfma) {      // element ((kb2*4 + jb)*64 + lane)*2 + e  =  M[jb*16 + (lane&15)][4*(2*kb2+e) + (lane>>4)], zero padded
         const int e = idx & 1, lane = (idx >> 1) & 63, jb = (idx >> 7) & 3, kb2 = idx >> 9;
         r = jb * 16 + (lane & 15);
         c = 4 * (2 * kb2 + e) + (lane >> 4);
      }
      else { r = idx / n; c = idx % n; }
      double out[3] = {0, 0, 0};
      if (r < n && c < n) {
         if (transposed) entry(c, r, out);
         else entry(r, c, out);
      }
      P[idx] = out[0];
      if (D && with_d) { dP[idx] = out[1]; ddP[idx] = out[2]; }
   }
}

__global__ void edge_pmat_kernel(EdgePmatArgs a);
__global__ void edge_mfma_kernel(EdgeArgs a);
__global__ void edge_combine_kernel(EdgeArgs a);

// The body of a combining kernel over rows of three values (edge_combine_kernel, attach_combine_kernel): the classes of every (row,
// pattern) and the chunks' sums of w lnf, w g1, w g2: grid (stride / 256, rows); a wave = one chunk of GRAD_CHUNK patterns.  partial:
// [3 n_rows + 1][n_chunks] = lnL, d1, d2 of the rows, row `row` of the group at out_row(row), then the present tree.
template <class OutRow> __device__ __forceinline__ void edge_combine_rows(const EdgeArgs &a, OutRow out_row)
{
   const NniArgs &o = a.o;
   const long p = (long)blockIdx.x * 256 + threadIdx.x;
   const bool present = (int)blockIdx.y == o.n_group;      // (a batch's first group is launched with a row more: the present tree)
   double acc[3] = {0, 0, 0};
   if (p < o.m.nb) {
      if (present) acc[0] = nni_combine(o, o.cap, p);
      else edge_combine(a, (int)blockIdx.y, p, acc);
   }
   for (int d = 0; d < 3; d++) acc[d] = score_wave_sum(acc[d]);
   long chunk;
   if (!score_chunk_lane(o, p, &chunk)) return;
   const long nr = o.n_swaps;
   if (present) { o.partial[3 * nr * o.n_chunks + chunk] = acc[0]; return; }
   const long row = out_row((int)blockIdx.y);
   for (int d = 0; d < 3; d++) o.partial[(d * nr + row) * o.n_chunks + chunk] = acc[d];
}

#endif

}  // namespace paml_amd

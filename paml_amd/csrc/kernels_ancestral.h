// Ancestral reconstruction at every internal node in one call (AncestralSeqs treesub.c:7071): marginal (AncestralMarginal / PostProbNode,
// treesub.c:6288, 6142) and joint (AncestralJointPPSG2000 treesub.c:6964; Pupko et al. 2000, the best assignment only).
//
// Marginal.  Two passes over the engine's own tree, per pattern h and class k, with P_v = P(t) of the branch above v (row = the father's
// state) and a tip's partial the indicator of its character set:
//   down   (post-order)  L_v(x) = prod_{s son of v} (P_s L_s)(x), rescaled by its maximum at the nodes SetNodeScale marked (NodeScale
//                        treesub.c:7200-7230: the factor's logarithm is carried, SL_v = the factors of v's whole subtree)
//   outer  (pre-order)   g_v(x) = sum_y P_v(x, y) g_f(y) prod_{s sibling of v} (P_s L_s)(y),      f = v's father, g_root = 1
//                        (a root that is a tip: g_root = the indicator of the tip's character set)
// g is the outer message G of the reversible model written through pi: G_v(x) = sum_y P_v(y, x) G_f(y) prod (P_s L_s)(y) with G_root = pi
// and pi_y P_v(y, x) = pi_x P_v(x, y) gives G_v = pi g_v — the same matrices as the down pass, no transposed copy and no division.
// On trees with scaling nodes g_v is rescaled by its maximum at every internal node; SG_v carries the logarithms (the father's, the
// siblings' subtrees' and its own).
//   posterior            q(x) = pi_x sum_k freqK_k e^{s_k - max_k s_k} L_vk(x) g_vk(x),  s_k = SL_vk + SG_vk;  post = q / sum_x q
//                        best = the lowest x among the maxima of post, best_prob = post[best] (the stored double)
// Products: 21..64 states (and 20 on a matrix-core engine) are sixteen patterns per wave on v_mfma_f64_16x16x4 with P(t) in the
// A-operand order the pruning kernels read (mfma_matvec, device_common.h; partials in the resident-partial layout part_index); 4 / 5 / 20
// states are one pattern per lane with the partial in registers.  Both read what the evaluation's own P(t) kernel wrote.
//
// Joint.  One class.  lnP_v = log(max(P_v, 1e-300)), lnpi = log(max(pi, 1e-300)) (anc_log_kernel).  With sons in the order of the tree's
// son lists (CSR order) and a tip's L_s(y) = max over the states c of its character set, ascending, of lnP_s[y][c]:
//   up     (post-order)  S_v(y) = 0 + L_{s1}(y) + L_{s2}(y) + ...                       (added in that order)
//                        L_v(x) = max_y (lnP_v[x][y] + S_v(y)),  C_v(x) = the LOWEST y that attains it       (v not the root)
//   root                 ln_best = max_y (lnpi[y] + S_root(y)), the lowest y; a root that is a tip maximises over its own set
//   down   (pre-order)   state_v = C_v(state_father)
// Only additions and comparisons of doubles once the logarithms are taken: nothing depends on contraction settings, on the batch a pattern
// falls in, the grid or the lane.  tests/ancestral_ref.py restates both definitions in numpy.
// Layout: a workgroup owns a tile of ANC_JTILE consecutive patterns, one per lane, and walks the tree node-outer; the node's lnP is staged
// in LDS (n^2 doubles: 29.8 KB at 61 states); a lane keeps the running maxima of sixteen states x at a time in registers and forms S_v(y)
// where it is used (a few loads per y, again for every block of x); L and the choice bytes are in the batch workspace [node][state][pattern]
// (the lane reads back only what it wrote itself).  Ordinary vector stores only; no atomics.
//
// The per-lane bodies (anc_lane_*, anc_joint_*) are plain functions of (arguments, class, pattern): a host program can call them in a loop
// (ANC_HOST_ONLY: no HIP at all), which is how they are run under the host sanitizers.
#pragma once
#ifndef ANC_HOST_ONLY
#include <hip/hip_runtime.h>

#include "device_common.h"
#define ANC_HD __host__ __device__ __forceinline__
#else
#include <cmath>
#define ANC_HD inline
#endif

namespace paml_amd {

#define ANC_TILE 64       // patterns per batch granule (one workgroup of the matrix-core kernels: four waves of sixteen)
#define ANC_JTILE 256     // patterns per workgroup of the joint kernel, one per lane

// the tree as the kernels read it: one int array (anc_tree_pack, engine_ancestral.hip)
struct AncTree {
   const int *sons_ptr;      // [n_nodes + 1]
   const int *sons;          // CSR son lists
   const int *father;        // [n_nodes], -1 at the root
   const int *post;          // [n_post] post-order: every internal node, then the root last (also when it is a tip)
   const int *pre;           // [n_pre] pre-order: the internal nodes other than the root
   const int *scale;         // [n_nodes] 1: a scaling node
   int n_post, n_pre, n_nodes, n_tips, n_int, root;
};

struct AncMargArgs {
   AncTree t;
   int n, K, gene, scaled, n_pi, n_query;
   long h0, nb, stride;                   // the batch: first pattern (engine index), patterns, row stride of the workspace (a multiple of ANC_TILE)
   const unsigned char *z; long z_stride; // [n_tips][z_stride] character codes
   const unsigned long long *code_mask;   // [n_codes] bit s: state s belongs to the code
   const double *P;                       // row-major [pset][n_nodes][n * n]
   const double *pint, *ptip;             // matrix-core engines: [pset][n_nodes][4096] / [pset][n_nodes][tip_words]
   long tip_words;
   const double *pi, *freqK;              // [n_pi][n], [K]
   const int *query;                      // [n_query] node - n_tips
   double *L, *G;                         // lanes: [K][n_int][n][stride]; matrix cores: [K][n_int][stride / 16][1024]
   double *SL, *SG;                       // [K][n_int][stride]
   double *post;                          // [n_query][stride][n]
   double *best_prob;                     // [n_query][stride]
   unsigned char *best;                   // [n_query][stride]
   int mfma;                              // layout of L and G
};

ANC_HD long anc_idx(const AncMargArgs &a, int k, int vi, int x, long p)
{
   if (!a.mfma) return (((long)k * a.t.n_int + vi) * a.n + x) * a.stride + p;
   const int m = x >> 2, lane = (x & 3) * 16 + (int)(p & 15);
   return (((long)k * a.t.n_int + vi) * (a.stride >> 4) + (p >> 4)) * 1024 + ((((m >> 1) * 64 + lane) << 1) | (m & 1));      // (part_index)
}

// (P_s L_s)(y) of a tip son: the sum of the row's entries over the code's states, ascending
template <int N> ANC_HD void anc_lane_tip_msg(const double *Ps, unsigned long long mask, double (&m)[N])
{
   for (int y = 0; y < N; y++) {
      double s = 0;
      for (int c = 0; c < N; c++)
         if ((mask >> c) & 1ull) s += Ps[y * N + c];
      m[y] = s;
   }
}
template <int N> ANC_HD void anc_lane_matvec(const double *Ps, const double (&x)[N], double (&m)[N])
{
   for (int y = 0; y < N; y++) {
      double s = 0;
      for (int c = 0; c < N; c++) s += Ps[y * N + c] * x[c];
      m[y] = s;
   }
}
// x *= (P_s L_s) of son s; the subtree's log factors are added to *ls
template <int N> ANC_HD void anc_lane_mul_son(const AncMargArgs &a, int k, long p, int s, double (&x)[N], double *ls)
{
   const long pset = (long)a.gene * a.K + k;
   const double *Ps = a.P + (pset * a.t.n_nodes + s) * (N * N);
   double m[N];
   if (s < a.t.n_tips) anc_lane_tip_msg<N>(Ps, a.code_mask[a.z[(long)s * a.z_stride + a.h0 + p]], m);
   else {
      double xs[N];
      const int si = s - a.t.n_tips;
      for (int c = 0; c < N; c++) xs[c] = a.L[anc_idx(a, k, si, c, p)];
      anc_lane_matvec<N>(Ps, xs, m);
      *ls += a.SL[((long)k * a.t.n_int + si) * a.stride + p];
   }
   for (int y = 0; y < N; y++) x[y] *= m[y];
}

// NodeScale (treesub.c:7200-7230) of a down partial
template <int N> ANC_HD double anc_lane_scale(double (&x)[N])
{
   double mx = 0;
   for (int c = 0; c < N; c++) mx = x[c] > mx ? x[c] : mx;
   if (mx < 1e-300) {
      for (int c = 0; c < N; c++) x[c] = 1;
      return -800;
   }
   for (int c = 0; c < N; c++) x[c] /= mx;
   return log(mx);
}

// the down pass of pattern p, class k
template <int N> ANC_HD void anc_lane_down(const AncMargArgs &a, int k, long p)
{
   const AncTree &t = a.t;
   for (int i = 0; i < t.n_post; i++) {
      const int v = t.post[i];
      if (v < t.n_tips) continue;      // (a root that is a tip: nobody reads its partial)
      double x[N], ls = 0;
      for (int c = 0; c < N; c++) x[c] = 1;
      for (int j = t.sons_ptr[v]; j < t.sons_ptr[v + 1]; j++) anc_lane_mul_son<N>(a, k, p, t.sons[j], x, &ls);
      if (a.scaled && t.scale[v]) ls += anc_lane_scale<N>(x);
      const int vi = v - t.n_tips;
      for (int c = 0; c < N; c++) a.L[anc_idx(a, k, vi, c, p)] = x[c];
      a.SL[((long)k * t.n_int + vi) * a.stride + p] = ls;
   }
}

// the outer pass of pattern p, class k
template <int N> ANC_HD void anc_lane_outer(const AncMargArgs &a, int k, long p)
{
   const AncTree &t = a.t;
   const long pset = (long)a.gene * a.K + k;
   if (t.root >= t.n_tips) {
      const int ri = t.root - t.n_tips;
      for (int c = 0; c < N; c++) a.G[anc_idx(a, k, ri, c, p)] = 1;
      a.SG[((long)k * t.n_int + ri) * a.stride + p] = 0;
   }
   for (int i = 0; i < t.n_pre; i++) {
      const int v = t.pre[i], f = t.father[v], vi = v - t.n_tips;
      double h[N], ls = 0;
      if (f >= t.n_tips) {
         const int fi = f - t.n_tips;
         for (int c = 0; c < N; c++) h[c] = a.G[anc_idx(a, k, fi, c, p)];
         ls = a.SG[((long)k * t.n_int + fi) * a.stride + p];
      }
      else {
         const unsigned long long mask = a.code_mask[a.z[(long)f * a.z_stride + a.h0 + p]];
         for (int c = 0; c < N; c++) h[c] = (mask >> c) & 1ull ? 1.0 : 0.0;
      }
      for (int j = t.sons_ptr[f]; j < t.sons_ptr[f + 1]; j++)
         if (t.sons[j] != v) anc_lane_mul_son<N>(a, k, p, t.sons[j], h, &ls);
      double g[N];
      anc_lane_matvec<N>(a.P + (pset * t.n_nodes + v) * (N * N), h, g);
      if (a.scaled) {
         double mx = 0;
         for (int c = 0; c < N; c++) mx = g[c] > mx ? g[c] : mx;
         if (mx > 0) {
            for (int c = 0; c < N; c++) g[c] /= mx;
            ls += log(mx);
         }
      }
      for (int c = 0; c < N; c++) a.G[anc_idx(a, k, vi, c, p)] = g[c];
      a.SG[((long)k * t.n_int + vi) * a.stride + p] = ls;
   }
}

// the posterior of query qi at pattern p: post, best, best_prob (the mixture relative to the largest class, as posterior_kernel)
ANC_HD void anc_posterior(const AncMargArgs &a, int qi, long p)
{
   const int n = a.n, vi = a.query[qi];
   const double *pi = a.pi + (long)(a.n_pi > 1 ? a.gene : 0) * n;
   double smax = 0;
   if (a.scaled) {
      smax = -1e300;
      for (int k = 0; k < a.K; k++) {
         const long si = ((long)k * a.t.n_int + vi) * a.stride + p;
         smax = fmax(smax, a.SL[si] + a.SG[si]);
      }
   }
   double *post = a.post + ((long)qi * a.stride + p) * n;
   double tot = 0;
   for (int x = 0; x < n; x++) {
      double v = 0;
      for (int k = 0; k < a.K; k++) {
         const long si = ((long)k * a.t.n_int + vi) * a.stride + p;
         const double cs = a.scaled ? exp(a.SL[si] + a.SG[si] - smax) : 1.0;
         const long li = anc_idx(a, k, vi, x, p);
         v += a.freqK[k] * cs * (a.L[li] * a.G[li]);
      }
      v *= pi[x];
      post[x] = v;
      tot += v;
   }
   const double inv = tot > 0 ? 1.0 / tot : 0.0;
   int b = 0;
   double bp = -1;
   for (int x = 0; x < n; x++) {
      const double v = post[x] * inv;
      post[x] = v;
      if (v > bp) { bp = v; b = x; }
   }
   a.best[(long)qi * a.stride + p] = (unsigned char)b;
   a.best_prob[(long)qi * a.stride + p] = post[b];
}

// ---- joint ---------------------------------------------------------------------------------------------------------------------------
struct AncJointArgs {
   AncTree t;
   int n, gene;
   long h0, nb, stride;
   const unsigned char *z; long z_stride;
   const unsigned long long *code_mask;
   const double *lnP;                     // [gene][n_nodes][n * n]
   const double *lnpi;                    // the gene's [n]
   double *L;                             // [n_int][n][stride]
   unsigned char *C;                      // [n_int][n][stride]
   unsigned char *state;                  // [n_int][stride]
   unsigned char *rootstate;              // [stride]
   double *ln_best;                       // [stride]
};

// L_s(y) of a tip son: the largest lnP_s[y][c] over the code's states c, ascending
ANC_HD double anc_joint_tip(const double *lnPs, int n, int y, unsigned long long mask)
{
   double best = -INFINITY;
   for (int c = 0; c < n; c++)
      if (((mask >> c) & 1ull) && lnPs[y * n + c] > best) best = lnPs[y * n + c];
   return best;
}

// S_v(y) of pattern p: the sons' L added in CSR order.  Formed where it is used — a handful of loads — instead of kept for all y: an array
// of 64 doubles per lane does not fit the registers beside the running maxima.
ANC_HD double anc_joint_S(const AncJointArgs &a, int v, long p, int y)
{
   const AncTree &t = a.t;
   const int n = a.n;
   double S = 0;
   for (int j = t.sons_ptr[v]; j < t.sons_ptr[v + 1]; j++) {
      const int s = t.sons[j];
      if (s < t.n_tips) {
         const unsigned long long mask = a.code_mask[a.z[(long)s * a.z_stride + a.h0 + p]];
         const double *lnPs = a.lnP + ((long)a.gene * t.n_nodes + s) * n * n;
         if ((mask & (mask - 1)) == 0 && mask) S += lnPs[y * n + (int)__builtin_ctzll(mask)];      // one state: a lookup
         else S += anc_joint_tip(lnPs, n, y, mask);
      }
      else S += a.L[((long)(s - t.n_tips) * n + y) * a.stride + p];
   }
   return S;
}

#define ANC_JX 16      // states x whose running maxima a lane keeps in registers at a time

// node v (not the root) of pattern p: L_v and the choice bytes; lnPv = the node's n x n table (LDS on the device).  x runs in blocks of
// ANC_JX, y ascending inside: per x the comparisons are in the order of the definition, so the lowest y wins among equal maxima.
ANC_HD void anc_joint_up(const AncJointArgs &a, int v, long p, const double *lnPv)
{
   const int n = a.n, vi = v - a.t.n_tips;
   for (int x0 = 0; x0 < n; x0 += ANC_JX) {
      double best[ANC_JX];
      int arg[ANC_JX];
      for (int i = 0; i < ANC_JX; i++) { best[i] = -INFINITY; arg[i] = 0; }
      for (int y = 0; y < n; y++) {
         const double S = anc_joint_S(a, v, p, y);
         for (int i = 0; i < ANC_JX; i++) {
            const int x = x0 + i < n ? x0 + i : n - 1;      // (past the end: the last row again, not stored)
            const double c = lnPv[x * n + y] + S;
            if (c > best[i]) { best[i] = c; arg[i] = y; }
         }
      }
      for (int i = 0; i < ANC_JX; i++)
         if (x0 + i < n) {
            a.L[((long)vi * n + x0 + i) * a.stride + p] = best[i];
            a.C[((long)vi * n + x0 + i) * a.stride + p] = (unsigned char)arg[i];
         }
   }
}

// the root, then every internal node's state out of its father's choice
ANC_HD void anc_joint_root_down(const AncJointArgs &a, long p)
{
   const AncTree &t = a.t;
   const int n = a.n;
   unsigned long long mask = ~0ull;
   if (t.root < t.n_tips) mask = a.code_mask[a.z[(long)t.root * a.z_stride + a.h0 + p]];
   double best = -INFINITY;
   int arg = 0;
   for (int y = 0; y < n; y++)
      if ((mask >> y) & 1ull) {
         const double c = a.lnpi[y] + anc_joint_S(a, t.root, p, y);
         if (c > best) { best = c; arg = y; }
      }
   a.ln_best[p] = best;
   a.rootstate[p] = (unsigned char)arg;
   if (t.root >= t.n_tips) a.state[(long)(t.root - t.n_tips) * a.stride + p] = (unsigned char)arg;
   for (int i = 0; i < t.n_pre; i++) {
      const int v = t.pre[i], f = t.father[v], vi = v - t.n_tips;
      const int sf = f == t.root ? (int)a.rootstate[p] : (int)a.state[(long)(f - t.n_tips) * a.stride + p];
      a.state[(long)vi * a.stride + p] = a.C[((long)vi * n + sf) * a.stride + p];
   }
}

#ifndef ANC_HOST_ONLY
// ---- kernels: defined in engine_ancestral.hip, launched from any unit of the library ---------------------------------------------

__global__ void anc_log_kernel(const double *P, long n_p, const double *pi, long n_q, double *lnP, double *lnpi);
__global__ void anc_posterior_kernel(AncMargArgs a);
__global__ void anc_mfma_kernel(AncMargArgs a, int outer);
__global__ void anc_joint_kernel(AncJointArgs a);

// Matrix cores: a workgroup of four waves owns ANC_TILE patterns of one class, sixteen per wave; lane = q * 16 + pattern, register m of a
// partial = state 4 m + q (the pruning kernels' layout).  A product stages the branch's P(t) block (A-operand order, 32 KB) in LDS.
// Lanes past the batch's end read the last pattern's codes and write into the padding of the workspace (stride is a multiple of the tile).
struct AncMfma {
   double *sP;
   int lane, wave, q;
   __device__ __forceinline__ void product(const double *block, const double (&x)[16], v4d (&acc)[4]) const
   {
      __syncthreads();      // (every wave is done reading the previous block)
      stage_p<4>(block, sP, wave, lane);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      mfma_matvec(sP, lane, x, acc);
   }
};

// x *= (P_s L_s) of son s
__device__ __forceinline__ void anc_mfma_mul_son(const AncMargArgs &a, const AncMfma &w, int k, long g16, long pc, int s, double (&x)[16], double *ls)
{
   const long pset = (long)a.gene * a.K + k;
   if (s < a.t.n_tips) {
      double2 v[8];
      tip_gather(a.ptip + pset * a.t.n_nodes * a.tip_words, a.tip_words, s, (int)a.z[(long)s * a.z_stride + a.h0 + pc], w.q, v);
#pragma unroll
      for (int i = 0; i < 8; i++) { x[2 * i] *= v[i].x; x[2 * i + 1] *= v[i].y; }
   }
   else {
      const int si = s - a.t.n_tips;
      double xs[16];
      part_load(a.L + (((long)k * a.t.n_int + si) * (a.stride >> 4) + g16) * 1024, w.lane, xs);
      v4d acc[4];
      w.product(a.pint + (pset * a.t.n_nodes + s) * 4096, xs, acc);
#pragma unroll
      for (int m = 0; m < 16; m++) x[m] *= acc[m >> 2][m & 3];
      *ls += a.SL[((long)k * a.t.n_int + si) * a.stride + pc];
   }
}

__device__ __forceinline__ double anc_mfma_max(const double (&x)[16])      // over the pattern's states: 16 registers x lane bits 4-5
{
   double mx = 0;
#pragma unroll
   for (int m = 0; m < 16; m++) mx = x[m] > mx ? x[m] : mx;
   double o = __shfl_xor(mx, 16);
   mx = o > mx ? o : mx;
   o = __shfl_xor(mx, 32);
   return o > mx ? o : mx;
}

#endif

}  // namespace paml_amd

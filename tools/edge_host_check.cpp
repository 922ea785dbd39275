// The per-lane bodies of kernels_edge.h (the row pass of 4 / 5 / 20 states and the combination of the classes; the down pass and the
// outer pass they build on are kernels_ancestral.h's and kernels_nni.h's) compiled for the HOST and called in a loop over (class or row,
// pattern) — thread indices emulated — so that they run under the host sanitizers:
//     g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -DEDGE_HOST_ONLY tools/edge_host_check.cpp -o edge_host_check
//     ./edge_host_check           (a 4-state and a 20-state problem made here; exit status 0 and "ok" lines when every number agrees)
// The reference is inside this program: every row's configuration is carried out on a copy of the son lists and the rearranged tree is
// pruned by a plain recursion in the linear domain (no scaling), class by class, with the override matrices in the places of the tree's;
// the derivatives are the same pruning with dP or d2P in the place of P_u (f is linear in every branch's matrix).  The trees are unrooted
// with a polytomy elsewhere, the tips carry ambiguity codes, two classes, scaling marks at every second internal node; the rows cover every
// listed edge, its three configurations, each of the five branches as u (a tip, v, f) and u = -1, with all five branches overridden (f
// among them where it is not the root) and with v and one son only; the 20-state problem also walks the rows in groups.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../paml_amd/csrc/kernels_edge.h"

using namespace paml_amd;

static unsigned long long rng_state = 88172645463325252ull;
static double rnd()      // xorshift64: the same problems on every run
{
   rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
   return (double)(rng_state >> 11) / 9007199254740992.0;
}

struct Tree {
   int n_tips, nn, root;
   std::vector<int> sons_ptr, sons;
};

// tips 0 .. n_tips - 1; the root has three sons, a ladder of binary nodes below it, the last one holding three tips (a polytomy)
static Tree make_tree(int n_tips)
{
   const int n_int = n_tips - 3;
   Tree t;
   t.n_tips = n_tips; t.nn = n_tips + n_int; t.root = n_tips;
   std::vector<std::vector<int>> s(t.nn);
   int tip = 0;
   s[t.root] = {tip, tip + 1, t.root + 1};
   tip += 2;
   for (int v = t.root + 1; v < t.nn - 1; v++) { s[v] = {v + 1, tip}; tip++; }
   s[t.nn - 1] = {tip, tip + 1, tip + 2};
   t.sons_ptr.assign(1, 0);
   for (int v = 0; v < t.nn; v++) {
      for (int c : s[v]) t.sons.push_back(c);
      t.sons_ptr.push_back((int)t.sons.size());
   }
   return t;
}

// the partial of node v on the tree (sons_ptr, sons) at pattern h, linear domain; mat[c] = the matrix of the branch above c
static void prune(const Tree &t, const std::vector<int> &sons, int n, int v, const std::vector<const double *> &mat, const unsigned char *z, int n_patt, const unsigned long long *mask,
                  long h, double *out)
{
   if (v < t.n_tips) {
      const unsigned long long m = mask[z[(long)v * n_patt + h]];
      for (int c = 0; c < n; c++) out[c] = (m >> c) & 1ull ? 1.0 : 0.0;
      return;
   }
   std::vector<double> l(n);
   for (int c = 0; c < n; c++) out[c] = 1;
   for (int j = t.sons_ptr[v]; j < t.sons_ptr[v + 1]; j++) {
      const int s = sons[j];
      prune(t, sons, n, s, mat, z, n_patt, mask, h, l.data());
      const double *Ps = mat[s];
      for (int y = 0; y < n; y++) {
         double m = 0;
         for (int c = 0; c < n; c++) m += Ps[y * n + c] * l[c];
         out[y] *= m;
      }
   }
}

static void random_matrix(double *M, int n, double diag, bool stochastic)
{
   for (int r = 0; r < n; r++) {
      double tot = 0;
      for (int c = 0; c < n; c++) { M[r * n + c] = (r == c ? diag : 0.05) + 0.3 * rnd(); tot += M[r * n + c]; }
      for (int c = 0; c < n; c++) M[r * n + c] = stochastic ? M[r * n + c] / tot : M[r * n + c] - tot / n;      // (a derivative's rows add up to 0)
   }
}

template <int N> static int run_case(int n_tips, int n_patt, int cap)
{
   const int n = N, K = 2;
   const Tree t = make_tree(n_tips);
   const int nn = t.nn, n_int = nn - n_tips, n_codes = n + 3;
   std::vector<int> father(nn, -1), pre, post, all_pre, stack(1, t.root), scale(nn, 0);
   while (!stack.empty()) {      // the orders of anc_tree_pack (engine_ancestral.hip)
      const int v = stack.back();
      stack.pop_back();
      all_pre.push_back(v);
      for (int j = t.sons_ptr[v + 1] - 1; j >= t.sons_ptr[v]; j--) { father[t.sons[j]] = v; stack.push_back(t.sons[j]); }
   }
   for (int v : all_pre)
      if (v >= n_tips && v != t.root) pre.push_back(v);
   post.assign(pre.rbegin(), pre.rend());
   post.push_back(t.root);
   for (int v = n_tips + 1; v < nn; v += 2) scale[v] = 1;

   std::vector<unsigned long long> mask(n_codes);
   for (int c = 0; c < n; c++) mask[c] = 1ull << c;
   mask[n] = (1ull << n) - 1;                  // the fully ambiguous code
   mask[n + 1] = 3ull;                         // two states
   mask[n + 2] = (1ull << (n - 1)) | 1ull;     // the first and the last
   std::vector<unsigned char> z((size_t)n_tips * n_patt);
   for (auto &c : z) c = (unsigned char)(rnd() < 0.15 ? n + (int)(rnd() * 3) : (int)(rnd() * n));
   std::vector<double> P((size_t)K * nn * n * n), pi(n), freqK = {0.3, 0.7}, weights(n_patt);
   for (int k = 0; k < K; k++)
      for (int v = 0; v < nn; v++) random_matrix(P.data() + ((size_t)k * nn + v) * n * n, n, 3.0 + k, true);
   double tot = 0;
   for (int c = 0; c < n; c++) { pi[c] = 0.2 + rnd(); tot += pi[c]; }
   for (int c = 0; c < n; c++) pi[c] /= tot;
   for (int h = 0; h < n_patt; h++) weights[h] = h % 5 == 2 ? 0.0 : 1.0 + (int)(rnd() * 4);

   // the rows: the list of paml_amd_edge_list (engine_edge.hip), restated, with every role of u
   std::vector<int> rows, ovr;
   int n_f_ovr = 0, n_u_tip = 0, n_u_f = 0, n_u_v = 0;
   for (int v = 0; v < nn; v++) {
      const int f = father[v];
      if (v == t.root || f < 0 || t.sons_ptr[v + 1] - t.sons_ptr[v] != 2) continue;
      const int nf = t.sons_ptr[f + 1] - t.sons_ptr[f];
      if (!(f != t.root && nf == 2) && !(f == t.root && nf == 3)) continue;
      int c[2], nc = 0;
      for (int j = t.sons_ptr[f]; j < t.sons_ptr[f + 1]; j++)
         if (t.sons[j] != v) c[nc++] = t.sons[j];
      const int s1 = t.sons[t.sons_ptr[v]], s2 = t.sons[t.sons_ptr[v] + 1];
      const int cfg[3][2] = {{-1, -1}, {s1, c[0]}, {nf == 2 ? s2 : s1, nf == 2 ? c[0] : c[1]}};
      const int five[5] = {s1, s2, v, c[0], nf == 2 ? f : c[1]};
      for (int g = 0; g < 3; g++) {
         for (int r = 0; r < 6; r++) {
            const int u = r < 5 ? five[r] : -1;
            rows.insert(rows.end(), {v, cfg[g][0], cfg[g][1], u});
            ovr.insert(ovr.end(), five, five + 5);
            n_f_ovr += nf == 2; n_u_tip += u >= 0 && u < n_tips; n_u_f += u == f; n_u_v += u == v;
         }
         rows.insert(rows.end(), {v, cfg[g][0], cfg[g][1], v});      // f not overridden, unused slots between
         ovr.insert(ovr.end(), {-1, v, -1, s2, -1});
      }
   }
   const int n_rows = (int)rows.size() / 4, psets = K;
   if (!n_f_ovr || !n_u_tip || !n_u_f || !n_u_v) { printf("FAILED: the rows do not cover every role\n"); return 1; }
   if (cap <= 0 || cap > n_rows) cap = n_rows;
   std::vector<double> OM((size_t)n_rows * psets * EDGE_MATS * n * n);
   for (int i = 0; i < n_rows; i++)
      for (int k = 0; k < K; k++)
         for (int j = 0; j < EDGE_MATS; j++) random_matrix(OM.data() + (((size_t)i * psets + k) * EDGE_MATS + j) * n * n, n, j < EDGE_SLOTS ? 2.0 + k : -1.0 - j, j < EDGE_SLOTS);

   const long stride = (n_patt + ANC_TILE - 1) / ANC_TILE * ANC_TILE;
   std::vector<double> L((size_t)K * n_int * n * stride), G(L.size()), SL((size_t)K * n_int * stride), SG(SL.size());
   std::vector<double> f((size_t)K * (cap + 1) * stride), f1(f.size()), f2(f.size()), sig(f.size()), lnf((size_t)(cap + 1) * stride), g1(lnf.size()), g2(lnf.size());
   std::vector<double> got((size_t)3 * n_rows * n_patt), got_sum((size_t)3 * n_rows, 0.0);
   EdgeArgs a{};
   AncMargArgs &m = a.o.m;
   m.t = AncTree{t.sons_ptr.data(), t.sons.data(), father.data(), post.data(), pre.data(), scale.data(), (int)post.size(), (int)pre.size(), nn, n_tips, n_int, t.root};
   m.n = n; m.K = K; m.gene = 0; m.scaled = 1; m.n_pi = 1; m.h0 = 0; m.nb = n_patt; m.stride = stride;
   m.z = z.data(); m.z_stride = n_patt; m.code_mask = mask.data(); m.P = P.data(); m.pi = pi.data(); m.freqK = freqK.data();
   m.L = L.data(); m.G = G.data(); m.SL = SL.data(); m.SG = SG.data(); m.mfma = 0;
   a.o.cap = cap; a.o.n_swaps = n_rows; a.o.f = f.data(); a.o.sig = sig.data(); a.o.weights = weights.data(); a.o.lnf = lnf.data();
   a.o.ref_node = t.sons[t.sons_ptr[t.root]];
   a.rows = rows.data(); a.ovr_node = ovr.data(); a.OM = OM.data(); a.psets = psets;
   a.f1 = f1.data(); a.f2 = f2.data(); a.g1 = g1.data(); a.g2 = g2.data();
   for (int k = 0; k < K; k++)
      for (long p = 0; p < n_patt; p++) anc_lane_down<N>(m, k, p);
   for (int k = 0; k < K; k++)
      for (long p = 0; p < n_patt; p++) nni_lane_outer<N>(a.o, k, p);
   for (int r0 = 0; r0 < n_rows; r0 += cap) {
      const int ng = r0 + cap <= n_rows ? cap : n_rows - r0;
      a.o.swap0 = r0; a.o.n_group = ng;
      for (int i = 0; i < ng; i++)
         for (int k = 0; k < K; k++)
            for (long p = 0; p < n_patt; p++) edge_lane_row<N>(a, k, p, i);
      for (int row = 0; row < ng; row++)      // (the device adds a chunk's 64 patterns in a butterfly and the chunks in a fixed order: another order of the same sum)
         for (long p = 0; p < n_patt; p++) {
            double out[3];
            edge_combine(a, row, p, out);
            const double val[3] = {lnf[(size_t)row * stride + p], g1[(size_t)row * stride + p], g2[(size_t)row * stride + p]};
            for (int d = 0; d < 3; d++) {
               got_sum[(size_t)d * n_rows + r0 + row] += out[d];
               got[((size_t)d * n_rows + r0 + row) * n_patt + p] = val[d];
            }
         }
   }

   // the plain restatement: every row's tree pruned from its root with the row's matrices
   double worst[3] = {0, 0, 0}, worst_sum[3] = {0, 0, 0};
   std::vector<double> part(n);
   for (int i = 0; i < n_rows; i++) {
      const int v = rows[4 * i], s = rows[4 * i + 1], x = rows[4 * i + 2], u = rows[4 * i + 3], fa = father[v];
      std::vector<int> sons = t.sons;
      if (s >= 0) {
         for (int j = t.sons_ptr[v]; j < t.sons_ptr[v + 1]; j++) if (sons[j] == s) { sons[j] = x; break; }
         for (int j = t.sons_ptr[fa]; j < t.sons_ptr[fa + 1]; j++) if (sons[j] == x) { sons[j] = s; break; }
      }
      double sum[3] = {0, 0, 0};
      for (long h = 0; h < n_patt; h++) {
         double fh[3] = {0, 0, 0};
         for (int k = 0; k < K; k++) {
            const double *om = OM.data() + ((size_t)i * psets + k) * EDGE_MATS * n * n;
            for (int d = 0; d < (u >= 0 ? 3 : 1); d++) {
               std::vector<const double *> mat(nn);
               for (int c = 0; c < nn; c++) mat[c] = P.data() + ((size_t)k * nn + c) * n * n;
               for (int j = 0; j < EDGE_SLOTS; j++)
                  if (ovr[5 * i + j] >= 0) mat[ovr[5 * i + j]] = om + (size_t)j * n * n;
               if (d) mat[u] = om + (size_t)(EDGE_SLOTS - 1 + d) * n * n;
               prune(t, sons, n, t.root, mat, z.data(), n_patt, mask.data(), h, part.data());
               double sc = 0;
               for (int c = 0; c < n; c++) sc += pi[c] * part[c];
               fh[d] += freqK[k] * sc;
            }
         }
         const double r1 = fh[1] / fh[0];
         const double ref[3] = {log(fh[0]), r1, fh[2] / fh[0] - r1 * r1};
         if (!(weights[h] > 0)) continue;
         for (int d = 0; d < 3; d++) {
            const double dv = fabs(ref[d] - got[((size_t)d * n_rows + i) * n_patt + h]) / (d ? fmax(1.0, fabs(ref[d])) : 1.0);
            sum[d] += weights[h] * ref[d];
            worst[d] = dv > worst[d] ? dv : worst[d];
         }
      }
      for (int d = 0; d < 3; d++) {
         const double dl = fabs(sum[d] - got_sum[(size_t)d * n_rows + i]) / fmax(1.0, fabs(sum[d]));
         worst_sum[d] = dl > worst_sum[d] ? dl : worst_sum[d];
         if (u < 0 && d && got_sum[(size_t)d * n_rows + i] != 0) worst_sum[d] = 1;      // (u = -1: both derivatives are 0)
      }
   }
   const bool ok = worst[0] <= 1e-11 && worst[1] <= 1e-10 && worst[2] <= 1e-10 && worst_sum[0] <= 1e-12 && worst_sum[1] <= 1e-10 && worst_sum[2] <= 1e-10;
   printf("%s: %d states, %d tips, %d patterns, %d rows in groups of %d: largest |lnf - restatement| %.3e, g1 %.3e, g2 %.3e (relative to max(1, |.|)); sums %.3e %.3e %.3e\n",
          ok ? "ok" : "FAILED", n, n_tips, n_patt, n_rows, cap, worst[0], worst[1], worst[2], worst_sum[0], worst_sum[1], worst_sum[2]);
   return ok ? 0 : 1;
}

int main()
{
   int bad = 0;
   bad += run_case<4>(9, 150, 0);
   bad += run_case<20>(7, 70, 4);
   return bad ? 1 : 0;
}

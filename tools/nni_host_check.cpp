// The per-lane bodies of kernels_nni.h (the down pass it takes from kernels_ancestral.h, the outer pass, the swap pass of 4 / 5 / 20
// states, the combination of the classes) compiled for the HOST and called in a loop over (class or row, pattern) — thread indices
// emulated — so that they run under the host sanitizers:
//     g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -DNNI_HOST_ONLY tools/nni_host_check.cpp -o nni_host_check
//     ./nni_host_check            (a 4-state and a 20-state problem made here; exit status 0 and "ok" lines when every number agrees)
// The reference is inside this program: every swap is carried out on a copy of the son lists and the rearranged tree is pruned by a
// plain recursion in the linear domain (no scaling), class by class.  The trees are unrooted with a polytomy, the tips carry ambiguity
// codes, two classes, scaling marks at every second internal node; the 20-state problem also walks the swaps in two groups of rows.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../paml_amd/csrc/kernels_nni.h"

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

// tips 0 .. n_tips - 1; the root has three sons (one of them a node with three sons: a polytomy), the rest is a ladder
static Tree make_tree(int n_tips)
{
   // internal nodes n_tips .. : root = n_tips; a chain of binary nodes, the last one holding three tips
   const int n_int = n_tips - 3;      // root (3 sons) + (n_int - 2) binary + one node with 3 sons = 2 + ... tips: 2 + (n_int - 2) + 3 = n_int + 3
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

// the partial of node v on the tree (sons_ptr, sons) at pattern h, class k, linear domain
static void prune(const Tree &t, const std::vector<int> &sons, int n, int v, const double *P, const unsigned char *z, int n_patt, const unsigned long long *mask, long h, double *out)
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
      prune(t, sons, n, s, P, z, n_patt, mask, h, l.data());
      const double *Ps = P + (long)s * n * n;
      for (int y = 0; y < n; y++) {
         double m = 0;
         for (int c = 0; c < n; c++) m += Ps[y * n + c] * l[c];
         out[y] *= m;
      }
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
      for (int v = 0; v < nn; v++) {
         double *Pv = P.data() + ((size_t)k * nn + v) * n * n;
         for (int r = 0; r < n; r++) {      // a row-stochastic matrix with a heavy diagonal, not symmetric
            double tot = 0;
            for (int c = 0; c < n; c++) { Pv[r * n + c] = (r == c ? 3.0 + k : 0.05) + 0.3 * rnd(); tot += Pv[r * n + c]; }
            for (int c = 0; c < n; c++) Pv[r * n + c] /= tot;
         }
      }
   double tot = 0;
   for (int c = 0; c < n; c++) { pi[c] = 0.2 + rnd(); tot += pi[c]; }
   for (int c = 0; c < n; c++) pi[c] /= tot;
   for (int h = 0; h < n_patt; h++) weights[h] = h % 5 == 2 ? 0.0 : 1.0 + (int)(rnd() * 4);

   // the canonical list (paml_amd_nni_list, engine_nni.hip), restated
   std::vector<int> swaps;
   for (int v = 0; v < nn; v++) {
      const int f = father[v], nv = t.sons_ptr[v + 1] - t.sons_ptr[v];
      if (v == t.root || f < 0 || nv == 0) continue;
      const bool half = f == t.root && t.sons_ptr[f + 1] - t.sons_ptr[f] == 3 && nv == 2;
      for (int i = t.sons_ptr[v]; i < (half ? t.sons_ptr[v] + 1 : t.sons_ptr[v + 1]); i++)
         for (int j = t.sons_ptr[f]; j < t.sons_ptr[f + 1]; j++)
            if (t.sons[j] != v) { swaps.push_back(v); swaps.push_back(t.sons[i]); swaps.push_back(t.sons[j]); }
   }
   const int n_swaps = (int)swaps.size() / 3;
   if (cap <= 0 || cap > n_swaps) cap = n_swaps;

   const long stride = (n_patt + ANC_TILE - 1) / ANC_TILE * ANC_TILE;
   std::vector<double> L((size_t)K * n_int * n * stride), G(L.size()), SL((size_t)K * n_int * stride), SG(SL.size());
   std::vector<double> f((size_t)K * (cap + 1) * stride), sig(f.size()), lnf((size_t)(cap + 1) * stride);
   std::vector<double> got_lnf((size_t)(n_swaps + 1) * n_patt), got_lnL(n_swaps + 1, 0.0);
   NniArgs a{};
   AncMargArgs &m = a.m;
   m.t = AncTree{t.sons_ptr.data(), t.sons.data(), father.data(), post.data(), pre.data(), scale.data(), (int)post.size(), (int)pre.size(), nn, n_tips, n_int, t.root};
   m.n = n; m.K = K; m.gene = 0; m.scaled = 1; m.n_pi = 1; m.h0 = 0; m.nb = n_patt; m.stride = stride;
   m.z = z.data(); m.z_stride = n_patt; m.code_mask = mask.data(); m.P = P.data(); m.pi = pi.data(); m.freqK = freqK.data();
   m.L = L.data(); m.G = G.data(); m.SL = SL.data(); m.SG = SG.data(); m.mfma = 0;
   a.swaps = swaps.data(); a.cap = cap; a.n_swaps = n_swaps; a.f = f.data(); a.sig = sig.data(); a.weights = weights.data(); a.lnf = lnf.data();
   a.ref_node = t.sons[t.sons_ptr[t.root]];
   for (int k = 0; k < K; k++)
      for (long p = 0; p < n_patt; p++) anc_lane_down<N>(m, k, p);
   for (int k = 0; k < K; k++)
      for (long p = 0; p < n_patt; p++) nni_lane_outer<N>(a, k, p);
   for (int s0 = 0; s0 < n_swaps; s0 += cap) {
      const int ng = s0 + cap <= n_swaps ? cap : n_swaps - s0;
      a.swap0 = s0; a.n_group = ng;
      for (int i = 0; i < ng; i++)
         for (int k = 0; k < K; k++)
            for (long p = 0; p < n_patt; p++) nni_lane_swap<N>(a, k, p, i);
      for (int row = 0; row < ng + (s0 == 0 ? 1 : 0); row++) {      // (the device adds a chunk's 64 patterns in a butterfly and the chunks in a fixed order: another order of the same sum)
         const int wr = row == ng ? cap : row, out = row == ng ? n_swaps : s0 + row;
         for (long p = 0; p < n_patt; p++) {
            got_lnL[out] += nni_combine(a, wr, p);
            got_lnf[(size_t)out * n_patt + p] = lnf[(size_t)wr * stride + p];
         }
      }
   }

   // the plain restatement: every rearranged tree pruned from its root
   double worst = 0, worst_l = 0;
   std::vector<double> part(n);
   for (int i = 0; i <= n_swaps; i++) {
      std::vector<int> sons = t.sons;
      if (i < n_swaps) {
         const int v = swaps[3 * i], s = swaps[3 * i + 1], x = swaps[3 * i + 2], fa = father[v];
         for (int j = t.sons_ptr[v]; j < t.sons_ptr[v + 1]; j++) if (sons[j] == s) { sons[j] = x; break; }
         for (int j = t.sons_ptr[fa]; j < t.sons_ptr[fa + 1]; j++) if (sons[j] == x) { sons[j] = s; break; }
      }
      double lnL = 0;
      for (long h = 0; h < n_patt; h++) {
         double fh = 0;
         for (int k = 0; k < K; k++) {
            prune(t, sons, n, t.root, P.data() + (size_t)k * nn * n * n, z.data(), n_patt, mask.data(), h, part.data());
            double s = 0;
            for (int c = 0; c < n; c++) s += pi[c] * part[c];
            fh += freqK[k] * s;
         }
         const double lf = log(fh), d = fabs(lf - got_lnf[(size_t)i * n_patt + h]);
         if (weights[h] > 0) { lnL += weights[h] * lf; worst = d > worst ? d : worst; }
      }
      const double dl = fabs(lnL - got_lnL[i]);
      worst_l = dl > worst_l ? dl : worst_l;
   }
   const bool ok = worst <= 1e-11 && worst_l <= 1e-9;
   printf("%s: %d states, %d tips, %d patterns, %d swaps in groups of %d: largest |lnf - restatement| %.3e, |lnL - restatement| %.3e\n", ok ? "ok" : "FAILED", n, n_tips,
          n_patt, n_swaps, cap, worst, worst_l);
   return ok ? 0 : 1;
}

int main()
{
   int bad = 0;
   bad += run_case<4>(9, 150, 0);
   bad += run_case<20>(7, 70, 3);
   return bad ? 1 : 0;
}

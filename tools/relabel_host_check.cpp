// The per-lane bodies of kernels_relabel.h (the down and outer passes it takes from kernels_ancestral.h and kernels_nni.h, the row pass of
// 4 / 5 / 20 states over a node's run of rows, the combination of the classes with lnfk) compiled for the HOST and called in a loop over
// (class or row, pattern) — thread indices emulated — so that they run under the host sanitizers:
//     g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -DRELABEL_HOST_ONLY tools/relabel_host_check.cpp -o relabel_host_check
//     ./relabel_host_check        (a 4-state and a 20-state problem made here; exit status 0 and "ok" lines when every number agrees)
// The reference is inside this program: the relabelled tree — the matrix of the branch above v replaced by the one of the new label — is
// pruned by a plain recursion in the linear domain (no scaling), class by class.  The trees are unrooted with a polytomy, the tips carry
// ambiguity codes, two classes, three labels (labels 1 and 2 share the model of class 0, so rows between them leave that class
// unchanged), scaling marks at every second internal node; the 20-state problem also walks the rows in two groups, which cuts a node's
// run of rows in two.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../paml_amd/csrc/kernels_relabel.h"

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

// tips 0 .. n_tips - 1; the root has three sons, then a ladder of binary nodes, the last node holding three tips: a polytomy
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

// the partial of node v at pattern h, linear domain; P: [nn][n * n] of one class
static void prune(const Tree &t, int n, int v, const double *P, const unsigned char *z, int n_patt, const unsigned long long *mask, long h, double *out)
{
   if (v < t.n_tips) {
      const unsigned long long m = mask[z[(long)v * n_patt + h]];
      for (int c = 0; c < n; c++) out[c] = (m >> c) & 1ull ? 1.0 : 0.0;
      return;
   }
   std::vector<double> l(n);
   for (int c = 0; c < n; c++) out[c] = 1;
   for (int j = t.sons_ptr[v]; j < t.sons_ptr[v + 1]; j++) {
      const int s = t.sons[j];
      prune(t, n, s, P, z, n_patt, mask, h, l.data());
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
   const int n = N, K = 2, NL = 3, n2 = n * n;
   const Tree t = make_tree(n_tips);
   const int nn = t.nn, n_int = nn - n_tips, n_codes = n + 3;
   std::vector<int> father(nn, -1), pre, post, all_pre, stack(1, t.root), scale(nn, 0), lab(nn);
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
   for (int v = 0; v < nn; v++) lab[v] = v % NL;

   std::vector<unsigned long long> mask(n_codes);
   for (int c = 0; c < n; c++) mask[c] = 1ull << c;
   mask[n] = (1ull << n) - 1;                  // the fully ambiguous code
   mask[n + 1] = 3ull;                         // two states
   mask[n + 2] = (1ull << (n - 1)) | 1ull;     // the first and the last
   std::vector<unsigned char> z((size_t)n_tips * n_patt);
   for (auto &c : z) c = (unsigned char)(rnd() < 0.15 ? n + (int)(rnd() * 3) : (int)(rnd() * n));
   // the models: model_of[k][label]; labels 1 and 2 share the model of class 0.  PM[model][node]: a row-stochastic matrix, not symmetric
   const int model_of[K][NL] = {{0, 2, 2}, {1, 3, 4}}, n_models = 5;
   std::vector<double> PM((size_t)n_models * nn * n2), pi(n), freqK = {0.3, 0.7}, weights(n_patt);
   for (int mo = 0; mo < n_models; mo++)
      for (int v = 0; v < nn; v++) {
         double *Pv = PM.data() + ((size_t)mo * nn + v) * n2;
         for (int r = 0; r < n; r++) {
            double tot = 0;
            for (int c = 0; c < n; c++) { Pv[r * n + c] = (r == c ? 2.0 + mo : 0.05) + 0.3 * rnd(); tot += Pv[r * n + c]; }
            for (int c = 0; c < n; c++) Pv[r * n + c] /= tot;
         }
      }
   std::vector<double> P((size_t)K * nn * n2);      // the present tree's
   for (int k = 0; k < K; k++)
      for (int v = 0; v < nn; v++) memcpy(P.data() + ((size_t)k * nn + v) * n2, PM.data() + ((size_t)model_of[k][lab[v]] * nn + v) * n2, sizeof(double) * n2);
   double tot = 0;
   for (int c = 0; c < n; c++) { pi[c] = 0.2 + rnd(); tot += pi[c]; }
   for (int c = 0; c < n; c++) pi[c] /= tot;
   for (int h = 0; h < n_patt; h++) weights[h] = h % 5 == 2 ? 0.0 : 1.0 + (int)(rnd() * 4);

   // the rows: every non-root node with every label, sorted by node as the engine sorts them; the caller's order is the reverse
   std::vector<int> rows, slots;
   for (int v = 0; v < nn; v++)
      for (int l = 0; v != t.root && l < NL; l++) { rows.push_back(v); rows.push_back((int)slots.size() / 2); rows.push_back(0); slots.push_back(v); slots.push_back(l); }
   const int n_rows = (int)rows.size() / 3, n_slots = n_rows, psets = K;
   for (int i = 0; i < n_rows; i++) rows[3 * i + 2] = n_rows - 1 - i;
   std::vector<unsigned char> changed((size_t)n_slots * psets);
   std::vector<double> OM((size_t)n_slots * psets * n2, NAN);      // (an unchanged class has no matrix: never read)
   for (int s = 0; s < n_slots; s++)
      for (int k = 0; k < K; k++) {
         const int v = slots[2 * s], l = slots[2 * s + 1];
         changed[(size_t)s * psets + k] = model_of[k][l] != model_of[k][lab[v]];
         if (changed[(size_t)s * psets + k]) memcpy(OM.data() + ((size_t)s * psets + k) * n2, PM.data() + ((size_t)model_of[k][l] * nn + v) * n2, sizeof(double) * n2);
      }
   if (cap <= 0 || cap > n_rows) cap = n_rows;

   const long stride = (n_patt + ANC_TILE - 1) / ANC_TILE * ANC_TILE;
   std::vector<double> L((size_t)K * n_int * n * stride), G(L.size()), SL((size_t)K * n_int * stride), SG(SL.size());
   std::vector<double> f((size_t)K * (cap + 1) * stride), sig(f.size()), lk(f.size()), lnf((size_t)(cap + 1) * stride);
   std::vector<double> got_lnf((size_t)(n_rows + 1) * n_patt), got_lk((size_t)(n_rows + 1) * K * n_patt), got_lnL(n_rows + 1, 0.0);
   RelabelArgs a{};
   NniArgs &o = a.o;
   AncMargArgs &m = o.m;
   m.t = AncTree{t.sons_ptr.data(), t.sons.data(), father.data(), post.data(), pre.data(), scale.data(), (int)post.size(), (int)pre.size(), nn, n_tips, n_int, t.root};
   m.n = n; m.K = K; m.gene = 0; m.scaled = 1; m.n_pi = 1; m.h0 = 0; m.nb = n_patt; m.stride = stride;
   m.z = z.data(); m.z_stride = n_patt; m.code_mask = mask.data(); m.P = P.data(); m.pi = pi.data(); m.freqK = freqK.data();
   m.L = L.data(); m.G = G.data(); m.SL = SL.data(); m.SG = SG.data(); m.mfma = 0;
   o.cap = cap; o.n_swaps = n_rows; o.f = f.data(); o.sig = sig.data(); o.weights = weights.data(); o.lnf = lnf.data();
   o.ref_node = t.sons[t.sons_ptr[t.root]];
   a.rows = rows.data(); a.changed = changed.data(); a.OM = OM.data(); a.psets = psets; a.lk = lk.data();
   for (int k = 0; k < K; k++)
      for (long p = 0; p < n_patt; p++) anc_lane_down<N>(m, k, p);
   for (int k = 0; k < K; k++)
      for (long p = 0; p < n_patt; p++) nni_lane_outer<N>(o, k, p);
   for (int s0 = 0; s0 < n_rows; s0 += cap) {
      const int ng = s0 + cap <= n_rows ? cap : n_rows - s0;
      o.swap0 = s0; o.n_group = ng;
      for (int i = 0; i < ng; i++)      // (the grid: a layer per row; the layers that start a node's run walk it)
         for (int k = 0; k < K; k++)
            for (long p = 0; p < n_patt; p++)
               if (relabel_run_start(a, i)) relabel_lane_node<N>(a, k, p, i);
      for (int row = 0; row < ng + (s0 == 0 ? 1 : 0); row++) {
         const int wr = row == ng ? cap : row, out = row == ng ? n_rows : rows[3 * (s0 + row) + 2];
         for (long p = 0; p < n_patt; p++) {
            got_lnL[out] += relabel_combine(a, wr, p);
            got_lnf[(size_t)out * n_patt + p] = lnf[(size_t)wr * stride + p];
            for (int k = 0; k < K; k++) got_lk[((size_t)out * K + k) * n_patt + p] = lk[((size_t)k * (cap + 1) + wr) * stride + p];
         }
      }
   }

   // the plain restatement: every relabelled tree pruned from its root; then the bytes of the classes that do not change
   double worst = 0, worst_l = 0, worst_k = 0;
   int bytes_bad = 0;
   std::vector<double> part(n), Pk((size_t)nn * n2);
   for (int i = 0; i <= n_rows; i++) {
      int v = -1, l = -1;
      for (int r = 0; i < n_rows && r < n_rows; r++)
         if (rows[3 * r + 2] == i) { v = rows[3 * r]; l = slots[2 * rows[3 * r + 1] + 1]; }
      double lnL = 0;
      for (long h = 0; h < n_patt; h++) {
         double fh = 0;
         for (int k = 0; k < K; k++) {
            memcpy(Pk.data(), P.data() + (size_t)k * nn * n2, sizeof(double) * nn * n2);
            if (v >= 0) memcpy(Pk.data() + (size_t)v * n2, PM.data() + ((size_t)model_of[k][l] * nn + v) * n2, sizeof(double) * n2);
            prune(t, n, t.root, Pk.data(), z.data(), n_patt, mask.data(), h, part.data());
            double s = 0;
            for (int c = 0; c < n; c++) s += pi[c] * part[c];
            fh += freqK[k] * s;
            const size_t ki = ((size_t)i * K + k) * n_patt + h, k0 = ((size_t)n_rows * K + k) * n_patt + h;
            if (weights[h] > 0) worst_k = fmax(worst_k, fabs(log(s) - got_lk[ki]));
            if (v >= 0 && model_of[k][l] == model_of[k][lab[v]]) bytes_bad += memcmp(&got_lk[ki], &got_lk[k0], 8) != 0;
         }
         const double lf = log(fh), d = fabs(lf - got_lnf[(size_t)i * n_patt + h]);
         if (weights[h] > 0) { lnL += weights[h] * lf; worst = d > worst ? d : worst; }
         if (v >= 0 && l == lab[v]) bytes_bad += memcmp(&got_lnf[(size_t)i * n_patt + h], &got_lnf[(size_t)n_rows * n_patt + h], 8) != 0;
      }
      const double dl = fabs(lnL - got_lnL[i]);
      worst_l = dl > worst_l ? dl : worst_l;
   }
   const bool ok = worst <= 1e-11 && worst_k <= 1e-11 && worst_l <= 1e-9 && bytes_bad == 0;
   printf("%s: %d states, %d tips, %d patterns, %d rows in groups of %d: largest |lnf - restatement| %.3e, |lnfk - restatement| %.3e, |lnL - restatement| %.3e, "
          "%d unchanged values with other bytes\n", ok ? "ok" : "FAILED", n, n_tips, n_patt, n_rows, cap, worst, worst_k, worst_l, bytes_bad);
   return ok ? 0 : 1;
}

int main()
{
   int bad = 0;
   bad += run_case<4>(9, 150, 0);
   bad += run_case<20>(7, 70, 16);
   return bad ? 1 : 0;
}

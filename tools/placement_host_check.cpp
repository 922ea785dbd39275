// The per-lane bodies of kernels_place.h (the down pass it takes from kernels_ancestral.h, the outer pass of kernels_nni.h, the edge pass
// of 4 / 5 / 20 states, the combination of the classes) compiled for the HOST and called in a loop over (class or row, pattern) — thread
// indices emulated — so that they run under the host sanitizers:
//     g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -DPLACE_HOST_ONLY tools/placement_host_check.cpp -o placement_host_check
//     ./placement_host_check      (a 4-state and a 20-state problem made here; exit status 0 and "ok" lines when every number agrees)
// The reference is inside this program: for every (query, edge, pendant) the enlarged tree is built (a new internal node on the branch, the
// query as a new tip) and pruned by a plain recursion in the linear domain (no scaling), class by class.  The trees are unrooted with a
// polytomy, the tips and the queries carry ambiguity codes, two classes, scaling marks at every second internal node; the 20-state problem
// also walks the edges in groups of rows.  Each problem runs at phi = 0.3, 0 and 1, always with a pendant of length 0 among the pendants.
// Matrices: P_v(s) = exp(s t_v Q_k) by a scaled Taylor series of a random rate matrix Q_k, so that P_v((1 - phi) t) P_v(phi t) = P_v(t)
// and P(0) = I hold as they do for the engine's builder.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../paml_amd/csrc/kernels_place.h"

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

// tips 0 .. n_tips - 1; the root has three sons, the last internal node has three sons (a polytomy), the rest is a ladder
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

// exp(t Q) of an n x n rate matrix: scaling and squaring of a Taylor series
static void expm(const std::vector<double> &Q, int n, double t, double *out)
{
   const int sq = 10;
   const double s = t / (1 << sq);
   std::vector<double> A((size_t)n * n), term((size_t)n * n, 0.0), sum((size_t)n * n, 0.0), tmp((size_t)n * n);
   for (int i = 0; i < n * n; i++) A[i] = s * Q[i];
   for (int i = 0; i < n; i++) term[i * n + i] = sum[i * n + i] = 1;
   for (int it = 1; it <= 12; it++) {
      for (int r = 0; r < n; r++)
         for (int c = 0; c < n; c++) {
            double x = 0;
            for (int j = 0; j < n; j++) x += term[r * n + j] * A[j * n + c];
            tmp[r * n + c] = x / it;
         }
      term = tmp;
      for (int i = 0; i < n * n; i++) sum[i] += term[i];
   }
   for (int it = 0; it < sq; it++) {
      for (int r = 0; r < n; r++)
         for (int c = 0; c < n; c++) {
            double x = 0;
            for (int j = 0; j < n; j++) x += sum[r * n + j] * sum[j * n + c];
            tmp[r * n + c] = x;
         }
      sum = tmp;
   }
   for (int i = 0; i < n * n; i++) out[i] = sum[i];
}

// the enlarged tree as the reference prunes it: node ids of the tree, plus nn = the new internal node and nn + 1 = the query tip
struct Big {
   const Tree *t;
   std::vector<std::vector<int>> sons;      // [nn + 2]
   const double *P, *Pup_v, *Pdn_v, *Ppend;     // the class's [nn][n * n]; the three matrices of this placement
   int v;
   const unsigned char *z, *qrow;
   int n_patt;
   const unsigned long long *mask;
};

static const double *big_matrix(const Big &b, int node, int n)
{
   if (node == b.t->nn) return b.Pup_v;
   if (node == b.t->nn + 1) return b.Ppend;
   if (node == b.v) return b.Pdn_v;
   return b.P + (long)node * n * n;
}

static void prune(const Big &b, int n, int node, long h, double *out)
{
   if (b.sons[node].empty()) {
      const unsigned long long m = b.mask[node == b.t->nn + 1 ? b.qrow[h] : b.z[(long)node * b.n_patt + h]];
      for (int c = 0; c < n; c++) out[c] = (m >> c) & 1ull ? 1.0 : 0.0;
      return;
   }
   std::vector<double> l(n);
   for (int c = 0; c < n; c++) out[c] = 1;
   for (int s : b.sons[node]) {
      prune(b, n, s, h, l.data());
      const double *Ps = big_matrix(b, s, n);
      for (int y = 0; y < n; y++) {
         double m = 0;
         for (int c = 0; c < n; c++) m += Ps[y * n + c] * l[c];
         out[y] *= m;
      }
   }
}

template <int N> static int run_case(int n_tips, int n_patt, int cap, double phi)
{
   const int n = N, K = 2, n_q = 3, n_pend = 2;
   const double pendant[n_pend] = {0.0, 0.35};
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
   std::vector<unsigned char> z((size_t)n_tips * n_patt), qz((size_t)n_q * n_patt);
   for (auto &c : z) c = (unsigned char)(rnd() < 0.15 ? n + (int)(rnd() * 3) : (int)(rnd() * n));
   for (auto &c : qz) c = (unsigned char)(rnd() < 0.15 ? n + (int)(rnd() * 3) : (int)(rnd() * n));
   for (int h = 0; h < n_patt; h++) qz[(size_t)2 * n_patt + h] = (unsigned char)n;      // the last query has no data

   std::vector<double> pi(n), freqK = {0.3, 0.7}, weights(n_patt), len(nn);
   std::vector<double> P((size_t)K * nn * n * n), Pup(P.size()), Pdn(P.size()), Ppend((size_t)K * n_pend * n * n);
   for (int v = 0; v < nn; v++) len[v] = 0.05 + 0.3 * rnd();
   for (int k = 0; k < K; k++) {
      std::vector<double> Q((size_t)n * n);      // a rate matrix that is not reversible
      for (int r = 0; r < n; r++) {
         double tot = 0;
         for (int c = 0; c < n; c++)
            if (c != r) { Q[r * n + c] = (0.2 + rnd()) * (1 + k) / n; tot += Q[r * n + c]; }
         Q[r * n + r] = -tot;
      }
      for (int v = 0; v < nn; v++) {
         expm(Q, n, len[v], P.data() + ((size_t)k * nn + v) * n * n);
         expm(Q, n, (1 - phi) * len[v], Pup.data() + ((size_t)k * nn + v) * n * n);
         expm(Q, n, phi * len[v], Pdn.data() + ((size_t)k * nn + v) * n * n);
      }
      for (int j = 0; j < n_pend; j++) expm(Q, n, pendant[j], Ppend.data() + ((size_t)k * n_pend + j) * n * n);
   }
   double tot = 0;
   for (int c = 0; c < n; c++) { pi[c] = 0.2 + rnd(); tot += pi[c]; }
   for (int c = 0; c < n; c++) pi[c] /= tot;
   for (int h = 0; h < n_patt; h++) weights[h] = h % 5 == 2 ? 0.0 : 1.0 + (int)(rnd() * 4);

   std::vector<int> edges;      // every edge, in an order of its own
   for (int v = nn - 1; v >= 0; v--)
      if (v != t.root) edges.push_back(v);
   const int n_edges = (int)edges.size();
   if (cap <= 0 || cap > n_edges) cap = n_edges;
   const long rows_edge = (long)n_q * n_pend, n_rows = rows_edge * n_edges;

   const long stride = (n_patt + ANC_TILE - 1) / ANC_TILE * ANC_TILE;
   std::vector<double> L((size_t)K * n_int * n * stride), G(L.size()), SL((size_t)K * n_int * stride), SG(SL.size());
   std::vector<double> f0((size_t)K * stride), sig0(f0.size()), lnf0(stride);
   std::vector<double> f((size_t)K * cap * rows_edge * stride), sig(f.size()), lnf((size_t)cap * rows_edge * stride);
   std::vector<double> got_lnf((size_t)(n_rows + 1) * n_patt), got_lnL(n_rows + 1, 0.0);
   PlaceArgs a{};
   NniArgs &o = a.o;
   AncMargArgs &m = o.m;
   m.t = AncTree{t.sons_ptr.data(), t.sons.data(), father.data(), post.data(), pre.data(), scale.data(), (int)post.size(), (int)pre.size(), nn, n_tips, n_int, t.root};
   m.n = n; m.K = K; m.gene = 0; m.scaled = 1; m.n_pi = 1; m.h0 = 0; m.nb = n_patt; m.stride = stride;
   m.z = z.data(); m.z_stride = n_patt; m.code_mask = mask.data(); m.P = P.data(); m.pi = pi.data(); m.freqK = freqK.data();
   m.L = L.data(); m.G = G.data(); m.SL = SL.data(); m.SG = SG.data(); m.mfma = 0;
   o.cap = 0; o.f = f0.data(); o.sig = sig0.data(); o.weights = weights.data(); o.lnf = lnf0.data();
   o.ref_node = t.sons[t.sons_ptr[t.root]];
   a.Pup = Pup.data(); a.Pdn = Pdn.data(); a.Ppend = Ppend.data(); a.qz = qz.data(); a.edges = edges.data();
   a.n_q = n_q; a.n_pend = n_pend; a.n_edges = n_edges; a.cap = cap; a.f = f.data(); a.sig = sig.data(); a.lnf = lnf.data();
   for (int k = 0; k < K; k++)
      for (long p = 0; p < n_patt; p++) anc_lane_down<N>(m, k, p);
   for (int k = 0; k < K; k++)
      for (long p = 0; p < n_patt; p++) nni_lane_outer<N>(o, k, p);
   for (long p = 0; p < n_patt; p++) {
      got_lnL[n_rows] += nni_combine(o, 0, p);
      got_lnf[(size_t)n_rows * n_patt + p] = lnf0[p];
   }
   for (int e0 = 0; e0 < n_edges; e0 += cap) {
      const int ng = e0 + cap <= n_edges ? cap : n_edges - e0;
      a.edge0 = e0; a.n_group = ng;
      for (int i = 0; i < ng; i++)
         for (int k = 0; k < K; k++)
            for (long p = 0; p < n_patt; p++) place_lane_edge<N>(a, k, p, i);
      for (long row = 0; row < rows_edge * ng; row++) {      // (the device adds a chunk's 64 patterns in a butterfly and the chunks in a fixed order: another order of the same sum)
         const long out = place_out_row(a, row);
         for (long p = 0; p < n_patt; p++) {
            got_lnL[out] += place_combine(a, row, p);
            got_lnf[(size_t)out * n_patt + p] = lnf[(size_t)row * stride + p];
         }
      }
   }

   // the plain restatement: every enlarged tree pruned from its root; row n_rows: the tree as it stands
   double worst = 0, worst_l = 0;
   std::vector<double> part(n);
   for (long row = 0; row <= n_rows; row++) {
      const int j = (int)(row % n_pend), i = (int)(row / n_pend % n_edges), qi = (int)(row / ((long)n_pend * n_edges));
      Big b{};
      b.t = &t; b.z = z.data(); b.n_patt = n_patt; b.mask = mask.data(); b.v = -1;
      b.sons.assign(nn + 2, std::vector<int>());
      for (int v = 0; v < nn; v++) b.sons[v].assign(t.sons.begin() + t.sons_ptr[v], t.sons.begin() + t.sons_ptr[v + 1]);
      if (row < n_rows) {
         const int v = edges[i], fa = father[v];
         for (int &c : b.sons[fa]) if (c == v) c = nn;
         b.sons[nn] = {v, nn + 1};
         b.v = v;
         b.qrow = qz.data() + (size_t)qi * n_patt;
      }
      double lnL = 0;
      for (long h = 0; h < n_patt; h++) {
         double fh = 0;
         for (int k = 0; k < K; k++) {
            b.P = P.data() + (size_t)k * nn * n * n;
            if (row < n_rows) {
               b.Pup_v = Pup.data() + ((size_t)k * nn + b.v) * n * n;
               b.Pdn_v = Pdn.data() + ((size_t)k * nn + b.v) * n * n;
               b.Ppend = Ppend.data() + ((size_t)k * n_pend + j) * n * n;
            }
            prune(b, n, t.root, h, part.data());
            double s = 0;
            for (int c = 0; c < n; c++) s += pi[c] * part[c];
            fh += freqK[k] * s;
         }
         const double lf = log(fh), d = fabs(lf - got_lnf[(size_t)row * n_patt + h]);
         if (weights[h] > 0) { lnL += weights[h] * lf; worst = d > worst ? d : worst; }
      }
      const double dl = fabs(lnL - got_lnL[row]);
      worst_l = dl > worst_l ? dl : worst_l;
   }
   // the query without data leaves the tree's own values, whatever the edge, the split and the pendant length
   double worst_m = 0;
   for (int i = 0; i < n_edges; i++)
      for (int j = 0; j < n_pend; j++)
         for (long h = 0; h < n_patt; h++) {
            const double d = fabs(got_lnf[(((size_t)2 * n_edges + i) * n_pend + j) * n_patt + h] - got_lnf[(size_t)n_rows * n_patt + h]);
            if (weights[h] > 0) worst_m = d > worst_m ? d : worst_m;
         }
   const bool ok = worst <= 1e-11 && worst_l <= 1e-9 && worst_m <= 1e-11;
   printf("%s: %d states, %d tips, %d patterns, phi %.1f, %d queries x %d edges x %d pendants, edges in groups of %d: largest |lnf - restatement| %.3e, "
          "|lnL - restatement| %.3e, |lnf of the empty query - lnf0| %.3e\n", ok ? "ok" : "FAILED", n, n_tips, n_patt, phi, n_q, n_edges, n_pend, cap, worst, worst_l, worst_m);
   return ok ? 0 : 1;
}

int main()
{
   int bad = 0;
   for (double phi : {0.3, 0.0, 1.0}) {
      bad += run_case<4>(9, 150, 0, phi);
      bad += run_case<20>(7, 70, 3, phi);
   }
   return bad ? 1 : 0;
}

// The per-lane bodies of kernels_attach.h (the down pass it takes from kernels_ancestral.h, the outer pass of kernels_nni.h, the row pass of
// 4 / 5 / 20 states, the combination of the classes of kernels_edge.h) compiled for the HOST and called in a loop over (class or row,
// pattern) — thread indices emulated — so that they run under the host sanitizers:
//     g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -DATTACH_HOST_ONLY tools/attach_host_check.cpp -o attach_host_check
//     ./attach_host_check      (a 4-state, a 5-state and a 20-state problem made here; exit status 0 and "ok" lines when every number agrees)
// The reference is inside this program: for every row the enlarged tree is built (a new internal node on the branch, the query as a new
// tip) and pruned by a plain recursion in the linear domain (no scaling), class by class, at the row's three lengths.  d1 is held against
// the central difference of that reference's lnL along the role's length (step 1e-5, every length >= 0.05), d2 against the central difference of the bodies' own
// d1 at the same two lengths; the shifted rows are rows of the same call.  The trees are unrooted with a polytomy, the tips and the
// queries carry ambiguity codes, two classes, scaling marks at every second internal node; the 20-state problem also walks the rows in
// groups that cut the runs of a node's rows.  Matrices: P(t) = exp(t Q_k) by a scaled Taylor series of a random rate matrix Q_k that is not
// reversible, dP = Q_k P, d2P = Q_k Q_k P; the pendant has a rate matrix of its own.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../paml_amd/csrc/kernels_attach.h"

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

static void matmul(const double *A, const double *B, int n, double *out)
{
   for (int r = 0; r < n; r++)
      for (int c = 0; c < n; c++) {
         double x = 0;
         for (int j = 0; j < n; j++) x += A[r * n + j] * B[j * n + c];
         out[r * n + c] = x;
      }
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
      matmul(term.data(), A.data(), n, tmp.data());
      for (int i = 0; i < n * n; i++) term[i] = tmp[i] / it;
      for (int i = 0; i < n * n; i++) sum[i] += term[i];
   }
   for (int it = 0; it < sq; it++) {
      matmul(sum.data(), sum.data(), n, tmp.data());
      sum = tmp;
   }
   for (int i = 0; i < n * n; i++) out[i] = sum[i];
}

// the enlarged tree as the reference prunes it: node ids of the tree, plus nn = the new internal node and nn + 1 = the query tip
struct Big {
   const Tree *t;
   std::vector<std::vector<int>> sons;      // [nn + 2]
   const double *P, *Pup_v, *Pdn_v, *Ppend;     // the class's [nn][n * n]; the three matrices of this row
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

template <int N> static int run_case(int n_tips, int n_patt, int cap)
{
   const int n = N, K = 2, n_q = 3;
   const double step = 1e-5;
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

   // the rows in the caller's order: every edge in an order of its own, the four roles, and for a role the two shifted rows
   std::vector<int> rows;       // [n_rows][3] = q, v, role
   std::vector<double> t3;      // [n_rows][3]
   std::vector<double> len(nn);
   for (int v = 0; v < nn; v++) len[v] = 0.2 + 0.3 * rnd();
   for (int v = nn - 1; v >= 0; v--) {
      if (v == t.root) continue;
      const double base[3] = {len[v] / 2 * (0.5 + 1.5 * rnd()), len[v] / 2 * (0.5 + 1.5 * rnd()), 0.1 * (0.5 + 1.5 * rnd())};
      for (int role = -1; role <= 2; role++)
         for (int s = 0; s < (role < 0 ? 1 : 3); s++) {      // s = 1, 2: the role's length + step, - step
            rows.insert(rows.end(), {(v + role + 1) % n_q, v, role});
            for (int j = 0; j < 3; j++) t3.push_back(base[j] + (j == role && s ? (s == 1 ? step : -step) : 0.0));
         }
   }
   const int n_rows = (int)rows.size() / 3;
   if (cap <= 0 || cap > n_rows) cap = n_rows;
   std::vector<int> order(n_rows), srows((size_t)4 * n_rows);      // sorted by node, then the caller's index (paml_amd_attach_scores)
   for (int i = 0; i < n_rows; i++) order[i] = i;
   std::sort(order.begin(), order.end(), [&](int x, int y) { return rows[3 * x + 1] != rows[3 * y + 1] ? rows[3 * x + 1] < rows[3 * y + 1] : x < y; });
   for (int i = 0; i < n_rows; i++) {
      const int c = order[i];
      srows[4 * i] = rows[3 * c + 1]; srows[4 * i + 1] = rows[3 * c]; srows[4 * i + 2] = rows[3 * c + 2]; srows[4 * i + 3] = c;
   }

   std::vector<double> pi(n), freqK = {0.3, 0.7}, weights(n_patt);
   std::vector<double> P((size_t)K * nn * n * n), AM((size_t)n_rows * K * ATTACH_MATS * n * n, 0.0), tmp((size_t)n * n);
   for (int k = 0; k < K; k++) {
      std::vector<double> Q((size_t)n * n), Qp((size_t)n * n);      // rate matrices that are not reversible: the tree's and the pendant's
      for (auto *M : {&Q, &Qp})
         for (int r = 0; r < n; r++) {
            double tot = 0;
            for (int c = 0; c < n; c++)
               if (c != r) { (*M)[r * n + c] = (0.2 + rnd()) * (1 + k) / n; tot += (*M)[r * n + c]; }
            (*M)[r * n + r] = -tot;
         }
      for (int v = 0; v < nn; v++) expm(Q, n, len[v], P.data() + ((size_t)k * nn + v) * n * n);
      for (int i = 0; i < n_rows; i++) {
         const int c = srows[4 * i + 3], role = srows[4 * i + 2];
         double *am = AM.data() + ((size_t)i * K + k) * ATTACH_MATS * n * n;
         for (int j = 0; j < 3; j++) expm(j == 2 ? Qp : Q, n, t3[3 * c + j], am + (size_t)j * n * n);
         if (role >= 0) {
            const std::vector<double> &R = role == 2 ? Qp : Q;
            matmul(R.data(), am + (size_t)role * n * n, n, am + (size_t)3 * n * n);
            matmul(R.data(), am + (size_t)3 * n * n, n, am + (size_t)4 * n * n);
         }
      }
   }
   double tot = 0;
   for (int c = 0; c < n; c++) { pi[c] = 0.2 + rnd(); tot += pi[c]; }
   for (int c = 0; c < n; c++) pi[c] /= tot;
   for (int h = 0; h < n_patt; h++) weights[h] = h % 5 == 2 ? 0.0 : 1.0 + (int)(rnd() * 4);

   const long stride = (n_patt + ANC_TILE - 1) / ANC_TILE * ANC_TILE;
   std::vector<double> L((size_t)K * n_int * n * stride), G(L.size()), SL((size_t)K * n_int * stride), SG(SL.size());
   std::vector<double> f((size_t)K * (cap + 1) * stride), f1(f.size()), f2(f.size()), sig(f.size()), lnf((size_t)(cap + 1) * stride), g1(lnf.size()), g2(lnf.size());
   std::vector<double> got_lnf((size_t)(n_rows + 1) * n_patt), got_lnL(n_rows + 1, 0.0), got_d1(n_rows, 0.0), got_d2(n_rows, 0.0);
   AttachArgs a{};
   NniArgs &o = a.e.o;
   AncMargArgs &m = o.m;
   m.t = AncTree{t.sons_ptr.data(), t.sons.data(), father.data(), post.data(), pre.data(), scale.data(), (int)post.size(), (int)pre.size(), nn, n_tips, n_int, t.root};
   m.n = n; m.K = K; m.gene = 0; m.scaled = 1; m.n_pi = 1; m.h0 = 0; m.nb = n_patt; m.stride = stride;
   m.z = z.data(); m.z_stride = n_patt; m.code_mask = mask.data(); m.P = P.data(); m.pi = pi.data(); m.freqK = freqK.data();
   m.L = L.data(); m.G = G.data(); m.SL = SL.data(); m.SG = SG.data(); m.mfma = 0;
   o.cap = cap; o.n_swaps = n_rows; o.f = f.data(); o.sig = sig.data(); o.weights = weights.data(); o.lnf = lnf.data();
   o.ref_node = t.sons[t.sons_ptr[t.root]];
   a.e.f1 = f1.data(); a.e.f2 = f2.data(); a.e.g1 = g1.data(); a.e.g2 = g2.data(); a.e.psets = K;
   a.rows = srows.data(); a.AM = AM.data(); a.qz = qz.data(); a.psets = K;
   for (int k = 0; k < K; k++)
      for (long p = 0; p < n_patt; p++) anc_lane_down<N>(m, k, p);
   for (int k = 0; k < K; k++)
      for (long p = 0; p < n_patt; p++) nni_lane_outer<N>(o, k, p);
   for (long p = 0; p < n_patt; p++) {
      got_lnL[n_rows] += nni_combine(o, cap, p);
      got_lnf[(size_t)n_rows * n_patt + p] = lnf[(size_t)cap * stride + p];
   }
   for (int r0 = 0; r0 < n_rows; r0 += cap) {
      const int ng = r0 + cap <= n_rows ? cap : n_rows - r0;
      o.swap0 = r0; o.n_group = ng;
      for (int i = 0; i < ng; i++)      // (the device: a grid layer per row, the layer of a row that starts a run walks the run)
         if (attach_run_start(a, i))
            for (int k = 0; k < K; k++)
               for (long p = 0; p < n_patt; p++) attach_lane_node<N>(a, k, p, i);
      for (int i = 0; i < ng; i++) {      // (the device adds a chunk's 64 patterns in a butterfly and the chunks in a fixed order: another order of the same sum)
         const int out = srows[4 * (r0 + i) + 3];
         for (long p = 0; p < n_patt; p++) {
            double acc[3];
            edge_combine(a.e, i, p, acc);
            got_lnL[out] += acc[0]; got_d1[out] += acc[1]; got_d2[out] += acc[2];
            got_lnf[(size_t)out * n_patt + p] = lnf[(size_t)i * stride + p];
         }
      }
   }

   // the plain restatement: every enlarged tree pruned from its root at the row's lengths; row n_rows: the tree as it stands
   double worst = 0, worst_l = 0;
   std::vector<double> part(n), ref_lnL(n_rows + 1, 0.0);
   std::vector<int> sorted_of(n_rows);
   for (int i = 0; i < n_rows; i++) sorted_of[srows[4 * i + 3]] = i;
   for (int row = 0; row <= n_rows; row++) {
      Big b{};
      b.t = &t; b.z = z.data(); b.n_patt = n_patt; b.mask = mask.data(); b.v = -1;
      b.sons.assign(nn + 2, std::vector<int>());
      for (int v = 0; v < nn; v++) b.sons[v].assign(t.sons.begin() + t.sons_ptr[v], t.sons.begin() + t.sons_ptr[v + 1]);
      if (row < n_rows) {
         const int v = rows[3 * row + 1], fa = father[v];
         for (int &c : b.sons[fa]) if (c == v) c = nn;
         b.sons[nn] = {v, nn + 1};
         b.v = v;
         b.qrow = qz.data() + (size_t)rows[3 * row] * n_patt;
      }
      for (long h = 0; h < n_patt; h++) {
         double fh = 0;
         for (int k = 0; k < K; k++) {
            b.P = P.data() + (size_t)k * nn * n * n;
            if (row < n_rows) {
               const double *am = AM.data() + ((size_t)sorted_of[row] * K + k) * ATTACH_MATS * n * n;
               b.Pup_v = am; b.Pdn_v = am + (size_t)n * n; b.Ppend = am + (size_t)2 * n * n;
            }
            prune(b, n, t.root, h, part.data());
            double s = 0;
            for (int c = 0; c < n; c++) s += pi[c] * part[c];
            fh += freqK[k] * s;
         }
         const double lf = log(fh), d = fabs(lf - got_lnf[(size_t)row * n_patt + h]);
         if (weights[h] > 0) {
            ref_lnL[row] += weights[h] * lf;
            worst = d > worst ? d : worst;
         }
      }
      const double dl = fabs(ref_lnL[row] - got_lnL[row]);
      worst_l = dl > worst_l ? dl : worst_l;
   }
   // the derivatives: a base row with a role is followed by its two shifted rows; role -1: both exactly 0
   double worst_1 = 0, worst_2 = 0, largest = 0;
   bool zeros = true;
   for (int row = 0; row < n_rows; row++) {
      if (rows[3 * row + 2] < 0) { zeros = zeros && got_d1[row] == 0 && got_d2[row] == 0; continue; }
      const double fd1 = (ref_lnL[row + 1] - ref_lnL[row + 2]) / (2 * step), fd2 = (got_d1[row + 1] - got_d1[row + 2]) / (2 * step);
      const double e1 = fabs(got_d1[row] - fd1) / fmax(1.0, fabs(fd1)), e2 = fabs(got_d2[row] - fd2) / fmax(1.0, fabs(fd2));
      worst_1 = e1 > worst_1 ? e1 : worst_1;
      worst_2 = e2 > worst_2 ? e2 : worst_2;
      largest = fmax(largest, fmax(fabs(got_d1[row]), fabs(got_d2[row])));
      row += 2;
   }
   // the differences' own error: truncation step^2 / 6 x the derivative two orders above the one differenced, which along a branch of
   // length t >= 0.05 reaches ~ 3 / t = 60 times the largest second derivative met (~ 7e3): 1e-10 / 6 x 4e5 ~ 7e-6 at the worst, against
   // max(1, |d|); rounding 1e-12 / step = 1e-7.  Allowance 1e-5; a wrong factor for a role is off by the order of d itself
   const bool ok = worst <= 1e-11 && worst_l <= 1e-9 && zeros && worst_1 <= 1e-5 && worst_2 <= 1e-5 && largest > 1;
   printf("%s: %d states, %d tips, %d patterns, %d rows in groups of %d: largest |lnf - restatement| %.3e, |lnL - restatement| %.3e; "
          "d1, d2 against central differences, relative to max(1, |d|): %.3e, %.3e (largest |d| %.3e); role -1 gives zeros: %s\n",
          ok ? "ok" : "FAILED", n, n_tips, n_patt, n_rows, cap, worst, worst_l, worst_1, worst_2, largest, zeros ? "yes" : "NO");
   return ok ? 0 : 1;
}

int main()
{
   int bad = 0;
   bad += run_case<4>(9, 150, 0);
   bad += run_case<5>(6, 70, 0);
   bad += run_case<20>(7, 70, 5);
   return bad ? 1 : 0;
}

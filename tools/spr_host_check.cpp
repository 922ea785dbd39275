// The per-lane bodies of kernels_spr.h (the down pass it takes from kernels_ancestral.h, the outer pass of kernels_nni.h, the walk over
// a prune's steps of 4 / 5 / 20 states, the combination of the classes) and the host's lists of steps (spr_plan.h) compiled for the
// HOST and called in a loop over (class or row, pattern) — thread indices emulated — so that they run under the host sanitizers:
//     g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -DSPR_HOST_ONLY tools/spr_host_check.cpp -o spr_host_check
//     ./spr_host_check            (a 4-state and a 20-state problem made here; exit status 0 and "ok" lines when every number agrees)
// The reference is inside this program: every move of the canonical list is carried out on a copy of the son lists, with the matrices
// of the three changed branches put in their places, and the rearranged tree is pruned by a plain recursion in the linear domain (no
// scaling), class by class.  The trees are unrooted with a polytomy away from the moves, the tips carry ambiguity codes, two classes,
// scaling marks at every second internal node, P(t) = exp(Q r_k t) of a rate matrix that is not reversible; the splits are 0.3, 0 and 1,
// and the 20-state problem walks the moves in groups of whole prunes.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../paml_amd/csrc/kernels_spr.h"

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

// tips 0 .. n_tips - 1; the root has three sons, below it a ladder of binary nodes with a cherry hung on every second of them, and at its
// end a node with three tips (a polytomy: its sons cannot be pruned, every other non-root node below the root's sons can)
static Tree make_tree(int n_ladder)
{
   std::vector<std::vector<int>> s;
   int n_tips = 2 + 3;
   for (int i = 0; i < n_ladder; i++) n_tips += i % 2 ? 2 : 1;
   int tip = 0, node = n_tips;
   Tree t;
   t.n_tips = n_tips; t.root = node++;
   s.assign(4 * n_tips, {});
   s[t.root] = {tip, tip + 1, node};
   tip += 2;
   for (int i = 0; i < n_ladder; i++) {
      const int v = node++;
      if (i % 2) {
         const int ch = node++;
         s[ch] = {tip, tip + 1};
         tip += 2;
         s[v] = {ch, node};
      }
      else s[v] = {node, tip++};
   }
   s[node] = {tip, tip + 1, tip + 2};
   t.nn = node + 1;
   t.sons_ptr.assign(1, 0);
   for (int v = 0; v < t.nn; v++) {
      for (int c : s[v]) t.sons.push_back(c);
      t.sons_ptr.push_back((int)t.sons.size());
   }
   return t;
}

// P = exp(Q t): scaling and squaring around a Taylor series
static void expm(const std::vector<double> &Q, int n, double t, double *P)
{
   int sq = 0;
   double nrm = 0;
   for (double q : Q) nrm = fmax(nrm, fabs(q * t));
   while (nrm * n > 0.25) { nrm /= 2; t /= 2; sq++; }
   std::vector<double> term(n * n, 0.0), next(n * n), sum(n * n, 0.0);
   for (int i = 0; i < n; i++) term[i * n + i] = sum[i * n + i] = 1;
   for (int it = 1; it <= 24; it++) {
      for (int i = 0; i < n; i++)
         for (int j = 0; j < n; j++) {
            double a = 0;
            for (int l = 0; l < n; l++) a += term[i * n + l] * Q[l * n + j];
            next[i * n + j] = a * t / it;
         }
      term = next;
      for (int i = 0; i < n * n; i++) sum[i] += term[i];
   }
   for (; sq > 0; sq--) {
      for (int i = 0; i < n; i++)
         for (int j = 0; j < n; j++) {
            double a = 0;
            for (int l = 0; l < n; l++) a += sum[i * n + l] * sum[l * n + j];
            next[i * n + j] = a;
         }
      sum = next;
   }
   for (int i = 0; i < n * n; i++) P[i] = sum[i];
}

// the partial of node v on the tree (sons_ptr, sons) with the nodes' matrices Pn[v] at pattern h, linear domain
static void prune(const Tree &t, const std::vector<int> &sons, int n, int v, const std::vector<const double *> &Pn, const unsigned char *z, int n_patt,
                  const unsigned long long *mask, long h, double *out)
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
      prune(t, sons, n, s, Pn, z, n_patt, mask, h, l.data());
      for (int y = 0; y < n; y++) {
         double m = 0;
         for (int c = 0; c < n; c++) m += Pn[s][y * n + c] * l[c];
         out[y] *= m;
      }
   }
}

template <int N> static int run_case(int n_ladder, int n_patt, int cap, double phi)
{
   const int n = N, K = 2;
   const Tree t = make_tree(n_ladder);
   const int nn = t.nn, n_tips = t.n_tips, n_int = nn - n_tips, n_codes = n + 3;
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
   // a rate matrix that is not reversible, two class rates, the four families of lengths
   std::vector<double> Q(n * n), branch(nn), pi(n), freqK = {0.3, 0.7}, rateK = {0.4, 1.6}, weights(n_patt);
   for (int r = 0; r < n; r++) {
      double tot = 0;
      for (int c = 0; c < n; c++)
         if (c != r) { Q[r * n + c] = (0.2 + rnd()) / n * (c > r ? 1.7 : 0.6); tot += Q[r * n + c]; }
      Q[r * n + r] = -tot;
   }
   for (int v = 0; v < nn; v++) branch[v] = 0.05 + 0.3 * rnd();
   const size_t fam = (size_t)K * nn * n * n;
   std::vector<double> P(fam), Pup(fam), Pdn(fam), Pm(fam);
   for (int k = 0; k < K; k++)
      for (int v = 0; v < nn; v++) {
         const size_t at = ((size_t)k * nn + v) * n * n;
         const double tm = branch[v] + (father[v] >= 0 && father[v] != t.root ? branch[father[v]] : 0.0);
         expm(Q, n, rateK[k] * branch[v], P.data() + at);
         expm(Q, n, rateK[k] * (1 - phi) * branch[v], Pup.data() + at);
         expm(Q, n, rateK[k] * phi * branch[v], Pdn.data() + at);
         expm(Q, n, rateK[k] * tm, Pm.data() + at);
      }
   double tot = 0;
   for (int c = 0; c < n; c++) { pi[c] = 0.2 + rnd(); tot += pi[c]; }
   for (int c = 0; c < n; c++) pi[c] /= tot;
   for (int h = 0; h < n_patt; h++) weights[h] = h % 5 == 2 ? 0.0 : 1.0 + (int)(rnd() * 4);

   const SprTreeView view{n_tips, nn, t.root, t.sons_ptr.data(), t.sons.data()};
   const int n_moves = spr_list(view, 0, nullptr, 0);
   if (n_moves < 1) { printf("FAILED: no moves\n"); return 1; }
   std::vector<int> moves(2 * (size_t)n_moves);
   if (spr_list(view, 0, moves.data(), n_moves) != n_moves) { printf("FAILED: the list changed its length\n"); return 1; }
   for (int i = 0; i + 1 < n_moves; i += 2) {      // not the sorted order: the plan sorts, the rows go back by plan.order
      std::swap(moves[2 * i], moves[2 * (n_moves - 1 - i)]);
      std::swap(moves[2 * i + 1], moves[2 * (n_moves - 1 - i) + 1]);
   }
   for (int i = 0; i < n_moves; i++)
      if (!spr_check_move(view, father, moves[2 * i], moves[2 * i + 1]).empty()) { printf("FAILED: the list holds an invalid move\n"); return 1; }
   SprPlan plan;
   spr_plan(view, father, n_moves, moves.data(), plan);
   if (cap <= 0 || cap > n_moves) cap = n_moves;
   if (cap < plan.max_rows) cap = plan.max_rows;

   const long stride = (n_patt + ANC_TILE - 1) / ANC_TILE * ANC_TILE;
   std::vector<double> L((size_t)K * n_int * n * stride), G(L.size()), Lp(L.size()), Ap(L.size());
   std::vector<double> SL((size_t)K * n_int * stride), SG(SL.size()), SLp(SL.size()), SAp(SL.size());
   std::vector<double> f((size_t)K * (cap + 1) * stride), sig(f.size()), lnf((size_t)(cap + 1) * stride);
   std::vector<double> got_lnf((size_t)(n_moves + 1) * n_patt), got_lnL(n_moves + 1, 0.0);
   SprArgs a{};
   NniArgs &o = a.o;
   AncMargArgs &m = o.m;
   m.t = AncTree{t.sons_ptr.data(), t.sons.data(), father.data(), post.data(), pre.data(), scale.data(), (int)post.size(), (int)pre.size(), nn, n_tips, n_int, t.root};
   m.n = n; m.K = K; m.gene = 0; m.scaled = 1; m.n_pi = 1; m.h0 = 0; m.nb = n_patt; m.stride = stride;
   m.z = z.data(); m.z_stride = n_patt; m.code_mask = mask.data(); m.P = P.data(); m.pi = pi.data(); m.freqK = freqK.data();
   m.L = L.data(); m.G = G.data(); m.SL = SL.data(); m.SG = SG.data(); m.mfma = 0;
   o.cap = cap; o.n_swaps = n_moves; o.f = f.data(); o.sig = sig.data(); o.weights = weights.data(); o.lnf = lnf.data();
   o.ref_node = t.sons[t.sons_ptr[t.root]];
   a.Pup = Pup.data(); a.Pdn = Pdn.data(); a.Pm = Pm.data();
   a.prunes = plan.prunes.data(); a.steps = plan.steps.data(); a.factors = plan.factors.data();
   a.Lp = Lp.data(); a.Ap = Ap.data(); a.SLp = SLp.data(); a.SAp = SAp.data();
   for (int k = 0; k < K; k++)
      for (long p = 0; p < n_patt; p++) anc_lane_down<N>(m, k, p);
   for (int k = 0; k < K; k++)
      for (long p = 0; p < n_patt; p++) nni_lane_outer<N>(o, k, p);
   int n_groups = 0;
   for (int ip0 = 0; ip0 < plan.n_prunes();) {      // groups of whole prunes, as engine_spr.hip forms them
      int ip1 = ip0, rows = 0;
      auto row_of = [&](int ip) { return ip < plan.n_prunes() ? plan.prunes[SPR_PRUNE_INTS * ip + 3] : n_moves; };
      while (ip1 < plan.n_prunes() && rows + row_of(ip1 + 1) - row_of(ip1) <= cap) { rows += row_of(ip1 + 1) - row_of(ip1); ip1++; }
      const int r0 = row_of(ip0);
      o.swap0 = r0; o.n_group = rows;
      for (int k = 0; k < K; k++)
         for (long p = 0; p < n_patt; p++)
            for (int ip = ip0; ip < ip1; ip++) spr_lane_prune<N>(a, k, p, ip);
      for (int row = 0; row < rows + (ip0 == 0 ? 1 : 0); row++) {      // (the device adds a chunk's 64 patterns in a butterfly and the chunks in a fixed order: another order of the same sum)
         const int wr = row == rows ? cap : row, out = row == rows ? n_moves : plan.order[r0 + row];
         for (long p = 0; p < n_patt; p++) {
            got_lnL[out] += nni_combine(o, wr, p);
            got_lnf[(size_t)out * n_patt + p] = lnf[(size_t)wr * stride + p];
         }
      }
      ip0 = ip1;
      n_groups++;
   }

   // the plain restatement: every rearranged tree pruned from its root
   double worst = 0, worst_l = 0;
   std::vector<double> part(n);
   for (int i = 0; i <= n_moves; i++) {
      std::vector<int> sons = t.sons;
      int s = -1, x = -1, fa = -1, c = -1;
      if (i < n_moves) {
         s = moves[2 * i]; x = moves[2 * i + 1]; fa = father[s]; c = spr_sibling(view, father, s);
         const int g = father[fa], fx = father[x] == fa ? g : father[x];
         for (int j = t.sons_ptr[g]; j < t.sons_ptr[g + 1]; j++) if (sons[j] == fa) { sons[j] = c; break; }
         for (int j = t.sons_ptr[fx]; j < t.sons_ptr[fx + 1]; j++) if (sons[j] == x) { sons[j] = fa; break; }
         sons[t.sons_ptr[fa]] = x; sons[t.sons_ptr[fa] + 1] = s;
      }
      double lnL = 0;
      for (long h = 0; h < n_patt; h++) {
         double fh = 0;
         for (int k = 0; k < K; k++) {
            std::vector<const double *> Pn(nn);
            for (int v = 0; v < nn; v++) Pn[v] = P.data() + ((size_t)k * nn + v) * n * n;
            if (i < n_moves) {
               Pn[c] = Pm.data() + ((size_t)k * nn + c) * n * n;
               Pn[fa] = Pup.data() + ((size_t)k * nn + x) * n * n;
               Pn[x] = Pdn.data() + ((size_t)k * nn + x) * n * n;
            }
            prune(t, sons, n, t.root, Pn, z.data(), n_patt, mask.data(), h, part.data());
            double sum = 0;
            for (int st = 0; st < n; st++) sum += pi[st] * part[st];
            fh += freqK[k] * sum;
         }
         const double lf = log(fh), d = fabs(lf - got_lnf[(size_t)i * n_patt + h]);
         if (weights[h] > 0) { lnL += weights[h] * lf; worst = d > worst ? d : worst; }
      }
      const double dl = fabs(lnL - got_lnL[i]);
      worst_l = dl > worst_l ? dl : worst_l;
   }
   const bool ok = worst <= 1e-11 && worst_l <= 1e-9;
   printf("%s: %d states, %d tips, %d patterns, phi %.1f, %d moves of %d prunes in %d groups (rows %d): largest |lnf - restatement| %.3e, |lnL - restatement| %.3e\n",
          ok ? "ok" : "FAILED", n, n_tips, n_patt, phi, n_moves, plan.n_prunes(), n_groups, cap, worst, worst_l);
   return ok ? 0 : 1;
}

int main()
{
   int bad = 0;
   bad += run_case<4>(5, 150, 0, 0.3);
   bad += run_case<4>(4, 70, 0, 0.0);
   bad += run_case<4>(4, 70, 7, 1.0);
   bad += run_case<20>(3, 40, 9, 0.3);
   return bad ? 1 : 0;
}

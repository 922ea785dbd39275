// The plan of hessian_plan.h and the per-lane bodies of kernels_hessian.h (on the down pass of kernels_ancestral.h and the outer pass of
// kernels_gradient.h at CURV = true, 4 / 5 / 20 states) compiled for the HOST and called in a loop over (class or row, pattern) — thread
// indices emulated — so that they run under the host sanitizers:
//     g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -DHESS_HOST_ONLY tools/hessian_host_check.cpp -o hessian_host_check
//     python tools/hessian_host_check.py ./hessian_host_check      (writes the cases, runs this, compares with tests/hessian_ref.py)
// usage: hessian_host_check run IN OUT.  IN: int32 n, K, n_nodes, n_tips, root, n_patt, n_codes, scaled, n_sons, n_list, cap; int32
//   sons_ptr[n_nodes + 1], sons[n_sons], scale[n_nodes], nodes[n_list]; uint8 z[n_tips][n_patt]; uint64 mask[n_codes]; double
//   P[K][n_nodes][n][n], dP likewise, d2P likewise, pi[n], freqK[K], weights[n_patt].  n_list = 0: every node.  cap: the most rows of a
//   group of sources (0: all pairs in one group).  OUT: double lnf[n_patt], grad[n_nodes], curv[n_nodes], lnL, hess[dim][dim].
// usage: hessian_host_check plan IN OUT.  IN: int32 n_tips, n_nodes, root, n_sons, n_list; sons_ptr, sons, nodes.  OUT: int32 n_sources,
//   n_steps, n_factors, n_pairs; sources, steps, factors, pairs as hessian_plan.h lays them out.  A list the plan refuses: exit code 3.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../paml_amd/csrc/kernels_hessian.h"

using namespace paml_amd;

template <typename T> static std::vector<T> rd(FILE *f, size_t n)
{
   std::vector<T> v(n);
   if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short input\n"); exit(2); }
   return v;
}

template <int N> static void passes(GradArgs &a)
{
   for (int k = 0; k < a.m.K; k++)
      for (long p = 0; p < a.m.nb; p++) anc_lane_down<N>(a.m, k, p);
   for (int k = 0; k < a.m.K; k++)
      for (long p = 0; p < a.m.nb; p++) grad_lane_outer<N, true>(a, k, p);
}

template <int N> static void sources(const HessArgs &a)
{
   for (int k = 0; k < a.g.m.K; k++)
      for (long p = 0; p < a.g.m.nb; p++)
         for (int is = a.source0; is < a.source0 + a.n_sources; is++) hess_lane_source<N>(a, k, p, is);
}

static int plan_mode(const char *in, const char *out)
{
   FILE *f = fopen(in, "rb");
   if (!f) { perror(in); return 2; }
   const std::vector<int> hd = rd<int>(f, 5);
   const int n_tips = hd[0], nn = hd[1], root = hd[2], n_sons = hd[3], n_list = hd[4];
   const std::vector<int> sons_ptr = rd<int>(f, nn + 1), sons = rd<int>(f, n_sons), nodes = rd<int>(f, n_list);
   fclose(f);
   const HessTreeView view{n_tips, nn, root, sons_ptr.data(), sons.data()};
   std::vector<int> father, pre;
   if (!hess_fathers(view, father, pre)) return 3;
   const std::string why = hess_check_nodes(view, nodes.data(), n_list);
   if (!why.empty()) { fprintf(stderr, "%s\n", why.c_str()); return 3; }
   HessPlan plan;
   hess_plan(view, father, pre, n_list, nodes.data(), plan);
   f = fopen(out, "wb");
   if (!f) { perror(out); return 2; }
   const int sz[4] = {plan.n_sources(), (int)plan.steps.size() / HESS_STEP_INTS, (int)plan.factors.size() / 2, plan.n_pairs()};
   fwrite(sz, sizeof(int), 4, f);
   for (const std::vector<int> *v : {&plan.sources, &plan.steps, &plan.factors, &plan.pairs}) fwrite(v->data(), sizeof(int), v->size(), f);
   fclose(f);
   return 0;
}

int main(int argc, char **argv)
{
   if (argc == 4 && !strcmp(argv[1], "plan")) return plan_mode(argv[2], argv[3]);
   if (argc != 4 || strcmp(argv[1], "run")) { fprintf(stderr, "usage: %s run|plan IN OUT\n", argv[0]); return 2; }
   FILE *f = fopen(argv[2], "rb");
   if (!f) { perror(argv[2]); return 2; }
   const std::vector<int> hd = rd<int>(f, 11);
   const int n = hd[0], K = hd[1], nn = hd[2], n_tips = hd[3], root = hd[4], n_patt = hd[5], n_codes = hd[6], scaled = hd[7], n_sons = hd[8], n_list = hd[9];
   const int n_int = nn - n_tips;
   const std::vector<int> sons_ptr = rd<int>(f, nn + 1), sons = rd<int>(f, n_sons), scale = rd<int>(f, nn), nodes = rd<int>(f, n_list);
   const std::vector<unsigned char> z = rd<unsigned char>(f, (size_t)n_tips * n_patt);
   const std::vector<unsigned long long> mask = rd<unsigned long long>(f, n_codes);
   const size_t pm = (size_t)K * nn * n * n;
   const std::vector<double> P = rd<double>(f, pm), dP = rd<double>(f, pm), d2P = rd<double>(f, pm), pi = rd<double>(f, n), freqK = rd<double>(f, K),
                             weights = rd<double>(f, n_patt);
   fclose(f);
   if (n != 4 && n != 5 && n != 20) { fprintf(stderr, "no lane kernel for %d states\n", n); return 2; }

   const HessTreeView view{n_tips, nn, root, sons_ptr.data(), sons.data()};
   std::vector<int> father, all_pre, pre, post, list(nodes);
   if (!hess_fathers(view, father, all_pre)) { fprintf(stderr, "not a tree\n"); return 2; }
   for (int v : all_pre)      // the orders of anc_tree_pack (engine_ancestral.hip)
      if (v >= n_tips && v != root) pre.push_back(v);
   post.assign(pre.rbegin(), pre.rend());
   post.push_back(root);
   if (n_list == 0)
      for (int v = 0; v < nn; v++)
         if (v != root) list.push_back(v);
   const std::string why = hess_check_nodes(view, list.data(), (int)list.size());
   if (!why.empty()) { fprintf(stderr, "%s\n", why.c_str()); return 3; }
   HessPlan plan;
   hess_plan(view, father, all_pre, (int)list.size(), list.data(), plan);
   const int n_pairs = plan.n_pairs(), cap = std::max(1, std::max(plan.max_rows, hd[10] > 0 ? std::min(hd[10], n_pairs) : n_pairs));

   // the workspace at exactly the sizes paml_amd_hessian allocates for one batch
   const long stride = (n_patt + ANC_TILE - 1) / ANC_TILE * ANC_TILE;
   std::vector<double> L((size_t)K * n_int * n * stride), G(L.size()), SL((size_t)K * n_int * stride), SG(SL.size()), Lp(L.size()), Ap(L.size()), SLp(SL.size()), SAp(SL.size());
   std::vector<double> num((size_t)K * nn * stride), den(num.size()), cur(num.size()), sig(num.size()), lnf(stride), scores((size_t)nn * stride), tot(2 * nn + 1, 0.0);
   std::vector<double> mm((size_t)K * cap * stride), msig(mm.size()), total(std::max(n_pairs, 1), 0.0);
   HessArgs a{};
   GradArgs &g = a.g;
   AncMargArgs &m = g.m;
   m.t = AncTree{sons_ptr.data(), sons.data(), father.data(), post.data(), pre.data(), scale.data(), (int)post.size(), (int)pre.size(), nn, n_tips, n_int, root};
   m.n = n; m.K = K; m.gene = 0; m.scaled = scaled; m.n_pi = 1; m.h0 = 0; m.nb = n_patt; m.stride = stride;
   m.z = z.data(); m.z_stride = n_patt; m.code_mask = mask.data(); m.P = P.data(); m.pi = pi.data(); m.freqK = freqK.data();
   m.L = L.data(); m.G = G.data(); m.SL = SL.data(); m.SG = SG.data(); m.mfma = 0;
   g.dP = dP.data(); g.d2P = d2P.data(); g.num = num.data(); g.den = den.data(); g.cur = cur.data(); g.sig = sig.data(); g.weights = weights.data();
   g.lnf = lnf.data(); g.scores = scores.data(); g.n_chunks = (n_patt + GRAD_CHUNK - 1) / GRAD_CHUNK; g.ref_node = sons[sons_ptr[root]];
   a.sources = plan.sources.data(); a.steps = plan.steps.data(); a.factors = plan.factors.data(); a.pairs = plan.pairs.data();
   a.cap = cap; a.Lp = Lp.data(); a.Ap = Ap.data(); a.SLp = SLp.data(); a.SAp = SAp.data(); a.mm = mm.data(); a.msig = msig.data(); a.total = total.data();
   if (n == 4) passes<4>(g);
   else if (n == 5) passes<5>(g);
   else passes<20>(g);
   for (int row = 0; row <= 2 * nn; row++)      // (the device adds a chunk's 64 patterns in a butterfly and the chunks in a fixed order: another order of the same sum)
      for (long p = 0; p < n_patt; p++) tot[row] += grad_combine<true>(g, row, p);
   for (int v = 0; v < nn; v++)
      for (long p = 0; p < n_patt; p++) hess_score(a, v, p);
   for (int is0 = 0; is0 < plan.n_sources();) {      // the groups: as many whole sources as the rows hold (paml_amd_hessian's rule)
      int is1 = is0, used = 0;
      while (is1 < plan.n_sources()) {
         const int r0 = plan.sources[HESS_SOURCE_INTS * is1 + 3], r1 = is1 + 1 < plan.n_sources() ? plan.sources[HESS_SOURCE_INTS * (is1 + 1) + 3] : n_pairs;
         if (used + (r1 - r0) > cap) break;
         used += r1 - r0;
         is1++;
      }
      a.source0 = is0; a.n_sources = is1 - is0; a.row0 = plan.sources[HESS_SOURCE_INTS * is0 + 3]; a.n_group = used;
      if (n == 4) sources<4>(a);
      else if (n == 5) sources<5>(a);
      else sources<20>(a);
      for (int row = 0; row < a.n_group; row++)
         for (long p = 0; p < n_patt; p++) total[a.row0 + row] += hess_combine(a, row, p);
      is0 = is1;
   }
   const int dim = n_list ? n_list : nn;
   std::vector<int> place(nn, -1);
   for (int i = 0; i < dim; i++) place[n_list ? nodes[i] : i] = i;
   std::vector<double> hess((size_t)dim * dim, 0.0);
   for (int i = 0; i < dim; i++) {
      const int v = n_list ? nodes[i] : i;
      if (v != root) hess[(size_t)i * dim + i] = tot[nn + v];
   }
   for (int r = 0; r < n_pairs; r++) {
      const int i = place[plan.pairs[2 * r]], j = place[plan.pairs[2 * r + 1]];
      hess[(size_t)i * dim + j] = hess[(size_t)j * dim + i] = total[r];
   }

   f = fopen(argv[3], "wb");
   if (!f) { perror(argv[3]); return 2; }
   fwrite(lnf.data(), sizeof(double), n_patt, f);
   fwrite(tot.data(), sizeof(double), 2 * nn + 1, f);
   fwrite(hess.data(), sizeof(double), hess.size(), f);
   fclose(f);
   return 0;
}

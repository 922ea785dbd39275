// The per-lane bodies of kernels_counts.h (the down pass of kernels_ancestral.h, the model gradient's outer pass that stores H_v, the
// scalar rows at the root's first son, the labels' products and the rows' terms) compiled for the HOST and called in a loop over (class
// or query, pattern) — thread indices emulated — so that they run under the host sanitizers:
//     g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -DCOUNTS_HOST_ONLY tools/counts_host_check.cpp -o counts_host_check
//     python tools/counts_host_check.py ./counts_host_check      (writes the cases, runs this, compares with tests/counts_ref.py)
// usage: counts_host_check IN OUT BATCH.  IN: int32 n, K, n_nodes, n_tips, root, n_patt, n_codes, scaled, n_sons, n_lab, n_query; int32
// sons_ptr[n_nodes + 1], sons[n_sons], scale[n_nodes], nodes[n_query]; uint8 z[n_tips][n_patt]; uint64 mask[n_codes]; double
// P[K][n_nodes][n][n], I[K][n_query][n_lab][n][n], pi[n], freqK[K], weights[n_patt].  BATCH: patterns per batch (a multiple of 64).
// OUT: double lnf[n_patt], site[n_lab][n_query][n_patt], counts[n_lab][n_query], lnL.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../paml_amd/csrc/kernels_counts.h"

using namespace paml_amd;

template <typename T> static std::vector<T> rd(FILE *f, size_t n)
{
   std::vector<T> v(n);
   if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short input\n"); exit(2); }
   return v;
}

template <int N> static void batch_of(CountsArgs &a)
{
   ModelGradArgs &g = a.g;
   for (int k = 0; k < g.m.K; k++)
      for (long p = 0; p < g.m.nb; p++) anc_lane_down<N>(g.m, k, p);
   for (int k = 0; k < g.m.K; k++)
      for (long p = 0; p < g.m.nb; p++) mg_lane_outer<N>(g, k, p);
   for (long p = 0; p < g.m.nb; p++) mg_coef(g, g.m.t.n_nodes, p);
   for (int qi = 0; qi < a.n_query; qi++)
      for (long p = 0; p < g.m.nb; p++) counts_lane<N>(a, qi, p);
}

int main(int argc, char **argv)
{
   if (argc != 4) { fprintf(stderr, "usage: %s IN OUT BATCH\n", argv[0]); return 2; }
   FILE *f = fopen(argv[1], "rb");
   if (!f) { perror(argv[1]); return 2; }
   const long batch = atol(argv[3]);
   if (batch < 64 || batch % 64) { fprintf(stderr, "BATCH must be a multiple of 64\n"); return 2; }
   const std::vector<int> hd = rd<int>(f, 11);
   const int n = hd[0], K = hd[1], nn = hd[2], n_tips = hd[3], root = hd[4], n_patt = hd[5], n_codes = hd[6], scaled = hd[7], n_sons = hd[8], n_lab = hd[9], nq = hd[10];
   const int n_int = nn - n_tips;
   const std::vector<int> sons_ptr = rd<int>(f, nn + 1), sons = rd<int>(f, n_sons), scale = rd<int>(f, nn), nodes = rd<int>(f, nq);
   const std::vector<unsigned char> z = rd<unsigned char>(f, (size_t)n_tips * n_patt);
   const std::vector<unsigned long long> mask = rd<unsigned long long>(f, n_codes);
   const std::vector<double> P = rd<double>(f, (size_t)K * nn * n * n), I = rd<double>(f, (size_t)K * nq * n_lab * n * n), pi = rd<double>(f, n), freqK = rd<double>(f, K),
                             weights = rd<double>(f, n_patt);
   fclose(f);
   if (n != 4 && n != 5 && n != 20) { fprintf(stderr, "no lane kernel for %d states\n", n); return 2; }
   if (n_lab < 1 || n_lab > COUNTS_MAX_LABELS) { fprintf(stderr, "n_lab out of range\n"); return 2; }

   // the orders of anc_tree_pack (engine_ancestral.hip)
   std::vector<int> father(nn, -1), pre, post, all_pre, stack(1, root);
   while (!stack.empty()) {
      const int v = stack.back();
      stack.pop_back();
      all_pre.push_back(v);
      for (int j = sons_ptr[v + 1] - 1; j >= sons_ptr[v]; j--) { father[sons[j]] = v; stack.push_back(sons[j]); }
   }
   for (int v : all_pre)
      if (v >= n_tips && v != root) pre.push_back(v);
   post.assign(pre.rbegin(), pre.rend());
   post.push_back(root);

   const long stride = batch;
   const int n_rows = n_lab * nq;
   std::vector<double> L((size_t)K * n_int * n * stride), G(L.size()), SL((size_t)K * n_int * stride), SG(SL.size());
   std::vector<double> H((size_t)K * nn * n * stride), den((size_t)K * nn * stride), sig(den.size());
   std::vector<double> R((size_t)K * n * stride), SR((size_t)K * stride), croot(SR.size()), rows((size_t)(1 + K) * stride), lnf(stride);
   std::vector<double> site((size_t)n_rows * stride), out_lnf(n_patt), out_site((size_t)n_rows * n_patt), total(n_rows + 1, 0.0);
   CountsArgs a{};
   ModelGradArgs &g = a.g;
   AncMargArgs &m = g.m;
   m.t = AncTree{sons_ptr.data(), sons.data(), father.data(), post.data(), pre.data(), scale.data(), (int)post.size(), (int)pre.size(), nn, n_tips, n_int, root};
   m.n = n; m.K = K; m.gene = 0; m.scaled = scaled; m.n_pi = 1; m.stride = stride;
   m.z = z.data(); m.z_stride = n_patt; m.code_mask = mask.data(); m.P = P.data(); m.pi = pi.data(); m.freqK = freqK.data();
   m.L = L.data(); m.G = G.data(); m.SL = SL.data(); m.SG = SG.data(); m.mfma = 0;
   g.H = H.data(); g.den = den.data(); g.sig = sig.data(); g.R = R.data(); g.SR = SR.data(); g.croot = croot.data(); g.rows = rows.data();
   g.lnf = lnf.data(); g.weights = weights.data(); g.ref_node = sons[sons_ptr[root]];
   a.I = I.data(); a.nodes = nodes.data(); a.n_query = nq; a.n_lab = n_lab; a.site = site.data();
   for (long h0 = 0; h0 < n_patt; h0 += batch) {
      const long nb = std::min<long>(batch, n_patt - h0);
      m.h0 = h0; m.nb = nb;
      if (n == 4) batch_of<4>(a);
      else if (n == 5) batch_of<5>(a);
      else batch_of<20>(a);
      for (long p = 0; p < nb; p++) {      // (the device adds a chunk's 64 patterns in a butterfly and the chunks in a fixed order: another order of the same sums)
         total[n_rows] += mg_row_term(g, 0, p);
         out_lnf[h0 + p] = lnf[p];
         for (int r = 0; r < n_rows; r++) {
            total[r] += counts_row_term(a, r, p);
            out_site[(size_t)r * n_patt + h0 + p] = site[(size_t)r * stride + p];
         }
      }
   }

   f = fopen(argv[2], "wb");
   if (!f) { perror(argv[2]); return 2; }
   fwrite(out_lnf.data(), sizeof(double), out_lnf.size(), f);
   fwrite(out_site.data(), sizeof(double), out_site.size(), f);
   fwrite(total.data(), sizeof(double), total.size(), f);
   fclose(f);
   return 0;
}

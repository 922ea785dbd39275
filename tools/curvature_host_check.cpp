// The per-lane bodies of kernels_gradient.h at CURV = true (kernels_curvature.h: the down pass of kernels_ancestral.h, the outer pass with
// both derivatives of 4 / 5 / 20 states, the combination of the classes over its 2 n_nodes + 1 rows) compiled for the HOST and called in a
// loop over (class or row, pattern) — thread indices emulated — so that they run under the host sanitizers:
//     g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -DCURV_HOST_ONLY tools/curvature_host_check.cpp -o curvature_host_check
//     python tools/curvature_host_check.py ./curvature_host_check      (writes the cases, runs this, compares with tests/curvature_ref.py)
// usage: curvature_host_check IN OUT.  IN: int32 n, K, n_nodes, n_tips, root, n_patt, n_codes, scaled, n_sons; int32 sons_ptr[n_nodes + 1],
// sons[n_sons], scale[n_nodes]; uint8 z[n_tips][n_patt]; uint64 mask[n_codes]; double P[K][n_nodes][n][n], dP likewise, d2P likewise, pi[n],
// freqK[K], weights[n_patt].  OUT: double lnf[n_patt], grad[n_nodes], curv[n_nodes], lnL.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../paml_amd/csrc/kernels_curvature.h"

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

int main(int argc, char **argv)
{
   if (argc != 3) { fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
   FILE *f = fopen(argv[1], "rb");
   if (!f) { perror(argv[1]); return 2; }
   const std::vector<int> hd = rd<int>(f, 9);
   const int n = hd[0], K = hd[1], nn = hd[2], n_tips = hd[3], root = hd[4], n_patt = hd[5], n_codes = hd[6], scaled = hd[7], n_sons = hd[8];
   const int n_int = nn - n_tips;
   const std::vector<int> sons_ptr = rd<int>(f, nn + 1), sons = rd<int>(f, n_sons), scale = rd<int>(f, nn);
   const std::vector<unsigned char> z = rd<unsigned char>(f, (size_t)n_tips * n_patt);
   const std::vector<unsigned long long> mask = rd<unsigned long long>(f, n_codes);
   const size_t pm = (size_t)K * nn * n * n;
   const std::vector<double> P = rd<double>(f, pm), dP = rd<double>(f, pm), d2P = rd<double>(f, pm), pi = rd<double>(f, n), freqK = rd<double>(f, K),
                             weights = rd<double>(f, n_patt);
   fclose(f);
   if (n != 4 && n != 5 && n != 20) { fprintf(stderr, "no lane kernel for %d states\n", n); return 2; }

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

   // the workspace at exactly the sizes paml_amd_curvature allocates for one batch: no scores array at CURV
   const long stride = (n_patt + ANC_TILE - 1) / ANC_TILE * ANC_TILE, n_chunks = (n_patt + GRAD_CHUNK - 1) / GRAD_CHUNK;
   std::vector<double> L((size_t)K * n_int * n * stride), G(L.size()), SL((size_t)K * n_int * stride), SG(SL.size());
   std::vector<double> num((size_t)K * nn * stride), den(num.size()), cur(num.size()), sig(num.size()), lnf(stride), tot(2 * nn + 1, 0.0);
   GradArgs a{};
   AncMargArgs &m = a.m;
   m.t = AncTree{sons_ptr.data(), sons.data(), father.data(), post.data(), pre.data(), scale.data(), (int)post.size(), (int)pre.size(), nn, n_tips, n_int, root};
   m.n = n; m.K = K; m.gene = 0; m.scaled = scaled; m.n_pi = 1; m.h0 = 0; m.nb = n_patt; m.stride = stride;
   m.z = z.data(); m.z_stride = n_patt; m.code_mask = mask.data(); m.P = P.data(); m.pi = pi.data(); m.freqK = freqK.data();
   m.L = L.data(); m.G = G.data(); m.SL = SL.data(); m.SG = SG.data(); m.mfma = 0;
   a.dP = dP.data(); a.d2P = d2P.data(); a.num = num.data(); a.den = den.data(); a.cur = cur.data(); a.sig = sig.data(); a.weights = weights.data();
   a.lnf = lnf.data(); a.n_chunks = n_chunks; a.ref_node = sons[sons_ptr[root]];
   if (n == 4) passes<4>(a);
   else if (n == 5) passes<5>(a);
   else passes<20>(a);
   for (int row = 0; row <= 2 * nn; row++)      // (the device adds a chunk's 64 patterns in a butterfly and the chunks in a fixed order: another order of the same sum)
      for (long p = 0; p < n_patt; p++) tot[row] += grad_combine<true>(a, row, p);

   f = fopen(argv[2], "wb");
   if (!f) { perror(argv[2]); return 2; }
   fwrite(lnf.data(), sizeof(double), n_patt, f);
   fwrite(tot.data(), sizeof(double), 2 * nn + 1, f);
   fclose(f);
   return 0;
}

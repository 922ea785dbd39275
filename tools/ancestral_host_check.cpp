// The per-lane bodies of kernels_ancestral.h (the outer-message passes of 4 / 5 / 20 states, the posterior, the max-sum joint walk of any
// number of states) compiled for the HOST and called in a loop over (class, pattern) — thread indices emulated — so that they run under
// the host sanitizers:
//     g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -DANC_HOST_ONLY tools/ancestral_host_check.cpp -o ancestral_host_check
//     python tools/ancestral_host_check.py ./ancestral_host_check        (writes the cases, runs this, compares with tests/ancestral_ref.py)
// usage: ancestral_host_check IN OUT.  IN: int32 n, K, n_nodes, n_tips, root, n_patt, n_codes, scaled, n_sons; int32 sons_ptr[n_nodes + 1],
// sons[n_sons], scale[n_nodes]; uint8 z[n_tips][n_patt]; uint64 mask[n_codes]; double P[K][n_nodes][n][n], pi[n], freqK[K].
// OUT: double post[n_int][n_patt][n] (zeros when the state count has no lane kernel); uint8 states[n_int][n_patt]; double ln_best[n_patt].
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../paml_amd/csrc/kernels_ancestral.h"

using namespace paml_amd;

template <typename T> static std::vector<T> rd(FILE *f, size_t n)
{
   std::vector<T> v(n);
   if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short input\n"); exit(2); }
   return v;
}

template <int N> static void marginal(AncMargArgs &a)
{
   for (int k = 0; k < a.K; k++)
      for (long p = 0; p < a.nb; p++) anc_lane_down<N>(a, k, p);
   for (int k = 0; k < a.K; k++)
      for (long p = 0; p < a.nb; p++) anc_lane_outer<N>(a, k, p);
   for (int q = 0; q < a.n_query; q++)
      for (long p = 0; p < a.nb; p++) anc_posterior(a, q, p);
}

static void joint(AncJointArgs &a)
{
   const int n2 = a.n * a.n;
   for (int i = 0; i + 1 < a.t.n_post; i++)      // node-outer, as the kernel
      for (long p = 0; p < a.nb; p++) anc_joint_up(a, a.t.post[i], p, a.lnP + (long)a.t.post[i] * n2);
   for (long p = 0; p < a.nb; p++) anc_joint_root_down(a, p);
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
   const std::vector<double> P = rd<double>(f, (size_t)K * nn * n * n), pi = rd<double>(f, n), freqK = rd<double>(f, K);
   fclose(f);

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
   const AncTree t{sons_ptr.data(), sons.data(), father.data(), post.data(), pre.data(), scale.data(), (int)post.size(), (int)pre.size(), nn, n_tips, n_int, root};

   const long stride = (n_patt + ANC_TILE - 1) / ANC_TILE * ANC_TILE;
   std::vector<int> query(n_int);
   for (int i = 0; i < n_int; i++) query[i] = i;
   std::vector<double> L((size_t)K * n_int * n * stride), G(L.size()), SL((size_t)K * n_int * stride), SG(SL.size());
   std::vector<double> postv((size_t)n_int * stride * n, 0.0), prob((size_t)n_int * stride);
   std::vector<unsigned char> best((size_t)n_int * stride);
   AncMargArgs a{};
   a.t = t; a.n = n; a.K = K; a.gene = 0; a.scaled = scaled; a.n_pi = 1; a.n_query = n_int; a.h0 = 0; a.nb = n_patt; a.stride = stride;
   a.z = z.data(); a.z_stride = n_patt; a.code_mask = mask.data(); a.P = P.data(); a.pi = pi.data(); a.freqK = freqK.data(); a.query = query.data();
   a.L = L.data(); a.G = G.data(); a.SL = SL.data(); a.SG = SG.data(); a.post = postv.data(); a.best_prob = prob.data(); a.best = best.data(); a.mfma = 0;
   if (n == 4) marginal<4>(a);
   else if (n == 5) marginal<5>(a);
   else if (n == 20) marginal<20>(a);

   std::vector<double> lnP((size_t)nn * n * n), lnpi(n), JL((size_t)n_int * n * stride), lnbest(stride);
   for (size_t i = 0; i < lnP.size(); i++) lnP[i] = log(fmax(P[i], 1e-300));      // (class 0)
   for (int i = 0; i < n; i++) lnpi[i] = log(fmax(pi[i], 1e-300));
   std::vector<unsigned char> C((size_t)n_int * n * stride), state((size_t)n_int * stride), rootstate(stride);
   AncJointArgs j{};
   j.t = t; j.n = n; j.gene = 0; j.h0 = 0; j.nb = n_patt; j.stride = stride; j.z = z.data(); j.z_stride = n_patt; j.code_mask = mask.data();
   j.lnP = lnP.data(); j.lnpi = lnpi.data(); j.L = JL.data(); j.C = C.data(); j.state = state.data(); j.rootstate = rootstate.data(); j.ln_best = lnbest.data();
   joint(j);

   f = fopen(argv[2], "wb");
   if (!f) { perror(argv[2]); return 2; }
   for (int q = 0; q < n_int; q++) fwrite(postv.data() + (size_t)q * stride * n, sizeof(double), (size_t)n_patt * n, f);
   for (int q = 0; q < n_int; q++) fwrite(state.data() + (size_t)q * stride, 1, n_patt, f);
   fwrite(lnbest.data(), sizeof(double), n_patt, f);
   fclose(f);
   return 0;
}

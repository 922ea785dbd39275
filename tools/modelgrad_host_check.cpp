// The per-lane bodies of kernels_modelgrad.h (the down pass of kernels_ancestral.h, the outer pass that stores H_v, the coefficients,
// the scalar rows' terms, the terms of W, the segment bookkeeping and Psi) compiled for the HOST and called in a loop over (class or
// node, pattern) — thread indices emulated — so that they run under the host sanitizers:
//     g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -DMODELGRAD_HOST_ONLY tools/modelgrad_host_check.cpp -o modelgrad_host_check
//     python tools/modelgrad_host_check.py ./modelgrad_host_check      (writes the cases, runs this, compares with tests/modelgrad_ref.py)
// usage: modelgrad_host_check IN OUT BATCH.  IN: int32 n, K, n_nodes, n_tips, root, n_patt, n_codes, scaled, n_sons; int32
// sons_ptr[n_nodes + 1], sons[n_sons], scale[n_nodes]; uint8 z[n_tips][n_patt]; uint64 mask[n_codes]; double P[K][n_nodes][n][n], pi[n],
// freqK[K], weights[n_patt].  BATCH: patterns per batch (a multiple of 64; the segments of W are walked as the engine walks them, a
// segment cut by a batch border carried on).  OUT: double W[K][n_nodes][n][n], rows[1 + K + n] (lnL, g_freqK, g_pi), psi[3].
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../paml_amd/csrc/kernels_modelgrad.h"

using namespace paml_amd;

template <typename T> static std::vector<T> rd(FILE *f, size_t n)
{
   std::vector<T> v(n);
   if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short input\n"); exit(2); }
   return v;
}

template <int N> static void passes(ModelGradArgs &a)
{
   for (int k = 0; k < a.m.K; k++)
      for (long p = 0; p < a.m.nb; p++) anc_lane_down<N>(a.m, k, p);
   for (int k = 0; k < a.m.K; k++)
      for (long p = 0; p < a.m.nb; p++) mg_lane_outer<N>(a, k, p);
}

int main(int argc, char **argv)
{
   if (argc != 4) { fprintf(stderr, "usage: %s IN OUT BATCH\n", argv[0]); return 2; }
   FILE *f = fopen(argv[1], "rb");
   if (!f) { perror(argv[1]); return 2; }
   const long batch = atol(argv[3]);
   if (batch < 64 || batch % 64) { fprintf(stderr, "BATCH must be a multiple of 64\n"); return 2; }
   const std::vector<int> hd = rd<int>(f, 9);
   const int n = hd[0], K = hd[1], nn = hd[2], n_tips = hd[3], root = hd[4], n_patt = hd[5], n_codes = hd[6], scaled = hd[7], n_sons = hd[8];
   const int n_int = nn - n_tips;
   const std::vector<int> sons_ptr = rd<int>(f, nn + 1), sons = rd<int>(f, n_sons), scale = rd<int>(f, nn);
   const std::vector<unsigned char> z = rd<unsigned char>(f, (size_t)n_tips * n_patt);
   const std::vector<unsigned long long> mask = rd<unsigned long long>(f, n_codes);
   const std::vector<double> P = rd<double>(f, (size_t)K * nn * n * n), pi = rd<double>(f, n), freqK = rd<double>(f, K), weights = rd<double>(f, n_patt);
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

   const long stride = batch, n_chunks = (n_patt + GRAD_CHUNK - 1) / GRAD_CHUNK;
   const int wn = n * n, n_rows = 1 + K + n;
   const size_t per_seg = (size_t)K * nn * wn;
   const long max_segs = (batch + MODELGRAD_SEG - 1) / MODELGRAD_SEG + 1;
   std::vector<double> L((size_t)K * n_int * n * stride), G(L.size()), SL((size_t)K * n_int * stride), SG(SL.size());
   std::vector<double> H((size_t)K * nn * n * stride), den((size_t)K * nn * stride), sig(den.size()), coef(den.size());
   std::vector<double> R((size_t)K * n * stride), SR((size_t)K * stride), croot(SR.size()), rows((size_t)(1 + K) * stride), lnf(stride);
   std::vector<double> carry(2 * per_seg), Wpart((size_t)max_segs * per_seg), W(per_seg, 0.0), total(n_rows, 0.0);
   ModelGradArgs a{};
   AncMargArgs &m = a.m;
   m.t = AncTree{sons_ptr.data(), sons.data(), father.data(), post.data(), pre.data(), scale.data(), (int)post.size(), (int)pre.size(), nn, n_tips, n_int, root};
   m.n = n; m.K = K; m.gene = 0; m.scaled = scaled; m.n_pi = 1; m.stride = stride;
   m.z = z.data(); m.z_stride = n_patt; m.code_mask = mask.data(); m.P = P.data(); m.pi = pi.data(); m.freqK = freqK.data();
   m.L = L.data(); m.G = G.data(); m.SL = SL.data(); m.SG = SG.data(); m.mfma = 0;
   a.H = H.data(); a.den = den.data(); a.sig = sig.data(); a.coef = coef.data(); a.R = R.data(); a.SR = SR.data(); a.croot = croot.data(); a.rows = rows.data();
   a.lnf = lnf.data(); a.weights = weights.data(); a.n_chunks = n_chunks; a.ref_node = sons[sons_ptr[root]];
   a.ld = n; a.wn = wn; a.Wpart = Wpart.data(); a.gene_len = n_patt;
   int flip = 0;
   for (long h0 = 0; h0 < n_patt; h0 += batch) {
      const long nb = std::min<long>(batch, n_patt - h0);
      m.h0 = h0; m.nb = nb; a.off0 = h0;
      a.carry_in = carry.data() + (size_t)flip * per_seg; a.carry_out = carry.data() + (size_t)(flip ^ 1) * per_seg;
      flip ^= 1;
      if (n == 4) passes<4>(a);
      else if (n == 5) passes<5>(a);
      else passes<20>(a);
      for (int v = 0; v <= nn; v++)
         for (long p = 0; p < nb; p++) mg_coef(a, v, p);
      for (int r = 0; r < n_rows; r++)      // (the device adds a chunk's 64 patterns in a butterfly and the chunks in a fixed order: another order of the same sum)
         for (long p = 0; p < nb; p++) total[r] += mg_row_term(a, r, p);
      const int n_segs = (int)((a.off0 + nb - 1) / MODELGRAD_SEG - a.off0 / MODELGRAD_SEG + 1);
      if (n_segs > max_segs) { fprintf(stderr, "more segments than the partials hold\n"); return 2; }
      int n_finished = 0;
      for (int si = 0; si < n_segs; si++) {
         const ModelGradSeg sg = mg_segment(a, si);
         if (sg.finished) n_finished++;
         for (int k = 0; k < K; k++)
            for (int v = 0; v < nn; v++) {
               if (v == root) continue;
               const size_t slot = (size_t)k * nn + v;
               double *dst = sg.finished ? Wpart.data() + ((size_t)si * K * nn + slot) * wn : a.carry_out + slot * wn;
               for (int y = 0; y < n; y++)
                  for (int x = 0; x < n; x++) {
                     double acc = sg.continued ? a.carry_in[slot * wn + y * n + x] : 0.0;
                     for (long p = sg.lo; p < sg.hi; p++) acc += mg_w_term(a, k, v, p, y, x);
                     dst[y * n + x] = acc;
                  }
            }
      }
      for (size_t i = 0; i < per_seg; i++)
         for (int si = 0; si < n_finished; si++) W[i] += Wpart[(size_t)si * per_seg + i];
   }
   const double psi[3] = {mg_psi(-1.0, -1.0, 0.3), mg_psi(-1.0, -1.0 - 1e-9, 0.3), mg_psi(-0.2, -3.0, 0.7)};

   f = fopen(argv[2], "wb");
   if (!f) { perror(argv[2]); return 2; }
   fwrite(W.data(), sizeof(double), W.size(), f);
   fwrite(total.data(), sizeof(double), total.size(), f);
   fwrite(psi, sizeof(double), 3, f);
   fclose(f);
   return 0;
}

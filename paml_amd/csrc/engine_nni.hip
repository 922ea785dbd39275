// engine_nni.hip — the lnL of every nearest-neighbour-interchange neighbour of the tree at the present branch lengths in one call
// (paml_amd_nni_scores) and the canonical list of swaps (paml_amd_nni_list, host only); the definition and the kernels in kernels_nni.h.
// P(t) comes from the evaluation's own builders (anc_pmat, engine_ancestral.hip), the down pass is the ancestral module's, the outer
// pass is the gradient's without the derivative.
// Built for gfx950 only (one of the translation units of libpaml_amd.so, see engine_state.h).
#include "engine_state.h"
#include "kernels_nni.h"
#include "ancestral_host.h"

static thread_local int nni_last_batches = 0;
static thread_local double nni_last_kernel_ms = 0;      // HIP events around the P(t) kernels and every batch's passes, summed

extern "C" void paml_amd_nni_info(int *last_batches, double *last_kernel_ms)
{
   if (last_batches) *last_batches = nni_last_batches;
   if (last_kernel_ms) *last_kernel_ms = nni_last_kernel_ms;
}

// The canonical list, in node order: every (s, x) of every internal v that is not the root, s over v's sons and x over its father's
// other sons, both in son-list order.  A binary v under a root with exactly three sons lists its first son only: there (s1, x1) and
// (s2, x2) are one unrooted tree, and so are (s1, x2) and (s2, x1).
extern "C" int paml_amd_nni_list(int n_tips, int n_nodes, int root, const int *sons_ptr, const int *sons, int *swaps, int cap)
{
   if (n_nodes < 1 || n_tips < 0 || root < 0 || root >= n_nodes || !sons_ptr || !sons) return PAML_AMD_EINVAL;
   std::vector<int> father(n_nodes, -1);
   for (int v = 0; v < n_nodes; v++)
      for (int j = sons_ptr[v]; j < sons_ptr[v + 1]; j++) {
         if (sons[j] < 0 || sons[j] >= n_nodes) return PAML_AMD_EINVAL;
         father[sons[j]] = v;
      }
   int count = 0;
   for (int v = 0; v < n_nodes; v++) {
      const int f = father[v], nv = sons_ptr[v + 1] - sons_ptr[v];
      if (v == root || f < 0 || nv == 0) continue;
      const bool half = f == root && sons_ptr[f + 1] - sons_ptr[f] == 3 && nv == 2;
      for (int i = sons_ptr[v]; i < (half ? sons_ptr[v] + 1 : sons_ptr[v + 1]); i++)
         for (int j = sons_ptr[f]; j < sons_ptr[f + 1]; j++) {
            if (sons[j] == v) continue;
            if (swaps) {
               if (count >= cap) return PAML_AMD_EINVAL;
               swaps[3 * count] = v; swaps[3 * count + 1] = sons[i]; swaps[3 * count + 2] = sons[j];
            }
            count++;
         }
   }
   return count;
}

namespace {

struct NniScratch : AncScratch {
   DevBuf<double> PT, f, sig, lnf, partial, out;
   DevBuf<int> swaps;
   ~NniScratch()
   {
      for (DevBuf<double> *b : {&PT, &f, &sig, &lnf, &partial, &out}) b->release();
      swaps.release();
   }
};

void nni_launch_lane(KernelKind kk, dim3 grid, hipStream_t st, const NniArgs &a, int pass)
{
   if (kk == KK_VALU4) hipLaunchKernelGGL(nni_lane_kernel<4>, grid, dim3(256), 0, st, a, pass);
   else if (kk == KK_VALU5) hipLaunchKernelGGL(nni_lane_kernel<5>, grid, dim3(256), 0, st, a, pass);
   else hipLaunchKernelGGL(nni_lane_kernel<20>, grid, dim3(256), 0, st, a, pass);
}

void nni_launch_lane_swap(KernelKind kk, dim3 grid, hipStream_t st, const NniArgs &a)
{
   if (kk == KK_VALU4) hipLaunchKernelGGL(nni_lane_swap_kernel<4>, grid, dim3(256), 0, st, a);
   else if (kk == KK_VALU5) hipLaunchKernelGGL(nni_lane_swap_kernel<5>, grid, dim3(256), 0, st, a);
   else hipLaunchKernelGGL(nni_lane_swap_kernel<20>, grid, dim3(256), 0, st, a);
}

}  // namespace

extern "C" int paml_amd_nni_scores(paml_amd_engine *e, const double *branch, const double *gene_rate, int n_swaps, const int *swaps, double *lnL0,
                                   double *lnL, double *lnf)
{
   enter(e);
   nni_last_batches = 0;
   nni_last_kernel_ms = 0;
   const char *who = "nni_scores";
   if (!e || !branch || !swaps || !lnL0 || !lnL) return fail(e, PAML_AMD_EINVAL, "nni_scores: null argument");
   if (n_swaps < 1) return fail(e, PAML_AMD_EINVAL, "nni_scores: n_swaps < 1");
   if (int rc = anc_common_checks(e, who)) return rc;
   if (e->world > 1) return fail(e, PAML_AMD_EUNSUPPORTED, "nni_scores: one rank only (this engine's communicator has " + std::to_string(e->world) + ")");
   const TreeDesc &T = e->tree;
   const int nn = T.n_nodes, n = e->n, K = e->K, G = e->n_genes, n_tips = e->n_tips, n_int = nn - n_tips;
   {
      std::vector<int> father(nn, -1);
      for (int v = 0; v < nn; v++)
         for (int j = T.sons_ptr[v]; j < T.sons_ptr[v + 1]; j++) father[T.sons[j]] = v;
      auto son_of = [&](int s, int v) {
         for (int j = T.sons_ptr[v]; j < T.sons_ptr[v + 1]; j++)
            if (T.sons[j] == s) return true;
         return false;
      };
      for (int i = 0; i < n_swaps; i++) {
         const int v = swaps[3 * i], s = swaps[3 * i + 1], x = swaps[3 * i + 2];
         const std::string at = "nni_scores: swap " + std::to_string(i) + ": ";
         if (v < 0 || v >= nn) return fail(e, PAML_AMD_EINVAL, at + "node " + std::to_string(v) + " is out of range");
         if (T.is_leaf(v)) return fail(e, PAML_AMD_EINVAL, at + "node " + std::to_string(v) + " is a tip");
         if (v == T.root || father[v] < 0) return fail(e, PAML_AMD_EINVAL, at + "node " + std::to_string(v) + " is the root");
         if (!son_of(s, v)) return fail(e, PAML_AMD_EINVAL, at + std::to_string(s) + " is not a son of " + std::to_string(v));
         if (x == v || !son_of(x, father[v]))
            return fail(e, PAML_AMD_EINVAL, at + std::to_string(x) + " is not a son of the father of " + std::to_string(v) + " other than it");
      }
   }
   const bool mfma = e->kk == KK_MFMA64;
   hipStream_t st = e->stream;
   NniScratch w;
   NniArgs a{};
   AncMargArgs &m = a.m;
   if (int rc = anc_tree_pack(e, who, w, &m.t)) return rc;
   if (int rc = anc_pmat(e, who, branch, gene_rate, w)) return rc;
   if (mfma) {
      HIPCHK(w.PT.ensure((size_t)G * K * nn * 4096));
      hipLaunchKernelGGL(nni_pt_kernel, dim3(nn, G * K), dim3(256), 0, st, (const double *)e->d_rowmajor.p, w.PT.p, n, nn, n_tips, T.root);
      HIPCHK(hipGetLastError());
   }
   HIPCHK(upload(w.swaps, swaps, (size_t)3 * n_swaps, st));
   HIPCHK(hipEventRecord(w.ev1, st));
   HIPCHK(hipStreamSynchronize(st));
   if (int rc = eigen_fail_check(e)) return rc;
   e->pmat_valid = true;      // (d_rowmajor holds every branch's P(t) in the tree's own orientation, as after the gradient)
   { float ms = 0; HIPCHK(hipEventElapsedTime(&ms, w.ev0, w.ev1)); nni_last_kernel_ms += ms; }

   // chunks of GRAD_CHUNK patterns counted from each gene's first pattern: a batch is whole chunks of one gene
   std::vector<long> chunk_base(G + 1, 0);
   for (int g = 0; g < G; g++) chunk_base[g + 1] = chunk_base[g] + (e->gene_off[g + 1] - e->gene_off[g] + GRAD_CHUNK - 1) / GRAD_CHUNK;
   const long n_chunks = chunk_base[G];
   HIPCHK(w.partial.ensure((size_t)(n_swaps + 1) * std::max<long>(n_chunks, 1)));
   HIPCHK(w.out.ensure((size_t)n_swaps + 1));

   // the workspace per pattern: the partials and the messages, then (2 K + 1) doubles per row (the swaps of a group and the present tree)
   const int ns = mfma ? 64 : n;      // doubles a partial takes per pattern
   const double fixed = 2.0 * K * n_int * (ns + 1) * 8, per_row = (2.0 * K + 1) * 8;
   double arena_mb = 256;
   if (const char *s = getenv("PAML_AMD_NNI_ARENA_MB")) { const double v = atof(s); if (v > 0) arena_mb = v; }
   int cap = n_swaps;
   if ((fixed + per_row * (n_swaps + 1)) * ANC_TILE > arena_mb * 1048576.0)      // one tile with all swaps does not fit: groups of swaps
      cap = (int)std::min<double>(n_swaps, std::max(1.0, floor((arena_mb * 1048576.0 / ANC_TILE - fixed) / per_row) - 1));
   cap = std::min(cap, 65535);      // (the lanes' swap pass has a grid row per swap)
   long batch = anc_batch(fixed + per_row * (cap + 1), e->n_patt, "PAML_AMD_NNI_ARENA_MB");
   for (;;) {      // halve the batch until it fits
      const size_t part = (size_t)K * n_int * ns * batch, sc = (size_t)K * n_int * batch, rows = (size_t)K * (cap + 1) * batch;
      if (w.L.ensure(part) == hipSuccess && w.G.ensure(part) == hipSuccess && w.SL.ensure(sc) == hipSuccess && w.SG.ensure(sc) == hipSuccess &&
          w.f.ensure(rows) == hipSuccess && w.sig.ensure(rows) == hipSuccess && w.lnf.ensure((size_t)(cap + 1) * batch) == hipSuccess)
         break;
      (void)hipGetLastError();
      for (DevBuf<double> *b : {&w.L, &w.G, &w.SL, &w.SG, &w.f, &w.sig, &w.lnf}) b->release();      // (ensure only grows: the retry starts from nothing)
      if (batch <= ANC_TILE) return fail(e, PAML_AMD_ENOMEM, "nni_scores: no device memory for one tile of patterns");
      batch = (batch / 2 + ANC_TILE - 1) / ANC_TILE * ANC_TILE;
   }
   m.n = n; m.K = K; m.scaled = T.n_scale > 0 ? 1 : 0; m.n_pi = e->n_pi; m.stride = batch;
   m.z = e->d_z.p; m.z_stride = e->n_patt; m.code_mask = e->d_code_mask.p;
   m.P = e->d_rowmajor.p; m.pint = e->d_pint.p; m.ptip = e->d_ptip.p; m.tip_words = (long)tip_words(e);
   m.pi = e->d_pi_plain.p; m.freqK = e->d_freqK.p;
   m.L = w.L.p; m.G = w.G.p; m.SL = w.SL.p; m.SG = w.SG.p; m.mfma = mfma ? 1 : 0;
   a.PT = w.PT.p; a.swaps = w.swaps.p; a.cap = cap; a.n_swaps = n_swaps; a.f = w.f.p; a.sig = w.sig.p; a.weights = e->d_weights.p;
   a.lnf = w.lnf.p; a.partial = w.partial.p; a.n_chunks = n_chunks;
   a.ref_node = T.sons[T.sons_ptr[T.root]];
   const long n_patt = e->n_patt;
   for (int g = 0; g < G; g++)
      for (long h0 = e->gene_off[g]; h0 < e->gene_off[g + 1]; h0 += batch) {
         const long nb = std::min<long>(batch, e->gene_off[g + 1] - h0);
         m.gene = g; m.h0 = h0; m.nb = nb;
         a.chunk0 = chunk_base[g] + (h0 - e->gene_off[g]) / GRAD_CHUNK;
         a.swap0 = 0; a.n_group = 0;
         const dim3 tiles((unsigned)((nb + ANC_TILE - 1) / ANC_TILE), K), lanes((unsigned)((nb + 255) / 256), K);
         HIPCHK(hipEventRecord(w.ev0, st));
         if (mfma) {
            hipLaunchKernelGGL(nni_unit_anc_mfma_kernel, tiles, dim3(256), 0, st, m, 0);
            HIPCHK(hipGetLastError());
            hipLaunchKernelGGL(nni_mfma_outer_kernel, tiles, dim3(256), 0, st, a);
            HIPCHK(hipGetLastError());
         }
         else
            for (int pass = 0; pass < 2; pass++) {
               nni_launch_lane(e->kk, lanes, st, a, pass);
               HIPCHK(hipGetLastError());
            }
         HIPCHK(hipEventRecord(w.ev1, st));
         for (int s0 = 0; s0 < n_swaps; s0 += cap) {
            const int ng = std::min(cap, n_swaps - s0);
            a.swap0 = s0; a.n_group = ng;
            if (s0) {      // (the batch's first group is timed with its down and outer passes)
               HIPCHK(hipStreamSynchronize(st));
               { float ms = 0; HIPCHK(hipEventElapsedTime(&ms, w.ev0, w.ev1)); nni_last_kernel_ms += ms; }
               HIPCHK(hipEventRecord(w.ev0, st));
            }
            if (mfma) hipLaunchKernelGGL(nni_mfma_kernel, tiles, dim3(256), 0, st, a);
            else nni_launch_lane_swap(e->kk, dim3(lanes.x, K, ng), st, a);
            HIPCHK(hipGetLastError());
            hipLaunchKernelGGL(nni_combine_kernel, dim3(lanes.x, ng + (s0 == 0 ? 1 : 0)), dim3(256), 0, st, a);
            HIPCHK(hipGetLastError());
            HIPCHK(hipEventRecord(w.ev1, st));
            // the group's rows to the caller's [n_swaps][n_patt]: one plain copy per swap
            if (lnf)
               for (int i = 0; i < ng; i++)
                  HIPCHK(hipMemcpyAsync(lnf + (size_t)(s0 + i) * n_patt + h0, w.lnf.p + (size_t)i * batch, (size_t)nb * 8, hipMemcpyDeviceToHost, st));
         }
         HIPCHK(hipStreamSynchronize(st));
         { float ms = 0; HIPCHK(hipEventElapsedTime(&ms, w.ev0, w.ev1)); nni_last_kernel_ms += ms; }
         nni_last_batches++;
      }
   HIPCHK(hipEventRecord(w.ev0, st));
   hipLaunchKernelGGL(nni_unit_grad_total_kernel, dim3(n_swaps + 1), dim3(256), 0, st, (const double *)w.partial.p, n_chunks, w.out.p);
   HIPCHK(hipGetLastError());
   HIPCHK(hipEventRecord(w.ev1, st));
   std::vector<double> out((size_t)n_swaps + 1);
   HIPCHK(hipMemcpyAsync(out.data(), w.out.p, ((size_t)n_swaps + 1) * 8, hipMemcpyDeviceToHost, st));
   HIPCHK(hipStreamSynchronize(st));
   { float ms = 0; HIPCHK(hipEventElapsedTime(&ms, w.ev0, w.ev1)); nni_last_kernel_ms += ms; }
   for (int i = 0; i < n_swaps; i++) lnL[i] = out[i];
   *lnL0 = out[n_swaps];
   return 0;
}

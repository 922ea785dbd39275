// engine_gradient.hip — the derivative of lnL with respect to every branch length and the per-pattern scores in one call
// (paml_amd_gradient); the definition and the kernels in kernels_gradient.h.  P(t) comes from the evaluation's own builders (anc_pmat,
// engine_ancestral.hip), the down pass is the ancestral module's.
// Built for gfx950 only (one of the translation units of libpaml_amd.so, see engine_state.h).
#include "engine_state.h"
#include "kernels_gradient.h"
#include "ancestral_host.h"

static thread_local int grad_last_batches = 0;
static thread_local double grad_last_kernel_ms = 0;      // HIP events around the P(t) / dP kernels and every batch's passes, summed

extern "C" void paml_amd_gradient_info(int *last_batches, double *last_kernel_ms)
{
   if (last_batches) *last_batches = grad_last_batches;
   if (last_kernel_ms) *last_kernel_ms = grad_last_kernel_ms;
}

namespace {

struct GradScratch : AncScratch {
   DevBuf<double> dP, PT, num, den, sig, scores, lnf, partial, out;
   ~GradScratch()
   {
      for (DevBuf<double> *b : {&dP, &PT, &num, &den, &sig, &scores, &lnf, &partial, &out}) b->release();
   }
};

void grad_launch_lane(KernelKind kk, dim3 grid, hipStream_t st, const GradArgs &a, int pass)
{
   if (kk == KK_VALU4) hipLaunchKernelGGL(grad_lane_kernel<4>, grid, dim3(256), 0, st, a, pass);
   else if (kk == KK_VALU5) hipLaunchKernelGGL(grad_lane_kernel<5>, grid, dim3(256), 0, st, a, pass);
   else hipLaunchKernelGGL(grad_lane_kernel<20>, grid, dim3(256), 0, st, a, pass);
}

}  // namespace

extern "C" int paml_amd_gradient(paml_amd_engine *e, const double *branch, const double *gene_rate, double *lnL, double *grad, double *lnf, double *scores)
{
   enter(e);
   grad_last_batches = 0;
   grad_last_kernel_ms = 0;
   const char *who = "gradient";
   if (!e || !branch || !lnL || !grad) return fail(e, PAML_AMD_EINVAL, "gradient: null argument");
   if (int rc = anc_common_checks(e, who)) return rc;
   if (e->world > 1) return fail(e, PAML_AMD_EUNSUPPORTED, "gradient: one rank only (this engine's communicator has " + std::to_string(e->world) + ")");
   for (size_t i = 0; i < e->eigen.size(); i++)
      if (e->eigen[i].kind == PAML_AMD_EIGEN_QMAT)
         return fail(e, PAML_AMD_EUNSUPPORTED, "gradient: the derivative of a rate-matrix (UNREST) set's P(t) needs a matrix product of its own");
   const TreeDesc &T = e->tree;
   const int nn = T.n_nodes, n = e->n, K = e->K, G = e->n_genes, n_tips = e->n_tips, n_int = nn - n_tips;
   if (nn < 2) return fail(e, PAML_AMD_EINVAL, "gradient: the tree has no branch");
   const bool mfma = e->kk == KK_MFMA64;
   hipStream_t st = e->stream;
   GradScratch w;
   GradArgs a{};
   AncMargArgs &m = a.m;
   if (int rc = anc_tree_pack(e, who, w, &m.t)) return rc;
   if (int rc = anc_pmat(e, who, branch, gene_rate, w)) return rc;
   {
      const size_t pn = (size_t)G * K * nn;
      HIPCHK(w.dP.ensure(pn * (mfma ? 4096 : n * n)));
      if (mfma) HIPCHK(w.PT.ensure(pn * 4096));
      GradPmatArgs ga{};
      ga.n = n; ga.K = K; ga.n_nodes = nn; ga.n_tips = n_tips; ga.root = T.root; ga.n_labels = e->n_labels; ga.rate_gs = e->rate_per_gene ? K : 0; ga.mfma = mfma ? 1 : 0;
      ga.label = e->d_label.p; ga.eigen_of = e->d_eigen_of.p; ga.eigen = e->d_eigen.p;
      ga.branch = e->d_branch.p; ga.rate = e->d_rate.p; ga.gene_rate = e->d_gene_rate.p; ga.qfactor = e->d_qfactor.p;
      ga.P = e->d_rowmajor.p; ga.dP = w.dP.p; ga.PT = w.PT.p;
      hipLaunchKernelGGL(grad_pmat_kernel, dim3(nn, G * K), dim3(256), 0, st, ga);
      HIPCHK(hipGetLastError());
   }
   HIPCHK(hipEventRecord(w.ev1, st));
   HIPCHK(hipStreamSynchronize(st));
   if (int rc = eigen_fail_check(e)) return rc;
   e->pmat_valid = true;      // (d_rowmajor holds every branch's P(t) in the tree's own orientation, as after the joint reconstruction)
   { float ms = 0; HIPCHK(hipEventElapsedTime(&ms, w.ev0, w.ev1)); grad_last_kernel_ms += ms; }

   // chunks of GRAD_CHUNK patterns counted from each gene's first pattern: a batch is whole chunks of one gene
   std::vector<long> chunk_base(G + 1, 0);
   for (int g = 0; g < G; g++) chunk_base[g + 1] = chunk_base[g] + (e->gene_off[g + 1] - e->gene_off[g] + GRAD_CHUNK - 1) / GRAD_CHUNK;
   const long n_chunks = chunk_base[G];
   HIPCHK(w.partial.ensure((size_t)(nn + 1) * std::max<long>(n_chunks, 1)));
   HIPCHK(w.out.ensure((size_t)nn + 1));

   const int ns = mfma ? 64 : n;      // doubles a partial takes per pattern
   const double per_patt = 2.0 * K * n_int * (ns + 1) * 8 + 3.0 * K * nn * 8 + (nn + 1) * 8.0;
   long batch = anc_batch(per_patt, e->n_patt, "PAML_AMD_GRAD_ARENA_MB");
   for (;;) {      // halve the batch until it fits
      const size_t part = (size_t)K * n_int * ns * batch, sc = (size_t)K * n_int * batch, cl = (size_t)K * nn * batch;
      if (w.L.ensure(part) == hipSuccess && w.G.ensure(part) == hipSuccess && w.SL.ensure(sc) == hipSuccess && w.SG.ensure(sc) == hipSuccess &&
          w.num.ensure(cl) == hipSuccess && w.den.ensure(cl) == hipSuccess && w.sig.ensure(cl) == hipSuccess &&
          w.scores.ensure((size_t)nn * batch) == hipSuccess && w.lnf.ensure((size_t)batch) == hipSuccess)
         break;
      (void)hipGetLastError();
      for (DevBuf<double> *b : {&w.L, &w.G, &w.SL, &w.SG, &w.num, &w.den, &w.sig, &w.scores, &w.lnf}) b->release();      // (ensure only grows: the retry starts from nothing)
      if (batch <= ANC_TILE) return fail(e, PAML_AMD_ENOMEM, "gradient: no device memory for one tile of patterns");
      batch = (batch / 2 + ANC_TILE - 1) / ANC_TILE * ANC_TILE;
   }
   m.n = n; m.K = K; m.scaled = T.n_scale > 0 ? 1 : 0; m.n_pi = e->n_pi; m.stride = batch;
   m.z = e->d_z.p; m.z_stride = e->n_patt; m.code_mask = e->d_code_mask.p;
   m.P = e->d_rowmajor.p; m.pint = e->d_pint.p; m.ptip = e->d_ptip.p; m.tip_words = (long)tip_words(e);
   m.pi = e->d_pi_plain.p; m.freqK = e->d_freqK.p;
   m.L = w.L.p; m.G = w.G.p; m.SL = w.SL.p; m.SG = w.SG.p; m.mfma = mfma ? 1 : 0;
   a.dP = w.dP.p; a.PT = w.PT.p; a.num = w.num.p; a.den = w.den.p; a.sig = w.sig.p; a.weights = e->d_weights.p;
   a.scores = w.scores.p; a.lnf = w.lnf.p; a.partial = w.partial.p; a.n_chunks = n_chunks;
   a.ref_node = T.sons[T.sons_ptr[T.root]];
   const long n_patt = e->n_patt;
   for (int g = 0; g < G; g++)
      for (long h0 = e->gene_off[g]; h0 < e->gene_off[g + 1]; h0 += batch) {
         const long nb = std::min<long>(batch, e->gene_off[g + 1] - h0);
         m.gene = g; m.h0 = h0; m.nb = nb;
         a.chunk0 = chunk_base[g] + (h0 - e->gene_off[g]) / GRAD_CHUNK;
         HIPCHK(hipEventRecord(w.ev0, st));
         if (mfma) {
            const dim3 grid((unsigned)((nb + ANC_TILE - 1) / ANC_TILE), K);
            hipLaunchKernelGGL(grad_unit_anc_mfma_kernel, grid, dim3(256), 0, st, m, 0);
            HIPCHK(hipGetLastError());
            hipLaunchKernelGGL(grad_mfma_kernel, grid, dim3(256), 0, st, a);
            HIPCHK(hipGetLastError());
         }
         else
            for (int pass = 0; pass < 2; pass++) {
               grad_launch_lane(e->kk, dim3((unsigned)((nb + 255) / 256), K), st, a, pass);
               HIPCHK(hipGetLastError());
            }
         hipLaunchKernelGGL(grad_combine_kernel, dim3((unsigned)((nb + 255) / 256), nn + 1), dim3(256), 0, st, a);
         HIPCHK(hipGetLastError());
         HIPCHK(hipEventRecord(w.ev1, st));
         // the batch's rows to the caller's [n_nodes][n_patt]: one plain copy per node
         if (scores)
            for (int v = 0; v < nn; v++)
               HIPCHK(hipMemcpyAsync(scores + (size_t)v * n_patt + h0, w.scores.p + (size_t)v * batch, (size_t)nb * 8, hipMemcpyDeviceToHost, st));
         if (lnf) HIPCHK(hipMemcpyAsync(lnf + h0, w.lnf.p, (size_t)nb * 8, hipMemcpyDeviceToHost, st));
         HIPCHK(hipStreamSynchronize(st));
         { float ms = 0; HIPCHK(hipEventElapsedTime(&ms, w.ev0, w.ev1)); grad_last_kernel_ms += ms; }
         grad_last_batches++;
      }
   HIPCHK(hipEventRecord(w.ev0, st));
   hipLaunchKernelGGL(grad_total_kernel, dim3(nn + 1), dim3(256), 0, st, (const double *)w.partial.p, n_chunks, w.out.p);
   HIPCHK(hipGetLastError());
   HIPCHK(hipEventRecord(w.ev1, st));
   std::vector<double> out((size_t)nn + 1);
   HIPCHK(hipMemcpyAsync(out.data(), w.out.p, ((size_t)nn + 1) * 8, hipMemcpyDeviceToHost, st));
   HIPCHK(hipStreamSynchronize(st));
   { float ms = 0; HIPCHK(hipEventElapsedTime(&ms, w.ev0, w.ev1)); grad_last_kernel_ms += ms; }
   for (int v = 0; v < nn; v++) grad[v] = v == T.root ? 0.0 : out[v];
   *lnL = out[nn];
   return 0;
}

// engine_spr.hip — the lnL of every requested subtree-prune-and-regraft neighbour of the tree at the present branch lengths in one call
// (paml_amd_spr_scores) and the canonical list of moves (paml_amd_spr_list, host only); the definition and the kernels in kernels_spr.h,
// the lists of steps in spr_plan.h.
// Every P(t) comes from the evaluation's own builder (anc_pmat, engine_ancestral.hip), which runs once per family of lengths on a branch
// vector of the tree's size with the tree's own labels: the upper parts (1 - phi) t_v, the lower parts phi t_v, the merged lengths
// t_v + t_father(v) stored at v, and last the tree's own lengths, so that d_rowmajor and pmat_valid are left as after
// paml_amd_nni_scores.  The down pass is the ancestral module's, the outer pass is the NNI module's.
// Built for gfx950 only (one of the translation units of libpaml_amd.so, see engine_state.h).
#include "engine_state.h"
#include "kernels_spr.h"
#include "ancestral_host.h"

static thread_local int spr_last_batches = 0;
static thread_local double spr_last_kernel_ms = 0;      // HIP events around the P(t) kernels and every batch's passes, summed

extern "C" void paml_amd_spr_info(int *last_batches, double *last_kernel_ms)
{
   if (last_batches) *last_batches = spr_last_batches;
   if (last_kernel_ms) *last_kernel_ms = spr_last_kernel_ms;
}

extern "C" int paml_amd_spr_list(int n_tips, int n_nodes, int root, const int *sons_ptr, const int *sons, int radius, int *moves, int cap)
{
   if (n_tips < 0) return PAML_AMD_EINVAL;
   const int n = spr_list(SprTreeView{n_tips, n_nodes, root, sons_ptr, sons}, radius, moves, cap);
   return n < 0 ? PAML_AMD_EINVAL : n;
}

namespace {

struct SprScratch : AncScratch {
   DevBuf<double> PT, Pup, Pdn, Pm, PTup, pint_dn, ptip_dn, pint_m, ptip_m, PTm, Lp, Ap, SLp, SAp, f, sig, lnf, partial, out;
   DevBuf<int> plan;
   ~SprScratch()
   {
      for (DevBuf<double> *b : {&PT, &Pup, &Pdn, &Pm, &PTup, &pint_dn, &ptip_dn, &pint_m, &ptip_m, &PTm, &Lp, &Ap, &SLp, &SAp, &f, &sig, &lnf, &partial, &out}) b->release();
      plan.release();
   }
};

void spr_launch_lane(KernelKind kk, dim3 grid, hipStream_t st, const SprArgs &a, int pass)
{
   if (kk == KK_VALU4) hipLaunchKernelGGL(spr_lane_kernel<4>, grid, dim3(256), 0, st, a, pass);
   else if (kk == KK_VALU5) hipLaunchKernelGGL(spr_lane_kernel<5>, grid, dim3(256), 0, st, a, pass);
   else hipLaunchKernelGGL(spr_lane_kernel<20>, grid, dim3(256), 0, st, a, pass);
}

// the builder's P(t) at `branch` with the tree's labels, waited for; its kernel time is added to the call's
int spr_pmat(paml_amd_engine *e, const char *who, const double *branch, const double *gene_rate, SprScratch &w)
{
   if (int rc = anc_pmat(e, who, branch, gene_rate, w)) return rc;
   HIPCHK(hipEventRecord(w.ev1, e->stream));
   HIPCHK(hipStreamSynchronize(e->stream));
   if (int rc = eigen_fail_check(e)) return rc;
   float ms = 0;
   HIPCHK(hipEventElapsedTime(&ms, w.ev0, w.ev1));
   spr_last_kernel_ms += ms;
   return 0;
}

}  // namespace

extern "C" int paml_amd_spr_scores(paml_amd_engine *e, const double *branch, const double *gene_rate, int n_moves, const int *moves, double phi,
                                   double *lnL0, double *lnL, double *lnf)
{
   enter(e);
   spr_last_batches = 0;
   spr_last_kernel_ms = 0;
   const char *who = "spr_scores";
   if (!e || !branch || !moves || !lnL0 || !lnL) return fail(e, PAML_AMD_EINVAL, "spr_scores: null argument");
   if (n_moves < 1) return fail(e, PAML_AMD_EINVAL, "spr_scores: n_moves < 1");
   if (!(phi >= 0 && phi <= 1)) return fail(e, PAML_AMD_EINVAL, "spr_scores: phi = " + std::to_string(phi) + " is outside [0, 1]");
   if (int rc = anc_common_checks(e, who)) return rc;
   if (e->world > 1) return fail(e, PAML_AMD_EUNSUPPORTED, "spr_scores: one rank only (this engine's communicator has " + std::to_string(e->world) + ")");
   const TreeDesc &T = e->tree;
   const int nn = T.n_nodes, n = e->n, K = e->K, G = e->n_genes, n_tips = e->n_tips, n_int = nn - n_tips;
   const long n_patt = e->n_patt;
   const SprTreeView view{n_tips, nn, T.root, T.sons_ptr.data(), T.sons.data()};
   std::vector<int> father;
   if (!spr_fathers(view, father)) return fail(e, PAML_AMD_EINVAL, "spr_scores: the tree's son lists name a node out of range");
   for (int i = 0; i < n_moves; i++) {
      const std::string why = spr_check_move(view, father, moves[2 * i], moves[2 * i + 1]);
      if (!why.empty()) return fail(e, PAML_AMD_EINVAL, "spr_scores: move " + std::to_string(i) + ": " + why);
   }
   SprPlan plan;
   spr_plan(view, father, n_moves, moves, plan);
   if (plan.max_rows > 65534) return fail(e, PAML_AMD_EUNSUPPORTED, "spr_scores: more than 65534 targets of one pruned subtree");

   const bool mfma = e->kk == KK_MFMA64;
   hipStream_t st = e->stream;
   SprScratch w;
   SprArgs a{};
   NniArgs &o = a.o;
   AncMargArgs &m = o.m;
   if (int rc = anc_tree_pack(e, who, w, &m.t)) return rc;
   const size_t psets = (size_t)G * K, pn = psets * nn, nn2 = (size_t)n * n, tw = tip_words(e);
   {
      // one run of the builder per family; what the kernels need of it is copied before the next run
      std::vector<double> b(nn);
      for (int v = 0; v < nn; v++) b[v] = (1 - phi) * branch[v];
      if (int rc = spr_pmat(e, who, b.data(), gene_rate, w)) return rc;
      if (mfma) {
         HIPCHK(w.PTup.ensure(pn * 4096));
         hipLaunchKernelGGL(spr_pt_kernel, dim3(nn, (unsigned)psets), dim3(256), 0, st, (const double *)e->d_rowmajor.p, w.PTup.p, n, nn, T.root);
         HIPCHK(hipGetLastError());
      }
      else {
         HIPCHK(w.Pup.ensure(pn * nn2));
         HIPCHK(hipMemcpyAsync(w.Pup.p, e->d_rowmajor.p, pn * nn2 * 8, hipMemcpyDeviceToDevice, st));
      }
      HIPCHK(hipStreamSynchronize(st));
      for (int v = 0; v < nn; v++) b[v] = phi * branch[v];
      if (int rc = spr_pmat(e, who, b.data(), gene_rate, w)) return rc;
      if (mfma) {
         HIPCHK(w.pint_dn.ensure(pn * 4096));
         HIPCHK(w.ptip_dn.ensure(pn * tw));
         HIPCHK(hipMemcpyAsync(w.pint_dn.p, e->d_pint.p, pn * 4096 * 8, hipMemcpyDeviceToDevice, st));
         HIPCHK(hipMemcpyAsync(w.ptip_dn.p, e->d_ptip.p, pn * tw * 8, hipMemcpyDeviceToDevice, st));
      }
      else {
         HIPCHK(w.Pdn.ensure(pn * nn2));
         HIPCHK(hipMemcpyAsync(w.Pdn.p, e->d_rowmajor.p, pn * nn2 * 8, hipMemcpyDeviceToDevice, st));
      }
      HIPCHK(hipStreamSynchronize(st));
      for (int v = 0; v < nn; v++) b[v] = branch[v] + (father[v] >= 0 && father[v] != T.root ? branch[father[v]] : 0.0);
      if (int rc = spr_pmat(e, who, b.data(), gene_rate, w)) return rc;
      if (mfma) {
         HIPCHK(w.pint_m.ensure(pn * 4096));
         HIPCHK(w.ptip_m.ensure(pn * tw));
         HIPCHK(w.PTm.ensure(pn * 4096));
         HIPCHK(hipMemcpyAsync(w.pint_m.p, e->d_pint.p, pn * 4096 * 8, hipMemcpyDeviceToDevice, st));
         HIPCHK(hipMemcpyAsync(w.ptip_m.p, e->d_ptip.p, pn * tw * 8, hipMemcpyDeviceToDevice, st));
         hipLaunchKernelGGL(spr_pt_kernel, dim3(nn, (unsigned)psets), dim3(256), 0, st, (const double *)e->d_rowmajor.p, w.PTm.p, n, nn, T.root);
         HIPCHK(hipGetLastError());
      }
      else {
         HIPCHK(w.Pm.ensure(pn * nn2));
         HIPCHK(hipMemcpyAsync(w.Pm.p, e->d_rowmajor.p, pn * nn2 * 8, hipMemcpyDeviceToDevice, st));
      }
      HIPCHK(hipStreamSynchronize(st));
   }
   // the tree's own lengths last: what the passes read, and what the engine keeps
   if (int rc = anc_pmat(e, who, branch, gene_rate, w)) return rc;
   if (mfma) {
      HIPCHK(w.PT.ensure(pn * 4096));
      hipLaunchKernelGGL(spr_pt_kernel, dim3(nn, (unsigned)psets), dim3(256), 0, st, (const double *)e->d_rowmajor.p, w.PT.p, n, nn, T.root);
      HIPCHK(hipGetLastError());
   }
   const size_t o_steps = plan.prunes.size(), o_factors = o_steps + plan.steps.size();
   {
      std::vector<int> pack(plan.prunes);
      pack.insert(pack.end(), plan.steps.begin(), plan.steps.end());
      pack.insert(pack.end(), plan.factors.begin(), plan.factors.end());
      pack.push_back(0);      // (a list without factors still has a buffer)
      HIPCHK(upload(w.plan, pack.data(), pack.size(), st));
      HIPCHK(hipEventRecord(w.ev1, st));
      HIPCHK(hipStreamSynchronize(st));      // (`pack` is on this stack)
   }
   if (int rc = eigen_fail_check(e)) return rc;
   e->pmat_valid = true;      // (d_rowmajor holds every branch's P(t) in the tree's own orientation, as after the gradient)
   { float ms = 0; HIPCHK(hipEventElapsedTime(&ms, w.ev0, w.ev1)); spr_last_kernel_ms += ms; }

   // chunks of GRAD_CHUNK patterns counted from each gene's first pattern: a batch is whole chunks of one gene
   std::vector<long> chunk_base(G + 1, 0);
   for (int g = 0; g < G; g++) chunk_base[g + 1] = chunk_base[g] + (e->gene_off[g + 1] - e->gene_off[g] + GRAD_CHUNK - 1) / GRAD_CHUNK;
   const long n_chunks = chunk_base[G];
   HIPCHK(w.partial.ensure((size_t)(n_moves + 1) * std::max<long>(n_chunks, 1)));
   HIPCHK(w.out.ensure((size_t)n_moves + 1));

   // the workspace per pattern: the partials and the messages of the tree and of one prune, then (2 K + 1) doubles per row (the moves of a
   // group and the present tree)
   const int ns = mfma ? 64 : n;      // doubles a partial takes per pattern
   const double fixed = 4.0 * K * n_int * (ns + 1) * 8, per_row = (2.0 * K + 1) * 8;
   double arena_mb = 256;
   if (const char *s = getenv("PAML_AMD_SPR_ARENA_MB")) { const double v = atof(s); if (v > 0) arena_mb = v; }
   int cap = n_moves;
   const double all_patt = (double)((n_patt + ANC_TILE - 1) / ANC_TILE * ANC_TILE);
   if ((fixed + per_row * (n_moves + 1)) * all_patt > arena_mb * 1048576.0)      // batches of patterns: the rows take no more of the workspace than
      cap = (int)std::min<double>(n_moves, std::max(1.0, floor(fixed / per_row) - 1));      // the partials do, so that a batch keeps the device busy
   if ((fixed + per_row * (cap + 1)) * ANC_TILE > arena_mb * 1048576.0)      // one tile with these rows does not fit: fewer
      cap = (int)std::min<double>(n_moves, std::max(1.0, floor((arena_mb * 1048576.0 / ANC_TILE - fixed) / per_row) - 1));
   cap = std::min(std::max(cap, plan.max_rows), 65534);      // (a prune is not split; the combining kernel has a grid row per row and one for the present tree)
   // the groups: as many whole prunes as the rows hold
   std::vector<int> group_first(1, 0);
   {
      int rows = 0;
      for (int ip = 0; ip < plan.n_prunes(); ip++) {
         const int r0 = plan.prunes[SPR_PRUNE_INTS * ip + 3], r1 = ip + 1 < plan.n_prunes() ? plan.prunes[SPR_PRUNE_INTS * (ip + 1) + 3] : n_moves;
         if (rows + (r1 - r0) > cap) { group_first.push_back(ip); rows = 0; }
         rows += r1 - r0;
      }
      group_first.push_back(plan.n_prunes());
   }
   long batch = anc_batch(fixed + per_row * (cap + 1), n_patt, "PAML_AMD_SPR_ARENA_MB");
   for (;;) {      // halve the batch until it fits
      const size_t part = (size_t)K * n_int * ns * batch, sc = (size_t)K * n_int * batch, rows = (size_t)K * (cap + 1) * batch;
      if (w.L.ensure(part) == hipSuccess && w.G.ensure(part) == hipSuccess && w.SL.ensure(sc) == hipSuccess && w.SG.ensure(sc) == hipSuccess &&
          w.Lp.ensure(part) == hipSuccess && w.Ap.ensure(part) == hipSuccess && w.SLp.ensure(sc) == hipSuccess && w.SAp.ensure(sc) == hipSuccess &&
          w.f.ensure(rows) == hipSuccess && w.sig.ensure(rows) == hipSuccess && w.lnf.ensure((size_t)(cap + 1) * batch) == hipSuccess)
         break;
      (void)hipGetLastError();
      for (DevBuf<double> *b : {&w.L, &w.G, &w.SL, &w.SG, &w.Lp, &w.Ap, &w.SLp, &w.SAp, &w.f, &w.sig, &w.lnf}) b->release();      // (ensure only grows: the retry starts from nothing)
      if (batch <= ANC_TILE) return fail(e, PAML_AMD_ENOMEM, "spr_scores: no device memory for one tile of patterns");
      batch = (batch / 2 + ANC_TILE - 1) / ANC_TILE * ANC_TILE;
   }
   m.n = n; m.K = K; m.scaled = T.n_scale > 0 ? 1 : 0; m.n_pi = e->n_pi; m.stride = batch;
   m.z = e->d_z.p; m.z_stride = n_patt; m.code_mask = e->d_code_mask.p;
   m.P = e->d_rowmajor.p; m.pint = e->d_pint.p; m.ptip = e->d_ptip.p; m.tip_words = (long)tw;
   m.pi = e->d_pi_plain.p; m.freqK = e->d_freqK.p;
   m.L = w.L.p; m.G = w.G.p; m.SL = w.SL.p; m.SG = w.SG.p; m.mfma = mfma ? 1 : 0;
   o.PT = w.PT.p; o.cap = cap; o.n_swaps = n_moves; o.f = w.f.p; o.sig = w.sig.p; o.weights = e->d_weights.p;
   o.lnf = w.lnf.p; o.partial = w.partial.p; o.n_chunks = n_chunks;
   o.ref_node = T.sons[T.sons_ptr[T.root]];
   a.Pup = w.Pup.p; a.Pdn = w.Pdn.p; a.Pm = w.Pm.p; a.PTup = w.PTup.p; a.pint_dn = w.pint_dn.p; a.ptip_dn = w.ptip_dn.p;
   a.pint_m = w.pint_m.p; a.ptip_m = w.ptip_m.p; a.PTm = w.PTm.p;
   a.prunes = w.plan.p; a.steps = w.plan.p + o_steps; a.factors = w.plan.p + o_factors;
   a.Lp = w.Lp.p; a.Ap = w.Ap.p; a.SLp = w.SLp.p; a.SAp = w.SAp.p;
   for (int g = 0; g < G; g++)
      for (long h0 = e->gene_off[g]; h0 < e->gene_off[g + 1]; h0 += batch) {
         const long nb = std::min<long>(batch, e->gene_off[g + 1] - h0);
         m.gene = g; m.h0 = h0; m.nb = nb;
         o.chunk0 = chunk_base[g] + (h0 - e->gene_off[g]) / GRAD_CHUNK;
         o.swap0 = 0; o.n_group = 0;
         const dim3 tiles((unsigned)((nb + ANC_TILE - 1) / ANC_TILE), K), lanes((unsigned)((nb + 255) / 256), K);
         HIPCHK(hipEventRecord(w.ev0, st));
         if (mfma) {
            hipLaunchKernelGGL(spr_unit_anc_mfma_kernel, tiles, dim3(256), 0, st, m, 0);
            HIPCHK(hipGetLastError());
            hipLaunchKernelGGL(spr_unit_nni_mfma_outer_kernel, tiles, dim3(256), 0, st, o);
            HIPCHK(hipGetLastError());
         }
         else
            for (int pass = 0; pass < 2; pass++) {
               spr_launch_lane(e->kk, lanes, st, a, pass);
               HIPCHK(hipGetLastError());
            }
         HIPCHK(hipEventRecord(w.ev1, st));
         for (size_t gi = 0; gi + 1 < group_first.size(); gi++) {
            const int ip0 = group_first[gi], ip1 = group_first[gi + 1];
            const int r0 = plan.prunes[SPR_PRUNE_INTS * ip0 + 3], r1 = ip1 < plan.n_prunes() ? plan.prunes[SPR_PRUNE_INTS * ip1 + 3] : n_moves;
            const int ng = r1 - r0;
            a.prune0 = ip0; a.n_prunes = ip1 - ip0;
            o.swap0 = r0; o.n_group = ng;
            if (gi) {      // (the batch's first group is timed with its down and outer passes)
               HIPCHK(hipStreamSynchronize(st));
               { float ms = 0; HIPCHK(hipEventElapsedTime(&ms, w.ev0, w.ev1)); spr_last_kernel_ms += ms; }
               HIPCHK(hipEventRecord(w.ev0, st));
            }
            if (mfma) hipLaunchKernelGGL(spr_mfma_kernel, tiles, dim3(256), 0, st, a);
            else spr_launch_lane(e->kk, lanes, st, a, 2);
            HIPCHK(hipGetLastError());
            hipLaunchKernelGGL(spr_unit_nni_combine_kernel, dim3(lanes.x, ng + (gi == 0 ? 1 : 0)), dim3(256), 0, st, o);
            HIPCHK(hipGetLastError());
            HIPCHK(hipEventRecord(w.ev1, st));
            // the group's rows to the caller's [n_moves][n_patt]: one plain copy per move
            if (lnf)
               for (int i = 0; i < ng; i++)
                  HIPCHK(hipMemcpyAsync(lnf + (size_t)plan.order[r0 + i] * n_patt + h0, w.lnf.p + (size_t)i * batch, (size_t)nb * 8, hipMemcpyDeviceToHost, st));
         }
         HIPCHK(hipStreamSynchronize(st));
         { float ms = 0; HIPCHK(hipEventElapsedTime(&ms, w.ev0, w.ev1)); spr_last_kernel_ms += ms; }
         spr_last_batches++;
      }
   HIPCHK(hipEventRecord(w.ev0, st));
   hipLaunchKernelGGL(spr_unit_grad_total_kernel, dim3(n_moves + 1), dim3(256), 0, st, (const double *)w.partial.p, n_chunks, w.out.p);
   HIPCHK(hipGetLastError());
   HIPCHK(hipEventRecord(w.ev1, st));
   std::vector<double> out((size_t)n_moves + 1);
   HIPCHK(hipMemcpyAsync(out.data(), w.out.p, ((size_t)n_moves + 1) * 8, hipMemcpyDeviceToHost, st));
   HIPCHK(hipStreamSynchronize(st));
   { float ms = 0; HIPCHK(hipEventElapsedTime(&ms, w.ev0, w.ev1)); spr_last_kernel_ms += ms; }
   for (int i = 0; i < n_moves; i++) lnL[plan.order[i]] = out[i];
   *lnL0 = out[n_moves];
   return 0;
}

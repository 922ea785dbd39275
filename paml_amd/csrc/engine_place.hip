// engine_place.hip — the lnL of the tree with one more tip hung on branch e, for every query sequence, every branch and every pendant
// length, in one call (paml_amd_placement_scores); the definition and the kernels in kernels_place.h.
// Every P(t) comes from the evaluation's own builders (anc_pmat, engine_ancestral.hip), which run once per family of lengths: the upper
// parts (1 - phi) t_v, the lower parts phi t_v, the pendant lengths (in the slots of the tips, every node labelled pendant_label), and last
// the tree's own lengths, so that d_rowmajor and pmat_valid are left as after paml_amd_nni_scores.  The down pass is the ancestral
// module's, the outer pass is the NNI module's.
// Built for gfx950 only (one of the translation units of libpaml_amd.so, see engine_state.h).
#include "engine_state.h"
#include "kernels_place.h"
#include "ancestral_host.h"

static thread_local int place_last_batches = 0;
static thread_local double place_last_kernel_ms = 0;      // HIP events around the P(t) kernels and every batch's passes, summed

extern "C" void paml_amd_placement_info(int *last_batches, double *last_kernel_ms)
{
   if (last_batches) *last_batches = place_last_batches;
   if (last_kernel_ms) *last_kernel_ms = place_last_kernel_ms;
}

namespace {

struct PlaceScratch : AncScratch {
   DevBuf<double> PT, Pup, Pdn, PTup, pint_dn, ptip_dn, Ppend, ptip_pend, f0, sig0, lnf0, f, sig, lnf, partial, out;
   DevBuf<int> edges, lab;
   DevBuf<unsigned char> qz;
   ~PlaceScratch()
   {
      for (DevBuf<double> *b : {&PT, &Pup, &Pdn, &PTup, &pint_dn, &ptip_dn, &Ppend, &ptip_pend, &f0, &sig0, &lnf0, &f, &sig, &lnf, &partial, &out}) b->release();
      edges.release(); lab.release(); qz.release();
   }
};

void place_launch_lane(KernelKind kk, dim3 grid, hipStream_t st, const PlaceArgs &a, int pass)
{
   if (kk == KK_VALU4) hipLaunchKernelGGL(place_lane_kernel<4>, grid, dim3(256), 0, st, a, pass);
   else if (kk == KK_VALU5) hipLaunchKernelGGL(place_lane_kernel<5>, grid, dim3(256), 0, st, a, pass);
   else hipLaunchKernelGGL(place_lane_kernel<20>, grid, dim3(256), 0, st, a, pass);
}

void place_launch_lane_edge(KernelKind kk, dim3 grid, hipStream_t st, const PlaceArgs &a)
{
   if (kk == KK_VALU4) hipLaunchKernelGGL(place_lane_edge_kernel<4>, grid, dim3(256), 0, st, a);
   else if (kk == KK_VALU5) hipLaunchKernelGGL(place_lane_edge_kernel<5>, grid, dim3(256), 0, st, a);
   else hipLaunchKernelGGL(place_lane_edge_kernel<20>, grid, dim3(256), 0, st, a);
}

// the builder's P(t) at `branch` (labels `d_label`, null: the tree's), waited for; its kernel time is added to the call's
int place_pmat(paml_amd_engine *e, const char *who, const double *branch, const double *gene_rate, PlaceScratch &w, const int *d_label)
{
   if (int rc = anc_pmat(e, who, branch, gene_rate, w, d_label)) return rc;
   HIPCHK(hipEventRecord(w.ev1, e->stream));
   HIPCHK(hipStreamSynchronize(e->stream));
   if (int rc = eigen_fail_check(e)) return rc;
   float ms = 0;
   HIPCHK(hipEventElapsedTime(&ms, w.ev0, w.ev1));
   place_last_kernel_ms += ms;
   return 0;
}

}  // namespace

extern "C" int paml_amd_placement_scores(paml_amd_engine *e, const double *branch, const double *gene_rate, int n_q, const unsigned char *qz,
                                         int n_edges, const int *edges, int n_pend, const double *pendant, double phi, int pendant_label,
                                         double *lnL0, double *lnL, double *lnf)
{
   enter(e);
   place_last_batches = 0;
   place_last_kernel_ms = 0;
   const char *who = "placement_scores";
   if (!e || !branch || !qz || !pendant || !lnL0 || !lnL) return fail(e, PAML_AMD_EINVAL, "placement_scores: null argument");
   if (n_q < 1) return fail(e, PAML_AMD_EINVAL, "placement_scores: n_q < 1");
   if (n_edges < 1) return fail(e, PAML_AMD_EINVAL, "placement_scores: n_edges < 1");
   if (n_pend < 1) return fail(e, PAML_AMD_EINVAL, "placement_scores: n_pend < 1");
   if (int rc = anc_common_checks(e, who)) return rc;
   if (e->world > 1) return fail(e, PAML_AMD_EUNSUPPORTED, "placement_scores: one rank only (this engine's communicator has " + std::to_string(e->world) + ")");
   const TreeDesc &T = e->tree;
   const int nn = T.n_nodes, n = e->n, K = e->K, G = e->n_genes, n_tips = e->n_tips, n_int = nn - n_tips;
   const long n_patt = e->n_patt;
   std::vector<int> edge_list;
   if (edges) {
      for (int i = 0; i < n_edges; i++) {
         const int v = edges[i];
         const std::string at = "placement_scores: edge " + std::to_string(i) + ": ";
         if (v < 0 || v >= nn) return fail(e, PAML_AMD_EINVAL, at + "node " + std::to_string(v) + " is out of range");
         if (v == T.root) return fail(e, PAML_AMD_EINVAL, at + "node " + std::to_string(v) + " is the root");
      }
      edge_list.assign(edges, edges + n_edges);
   }
   else {
      for (int v = 0; v < nn; v++)
         if (v != T.root) edge_list.push_back(v);
      if (n_edges != (int)edge_list.size())
         return fail(e, PAML_AMD_EINVAL, "placement_scores: n_edges = " + std::to_string(n_edges) + " with a null list: the tree has " + std::to_string(edge_list.size()) + " edges");
   }
   if (!(phi >= 0 && phi <= 1)) return fail(e, PAML_AMD_EINVAL, "placement_scores: phi = " + std::to_string(phi) + " is outside [0, 1]");
   for (int j = 0; j < n_pend; j++)
      if (!(pendant[j] >= 0) || !std::isfinite(pendant[j]))
         return fail(e, PAML_AMD_EINVAL, "placement_scores: pendant " + std::to_string(j) + " is negative or not finite");
   if (pendant_label < 0 || pendant_label >= e->n_labels)
      return fail(e, PAML_AMD_EINVAL, "placement_scores: pendant_label = " + std::to_string(pendant_label) + " is outside the class tables' " + std::to_string(e->n_labels) + " labels");
   // the queries' codes in the engine's own numbering
   std::vector<unsigned char> qcodes((size_t)n_q * n_patt);
   for (int qi = 0; qi < n_q; qi++)
      for (long h = 0; h < n_patt; h++) {
         const int c = qz[(size_t)qi * n_patt + h];
         if (c >= e->n_codes || e->code_nch[c] < 1)
            return fail(e, PAML_AMD_EINVAL, "placement_scores: query " + std::to_string(qi) + ", pattern " + std::to_string(h) + ": character code " + std::to_string(c) +
                                                (c >= e->n_codes ? " >= n_codes" : " has an empty state set"));
         qcodes[(size_t)qi * n_patt + h] = e->code_new_of[c];
      }
   std::vector<int> slots;      // where a pendant length's P(t) is built: the tips (their column tables are made for leaves only)
   for (int v = 0; v < n_tips; v++)
      if (v != T.root && T.is_leaf(v)) slots.push_back(v);
   if (slots.empty()) return fail(e, PAML_AMD_EINVAL, "placement_scores: the tree has no tip below its root");

   const bool mfma = e->kk == KK_MFMA64;
   hipStream_t st = e->stream;
   PlaceScratch w;
   PlaceArgs a{};
   NniArgs &o = a.o;
   AncMargArgs &m = o.m;
   if (int rc = anc_tree_pack(e, who, w, &m.t)) return rc;
   const size_t psets = (size_t)G * K, pn = psets * nn, nn2 = (size_t)n * n, tw = tip_words(e);
   {
      // the upper and the lower part of every branch
      std::vector<double> b(nn);
      for (int v = 0; v < nn; v++) b[v] = (1 - phi) * branch[v];
      if (int rc = place_pmat(e, who, b.data(), gene_rate, w, nullptr)) return rc;
      if (mfma) {
         HIPCHK(w.PTup.ensure(pn * 4096));
         hipLaunchKernelGGL(place_pt_kernel, dim3(nn, (unsigned)psets), dim3(256), 0, st, (const double *)e->d_rowmajor.p, w.PTup.p, n, nn, T.root);
         HIPCHK(hipGetLastError());
         HIPCHK(hipStreamSynchronize(st));
      }
      else {
         HIPCHK(w.Pup.ensure(pn * nn2));
         HIPCHK(hipMemcpyAsync(w.Pup.p, e->d_rowmajor.p, pn * nn2 * 8, hipMemcpyDeviceToDevice, st));
         HIPCHK(hipStreamSynchronize(st));
      }
      for (int v = 0; v < nn; v++) b[v] = phi * branch[v];
      if (int rc = place_pmat(e, who, b.data(), gene_rate, w, nullptr)) return rc;
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
      // the pendant lengths, as many per run of the builder as the tree has tips
      std::vector<int> lab(nn, pendant_label);
      HIPCHK(upload(w.lab, lab.data(), lab.size(), st));
      HIPCHK(hipStreamSynchronize(st));
      if (mfma) HIPCHK(w.ptip_pend.ensure(psets * n_pend * tw));
      else HIPCHK(w.Ppend.ensure(psets * n_pend * nn2));
      for (int j0 = 0; j0 < n_pend; j0 += (int)slots.size()) {
         const int nj = std::min<int>((int)slots.size(), n_pend - j0);
         std::fill(b.begin(), b.end(), 0.0);
         for (int j = 0; j < nj; j++) b[slots[j]] = pendant[j0 + j];
         if (int rc = place_pmat(e, who, b.data(), gene_rate, w, w.lab.p)) return rc;
         for (size_t ps = 0; ps < psets; ps++)
            for (int j = 0; j < nj; j++) {
               const size_t from = ps * nn + slots[j], to = ps * n_pend + j0 + j;
               if (mfma) HIPCHK(hipMemcpyAsync(w.ptip_pend.p + to * tw, e->d_ptip.p + from * tw, tw * 8, hipMemcpyDeviceToDevice, st));
               else HIPCHK(hipMemcpyAsync(w.Ppend.p + to * nn2, e->d_rowmajor.p + from * nn2, nn2 * 8, hipMemcpyDeviceToDevice, st));
            }
         HIPCHK(hipStreamSynchronize(st));
      }
   }
   // the tree's own lengths last: what the passes read, and what the engine keeps
   if (int rc = anc_pmat(e, who, branch, gene_rate, w)) return rc;
   if (mfma) {
      HIPCHK(w.PT.ensure(pn * 4096));
      hipLaunchKernelGGL(place_unit_nni_pt_kernel, dim3(nn, (unsigned)psets), dim3(256), 0, st, (const double *)e->d_rowmajor.p, w.PT.p, n, nn, n_tips, T.root);
      HIPCHK(hipGetLastError());
   }
   HIPCHK(upload(w.edges, edge_list.data(), edge_list.size(), st));
   HIPCHK(upload(w.qz, qcodes.data(), qcodes.size(), st));
   HIPCHK(hipEventRecord(w.ev1, st));
   HIPCHK(hipStreamSynchronize(st));
   if (int rc = eigen_fail_check(e)) return rc;
   e->pmat_valid = true;      // (d_rowmajor holds every branch's P(t) in the tree's own orientation, as after the gradient)
   { float ms = 0; HIPCHK(hipEventElapsedTime(&ms, w.ev0, w.ev1)); place_last_kernel_ms += ms; }

   // chunks of GRAD_CHUNK patterns counted from each gene's first pattern: a batch is whole chunks of one gene
   std::vector<long> chunk_base(G + 1, 0);
   for (int g = 0; g < G; g++) chunk_base[g + 1] = chunk_base[g] + (e->gene_off[g + 1] - e->gene_off[g] + GRAD_CHUNK - 1) / GRAD_CHUNK;
   const long n_chunks = chunk_base[G];
   const long rows_edge = (long)n_q * n_pend, n_rows = rows_edge * n_edges;
   HIPCHK(w.partial.ensure((size_t)(n_rows + 1) * std::max<long>(n_chunks, 1)));
   HIPCHK(w.out.ensure((size_t)n_rows + 1));

   // the workspace per pattern: the partials and the messages, then (2 K + 1) doubles per row (the present tree's, and n_q n_pend per edge of a group)
   const int ns = mfma ? 64 : n;      // doubles a partial takes per pattern
   const double fixed = 2.0 * K * n_int * (ns + 1) * 8 + (2.0 * K + 1) * 8, per_edge = (2.0 * K + 1) * 8 * rows_edge;
   double arena_mb = 256;
   if (const char *s = getenv("PAML_AMD_PLACE_ARENA_MB")) { const double v = atof(s); if (v > 0) arena_mb = v; }
   int cap = n_edges;
   if ((fixed + per_edge * n_edges) * ANC_TILE > arena_mb * 1048576.0)      // one tile with all rows does not fit: groups of edges
      cap = (int)std::min<double>(n_edges, std::max(1.0, floor((arena_mb * 1048576.0 / ANC_TILE - fixed) / per_edge)));
   cap = std::min(cap, 65535);      // (the lanes' edge pass has a grid layer per edge)
   long batch = anc_batch(fixed + per_edge * cap, n_patt, "PAML_AMD_PLACE_ARENA_MB");
   for (;;) {      // halve the batch until it fits
      const size_t part = (size_t)K * n_int * ns * batch, sc = (size_t)K * n_int * batch, rows = (size_t)K * cap * rows_edge * batch;
      if (w.L.ensure(part) == hipSuccess && w.G.ensure(part) == hipSuccess && w.SL.ensure(sc) == hipSuccess && w.SG.ensure(sc) == hipSuccess &&
          w.f0.ensure((size_t)K * batch) == hipSuccess && w.sig0.ensure((size_t)K * batch) == hipSuccess && w.lnf0.ensure((size_t)batch) == hipSuccess &&
          w.f.ensure(rows) == hipSuccess && w.sig.ensure(rows) == hipSuccess && w.lnf.ensure((size_t)cap * rows_edge * batch) == hipSuccess)
         break;
      (void)hipGetLastError();
      for (DevBuf<double> *b : {&w.L, &w.G, &w.SL, &w.SG, &w.f0, &w.sig0, &w.lnf0, &w.f, &w.sig, &w.lnf}) b->release();      // (ensure only grows: the retry starts from nothing)
      if (batch <= ANC_TILE) return fail(e, PAML_AMD_ENOMEM, "placement_scores: no device memory for one tile of patterns");
      batch = (batch / 2 + ANC_TILE - 1) / ANC_TILE * ANC_TILE;
   }
   m.n = n; m.K = K; m.scaled = T.n_scale > 0 ? 1 : 0; m.n_pi = e->n_pi; m.stride = batch;
   m.z = e->d_z.p; m.z_stride = n_patt; m.code_mask = e->d_code_mask.p;
   m.P = e->d_rowmajor.p; m.pint = e->d_pint.p; m.ptip = e->d_ptip.p; m.tip_words = (long)tw;
   m.pi = e->d_pi_plain.p; m.freqK = e->d_freqK.p;
   m.L = w.L.p; m.G = w.G.p; m.SL = w.SL.p; m.SG = w.SG.p; m.mfma = mfma ? 1 : 0;
   o.PT = w.PT.p; o.cap = 0; o.f = w.f0.p; o.sig = w.sig0.p; o.weights = e->d_weights.p; o.lnf = w.lnf0.p; o.n_chunks = n_chunks;
   o.ref_node = T.sons[T.sons_ptr[T.root]];
   a.Pup = w.Pup.p; a.Pdn = w.Pdn.p; a.PTup = w.PTup.p; a.pint_dn = w.pint_dn.p; a.ptip_dn = w.ptip_dn.p; a.Ppend = w.Ppend.p; a.ptip_pend = w.ptip_pend.p;
   a.qz = w.qz.p; a.edges = w.edges.p; a.n_q = n_q; a.n_pend = n_pend; a.n_edges = n_edges; a.cap = cap;
   a.f = w.f.p; a.sig = w.sig.p; a.lnf = w.lnf.p; a.partial = w.partial.p;
   for (int g = 0; g < G; g++)
      for (long h0 = e->gene_off[g]; h0 < e->gene_off[g + 1]; h0 += batch) {
         const long nb = std::min<long>(batch, e->gene_off[g + 1] - h0);
         m.gene = g; m.h0 = h0; m.nb = nb;
         o.chunk0 = chunk_base[g] + (h0 - e->gene_off[g]) / GRAD_CHUNK;
         a.edge0 = 0; a.n_group = 0;
         const dim3 tiles((unsigned)((nb + ANC_TILE - 1) / ANC_TILE), K), lanes((unsigned)((nb + 255) / 256), K);
         HIPCHK(hipEventRecord(w.ev0, st));
         if (mfma) {
            hipLaunchKernelGGL(place_unit_anc_mfma_kernel, tiles, dim3(256), 0, st, m, 0);
            HIPCHK(hipGetLastError());
            hipLaunchKernelGGL(place_unit_nni_mfma_outer_kernel, tiles, dim3(256), 0, st, o);
            HIPCHK(hipGetLastError());
         }
         else
            for (int pass = 0; pass < 2; pass++) {
               place_launch_lane(e->kk, lanes, st, a, pass);
               HIPCHK(hipGetLastError());
            }
         hipLaunchKernelGGL(place_present_kernel, dim3(lanes.x), dim3(256), 0, st, a);
         HIPCHK(hipGetLastError());
         HIPCHK(hipEventRecord(w.ev1, st));
         for (int e0 = 0; e0 < n_edges; e0 += cap) {
            const int ng = std::min(cap, n_edges - e0);
            a.edge0 = e0; a.n_group = ng;
            if (e0) {      // (the batch's first group is timed with its down and outer passes)
               HIPCHK(hipStreamSynchronize(st));
               { float ms = 0; HIPCHK(hipEventElapsedTime(&ms, w.ev0, w.ev1)); place_last_kernel_ms += ms; }
               HIPCHK(hipEventRecord(w.ev0, st));
            }
            if (mfma) hipLaunchKernelGGL(place_mfma_kernel, tiles, dim3(256), 0, st, a);
            else place_launch_lane_edge(e->kk, dim3(lanes.x, K, ng), st, a);
            HIPCHK(hipGetLastError());
            const long rows = rows_edge * ng;
            for (long r0 = 0; r0 < rows; r0 += 65535) {
               hipLaunchKernelGGL(place_combine_kernel, dim3(lanes.x, (unsigned)std::min<long>(65535, rows - r0)), dim3(256), 0, st, a, r0);
               HIPCHK(hipGetLastError());
            }
            HIPCHK(hipEventRecord(w.ev1, st));
            // the group's rows to the caller's [n_q][n_edges][n_pend][n_patt]: one plain copy per row
            if (lnf)
               for (long r = 0; r < rows; r++)
                  HIPCHK(hipMemcpyAsync(lnf + (size_t)place_out_row(a, r) * n_patt + h0, w.lnf.p + (size_t)r * batch, (size_t)nb * 8, hipMemcpyDeviceToHost, st));
         }
         HIPCHK(hipStreamSynchronize(st));
         { float ms = 0; HIPCHK(hipEventElapsedTime(&ms, w.ev0, w.ev1)); place_last_kernel_ms += ms; }
         place_last_batches++;
      }
   HIPCHK(hipEventRecord(w.ev0, st));
   hipLaunchKernelGGL(place_unit_grad_total_kernel, dim3((unsigned)(n_rows + 1)), dim3(256), 0, st, (const double *)w.partial.p, n_chunks, w.out.p);
   HIPCHK(hipGetLastError());
   HIPCHK(hipEventRecord(w.ev1, st));
   std::vector<double> out((size_t)n_rows + 1);
   HIPCHK(hipMemcpyAsync(out.data(), w.out.p, ((size_t)n_rows + 1) * 8, hipMemcpyDeviceToHost, st));
   HIPCHK(hipStreamSynchronize(st));
   { float ms = 0; HIPCHK(hipEventElapsedTime(&ms, w.ev0, w.ev1)); place_last_kernel_ms += ms; }
   for (long i = 0; i < n_rows; i++) lnL[i] = out[i];
   *lnL0 = out[n_rows];
   return 0;
}

// engine_place.hip — the lnL of the tree with one more tip hung on branch e, for every query sequence, every branch and every pendant
// length, in one call (paml_amd_placement_scores); the definition in kernels_place.h, the kernels here.
// Every P(t) comes from the evaluation's own builders (anc_pmat, engine_ancestral.hip), which run once per family of lengths: the upper
// parts (1 - phi) t_v, the lower parts phi t_v, the pendant lengths (in the slots of the tips, every node labelled pendant_label), and last
// the tree's own lengths, so that d_rowmajor and pmat_valid are left as after paml_amd_nni_scores.  The down pass is the ancestral
// module's, the outer pass is the NNI module's.
// The host side that is not this call's own is the score calls' skeleton (score_host.h, defined in engine_ancestral.hip).
// Built for gfx950 only (one of the translation units of libpaml_amd.so, see engine_state.h).
#include "engine_state.h"
#include "kernels_place.h"
#include "score_host.h"

static thread_local AncCallInfo place_info;

extern "C" void paml_amd_placement_info(int *last_batches, double *last_kernel_ms) { place_info.read(last_batches, last_kernel_ms); }

namespace paml_amd {

// one (pattern, class, edge) per lane: grid (patterns / 256, K, edges of the group)
template <int N> __global__ __launch_bounds__(256) void place_lane_edge_kernel(PlaceArgs a)
{
   const long p = (long)blockIdx.x * 256 + threadIdx.x;
   if (p >= a.o.m.nb) return;
   place_lane_edge<N>(a, blockIdx.y, p, blockIdx.z);
}

// Matrix cores: four waves own ANC_TILE patterns of one class and loop over the group's edges; lane = q * 16 + pattern, register m =
// state 4 m + q.  Per edge: H_v, one product with P_v^T((1 - phi) t), one product with P_v(phi t) (a tip: a gather from its column
// table), W_v in registers; per (query, pendant) one gather from the pendant's column table and one dot product.  Grid (stride / ANC_TILE, K).
__global__ __launch_bounds__(256) void place_mfma_kernel(PlaceArgs a)
{
   __shared__ __attribute__((aligned(16))) double sP[4096];
   const AncMargArgs &m = a.o.m;
   const AncTree &t = m.t;
   const ScoreTile c = score_tile(m);
   const int lane = c.lane, q = c.q, k = c.k;
   const long g16 = c.g16, p = c.p, pc = c.pc, pset = c.pset;
   const AncMfma w{sP, lane, c.wave, q};
   const double *tabs = a.ptip_pend + pset * a.n_pend * m.tip_words;
   for (int i = 0; i < a.n_group; i++) {
      const int v = a.edges[a.edge0 + i];
      double h[16], u[16], ls;
      score_mfma_hv(m, w, c, v, h, &ls);
      const long slot = pset * t.n_nodes + v;
      v4d acc[4];
      w.product(a.PTup + slot * 4096, h, acc);      // U_v = P_v((1 - phi) t)^T H_v
#pragma unroll
      for (int j = 0; j < 16; j++) u[j] = acc[j >> 2][j & 3];
      if (v < t.n_tips) {      // (uniform over the workgroup) D_v of a tip: its column table of P_v(phi t)
         double2 tv[8];
         tip_gather(a.ptip_dn + pset * t.n_nodes * m.tip_words, m.tip_words, v, (int)m.z[(long)v * m.z_stride + m.h0 + pc], q, tv);
#pragma unroll
         for (int j = 0; j < 8; j++) { u[2 * j] *= tv[j].x; u[2 * j + 1] *= tv[j].y; }
      }
      else {
         const int vi = v - t.n_tips;
         double x[16];
         part_load(m.L + (((long)k * t.n_int + vi) * (m.stride >> 4) + g16) * 1024, lane, x);
         w.product(a.pint_dn + slot * 4096, x, acc);      // D_v = P_v(phi t) L_v
#pragma unroll
         for (int j = 0; j < 16; j++) u[j] *= acc[j >> 2][j & 3];
         ls += m.SL[((long)k * t.n_int + vi) * m.stride + pc];
      }
      for (int qi = 0; qi < a.n_q; qi++) {
         const int code = (int)a.qz[(long)qi * m.z_stride + m.h0 + pc];
         for (int j = 0; j < a.n_pend; j++) {
            double2 tv[8];
            tip_gather(tabs, m.tip_words, j, code, q, tv);
            double y[16];
#pragma unroll
            for (int c = 0; c < 8; c++) { y[2 * c] = tv[c].x; y[2 * c + 1] = tv[c].y; }
            const double fk = grad_mfma_dot(u, y);
            const long oi = place_out_idx(a, k, place_row(a, i, qi, j), p);
            if (q == 0) { a.f[oi] = fk; a.sig[oi] = ls; }
         }
      }
   }
}

// the classes of every (row, pattern) and the chunks' sums: grid (stride / 256, rows of the slice); a wave = one chunk of GRAD_CHUNK
// patterns.  row0: the slice's first row (a grid has 65535 rows at most)
__global__ __launch_bounds__(256) void place_combine_kernel(PlaceArgs a, long row0)
{
   const long p = (long)blockIdx.x * 256 + threadIdx.x;
   const long row = row0 + blockIdx.y;
   const double acc = score_wave_sum(p < a.o.m.nb ? place_combine(a, row, p) : 0.0);
   long chunk;
   if (score_chunk_lane(a.o, p, &chunk)) a.partial[place_out_row(a, row) * a.o.n_chunks + chunk] = acc;
}

// the present tree's row (the outer pass left f_hk and sigma in o.f / o.sig): grid (stride / 256)
__global__ __launch_bounds__(256) void place_present_kernel(PlaceArgs a)
{
   const long p = (long)blockIdx.x * 256 + threadIdx.x;
   const double acc = score_wave_sum(p < a.o.m.nb ? nni_combine(a.o, 0, p) : 0.0);
   long chunk;
   if (score_chunk_lane(a.o, p, &chunk)) a.partial[(long)a.n_q * a.n_edges * a.n_pend * a.o.n_chunks + chunk] = acc;
}
}  // namespace paml_amd

namespace {

struct PlaceScratch : ScoreScratch {      // (f, sig, lnf: the present tree's row; rf, rsig, rlnf: the rows of a group)
   using ScoreScratch::ScoreScratch;
   DevBuf<double> Pup, Pdn, PTup, pint_dn, ptip_dn, Ppend, ptip_pend, rf, rsig, rlnf;
   DevBuf<int> edges, lab;
   DevBuf<unsigned char> qz;
};

}  // namespace

extern "C" int paml_amd_placement_scores(paml_amd_engine *e, const double *branch, const double *gene_rate, int n_q, const unsigned char *qz,
                                         int n_edges, const int *edges, int n_pend, const double *pendant, double phi, int pendant_label,
                                         double *lnL0, double *lnL, double *lnf)
{
   enter(e);
   place_info = AncCallInfo{};
   const char *who = "placement_scores";
   if (!e || !branch || !qz || !pendant || !lnL0 || !lnL) return fail(e, PAML_AMD_EINVAL, "placement_scores: null argument");
   if (n_q < 1) return fail(e, PAML_AMD_EINVAL, "placement_scores: n_q < 1");
   if (n_edges < 1) return fail(e, PAML_AMD_EINVAL, "placement_scores: n_edges < 1");
   if (n_pend < 1) return fail(e, PAML_AMD_EINVAL, "placement_scores: n_pend < 1");
   if (int rc = score_begin(e, who, nullptr)) return rc;
   const TreeDesc &T = e->tree;
   const int nn = T.n_nodes, n = e->n, K = e->K, G = e->n_genes, n_tips = e->n_tips;
   const long n_patt = e->n_patt;
   std::vector<int> edge_list;
   if (edges) {
      for (int i = 0; i < n_edges; i++) {
         const int v = edges[i];
         if (int rc = score_check_node(e, "placement_scores: edge " + std::to_string(i) + ": ", v, nullptr, false)) return rc;
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
      if (int rc = score_query_codes(e, "placement_scores: ", qi, qz, qcodes.data())) return rc;
   std::vector<int> slots;      // where a pendant length's P(t) is built: the tips (their column tables are made for leaves only)
   for (int v = 0; v < n_tips; v++)
      if (v != T.root && T.is_leaf(v)) slots.push_back(v);
   if (slots.empty()) return fail(e, PAML_AMD_EINVAL, "placement_scores: the tree has no tip below its root");

   const bool mfma = e->kk == KK_MFMA64;
   hipStream_t st = e->stream;
   PlaceScratch w(place_info);
   PlaceArgs a{};
   NniArgs &o = a.o;
   AncMargArgs &m = o.m;
   if (int rc = anc_tree_pack(e, who, w, &m.t)) return rc;
   const size_t psets = (size_t)G * K, nn2 = (size_t)n * n, tw = tip_words(e);
   {
      // the upper and the lower part of every branch
      std::vector<double> b(nn);
      for (int v = 0; v < nn; v++) b[v] = (1 - phi) * branch[v];
      if (int rc = anc_pmat_waited(e, who, b.data(), gene_rate, w)) return rc;
      if (int rc = anc_keep_pmat(e, nullptr, nullptr, &w.PTup, w.Pup)) return rc;
      for (int v = 0; v < nn; v++) b[v] = phi * branch[v];
      if (int rc = anc_pmat_waited(e, who, b.data(), gene_rate, w)) return rc;
      if (int rc = anc_keep_pmat(e, &w.pint_dn, &w.ptip_dn, nullptr, w.Pdn)) return rc;
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
         if (int rc = anc_pmat_waited(e, who, b.data(), gene_rate, w, w.lab.p)) return rc;
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
   if (int rc = score_present_pmat(e, who, branch, gene_rate, w)) return rc;
   HIPCHK(upload(w.edges, edge_list.data(), edge_list.size(), st));
   HIPCHK(upload(w.qz, qcodes.data(), qcodes.size(), st));
   if (int rc = anc_pmat_wait(e, w)) return rc;
   e->pmat_valid = true;      // (d_rowmajor holds every branch's P(t) in the tree's own orientation, as after the gradient)

   // the workspace per pattern: the partials and the messages, then (2 K + 1) doubles per row (the present tree's, and n_q n_pend per edge of a group)
   const long rows_edge = (long)n_q * n_pend, n_rows = rows_edge * n_edges;
   const double per_row = (2.0 * K + 1) * 8;
   ScorePlan plan;
   // (the edges are what is grouped; no extra row: the present tree's is counted in the fixed part)
   if (int rc = score_plan(e, w, &plan, "PAML_AMD_PLACE_ARENA_MB", per_row * rows_edge, n_edges, n_rows, 0, score_fixed(e) + per_row)) return rc;
   const int cap = plan.cap;      // edges of a group (the lanes' edge pass has a grid layer per edge)
   const size_t rows = (size_t)K * cap * rows_edge;
   if (int rc = score_alloc(e, who, w, plan, {{&w.f, (size_t)K}, {&w.sig, (size_t)K}, {&w.lnf, 1}, {&w.rf, rows}, {&w.rsig, rows}, {&w.rlnf, (size_t)cap * rows_edge}})) return rc;
   score_fill(o, w, e, plan, 0);
   o.cap = 0;      // (the passes' workspace is the present tree's row alone; the groups' rows are PlaceArgs's own)
   a.Pup = w.Pup.p; a.Pdn = w.Pdn.p; a.PTup = w.PTup.p; a.pint_dn = w.pint_dn.p; a.ptip_dn = w.ptip_dn.p; a.Ppend = w.Ppend.p; a.ptip_pend = w.ptip_pend.p;
   a.qz = w.qz.p; a.edges = w.edges.p; a.n_q = n_q; a.n_pend = n_pend; a.n_edges = n_edges; a.cap = cap;
   a.f = w.rf.p; a.sig = w.rsig.p; a.lnf = w.rlnf.p; a.partial = w.partial.p;
   auto group = [&](int gi) { a.edge0 = gi * cap; a.n_group = std::min(cap, n_edges - a.edge0); };      // groups of `cap` edges in list order
   if (int rc = anc_score_batches(
          e, w, o, plan.batch, score_n_groups(n_edges, cap),
          [&](int gi, dim3 tiles, dim3 lanes) {
             group(gi);
             if (mfma) hipLaunchKernelGGL(place_mfma_kernel, tiles, dim3(256), 0, st, a);
             else anc_lanes(e->kk, [&](auto N) { hipLaunchKernelGGL(place_lane_edge_kernel<N()>, dim3(lanes.x, K, a.n_group), dim3(256), 0, st, a); });
          },
          [&](int, dim3 lanes) {      // (a grid has 65535 rows at most)
             const long rows = rows_edge * a.n_group;
             for (long r0 = 0; r0 < rows; r0 += 65535)
                hipLaunchKernelGGL(place_combine_kernel, dim3(lanes.x, (unsigned)std::min<long>(65535, rows - r0)), dim3(256), 0, st, a, r0);
          },
          [&](int, long h0, long nb) {      // the group's rows to the caller's [n_q][n_edges][n_pend][n_patt]
             return score_copy_rows(e, w.rlnf.p, plan.batch, 0, rows_edge * a.n_group, lnf, h0, nb, [&](long r) { return place_out_row(a, r); });
          },
          [&](dim3 lanes) {      // the present tree's row, by a kernel of its own
             a.edge0 = 0; a.n_group = 0;
             hipLaunchKernelGGL(place_present_kernel, dim3(lanes.x), dim3(256), 0, st, a);
          }))
      return rc;
   return score_totals(e, w, plan, n_rows, nullptr, lnL0, {lnL});
}

// engine_relabel.hip — the lnL of the tree with the label of one branch changed, for many (branch, label) rows in one call
// (paml_amd_relabel_scores), with the per-class, per-pattern values a host needs to re-mix the site classes; the definition in
// kernels_relabel.h, the kernels here.  The tree's own P(t) comes from the evaluation's builders (anc_pmat, engine_ancestral.hip), the
// override matrices from the edge call's formulas (edge_pmat_fill, kernels_edge.h), the down pass is the ancestral module's, the outer
// pass is the NNI call's.
// The host side that is not this call's own is the score calls' skeleton (score_host.h, defined in engine_ancestral.hip).
// Built for gfx950 only (one of the translation units of libpaml_amd.so, see engine_state.h).
#include <algorithm>
#include <map>

#include "engine_state.h"
#include "kernels_relabel.h"
#include "kernels_edge.h"
#include "score_host.h"

static thread_local AncCallInfo relabel_info;

extern "C" void paml_amd_relabel_info(int *last_batches, double *last_kernel_ms) { relabel_info.read(last_batches, last_kernel_ms); }

namespace paml_amd {

// P' of every (matrix slot, parameter set) whose class the slot's label changes: grid (slots, gene x class)
__global__ __launch_bounds__(256) void relabel_pmat_kernel(RelabelPmatArgs a)
{
   const int slot = blockIdx.x, pset = blockIdx.y;
   if (!a.changed[(long)slot * a.psets + pset]) return;      // (uniform over the workgroup)
   __shared__ double sE[64], sM[64];
   const int v = a.slots[2 * slot], lab = a.slots[2 * slot + 1];
   edge_pmat_fill<false>(a.g, pset, lab, a.g.branch[v], false, false, sE, sM, a.OM + ((long)slot * a.psets + pset) * a.msz, nullptr, nullptr);
}

// one pattern per lane, the row pass: grid (patterns / 256, K, rows of the group); the block of a row that starts a node's run walks the run
template <int N> __global__ __launch_bounds__(256) void relabel_lane_kernel(RelabelArgs a)
{
   const long p = (long)blockIdx.x * 256 + threadIdx.x;
   if (p >= a.o.m.nb || !relabel_run_start(a, blockIdx.z)) return;
   relabel_lane_node<N>(a, blockIdx.y, p, blockIdx.z);
}

// Matrix cores, the row pass: four waves own ANC_TILE patterns of one class and loop over the group's rows; H_v (h) and L_v (l) are
// formed where the node changes and held in registers over the node's rows.  Grid (stride / ANC_TILE, K).
__global__ __launch_bounds__(256) void relabel_mfma_kernel(RelabelArgs a)
{
   __shared__ __attribute__((aligned(16))) double sP[4096];
   const AncMargArgs &m = a.o.m;
   const AncTree &t = m.t;
   const ScoreTile c = score_tile(m);
   const int lane = c.lane, q = c.q, k = c.k;
   const long p = c.p, pc = c.pc, pset = c.pset;
   const AncMfma w{sP, lane, c.wave, q};
   const long o0 = nni_out_idx(a.o, k, a.o.cap, p);
   double h[16], l[16], ls = 0;
   int v_held = -1;
   for (int i = 0; i < a.o.n_group; i++) {
      const int *rw = a.rows + 3L * (a.o.swap0 + i);
      const int v = rw[0], slot = rw[1];
      const long oi = nni_out_idx(a.o, k, i, p);
      if (!a.changed[(long)slot * a.psets + pset]) {      // (uniform over the workgroup) the present tree's values
         if (q == 0) { a.o.f[oi] = a.o.f[o0]; a.o.sig[oi] = a.o.sig[o0]; }
         continue;
      }
      if (v != v_held) {
         score_mfma_hv(m, w, c, v, h, &ls);
         if (v < t.n_tips) {      // a tip: its code's indicator through the product
            const unsigned long long mask = m.code_mask[m.z[(long)v * m.z_stride + m.h0 + pc]];
#pragma unroll
            for (int j = 0; j < 16; j++) l[j] = (mask >> (4 * j + q)) & 1ull ? 1.0 : 0.0;
         }
         else {
            score_mfma_lv(m, c, v, l, &ls);
         }
         v_held = v;
      }
      v4d acc[4];
      w.product(a.OM + ((long)slot * a.psets + pset) * 4096, l, acc);
      double y[16];
#pragma unroll
      for (int j = 0; j < 16; j++) y[j] = acc[j >> 2][j & 3];
      const double fk = grad_mfma_dot(h, y);
      if (q == 0) { a.o.f[oi] = fk; a.o.sig[oi] = ls; }
   }
}

// the classes of every (row, pattern) and the chunks' sums: grid (stride / 256, rows); a wave = one chunk of GRAD_CHUNK patterns.  A
// row's chunks go to the caller's index of the row.
__global__ __launch_bounds__(256) void relabel_combine_kernel(RelabelArgs a)
{
   const long p = (long)blockIdx.x * 256 + threadIdx.x;
   const bool present = (int)blockIdx.y == a.o.n_group;      // (a batch's first group is launched with a row more: the present tree)
   const int row = present ? a.o.cap : (int)blockIdx.y;
   const double acc = score_wave_sum(p < a.o.m.nb ? relabel_combine(a, row, p) : 0.0);
   const long out_row = present ? a.o.n_swaps : a.rows[3L * (a.o.swap0 + row) + 2];
   long chunk;
   if (score_chunk_lane(a.o, p, &chunk)) a.o.partial[out_row * a.o.n_chunks + chunk] = acc;
}
}  // namespace paml_amd

namespace {

struct RelabelScratch : ScoreScratch {
   using ScoreScratch::ScoreScratch;
   DevBuf<double> OM, lk;
   DevBuf<int> rows, slots, lab;
   DevBuf<unsigned char> changed;
};

}  // namespace

extern "C" int paml_amd_relabel_scores(paml_amd_engine *e, const double *branch, const double *gene_rate, const int *base_label, int n_rows, const int *rows,
                                       double *lnL0, double *lnL, double *lnf, double *lnfk0, double *lnfk)
{
   enter(e);
   relabel_info = AncCallInfo{};
   const char *who = "relabel_scores";
   if (!e || !branch || !rows || !lnL0 || !lnL) return fail(e, PAML_AMD_EINVAL, "relabel_scores: null argument");
   if (n_rows < 1) return fail(e, PAML_AMD_EINVAL, "relabel_scores: n_rows < 1");
   if ((lnfk0 != nullptr) != (lnfk != nullptr)) return fail(e, PAML_AMD_EINVAL, "relabel_scores: lnfk0 and lnfk are asked for together or not at all");
   if (int rc = score_begin(e, who, "the override P(t) of a rate-matrix (UNREST) set needs a matrix product of its own")) return rc;
   const TreeDesc &T = e->tree;
   const int nn = T.n_nodes, n = e->n, K = e->K, G = e->n_genes, NL = e->n_labels;
   const int psets = G * K;
   std::vector<int> lab(T.label.begin(), T.label.end());
   if (base_label) {
      for (int v = 0; v < nn; v++)
         if (base_label[v] < 0 || base_label[v] >= NL)
            return fail(e, PAML_AMD_EINVAL, "relabel_scores: base_label of node " + std::to_string(v) + " = " + std::to_string(base_label[v]) + " is outside the class tables' " + std::to_string(NL) + " labels");
      lab.assign(base_label, base_label + nn);
   }
   {
      const std::vector<int> father = score_fathers(T);
      for (int i = 0; i < n_rows; i++) {
         const int v = rows[2 * i], l = rows[2 * i + 1];
         const std::string at = "relabel_scores: row " + std::to_string(i) + ": ";
         if (int rc = score_check_node(e, at, v, &father, false)) return rc;
         if (l < 0 || l >= NL) return fail(e, PAML_AMD_EINVAL, at + "label " + std::to_string(l) + " is outside the class tables' " + std::to_string(NL) + " labels");
      }
   }
   // the rows sorted by node (then label, then the caller's index); one matrix slot per distinct (node, label)
   std::vector<int> order(n_rows);
   for (int i = 0; i < n_rows; i++) order[i] = i;
   std::sort(order.begin(), order.end(), [&](int x, int y) {
      if (rows[2 * x] != rows[2 * y]) return rows[2 * x] < rows[2 * y];
      if (rows[2 * x + 1] != rows[2 * y + 1]) return rows[2 * x + 1] < rows[2 * y + 1];
      return x < y;
   });
   std::vector<int> srows((size_t)3 * n_rows), slots;
   for (int i = 0; i < n_rows; i++) {
      const int v = rows[2 * order[i]], l = rows[2 * order[i] + 1];
      if (slots.empty() || slots[slots.size() - 2] != v || slots.back() != l) { slots.push_back(v); slots.push_back(l); }
      srows[3 * i] = v; srows[3 * i + 1] = (int)(slots.size() / 2) - 1; srows[3 * i + 2] = order[i];
   }
   const int n_slots = (int)(slots.size() / 2);
   std::vector<unsigned char> changed((size_t)n_slots * psets);
   for (int s = 0; s < n_slots; s++) {
      const int now = lab[slots[2 * s]], l = slots[2 * s + 1];
      for (int g = 0; g < G; g++)
         for (int k = 0; k < K; k++)
            changed[(size_t)s * psets + g * K + k] =
               e->h_eigen_of[((size_t)g * K + k) * NL + l] != e->h_eigen_of[((size_t)g * K + k) * NL + now] || e->h_qfactor[(size_t)k * NL + l] != e->h_qfactor[(size_t)k * NL + now];
   }

   const bool mfma = e->kk == KK_MFMA64;
   hipStream_t st = e->stream;
   RelabelScratch w(relabel_info);
   RelabelArgs a{};
   NniArgs &o = a.o;
   AncMargArgs &m = o.m;
   if (int rc = anc_tree_pack(e, who, w, &m.t)) return rc;
   if (base_label) {
      HIPCHK(upload(w.lab, lab.data(), lab.size(), st));
      HIPCHK(hipStreamSynchronize(st));
   }
   if (int rc = score_present_pmat(e, who, branch, gene_rate, w, base_label ? w.lab.p : nullptr)) return rc;
   const long msz = mfma ? 4096 : (long)n * n;
   HIPCHK(upload(w.rows, srows.data(), srows.size(), st));
   HIPCHK(upload(w.slots, slots.data(), slots.size(), st));
   HIPCHK(upload(w.changed, changed.data(), changed.size(), st));
   HIPCHK(w.OM.ensure((size_t)n_slots * psets * msz));
   {
      RelabelPmatArgs pa{};
      pa.g = grad_pmat_args(e);
      pa.g.label = nullptr;      // (a slot names its label)
      pa.slots = w.slots.p; pa.changed = w.changed.p; pa.OM = w.OM.p; pa.msz = msz; pa.psets = psets;
      hipLaunchKernelGGL(relabel_pmat_kernel, dim3((unsigned)n_slots, psets), dim3(256), 0, st, pa);
      HIPCHK(hipGetLastError());
   }
   if (int rc = anc_pmat_wait(e, w)) return rc;      // (the sorted lists are on this stack: waited for here)
   e->pmat_valid = !base_label;      // (d_rowmajor holds every branch's P(t) under the labels of this call: the tree's own are built again below)

   // the workspace per pattern: the partials and the messages, then (3 K + 1) doubles per row (the rows of a group and the present tree):
   // f_hk, sigma and lnfk of every class, and lnf
   ScorePlan plan;
   if (int rc = score_plan(e, w, &plan, "PAML_AMD_RELABEL_ARENA_MB", (3.0 * K + 1) * 8, n_rows, n_rows)) return rc;
   const int cap = plan.cap;
   const long n_patt = e->n_patt;
   const size_t kr = (size_t)K * (cap + 1);
   if (int rc = score_alloc(e, who, w, plan, {{&w.f, kr}, {&w.sig, kr}, {&w.lk, kr}, {&w.lnf, (size_t)cap + 1}})) return rc;
   score_fill(o, w, e, plan, n_rows);
   a.rows = w.rows.p; a.changed = w.changed.p; a.OM = w.OM.p; a.psets = psets; a.lk = lnfk ? w.lk.p : nullptr;
   auto caller_index = [&](long i) { return srows[3 * (size_t)i + 2]; };      // of row i of the sorted list
   if (int rc = anc_score_batches(
          e, w, o, plan.batch, score_n_groups(n_rows, cap),
          [&](int gi, dim3 tiles, dim3 lanes) {
             score_group(o, cap, n_rows, gi);      // (of the sorted list)
             if (mfma) hipLaunchKernelGGL(relabel_mfma_kernel, tiles, dim3(256), 0, st, a);
             else anc_lanes(e->kk, [&](auto N) { hipLaunchKernelGGL(relabel_lane_kernel<N()>, dim3(lanes.x, K, o.n_group), dim3(256), 0, st, a); });
          },
          [&](int gi, dim3 lanes) { hipLaunchKernelGGL(relabel_combine_kernel, dim3(lanes.x, o.n_group + (gi == 0 ? 1 : 0)), dim3(256), 0, st, a); },
          [&](int gi, long h0, long nb) {      // the group's rows to the caller's arrays, at the caller's index: one plain copy per row (and class)
             if (int rc = score_copy_rows(e, w.lnf.p, plan.batch, o.swap0, o.n_group, lnf, h0, nb, caller_index)) return rc;
             const size_t bytes = (size_t)nb * 8, row_stride = (size_t)plan.batch;
             for (int i = 0; lnfk && i < o.n_group; i++)
                for (int k = 0; k < K; k++)
                   HIPCHK(hipMemcpyAsync(lnfk + ((size_t)caller_index(o.swap0 + i) * K + k) * n_patt + h0, w.lk.p + ((size_t)k * (cap + 1) + i) * row_stride, bytes,
                                         hipMemcpyDeviceToHost, st));
             for (int k = 0; gi == 0 && lnfk0 && k < K; k++)
                HIPCHK(hipMemcpyAsync(lnfk0 + (size_t)k * n_patt + h0, w.lk.p + ((size_t)k * (cap + 1) + cap) * row_stride, bytes, hipMemcpyDeviceToHost, st));
             return 0;
          }))
      return rc;
   if (int rc = score_totals(e, w, plan, n_rows, nullptr, lnL0, {lnL})) return rc;
   if (base_label) {      // the tree's own matrices again: what paml_amd_get_pmat and the next call find
      if (int rc = anc_pmat_waited(e, who, branch, gene_rate, w)) return rc;
      e->pmat_valid = true;
   }
   return 0;
}

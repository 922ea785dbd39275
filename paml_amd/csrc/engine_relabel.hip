// engine_relabel.hip — the lnL of the tree with the label of one branch changed, for many (branch, label) rows in one call
// (paml_amd_relabel_scores), with the per-class, per-pattern values a host needs to re-mix the site classes; the definition in
// kernels_relabel.h, the kernels here.  The tree's own P(t) comes from the evaluation's builders (anc_pmat, engine_ancestral.hip), the
// override matrices from the edge call's formulas (edge_pmat_fill, kernels_edge.h), the down pass is the ancestral module's, the outer
// pass is the NNI call's.
// Built for gfx950 only (one of the translation units of libpaml_amd.so, see engine_state.h).
#include <algorithm>
#include <map>

#include "engine_state.h"
#include "kernels_relabel.h"
#include "kernels_edge.h"
#include "ancestral_host.h"

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
   const int tid = threadIdx.x, lane = tid & 63;
   const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
   const int q = lane >> 4, k = blockIdx.y;
   const AncMfma w{sP, lane, wave, q};
   const long g16 = (long)blockIdx.x * 4 + wave, p = g16 * 16 + (lane & 15);
   const long pc = p < m.nb ? p : m.nb - 1;      // (lanes past the batch's end read the last pattern and write into the padding: p < stride)
   const long pset = (long)m.gene * m.K + k;
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
         const int f = t.father[v];
         nni_mfma_father(m, k, g16, pc, lane, q, f, h, &ls);
         for (int j = t.sons_ptr[f]; j < t.sons_ptr[f + 1]; j++)
            if (t.sons[j] != v) anc_mfma_mul_son(m, w, k, g16, pc, t.sons[j], h, &ls);
         if (v < t.n_tips) {      // a tip: its code's indicator through the product
            const unsigned long long mask = m.code_mask[m.z[(long)v * m.z_stride + m.h0 + pc]];
#pragma unroll
            for (int j = 0; j < 16; j++) l[j] = (mask >> (4 * j + q)) & 1ull ? 1.0 : 0.0;
         }
         else {
            part_load(m.L + (((long)k * t.n_int + v - t.n_tips) * (m.stride >> 4) + g16) * 1024, lane, l);
            ls += m.SL[((long)k * t.n_int + v - t.n_tips) * m.stride + pc];
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
   double acc = p < a.o.m.nb ? relabel_combine(a, row, p) : 0.0;
#pragma unroll
   for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off);
   const long chunk = a.o.chunk0 + (p >> 6);
   const long out_row = present ? a.o.n_swaps : a.rows[3L * (a.o.swap0 + row) + 2];
   if ((threadIdx.x & 63) == 0 && (p & ~63L) < a.o.m.nb) a.o.partial[out_row * a.o.n_chunks + chunk] = acc;
}
}  // namespace paml_amd

namespace {

struct RelabelScratch : AncScratch {
   using AncScratch::AncScratch;
   DevBuf<double> PT, OM, f, sig, lk, lnf, partial, out;
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
   if (int rc = anc_common_checks(e, who)) return rc;
   if (e->world > 1) return fail(e, PAML_AMD_EUNSUPPORTED, "relabel_scores: one rank only (this engine's communicator has " + std::to_string(e->world) + ")");
   for (size_t i = 0; i < e->eigen.size(); i++)
      if (e->eigen[i].kind == PAML_AMD_EIGEN_QMAT)
         return fail(e, PAML_AMD_EUNSUPPORTED, "relabel_scores: the override P(t) of a rate-matrix (UNREST) set needs a matrix product of its own");
   const TreeDesc &T = e->tree;
   const int nn = T.n_nodes, n = e->n, K = e->K, G = e->n_genes, n_tips = e->n_tips, n_int = nn - n_tips, NL = e->n_labels;
   const int psets = G * K;
   std::vector<int> lab(T.label.begin(), T.label.end());
   if (base_label) {
      for (int v = 0; v < nn; v++)
         if (base_label[v] < 0 || base_label[v] >= NL)
            return fail(e, PAML_AMD_EINVAL, "relabel_scores: base_label of node " + std::to_string(v) + " = " + std::to_string(base_label[v]) + " is outside the class tables' " + std::to_string(NL) + " labels");
      lab.assign(base_label, base_label + nn);
   }
   {
      std::vector<int> father(nn, -1);
      for (int v = 0; v < nn; v++)
         for (int j = T.sons_ptr[v]; j < T.sons_ptr[v + 1]; j++) father[T.sons[j]] = v;
      for (int i = 0; i < n_rows; i++) {
         const int v = rows[2 * i], l = rows[2 * i + 1];
         const std::string at = "relabel_scores: row " + std::to_string(i) + ": ";
         if (v < 0 || v >= nn) return fail(e, PAML_AMD_EINVAL, at + "node " + std::to_string(v) + " is out of range");
         if (v == T.root || father[v] < 0) return fail(e, PAML_AMD_EINVAL, at + "node " + std::to_string(v) + " is the root");
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
   if (int rc = anc_pmat(e, who, branch, gene_rate, w, base_label ? w.lab.p : nullptr)) return rc;
   if (mfma) {
      HIPCHK(w.PT.ensure((size_t)psets * nn * 4096));
      hipLaunchKernelGGL(nni_pt_kernel, dim3(nn, psets), dim3(256), 0, st, (const double *)e->d_rowmajor.p, w.PT.p, n, nn, n_tips, T.root);
      HIPCHK(hipGetLastError());
   }
   const long msz = mfma ? 4096 : (long)n * n;
   HIPCHK(upload(w.rows, srows.data(), srows.size(), st));
   HIPCHK(upload(w.slots, slots.data(), slots.size(), st));
   HIPCHK(upload(w.changed, changed.data(), changed.size(), st));
   HIPCHK(w.OM.ensure((size_t)n_slots * psets * msz));
   {
      RelabelPmatArgs pa{};
      GradPmatArgs &ga = pa.g;
      ga.n = n; ga.K = K; ga.n_nodes = nn; ga.n_tips = n_tips; ga.root = T.root; ga.n_labels = NL; ga.rate_gs = e->rate_per_gene ? K : 0; ga.mfma = mfma ? 1 : 0;
      ga.eigen_of = e->d_eigen_of.p; ga.eigen = e->d_eigen.p; ga.branch = e->d_branch.p;
      ga.rate = e->d_rate.p; ga.gene_rate = e->d_gene_rate.p; ga.qfactor = e->d_qfactor.p;
      pa.slots = w.slots.p; pa.changed = w.changed.p; pa.OM = w.OM.p; pa.msz = msz; pa.psets = psets;
      hipLaunchKernelGGL(relabel_pmat_kernel, dim3((unsigned)n_slots, psets), dim3(256), 0, st, pa);
      HIPCHK(hipGetLastError());
   }
   if (int rc = anc_pmat_wait(e, w)) return rc;      // (the sorted lists are on this stack: waited for here)
   e->pmat_valid = !base_label;      // (d_rowmajor holds every branch's P(t) under the labels of this call: the tree's own are built again below)

   const std::vector<long> chunk_base = anc_chunk_base(e);
   const long n_chunks = chunk_base[G];
   HIPCHK(w.partial.ensure((size_t)(n_rows + 1) * std::max<long>(n_chunks, 1)));
   HIPCHK(w.out.ensure((size_t)n_rows + 1));

   // the workspace per pattern: the partials and the messages, then (3 K + 1) doubles per row (the rows of a group and the present tree):
   // f_hk, sigma and lnfk of every class, and lnf
   const int ns = mfma ? 64 : n;      // doubles a partial takes per pattern
   const double fixed = 2.0 * K * n_int * (ns + 1) * 8, per_row = (3.0 * K + 1) * 8;
   const double arena_mb = anc_arena_mb("PAML_AMD_RELABEL_ARENA_MB");
   int cap = n_rows;
   if ((fixed + per_row * (n_rows + 1)) * ANC_TILE > arena_mb * 1048576.0)      // one tile with all rows does not fit: groups of rows
      cap = (int)std::min<double>(n_rows, std::max(1.0, floor((arena_mb * 1048576.0 / ANC_TILE - fixed) / per_row) - 1));
   cap = std::min(cap, 65535);      // (the lanes' row pass has a grid layer per row)
   long batch = anc_batch(fixed + per_row * (cap + 1), e->n_patt, "PAML_AMD_RELABEL_ARENA_MB");
   {
      const size_t part = (size_t)K * n_int * ns, sc = (size_t)K * n_int, kr = (size_t)K * (cap + 1);
      if (int rc = anc_alloc(e, who, {{&w.L, part}, {&w.G, part}, {&w.SL, sc}, {&w.SG, sc}, {&w.f, kr}, {&w.sig, kr}, {&w.lk, kr}, {&w.lnf, (size_t)cap + 1}}, &batch)) return rc;
   }
   anc_fill(e, w, batch, m);
   o.PT = w.PT.p; o.cap = cap; o.n_swaps = n_rows; o.f = w.f.p; o.sig = w.sig.p; o.weights = e->d_weights.p;
   o.lnf = w.lnf.p; o.partial = w.partial.p; o.n_chunks = n_chunks;
   o.ref_node = T.sons[T.sons_ptr[T.root]];
   a.rows = w.rows.p; a.changed = w.changed.p; a.OM = w.OM.p; a.psets = psets; a.lk = lnfk ? w.lk.p : nullptr;
   const long n_patt = e->n_patt;
   auto group = [&](int gi) { o.swap0 = gi * cap; o.n_group = std::min(cap, n_rows - o.swap0); };      // groups of `cap` rows of the sorted list
   if (int rc = anc_score_batches(
          e, w, o, batch, (n_rows + cap - 1) / cap,
          [&](dim3 lanes, int pass) { anc_lanes(e->kk, [&](auto N) { hipLaunchKernelGGL(nni_lane_kernel<N()>, lanes, dim3(256), 0, st, o, pass); }); },
          [](dim3) {},      // (the present tree's row is combined with the batch's first group)
          [&](int gi, dim3 tiles, dim3 lanes) {
             group(gi);
             if (mfma) hipLaunchKernelGGL(relabel_mfma_kernel, tiles, dim3(256), 0, st, a);
             else anc_lanes(e->kk, [&](auto N) { hipLaunchKernelGGL(relabel_lane_kernel<N()>, dim3(lanes.x, K, o.n_group), dim3(256), 0, st, a); });
          },
          [&](int gi, dim3 lanes) { hipLaunchKernelGGL(relabel_combine_kernel, dim3(lanes.x, o.n_group + (gi == 0 ? 1 : 0)), dim3(256), 0, st, a); },
          [&](int gi, long h0, long nb) {      // the group's rows to the caller's arrays, at the caller's index: one plain copy per row (and class)
             const size_t bytes = (size_t)nb * 8, row_stride = (size_t)batch;
             for (int i = 0; i < o.n_group; i++) {
                const size_t ci = (size_t)srows[3 * (size_t)(o.swap0 + i) + 2];
                if (lnf) HIPCHK(hipMemcpyAsync(lnf + ci * n_patt + h0, w.lnf.p + (size_t)i * row_stride, bytes, hipMemcpyDeviceToHost, st));
                for (int k = 0; lnfk && k < K; k++)
                   HIPCHK(hipMemcpyAsync(lnfk + (ci * K + k) * n_patt + h0, w.lk.p + ((size_t)k * (cap + 1) + i) * row_stride, bytes, hipMemcpyDeviceToHost, st));
             }
             for (int k = 0; gi == 0 && lnfk0 && k < K; k++)
                HIPCHK(hipMemcpyAsync(lnfk0 + (size_t)k * n_patt + h0, w.lk.p + ((size_t)k * (cap + 1) + cap) * row_stride, bytes, hipMemcpyDeviceToHost, st));
             return 0;
          }))
      return rc;
   std::vector<double> out((size_t)n_rows + 1);
   if (int rc = anc_totals(e, w, w.partial.p, n_chunks, w.out.p, out)) return rc;
   for (int i = 0; i < n_rows; i++) lnL[i] = out[i];
   *lnL0 = out[n_rows];
   if (base_label) {      // the tree's own matrices again: what paml_amd_get_pmat and the next call find
      if (int rc = anc_pmat_waited(e, who, branch, gene_rate, w)) return rc;
      e->pmat_valid = true;
   }
   return 0;
}

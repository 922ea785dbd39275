// engine_edge.hip — the lnL of configurations of internal edges at trial lengths of the five branches around them, with the first and
// second derivative along one of them, in one call (paml_amd_edge_scores), and the list of edges that have the three configurations
// (paml_amd_edge_list, host only); the definition in kernels_edge.h, the kernels here.  The tree's own P(t) comes from the evaluation's
// builders (anc_pmat, engine_ancestral.hip), the down pass is the ancestral module's, the outer pass is the NNI call's.
// The host side that is not this call's own is the score calls' skeleton (score_host.h, defined in engine_ancestral.hip).
// Built for gfx950 only (one of the translation units of libpaml_amd.so, see engine_state.h).
#include "engine_state.h"
#include "kernels_edge.h"
#include "score_host.h"

static thread_local AncCallInfo edge_info;

extern "C" void paml_amd_edge_info(int *last_batches, double *last_kernel_ms) { edge_info.read(last_batches, last_kernel_ms); }

namespace paml_amd {

// P(t) of every (row, override slot, parameter set), and dP, d^2P for the slot of u: grid (rows x 5, gene x class).  The formulas are
// pmat_deriv_kernel's, term for term (edge_pmat_fill, kernels_edge.h).  Matrix cores: the A-operand order, transposed for f.
__global__ __launch_bounds__(256) void edge_pmat_kernel(EdgePmatArgs a)
{
   const GradPmatArgs &g = a.g;
   const int row = blockIdx.x / EDGE_SLOTS, slot = blockIdx.x % EDGE_SLOTS, pset = blockIdx.y;
   const int node = a.ovr_node[(long)row * EDGE_SLOTS + slot];
   if (node < 0) return;
   const bool with_d = node == a.rows[4L * row + 3], transposed = g.mfma && node == a.father[a.rows[4L * row]];
   __shared__ double sE[64], sM[64];
   double *P = a.OM + (((long)row * a.psets + pset) * EDGE_MATS + slot) * a.msz;
   double *dP = a.OM + (((long)row * a.psets + pset) * EDGE_MATS + EDGE_SLOTS) * a.msz, *ddP = dP + a.msz;
   edge_pmat_fill<true>(g, pset, g.label[node], a.ovr_t[(long)row * EDGE_SLOTS + slot], with_d, transposed, sE, sM, P, dP, ddP);
}

// one pattern per lane, the row pass: grid (patterns / 256, K, rows of the group)
template <int N> __global__ __launch_bounds__(256) void edge_lane_row_kernel(EdgeArgs a)
{
   const long p = (long)blockIdx.x * 256 + threadIdx.x;
   if (p >= a.o.m.nb) return;
   edge_lane_row<N>(a, blockIdx.y, p, blockIdx.z);
}

// x *= (M L_c) of node c: `blk` the branch's matrix in the A-operand order, or null: the tree's own (a tip: its column table)
__device__ __forceinline__ void edge_mfma_msg(const AncMargArgs &m, const AncMfma &w, int k, long g16, long pc, int c, const double *blk, double (&x)[16])
{
   const AncTree &t = m.t;
   const long pset = (long)m.gene * m.K + k;
   if (c < t.n_tips && !blk) {
      double2 tv[8];
      tip_gather(m.ptip + pset * t.n_nodes * m.tip_words, m.tip_words, c, (int)m.z[(long)c * m.z_stride + m.h0 + pc], w.q, tv);
#pragma unroll
      for (int i = 0; i < 8; i++) { x[2 * i] *= tv[i].x; x[2 * i + 1] *= tv[i].y; }
      return;
   }
   double xs[16];
   if (c < t.n_tips) {      // an overridden tip: its code's indicator through the product
      const unsigned long long mask = m.code_mask[m.z[(long)c * m.z_stride + m.h0 + pc]];
#pragma unroll
      for (int j = 0; j < 16; j++) xs[j] = (mask >> (4 * j + w.q)) & 1ull ? 1.0 : 0.0;
   }
   else part_load(m.L + (((long)k * t.n_int + c - t.n_tips) * (m.stride >> 4) + g16) * 1024, w.lane, xs);
   v4d acc[4];
   w.product(blk ? blk : m.pint + (pset * t.n_nodes + c) * 4096, xs, acc);
#pragma unroll
   for (int j = 0; j < 16; j++) x[j] *= acc[j >> 2][j & 3];
}

// Matrix cores, the row pass: four waves own ANC_TILE patterns of one class and loop over the group's rows; the three derivative orders
// are walked one after the other with the side that does not carry u held.  Grid (stride / ANC_TILE, K).
__global__ __launch_bounds__(256) void edge_mfma_kernel(EdgeArgs a)
{
   __shared__ __attribute__((aligned(16))) double sP[4096];
   const AncMargArgs &m = a.o.m;
   const AncTree &t = m.t;
   const ScoreTile c = score_tile(m);
   const int lane = c.lane, q = c.q, k = c.k, n = m.n;
   const long g16 = c.g16, p = c.p, pc = c.pc, pset = c.pset;
   const AncMfma w{sP, lane, c.wave, q};
   for (int i = 0; i < a.o.n_group; i++) {
      const int gi = a.o.swap0 + i;
      const int *rw = a.rows + 4L * gi, *on = a.ovr_node + (long)EDGE_SLOTS * gi;
      const int v = rw[0], s = rw[1], x = rw[2], u = rw[3], f = t.father[v];
      const double *om = a.OM + ((long)gi * a.psets + pset) * EDGE_MATS * 4096;
      auto blk = [&](int c, int d) -> const double * {      // d > 0: c = u; null: the tree's own
         if (d) return om + (long)(EDGE_SLOTS - 1 + d) * 4096;
         const int j = edge_slot_of(on, c);
         return j >= 0 ? om + (long)j * 4096 : nullptr;
      };
      const double *pv0 = blk(v, 0) ? blk(v, 0) : m.pint + (pset * t.n_nodes + v) * 4096;
      const int nd = u >= 0 ? 3 : 1;
      const bool f_ovr = edge_slot_of(on, f) >= 0;
      int side = u < 0 ? 0 : u == v ? 1 : u == f ? 4 : 2;      // (2: a son; 3 below if it hangs on f)
      double h[16], l[16], hff[16], ls = 0;
      v4d acc[4];
      if (!f_ovr) nni_mfma_father(m, k, g16, pc, lane, q, f, h, &ls);
      else {
         const int ff = t.father[f];
         nni_mfma_father(m, k, g16, pc, lane, q, ff, hff, &ls);
         for (int j = t.sons_ptr[ff]; j < t.sons_ptr[ff + 1]; j++)
            if (t.sons[j] != f) anc_mfma_mul_son(m, w, k, g16, pc, t.sons[j], hff, &ls);
         if (u == f) {
#pragma unroll
            for (int j = 0; j < 16; j++) h[j] = 4 * j + q < n ? 1.0 : 0.0;
         }
         else {
            w.product(blk(f, 0), hff, acc);      // (the slot of f holds P_f^T)
#pragma unroll
            for (int j = 0; j < 16; j++) h[j] = acc[j >> 2][j & 3];
         }
      }
      for (int j = t.sons_ptr[f]; j < t.sons_ptr[f + 1]; j++) {
         int c = t.sons[j];
         if (c == v) continue;
         if (c == x) c = s;
         if (c >= t.n_tips) ls += m.SL[((long)k * t.n_int + c - t.n_tips) * m.stride + pc];
         if (c == u) { side = 3; continue; }
         edge_mfma_msg(m, w, k, g16, pc, c, blk(c, 0), h);
      }
#pragma unroll
      for (int j = 0; j < 16; j++) l[j] = 4 * j + q < n ? 1.0 : 0.0;
      for (int j = t.sons_ptr[v]; j < t.sons_ptr[v + 1]; j++) {
         int c = t.sons[j];
         if (c == s) c = x;
         if (c >= t.n_tips) ls += m.SL[((long)k * t.n_int + c - t.n_tips) * m.stride + pc];
         if (c == u) continue;
         edge_mfma_msg(m, w, k, g16, pc, c, blk(c, 0), l);
      }
      if (side >= 3) {      // u on the father's side: Z = P_v X once, in l
         w.product(pv0, l, acc);
#pragma unroll
         for (int j = 0; j < 16; j++) l[j] = acc[j >> 2][j & 3];
      }
      double fd[3] = {0, 0, 0};
      for (int d = 0; d < nd; d++) {
         double y[16];
         if (side <= 2) {
#pragma unroll
            for (int j = 0; j < 16; j++) y[j] = l[j];
            if (side == 2) edge_mfma_msg(m, w, k, g16, pc, u, blk(u, d), y);
            w.product(side == 1 ? blk(v, d) : pv0, y, acc);
#pragma unroll
            for (int j = 0; j < 16; j++) y[j] = acc[j >> 2][j & 3];
            fd[d] = grad_mfma_dot(h, y);
         }
         else {
#pragma unroll
            for (int j = 0; j < 16; j++) y[j] = h[j];
            if (side == 3) edge_mfma_msg(m, w, k, g16, pc, u, blk(u, d), y);
            else {
               w.product(blk(f, d), hff, acc);
#pragma unroll
               for (int j = 0; j < 16; j++) y[j] *= acc[j >> 2][j & 3];
            }
            fd[d] = grad_mfma_dot(y, l);
         }
      }
      const long oi = nni_out_idx(a.o, k, i, p);
      if (q == 0) { a.o.f[oi] = fd[0]; a.f1[oi] = fd[1]; a.f2[oi] = fd[2]; a.o.sig[oi] = ls; }
   }
}

// the rows' chunks go to their place in the list (edge_combine_rows, kernels_edge.h)
__global__ __launch_bounds__(256) void edge_combine_kernel(EdgeArgs a)
{
   edge_combine_rows(a, [&](int row) { return a.o.swap0 + row; });
}
}  // namespace paml_amd

// Every internal v that is not the root, has exactly two sons (s1, s2) and whose father f is either a non-root node with two sons (v and
// c) or a root with exactly three sons (v, c1, c2), in node order: the present configuration (v, -1, -1) and the two swaps
// paml_amd_nni_list gives for that v — (s1, c), (s2, c), or (s1, c1), (s1, c2) under the root — and the five branches around the edge:
// s1, s2, v, then c and f, or c1 and c2.
extern "C" int paml_amd_edge_list(int n_tips, int n_nodes, int root, const int *sons_ptr, const int *sons, int *edges, int *five, int cap)
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
      const int f = father[v];
      if (v == root || f < 0 || sons_ptr[v + 1] - sons_ptr[v] != 2) continue;
      const int nf = sons_ptr[f + 1] - sons_ptr[f];
      if (!(f != root && nf == 2) && !(f == root && nf == 3)) continue;
      int c[2], nc = 0;
      for (int j = sons_ptr[f]; j < sons_ptr[f + 1]; j++)
         if (sons[j] != v) c[nc++] = sons[j];
      const int s1 = sons[sons_ptr[v]], s2 = sons[sons_ptr[v] + 1];
      if (edges || five) {
         if (count >= cap) return PAML_AMD_EINVAL;
         if (edges) {
            const int cfg[9] = {v, -1, -1, v, s1, c[0], v, nf == 2 ? s2 : s1, nf == 2 ? c[0] : c[1]};
            for (int i = 0; i < 9; i++) edges[9 * count + i] = cfg[i];
         }
         if (five) {
            const int fv[5] = {s1, s2, v, c[0], nf == 2 ? f : c[1]};
            for (int i = 0; i < 5; i++) five[5 * count + i] = fv[i];
         }
      }
      count++;
   }
   return count;
}

namespace {

struct EdgeScratch : ScoreScratch {
   using ScoreScratch::ScoreScratch;
   DevBuf<double> OM, ovr_t, f1, f2, g1, g2;
   DevBuf<int> rows, ovr_node;
};

}  // namespace

extern "C" int paml_amd_edge_scores(paml_amd_engine *e, const double *branch, const double *gene_rate, int n_rows, const int *rows, const int *ovr_node,
                                    const double *ovr_t, double *lnL0, double *lnL, double *d1, double *d2, double *lnf)
{
   enter(e);
   edge_info = AncCallInfo{};
   const char *who = "edge_scores";
   if (!e || !branch || !rows || !ovr_node || !ovr_t || !lnL0 || !lnL || !d1 || !d2) return fail(e, PAML_AMD_EINVAL, "edge_scores: null argument");
   if (n_rows < 1) return fail(e, PAML_AMD_EINVAL, "edge_scores: n_rows < 1");
   if (int rc = score_begin(e, who, "the derivative of a rate-matrix (UNREST) set's P(t) needs a matrix product of its own")) return rc;
   const TreeDesc &T = e->tree;
   const int nn = T.n_nodes, n = e->n, K = e->K, G = e->n_genes;
   {
      const std::vector<int> father = score_fathers(T);
      for (int i = 0; i < n_rows; i++) {
         const int v = rows[4 * i], s = rows[4 * i + 1], x = rows[4 * i + 2], u = rows[4 * i + 3];
         const std::string at = "edge_scores: row " + std::to_string(i) + ": ";
         if (int rc = score_check_node(e, at, v, &father, true)) return rc;
         const int f = father[v];
         if (s != -1 || x != -1) {
            if (!score_son_of(T, s, v)) return fail(e, PAML_AMD_EINVAL, at + std::to_string(s) + " is not a son of " + std::to_string(v));
            if (x == v || !score_son_of(T, x, f))
               return fail(e, PAML_AMD_EINVAL, at + std::to_string(x) + " is not a son of the father of " + std::to_string(v) + " other than it");
         }
         bool u_listed = u == -1;
         for (int j = 0; j < EDGE_SLOTS; j++) {
            const int c = ovr_node[EDGE_SLOTS * i + j];
            if (c == -1) continue;
            if (c == f && f == T.root) return fail(e, PAML_AMD_EINVAL, at + "override node " + std::to_string(c) + " is the root: no branch above it");
            if (c < 0 || c >= nn || !(c == v || c == f || score_son_of(T, c, v) || score_son_of(T, c, f)))
               return fail(e, PAML_AMD_EINVAL, at + "override node " + std::to_string(c) + " is not a branch around the edge");
            for (int j2 = 0; j2 < j; j2++)
               if (ovr_node[EDGE_SLOTS * i + j2] == c) return fail(e, PAML_AMD_EINVAL, at + "override node " + std::to_string(c) + " is listed twice");
            u_listed = u_listed || c == u;
         }
         if (!u_listed) return fail(e, PAML_AMD_EINVAL, at + "u = " + std::to_string(u) + " is not among the override nodes");
      }
   }
   const bool mfma = e->kk == KK_MFMA64;
   hipStream_t st = e->stream;
   EdgeScratch w(edge_info);
   EdgeArgs a{};
   NniArgs &o = a.o;
   if (int rc = anc_tree_pack(e, who, w, &o.m.t)) return rc;
   if (int rc = score_present_pmat(e, who, branch, gene_rate, w)) return rc;
   const long msz = mfma ? 4096 : (long)n * n;
   HIPCHK(upload(w.rows, rows, (size_t)4 * n_rows, st));
   HIPCHK(upload(w.ovr_node, ovr_node, (size_t)EDGE_SLOTS * n_rows, st));
   HIPCHK(upload(w.ovr_t, ovr_t, (size_t)EDGE_SLOTS * n_rows, st));
   HIPCHK(w.OM.ensure((size_t)n_rows * G * K * EDGE_MATS * msz));
   {
      EdgePmatArgs pa{};
      pa.g = grad_pmat_args(e);
      pa.father = o.m.t.father; pa.rows = w.rows.p; pa.ovr_node = w.ovr_node.p; pa.ovr_t = w.ovr_t.p; pa.OM = w.OM.p; pa.msz = msz; pa.psets = G * K;
      hipLaunchKernelGGL(edge_pmat_kernel, dim3((unsigned)n_rows * EDGE_SLOTS, G * K), dim3(256), 0, st, pa);
      HIPCHK(hipGetLastError());
   }
   if (int rc = anc_pmat_wait(e, w)) return rc;
   e->pmat_valid = true;      // (d_rowmajor holds every branch's P(t) of the tree at `branch`, in the tree's own orientation, as after nni_scores)

   // the workspace per pattern: the partials and the messages, then (4 K + 3) doubles per row (the rows of a group and the present tree)
   ScorePlan plan;
   if (int rc = score_plan(e, w, &plan, "PAML_AMD_EDGE_ARENA_MB", (4.0 * K + 3) * 8, n_rows, 3L * n_rows)) return rc;
   const int cap = plan.cap;
   const size_t kr = (size_t)K * (cap + 1), r1 = (size_t)cap + 1;
   if (int rc = score_alloc(e, who, w, plan, {{&w.f, kr}, {&w.f1, kr}, {&w.f2, kr}, {&w.sig, kr}, {&w.lnf, r1}, {&w.g1, r1}, {&w.g2, r1}})) return rc;
   score_fill(o, w, e, plan, n_rows);
   a.rows = w.rows.p; a.ovr_node = w.ovr_node.p; a.OM = w.OM.p; a.psets = G * K;
   a.f1 = w.f1.p; a.f2 = w.f2.p; a.g1 = w.g1.p; a.g2 = w.g2.p;
   if (int rc = anc_score_batches(
          e, w, o, plan.batch, score_n_groups(n_rows, cap),
          [&](int gi, dim3 tiles, dim3 lanes) {
             score_group(o, cap, n_rows, gi);
             if (mfma) hipLaunchKernelGGL(edge_mfma_kernel, tiles, dim3(256), 0, st, a);
             else anc_lanes(e->kk, [&](auto N) { hipLaunchKernelGGL(edge_lane_row_kernel<N()>, dim3(lanes.x, K, o.n_group), dim3(256), 0, st, a); });
          },
          [&](int gi, dim3 lanes) { hipLaunchKernelGGL(edge_combine_kernel, dim3(lanes.x, o.n_group + (gi == 0 ? 1 : 0)), dim3(256), 0, st, a); },
          [&](int, long h0, long nb) {      // the group's rows to the caller's [n_rows][n_patt]
             return score_copy_rows(e, w.lnf.p, plan.batch, o.swap0, o.n_group, lnf, h0, nb, [](long i) { return i; });
          }))
      return rc;
   return score_totals(e, w, plan, n_rows, nullptr, lnL0, {lnL, d1, d2});
}

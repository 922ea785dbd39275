// engine_nni.hip — the lnL of every nearest-neighbour-interchange neighbour of the tree at the present branch lengths in one call
// (paml_amd_nni_scores) and the canonical list of swaps (paml_amd_nni_list, host only); the definition in kernels_nni.h, the kernels here.
// P(t) comes from the evaluation's own builders (anc_pmat, engine_ancestral.hip), the down pass is the ancestral module's, the outer
// pass is the gradient's without the derivative.
// The host side that is not this call's own is the score calls' skeleton (score_host.h, defined in engine_ancestral.hip).
// Built for gfx950 only (one of the translation units of libpaml_amd.so, see engine_state.h).
#include "engine_state.h"
#include "kernels_nni.h"
#include "score_host.h"

static thread_local AncCallInfo nni_info;

extern "C" void paml_amd_nni_info(int *last_batches, double *last_kernel_ms) { nni_info.read(last_batches, last_kernel_ms); }

namespace paml_amd {

// P_v^T of every (parameter set, internal node) in the A-operand order (the index formula of grad_pmat_kernel): grid (n_nodes, gene x class)
__global__ __launch_bounds__(256) void nni_pt_kernel(const double *P, double *PT, int n, int n_nodes, int n_tips, int root)
{
   const int node = blockIdx.x;
   if (node == root || node < n_tips) return;
   const long slot = (long)blockIdx.y * n_nodes + node;
   const double *Pv = P + slot * n * n;
   double *tf = PT + slot * 4096;
   for (int idx = threadIdx.x; idx < 4096; idx += 256) {
      const int e = idx & 1, lane = (idx >> 1) & 63, jb = (idx >> 7) & 3, kb2 = idx >> 9;
      const int r = jb * 16 + (lane & 15), c = 4 * (2 * kb2 + e) + (lane >> 4);
      tf[idx] = r < n && c < n ? Pv[c * n + r] : 0.0;
   }
}

// P_v^T of every (parameter set, node other than the root) in the A-operand order (the index formula of nni_pt_kernel, which leaves
// the tips out): grid (n_nodes, gene x class)
__global__ __launch_bounds__(256) void nni_pt_all_kernel(const double *P, double *PT, int n, int n_nodes, int root)
{
   const int node = blockIdx.x;
   if (node == root) return;
   const long slot = (long)blockIdx.y * n_nodes + node;
   const double *Pv = P + slot * n * n;
   double *tf = PT + slot * 4096;
   for (int idx = threadIdx.x; idx < 4096; idx += 256) {
      const int e = idx & 1, lane = (idx >> 1) & 63, jb = (idx >> 7) & 3, kb2 = idx >> 9;
      const int r = jb * 16 + (lane & 15), c = 4 * (2 * kb2 + e) + (lane >> 4);
      tf[idx] = r < n && c < n ? Pv[c * n + r] : 0.0;
   }
}

// one pattern per lane, the swap pass: grid (patterns / 256, K, swaps of the group)
template <int N> __global__ __launch_bounds__(256) void nni_lane_swap_kernel(NniArgs a)
{
   const long p = (long)blockIdx.x * 256 + threadIdx.x;
   if (p >= a.m.nb) return;
   nni_lane_swap<N>(a, blockIdx.y, p, blockIdx.z);
}

// Matrix cores, the outer pass without the derivative (grad_mfma_kernel's walk over the internal nodes, then ref_node when it is a tip):
// lane = q * 16 + pattern, register m = state 4 m + q.  Grid (stride / ANC_TILE, K).
__global__ __launch_bounds__(256) void nni_mfma_outer_kernel(NniArgs a)
{
   __shared__ __attribute__((aligned(16))) double sP[4096];
   const AncMargArgs &m = a.m;
   const AncTree &t = m.t;
   const int tid = threadIdx.x, lane = tid & 63, n = m.n;
   const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
   const int q = lane >> 4, k = blockIdx.y;
   const AncMfma w{sP, lane, wave, q};
   const long g16 = (long)blockIdx.x * 4 + wave, p = g16 * 16 + (lane & 15);
   const long pc = p < m.nb ? p : m.nb - 1;      // (lanes past the batch's end read the last pattern and write into the padding: p < stride)
   const long pset = (long)m.gene * m.K + k;
   if (t.root >= t.n_tips) {
      const double *pi = m.pi + (long)(m.n_pi > 1 ? m.gene : 0) * n;
      const int ri = t.root - t.n_tips;
      double x[16];
#pragma unroll
      for (int i = 0; i < 16; i++) x[i] = 4 * i + q < n ? pi[4 * i + q] : 0.0;
      part_store(m.G + (((long)k * t.n_int + ri) * (m.stride >> 4) + g16) * 1024, lane, x);
      if (q == 0) m.SG[((long)k * t.n_int + ri) * m.stride + p] = 0;
   }
   const int n_walk = t.n_pre + (a.ref_node < t.n_tips ? 1 : 0);
   for (int i = 0; i < n_walk; i++) {
      const int v = i < t.n_pre ? t.pre[i] : a.ref_node;
      const int f = t.father[v];
      double h[16], ls;
      __syncthreads();      // (SG of the father was stored by the pattern's q = 0 lane: a workgroup-scope fence before the other lanes read it)
      nni_mfma_father(m, k, g16, pc, lane, q, f, h, &ls);
      for (int j = t.sons_ptr[f]; j < t.sons_ptr[f + 1]; j++)
         if (t.sons[j] != v) anc_mfma_mul_son(m, w, k, g16, pc, t.sons[j], h, &ls);
      const long oi = nni_out_idx(a, k, a.cap, p);
      double x[16], y[16];
      if (v < t.n_tips) {      // ref_node, a tip: P_v L_v from the tip's column table
         double2 tv[8];
         tip_gather(m.ptip + pset * t.n_nodes * m.tip_words, m.tip_words, v, (int)m.z[(long)v * m.z_stride + m.h0 + pc], q, tv);
#pragma unroll
         for (int j = 0; j < 8; j++) { y[2 * j] = tv[j].x; y[2 * j + 1] = tv[j].y; }
         const double den = grad_mfma_dot(h, y);
         if (q == 0) { a.f[oi] = den; a.sig[oi] = ls; }
         continue;
      }
      const int vi = v - t.n_tips;
      v4d acc[4];
      w.product(a.PT + (pset * t.n_nodes + v) * 4096, h, acc);      // A_v = P_v^T H_v
#pragma unroll
      for (int j = 0; j < 16; j++) y[j] = acc[j >> 2][j & 3];
      if (v == a.ref_node) {      // (uniform over the workgroup) sum_x A_v(x) L_v(x) before A_v is rescaled, as grad_mfma_kernel
         part_load(m.L + (((long)k * t.n_int + vi) * (m.stride >> 4) + g16) * 1024, lane, x);
         const double den = grad_mfma_dot(y, x);
         if (q == 0) { a.f[oi] = den; a.sig[oi] = ls + m.SL[((long)k * t.n_int + vi) * m.stride + pc]; }
      }
      if (m.scaled) {
         const double mx = anc_mfma_max(y);
         if (mx > 0) {
#pragma unroll
            for (int j = 0; j < 16; j++) y[j] /= mx;
            ls += log(mx);
         }
      }
      part_store(m.G + (((long)k * t.n_int + vi) * (m.stride >> 4) + g16) * 1024, lane, y);
      if (q == 0) m.SG[((long)k * t.n_int + vi) * m.stride + p] = ls;
   }
}

// Matrix cores, the swap pass: four waves own ANC_TILE patterns of one class and loop over the group's swaps.  Grid (stride / ANC_TILE, K).
__global__ __launch_bounds__(256) void nni_mfma_kernel(NniArgs a)
{
   __shared__ __attribute__((aligned(16))) double sP[4096];
   const AncMargArgs &m = a.m;
   const AncTree &t = m.t;
   const ScoreTile c = score_tile(m);
   const int lane = c.lane, q = c.q, k = c.k, n = m.n;
   const long g16 = c.g16, p = c.p, pc = c.pc, pset = c.pset;
   const AncMfma w{sP, lane, c.wave, q};
   for (int i = 0; i < a.n_group; i++) {
      const int *sw = a.swaps + 3L * (a.swap0 + i);
      const int v = sw[0], s = sw[1], x = sw[2], f = t.father[v];
      double h[16], l[16], ls;
      nni_mfma_father(m, k, g16, pc, lane, q, f, h, &ls);
      anc_mfma_mul_son(m, w, k, g16, pc, s, h, &ls);
      for (int j = t.sons_ptr[f]; j < t.sons_ptr[f + 1]; j++)
         if (t.sons[j] != v && t.sons[j] != x) anc_mfma_mul_son(m, w, k, g16, pc, t.sons[j], h, &ls);
#pragma unroll
      for (int j = 0; j < 16; j++) l[j] = 4 * j + q < n ? 1.0 : 0.0;
      anc_mfma_mul_son(m, w, k, g16, pc, x, l, &ls);
      for (int j = t.sons_ptr[v]; j < t.sons_ptr[v + 1]; j++)
         if (t.sons[j] != s) anc_mfma_mul_son(m, w, k, g16, pc, t.sons[j], l, &ls);
      v4d acc[4];
      w.product(m.pint + (pset * t.n_nodes + v) * 4096, l, acc);
      double y[16];
#pragma unroll
      for (int j = 0; j < 16; j++) y[j] = acc[j >> 2][j & 3];
      const double fk = grad_mfma_dot(h, y);
      const long oi = nni_out_idx(a, k, i, p);
      if (q == 0) { a.f[oi] = fk; a.sig[oi] = ls; }
   }
}

// the classes of every (row, pattern) and the chunks' sums: grid (stride / 256, rows); a wave = one chunk of GRAD_CHUNK patterns
__global__ __launch_bounds__(256) void nni_combine_kernel(NniArgs a)
{
   const long p = (long)blockIdx.x * 256 + threadIdx.x;
   const bool present = (int)blockIdx.y == a.n_group;      // (a batch's first group is launched with a row more: the present tree)
   const int row = present ? a.cap : (int)blockIdx.y;
   const double acc = score_wave_sum(p < a.m.nb ? nni_combine(a, row, p) : 0.0);
   const long out_row = present ? a.n_swaps : a.swap0 + row;
   long chunk;
   if (score_chunk_lane(a, p, &chunk)) a.partial[out_row * a.n_chunks + chunk] = acc;
}
}  // namespace paml_amd

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

struct NniScratch : ScoreScratch {
   using ScoreScratch::ScoreScratch;
   DevBuf<int> swaps;
};

}  // namespace

extern "C" int paml_amd_nni_scores(paml_amd_engine *e, const double *branch, const double *gene_rate, int n_swaps, const int *swaps, double *lnL0,
                                   double *lnL, double *lnf)
{
   enter(e);
   nni_info = AncCallInfo{};
   const char *who = "nni_scores";
   if (!e || !branch || !swaps || !lnL0 || !lnL) return fail(e, PAML_AMD_EINVAL, "nni_scores: null argument");
   if (n_swaps < 1) return fail(e, PAML_AMD_EINVAL, "nni_scores: n_swaps < 1");
   if (int rc = score_begin(e, who, nullptr)) return rc;
   const TreeDesc &T = e->tree;
   const int K = e->K;
   {
      const std::vector<int> father = score_fathers(T);
      for (int i = 0; i < n_swaps; i++) {
         const int v = swaps[3 * i], s = swaps[3 * i + 1], x = swaps[3 * i + 2];
         const std::string at = "nni_scores: swap " + std::to_string(i) + ": ";
         if (int rc = score_check_node(e, at, v, &father, true)) return rc;
         if (!score_son_of(T, s, v)) return fail(e, PAML_AMD_EINVAL, at + std::to_string(s) + " is not a son of " + std::to_string(v));
         if (x == v || !score_son_of(T, x, father[v]))
            return fail(e, PAML_AMD_EINVAL, at + std::to_string(x) + " is not a son of the father of " + std::to_string(v) + " other than it");
      }
   }
   const bool mfma = e->kk == KK_MFMA64;
   hipStream_t st = e->stream;
   NniScratch w(nni_info);
   NniArgs a{};
   if (int rc = anc_tree_pack(e, who, w, &a.m.t)) return rc;
   if (int rc = score_present_pmat(e, who, branch, gene_rate, w)) return rc;
   HIPCHK(upload(w.swaps, swaps, (size_t)3 * n_swaps, st));
   if (int rc = anc_pmat_wait(e, w)) return rc;
   e->pmat_valid = true;      // (d_rowmajor holds every branch's P(t) in the tree's own orientation, as after the gradient)

   // the workspace per pattern: the partials and the messages, then (2 K + 1) doubles per row (the swaps of a group and the present tree)
   ScorePlan plan;
   if (int rc = score_plan(e, w, &plan, "PAML_AMD_NNI_ARENA_MB", (2.0 * K + 1) * 8, n_swaps, n_swaps)) return rc;
   const int cap = plan.cap;
   const size_t rows = (size_t)K * (cap + 1);
   if (int rc = score_alloc(e, who, w, plan, {{&w.f, rows}, {&w.sig, rows}, {&w.lnf, (size_t)cap + 1}})) return rc;
   score_fill(a, w, e, plan, n_swaps);
   a.swaps = w.swaps.p;
   if (int rc = anc_score_batches(
          e, w, a, plan.batch, score_n_groups(n_swaps, cap),
          [&](int gi, dim3 tiles, dim3 lanes) {
             score_group(a, cap, n_swaps, gi);
             if (mfma) hipLaunchKernelGGL(nni_mfma_kernel, tiles, dim3(256), 0, st, a);
             else anc_lanes(e->kk, [&](auto N) { hipLaunchKernelGGL(nni_lane_swap_kernel<N()>, dim3(lanes.x, K, a.n_group), dim3(256), 0, st, a); });
          },
          [&](int gi, dim3 lanes) { hipLaunchKernelGGL(nni_combine_kernel, dim3(lanes.x, a.n_group + (gi == 0 ? 1 : 0)), dim3(256), 0, st, a); },
          [&](int, long h0, long nb) {      // the group's rows to the caller's [n_swaps][n_patt]
             return score_copy_rows(e, w.lnf.p, plan.batch, a.swap0, a.n_group, lnf, h0, nb, [](long i) { return i; });
          }))
      return rc;
   return score_totals(e, w, plan, n_swaps, nullptr, lnL0, {lnL});
}

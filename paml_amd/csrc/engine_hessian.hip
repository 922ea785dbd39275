// engine_hessian.hip — lnL, its gradient and its Hessian over all branch lengths in one call (paml_amd_hessian); the definition in
// kernels_hessian.h, the kernels here, the lists of steps in hessian_plan.h.  P(t), dP, d2P and P^T come from the curvature call's
// builders (anc_pmat, curv_pmat_kernel), the down pass is the ancestral module's, the outer pass, the combination of lnL, grad and the
// diagonal and their totals are paml_amd_curvature's own kernels: those results have its bytes.
// Built for gfx950 only (one of the translation units of libpaml_amd.so, see engine_state.h).
#include "engine_state.h"
#include "kernels_curvature.h"
#include "kernels_hessian.h"
#include "ancestral_host.h"

static thread_local AncCallInfo hess_info;

extern "C" void paml_amd_hessian_info(int *last_batches, double *last_kernel_ms) { hess_info.read(last_batches, last_kernel_ms); }

namespace paml_amd {

// one (pattern, class) per lane: grid (patterns / 256, K); the group's sources one after the other
template <int N> __global__ __launch_bounds__(256) void hess_lane_kernel(HessArgs a)
{
   const long p = (long)blockIdx.x * 256 + threadIdx.x;
   if (p >= a.g.m.nb) return;
   for (int is = a.source0; is < a.source0 + a.n_sources; is++) hess_lane_source<N>(a, blockIdx.y, p, is);
}

// Matrix cores: four waves own ANC_TILE patterns of one class and loop over the group's sources and their steps; lane = q * 16 + pattern,
// register m = state 4 m + q.  Every branch below is uniform over the workgroup (the steps are the same for all patterns), so the
// barriers inside the products are met by all four waves.  Grid (stride / ANC_TILE, K).
__global__ __launch_bounds__(256) void hess_mfma_kernel(HessArgs a)
{
   __shared__ __attribute__((aligned(16))) double sP[4096];
   const AncMargArgs &m = a.g.m;
   const AncTree &t = m.t;
   const int tid = threadIdx.x, lane = tid & 63, n = m.n;
   const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
   const int q = lane >> 4, k = blockIdx.y;
   const AncMfma w{sP, lane, wave, q};
   const long g16 = (long)blockIdx.x * 4 + wave, p = g16 * 16 + (lane & 15);
   const long pc = p < m.nb ? p : m.nb - 1;      // (lanes past the batch's end read the last pattern and write into the padding: p < stride)
   const long pset = (long)m.gene * m.K + k;
   const long part = (long)k * t.n_int * (m.stride >> 4) + g16, sc = (long)k * t.n_int * m.stride;      // (+ node * (stride >> 4), * 1024; + node * stride)
   for (int is = a.source0; is < a.source0 + a.n_sources; is++) {
      const int *sr = a.sources + (long)HESS_SOURCE_INTS * is;
      for (int i = sr[1]; i < sr[1] + sr[2]; i++) {
         const int *st = a.steps + (long)HESS_STEP_INTS * i;
         const int op = st[0], node = st[1];
         double h[16], ls = 0;
         __syncthreads();      // (SLp / SAp of an earlier step were stored by the pattern's q = 0 lane: a workgroup-scope fence before the other lanes read them)
         if (st[2] == HESS_HEAD_ONES) {
#pragma unroll
            for (int j = 0; j < 16; j++) h[j] = 4 * j + q < n ? 1.0 : 0.0;
         }
         else if (st[2] == HESS_HEAD_PRESENT) nni_mfma_father(m, k, g16, pc, lane, q, st[3], h, &ls);
         else {
            const int fi = st[3] - t.n_tips;
            part_load(a.Ap + (part + (long)fi * (m.stride >> 4)) * 1024, lane, h);      // (this lane's own stores)
            ls = a.SAp[sc + (long)fi * m.stride + pc];
         }
         for (int j = st[4]; j < st[4] + st[5]; j++) {
            const int kind = a.factors[2 * j], s = a.factors[2 * j + 1];
            if (kind == HESS_FAC_PRESENT) spr_mfma_mul(m, w, m.pint, m.ptip, m.L, m.SL, k, g16, pc, s, h, &ls);
            else if (kind == HESS_FAC_SOURCE) hess_mfma_mul_d(m, w, a.g.dP, m.L, m.SL, k, g16, pc, s, h, &ls);
            else spr_mfma_mul(m, w, m.pint, m.ptip, a.Lp, a.SLp, k, g16, pc, s, h, &ls);
         }
         if (op == HESS_UP) {
            const int vi = node - t.n_tips;
            hess_mfma_rescale(m, h, &ls);
            part_store(a.Lp + (part + (long)vi * (m.stride >> 4)) * 1024, lane, h);
            if (q == 0) a.SLp[sc + (long)vi * m.stride + p] = ls;
            continue;
         }
         if (op == HESS_OUT) {
            const int vi = node - t.n_tips;
            v4d acc[4];
            w.product(a.g.PT + (pset * t.n_nodes + node) * 4096, h, acc);      // P^T H'
            double x[16];
#pragma unroll
            for (int j = 0; j < 16; j++) x[j] = acc[j >> 2][j & 3];
            hess_mfma_rescale(m, x, &ls);
            part_store(a.Ap + (part + (long)vi * (m.stride >> 4)) * 1024, lane, x);
            if (q == 0) a.SAp[sc + (long)vi * m.stride + p] = ls;
            continue;
         }
         hess_mfma_mul_d(m, w, a.g.dP, st[6] ? a.Lp : m.L, st[6] ? a.SLp : m.SL, k, g16, pc, node, h, &ls);      // H' o (dP L)
         double mk = 0;
#pragma unroll
         for (int j = 0; j < 16; j++) mk += h[j];
         mk += __shfl_xor(mk, 16);
         mk += __shfl_xor(mk, 32);
         const long oi = hess_out_idx(a, k, st[7] - a.row0, p);
         if (q == 0) { a.mm[oi] = mk; a.msig[oi] = ls; }
      }
   }
}

// grid (stride / 256, n_nodes)
__global__ __launch_bounds__(256) void hess_score_kernel(HessArgs a)
{
   const long p = (long)blockIdx.x * 256 + threadIdx.x;
   if (p < a.g.m.nb) hess_score(a, blockIdx.y, p);
}

// the classes of every (pair of the group, pattern) and the chunks' sums: grid (stride / 256, n_group); a wave = one chunk of GRAD_CHUNK
// patterns, the gradient's butterfly
__global__ __launch_bounds__(256) void hess_combine_kernel(HessArgs a)
{
   const long p = (long)blockIdx.x * 256 + threadIdx.x;
   const int row = blockIdx.y;
   double acc = p < a.g.m.nb ? hess_combine(a, row, p) : 0.0;
#pragma unroll
   for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off);
   if ((threadIdx.x & 63) == 0 && (p & ~63L) < a.g.m.nb) a.part[(p >> 6) * a.cap + row] = acc;
}

// a lane per pair of the group: the batch's chunks added to the pair's total one after the other.  grid (n_group / 256)
__global__ __launch_bounds__(256) void hess_total_kernel(HessArgs a, int n_chunks_batch)
{
   const int row = blockIdx.x * 256 + threadIdx.x;
   if (row >= a.n_group) return;
   double s = a.total[a.row0 + row];
   for (int c = 0; c < n_chunks_batch; c++) s += a.part[(long)c * a.cap + row];
   a.total[a.row0 + row] = s;
}

}  // namespace paml_amd

namespace {

struct HessScratch : AncScratch {
   using AncScratch::AncScratch;
   DevBuf<double> dP, d2P, PT, num, den, cur, sig, lnf, scores, partial, out, Lp, Ap, SLp, SAp, mm, msig, part, total;
   DevBuf<int> plan;
};

}  // namespace

extern "C" int paml_amd_hessian(paml_amd_engine *e, const double *branch, const double *gene_rate, const int *nodes, int n_list, double *lnL, double *grad,
                                double *hess, double *lnf)
{
   enter(e);
   hess_info = AncCallInfo{};
   const char *who = "hessian";
   if (!e || !branch || !lnL || !grad || !hess) return fail(e, PAML_AMD_EINVAL, "hessian: null argument");
   if (!(e->have_tips && e->have_tree && e->have_pi && e->have_classes) || e->eigen.empty())
      return fail(e, PAML_AMD_EINVAL, "hessian: called before set_tips/set_tree/set_pi/set_classes/set_eigen");
   if (int rc = anc_begin(e, who, "the derivatives of a rate-matrix (UNREST) set's P(t) need matrix products of their own")) return rc;
   const TreeDesc &T = e->tree;
   const int nn = T.n_nodes, n = e->n, K = e->K, G = e->n_genes, n_tips = e->n_tips, n_int = nn - n_tips;
   if (nn > 65535) return fail(e, PAML_AMD_EUNSUPPORTED, "hessian: more than 65535 nodes");
   if ((nodes == nullptr) != (n_list == 0) || n_list < 0) return fail(e, PAML_AMD_EINVAL, "hessian: nodes and n_list do not agree (NULL, 0: every node)");
   const HessTreeView view{n_tips, nn, T.root, T.sons_ptr.data(), T.sons.data()};
   std::vector<int> father, pre, list;
   if (!hess_fathers(view, father, pre)) return fail(e, PAML_AMD_EINVAL, "hessian: the tree does not reach every node from its root");
   if (nodes) {
      const std::string why = hess_check_nodes(view, nodes, n_list);
      if (!why.empty()) return fail(e, PAML_AMD_EINVAL, "hessian: " + why);
      list.assign(nodes, nodes + n_list);
   }
   else
      for (int v = 0; v < nn; v++)
         if (v != T.root) list.push_back(v);
   HessPlan plan;
   hess_plan(view, father, pre, (int)list.size(), list.data(), plan);
   const int n_pairs = plan.n_pairs();

   const bool mfma = e->kk == KK_MFMA64;
   hipStream_t st = e->stream;
   HessScratch w(hess_info);
   HessArgs a{};
   GradArgs &ga = a.g;
   AncMargArgs &m = ga.m;
   if (int rc = anc_tree_pack(e, who, w, &m.t)) return rc;
   if (int rc = anc_pmat(e, who, branch, gene_rate, w)) return rc;
   if (int rc = grad_dpmat(e, w.dP, &w.d2P, w.PT)) return rc;
   const size_t o_steps = plan.sources.size(), o_factors = o_steps + plan.steps.size(), o_pairs = o_factors + plan.factors.size();
   {
      std::vector<int> pack(plan.sources);
      pack.insert(pack.end(), plan.steps.begin(), plan.steps.end());
      pack.insert(pack.end(), plan.factors.begin(), plan.factors.end());
      pack.insert(pack.end(), plan.pairs.begin(), plan.pairs.end());
      pack.push_back(0);      // (a list without pairs still has a buffer)
      HIPCHK(upload(w.plan, pack.data(), pack.size(), st));
      if (int rc = anc_pmat_wait(e, w)) return rc;      // (`pack` is on this stack)
   }
   e->pmat_valid = true;      // (d_rowmajor holds every branch's P(t) in the tree's own orientation, as after paml_amd_gradient)

   const long n_chunks = anc_chunk_base(e)[G];
   const int rows = 2 * nn + 1;      // w s_v, w c_v, w lnf: the curvature's rows
   HIPCHK(w.partial.ensure((size_t)rows * std::max<long>(n_chunks, 1)));
   HIPCHK(w.out.ensure((size_t)rows));
   HIPCHK(w.total.ensure((size_t)std::max(n_pairs, 1)));
   HIPCHK(hipMemsetAsync(w.total.p, 0, (size_t)std::max(n_pairs, 1) * 8, st));

   // the workspace per pattern: the curvature's, L' and A' of one source, the scores; then (2 K + 1 / 64) doubles per row of a group
   const int ns = mfma ? 64 : n;
   const double fixed = hess_bytes_per_pattern(K, n_int, nn, ns), per_row = hess_bytes_per_row(K);
   const double arena = anc_arena_mb("PAML_AMD_HESS_ARENA_MB") * 1048576.0;
   int cap = std::max(n_pairs, 1);
   const double all_patt = (double)((e->n_patt + ANC_TILE - 1) / ANC_TILE * ANC_TILE);
   if ((fixed + per_row * cap) * all_patt > arena)      // batches of patterns: the rows take no more of the workspace than the rest does
      cap = (int)std::min<double>(cap, std::max(1.0, floor(fixed / per_row)));
   if ((fixed + per_row * cap) * ANC_TILE > arena)      // one tile with these rows does not fit: fewer
      cap = (int)std::min<double>(cap, std::max(1.0, floor((arena / ANC_TILE - fixed) / per_row)));
   cap = std::min(std::max(cap, std::max(plan.max_rows, 1)), 65535);      // (a source is not split; the combining kernel has a grid row per pair)
   std::vector<int> group_first(1, 0);      // the groups: as many whole sources as the rows hold
   {
      int used = 0;
      for (int is = 0; is < plan.n_sources(); is++) {
         const int r0 = plan.sources[HESS_SOURCE_INTS * is + 3], r1 = is + 1 < plan.n_sources() ? plan.sources[HESS_SOURCE_INTS * (is + 1) + 3] : n_pairs;
         if (used + (r1 - r0) > cap) { group_first.push_back(is); used = 0; }
         used += r1 - r0;
      }
      if (plan.n_sources() > 0) group_first.push_back(plan.n_sources());
   }
   const int n_groups = (int)group_first.size() - 1;
   long batch = anc_batch(fixed + per_row * cap, e->n_patt, "PAML_AMD_HESS_ARENA_MB");
   {
      const size_t part = (size_t)K * n_int * ns, sc = (size_t)K * n_int, cl = (size_t)K * nn, rw = (size_t)K * cap;
      if (int rc = anc_alloc(e, who, {{&w.L, part}, {&w.G, part}, {&w.SL, sc}, {&w.SG, sc}, {&w.num, cl}, {&w.den, cl}, {&w.cur, cl}, {&w.sig, cl}, {&w.lnf, 1},
                                      {&w.Lp, part}, {&w.Ap, part}, {&w.SLp, sc}, {&w.SAp, sc}, {&w.scores, (size_t)nn}, {&w.mm, rw}, {&w.msig, rw}}, &batch))
         return rc;
   }
   HIPCHK(w.part.ensure((size_t)(batch / GRAD_CHUNK) * cap));
   anc_fill(e, w, batch, m);
   ga.dP = w.dP.p; ga.d2P = w.d2P.p; ga.PT = w.PT.p; ga.num = w.num.p; ga.den = w.den.p; ga.cur = w.cur.p; ga.sig = w.sig.p; ga.weights = e->d_weights.p;
   ga.lnf = w.lnf.p; ga.scores = w.scores.p; ga.partial = w.partial.p; ga.n_chunks = n_chunks;
   ga.ref_node = T.sons[T.sons_ptr[T.root]];
   a.sources = w.plan.p; a.steps = w.plan.p + o_steps; a.factors = w.plan.p + o_factors; a.pairs = w.plan.p + o_pairs;
   a.cap = cap; a.Lp = w.Lp.p; a.Ap = w.Ap.p; a.SLp = w.SLp.p; a.SAp = w.SAp.p; a.mm = w.mm.p; a.msig = w.msig.p; a.part = w.part.p; a.total = w.total.p;
   if (int rc = anc_batches(
          e, w, m, &ga.chunk0, batch, [&](const AncBatch &b) { hipLaunchKernelGGL(curv_mfma_kernel, b.tiles, dim3(256), 0, st, ga); },
          [&](const AncBatch &b, int pass) { anc_lanes(e->kk, [&](auto N) { hipLaunchKernelGGL(curv_lane_kernel<N()>, b.lanes, dim3(256), 0, st, ga, pass); }); },
          [&](const AncBatch &b) {
             hipLaunchKernelGGL(curv_combine_kernel, dim3(b.lanes.x, rows), dim3(256), 0, st, ga);
             HIPCHK(hipGetLastError());
             hipLaunchKernelGGL(hess_score_kernel, dim3(b.lanes.x, nn), dim3(256), 0, st, a);
             HIPCHK(hipGetLastError());
             for (int gi = 0; gi < n_groups; gi++) {
                const int is0 = group_first[gi], is1 = group_first[gi + 1];
                a.source0 = is0; a.n_sources = is1 - is0;
                a.row0 = plan.sources[HESS_SOURCE_INTS * is0 + 3];
                a.n_group = (is1 < plan.n_sources() ? plan.sources[HESS_SOURCE_INTS * is1 + 3] : n_pairs) - a.row0;
                if (mfma) hipLaunchKernelGGL(hess_mfma_kernel, b.tiles, dim3(256), 0, st, a);
                else anc_lanes(e->kk, [&](auto N) { hipLaunchKernelGGL(hess_lane_kernel<N()>, b.lanes, dim3(256), 0, st, a); });
                HIPCHK(hipGetLastError());
                hipLaunchKernelGGL(hess_combine_kernel, dim3(b.lanes.x, a.n_group), dim3(256), 0, st, a);
                HIPCHK(hipGetLastError());
                hipLaunchKernelGGL(hess_total_kernel, dim3((unsigned)((a.n_group + 255) / 256)), dim3(256), 0, st, a, (int)((b.nb + GRAD_CHUNK - 1) / GRAD_CHUNK));
                HIPCHK(hipGetLastError());
             }
             return 0;
          },
          [&](const AncBatch &b) {
             if (lnf) HIPCHK(hipMemcpyAsync(lnf + b.h0, w.lnf.p, (size_t)b.nb * 8, hipMemcpyDeviceToHost, st));
             return 0;
          }))
      return rc;
   std::vector<double> out((size_t)rows), total((size_t)std::max(n_pairs, 1));
   HIPCHK(hipMemcpyAsync(total.data(), w.total.p, total.size() * 8, hipMemcpyDeviceToHost, st));
   if (int rc = anc_totals(e, w, w.partial.p, n_chunks, w.out.p, out)) return rc;
   for (int v = 0; v < nn; v++) grad[v] = v == T.root ? 0.0 : out[v];
   *lnL = out[2 * nn];
   // the caller's matrix: the diagonal from the curvature's rows, every pair mirrored
   const int dim = nodes ? n_list : nn;
   std::vector<int> place(nn, -1);
   for (int i = 0; i < dim; i++) place[nodes ? nodes[i] : i] = i;
   std::fill(hess, hess + (size_t)dim * dim, 0.0);
   for (int i = 0; i < dim; i++) {
      const int v = nodes ? nodes[i] : i;
      if (v != T.root) hess[(size_t)i * dim + i] = out[nn + v];
   }
   for (int r = 0; r < n_pairs; r++) {
      const int i = place[plan.pairs[2 * r]], j = place[plan.pairs[2 * r + 1]];
      hess[(size_t)i * dim + j] = hess[(size_t)j * dim + i] = total[r];
   }
   return 0;
}

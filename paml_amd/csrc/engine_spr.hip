// engine_spr.hip — the lnL of every requested subtree-prune-and-regraft neighbour of the tree at the present branch lengths in one call
// (paml_amd_spr_scores) and the canonical list of moves (paml_amd_spr_list, host only); the definition in kernels_spr.h, the kernels here,
// the lists of steps in spr_plan.h.
// Every P(t) comes from the evaluation's own builder (anc_pmat, engine_ancestral.hip), which runs once per family of lengths on a branch
// vector of the tree's size with the tree's own labels: the upper parts (1 - phi) t_v, the lower parts phi t_v, the merged lengths
// t_v + t_father(v) stored at v, and last the tree's own lengths, so that d_rowmajor and pmat_valid are left as after
// paml_amd_nni_scores.  The down pass is the ancestral module's, the outer pass is the NNI module's.
// The host side that is not this call's own is the score calls' skeleton (score_host.h, defined in engine_ancestral.hip).
// Built for gfx950 only (one of the translation units of libpaml_amd.so, see engine_state.h).
#include "engine_state.h"
#include "kernels_spr.h"
#include "score_host.h"

static thread_local AncCallInfo spr_info;

extern "C" void paml_amd_spr_info(int *last_batches, double *last_kernel_ms) { spr_info.read(last_batches, last_kernel_ms); }

namespace paml_amd {

// one pattern per lane: grid (patterns / 256, K); pass 0: the down pass, 1: the outer pass, 2: the group's prunes
template <int N> __global__ __launch_bounds__(256) void spr_lane_kernel(SprArgs a, int pass)
{
   const long p = (long)blockIdx.x * 256 + threadIdx.x;
   if (p >= a.o.m.nb) return;
   if (pass == 0) anc_lane_down<N>(a.o.m, blockIdx.y, p);
   else if (pass == 1) nni_lane_outer<N>(a.o, blockIdx.y, p);
   else
      for (int ip = a.prune0; ip < a.prune0 + a.n_prunes; ip++) spr_lane_prune<N>(a, blockIdx.y, p, ip);
}

// Matrix cores: four waves own ANC_TILE patterns of one class and loop over the group's prunes and their steps; lane = q * 16 + pattern,
// register m = state 4 m + q.  Every branch below is uniform over the workgroup (the steps are the same for all patterns), so the
// barriers inside the products are met by all four waves.  Grid (stride / ANC_TILE, K).
__global__ __launch_bounds__(256) void spr_mfma_kernel(SprArgs a)
{
   __shared__ __attribute__((aligned(16))) double sP[4096];
   const AncMargArgs &m = a.o.m;
   const AncTree &t = m.t;
   const ScoreTile c = score_tile(m);
   const int lane = c.lane, q = c.q, k = c.k, n = m.n;
   const long g16 = c.g16, p = c.p, pc = c.pc, pset = c.pset;
   const AncMfma w{sP, lane, c.wave, q};
   const long part = (long)k * t.n_int * (m.stride >> 4) + g16, sc = (long)k * t.n_int * m.stride;      // (+ node * (stride >> 4), * 1024; + node * stride)
   for (int ip = a.prune0; ip < a.prune0 + a.n_prunes; ip++) {
      const int *pr = a.prunes + (long)SPR_PRUNE_INTS * ip;
      double ms[16], ls_s = 0;      // P_s L_s, once per s
#pragma unroll
      for (int j = 0; j < 16; j++) ms[j] = 4 * j + q < n ? 1.0 : 0.0;
      spr_mfma_mul(m, w, m.pint, m.ptip, m.L, m.SL, k, g16, pc, pr[0], ms, &ls_s);
      for (int is = pr[1]; is < pr[1] + pr[2]; is++) {
         const int *st = a.steps + (long)SPR_STEP_INTS * is;
         const int op = st[0], node = st[1];
         double h[16], ls = 0;
         __syncthreads();      // (SLp / SAp of an earlier step were stored by the pattern's q = 0 lane: a workgroup-scope fence before the other lanes read them)
         if (st[2] == SPR_HEAD_ONES) {
#pragma unroll
            for (int j = 0; j < 16; j++) h[j] = 4 * j + q < n ? 1.0 : 0.0;
         }
         else if (st[2] == SPR_HEAD_PRESENT) nni_mfma_father(m, k, g16, pc, lane, q, st[3], h, &ls);
         else {
            const int fi = st[3] - t.n_tips;
            part_load(a.Ap + (part + (long)fi * (m.stride >> 4)) * 1024, lane, h);      // (this lane's own stores)
            ls = a.SAp[sc + (long)fi * m.stride + pc];
         }
         for (int j = st[4]; j < st[4] + st[5]; j++) {
            const int kind = a.factors[2 * j], u = a.factors[2 * j + 1];
            if (kind == SPR_FAC_PRESENT) spr_mfma_mul(m, w, m.pint, m.ptip, m.L, m.SL, k, g16, pc, u, h, &ls);
            else if (kind == SPR_FAC_MERGED) spr_mfma_mul(m, w, a.pint_m, a.ptip_m, m.L, m.SL, k, g16, pc, u, h, &ls);
            else spr_mfma_mul(m, w, m.pint, m.ptip, a.Lp, a.SLp, k, g16, pc, u, h, &ls);
         }
         const long slot = pset * t.n_nodes + node;
         if (op == SPR_UP) {
            const int vi = node - t.n_tips;
            spr_mfma_rescale(m, h, &ls);
            part_store(a.Lp + (part + (long)vi * (m.stride >> 4)) * 1024, lane, h);
            if (q == 0) a.SLp[sc + (long)vi * m.stride + p] = ls;
            continue;
         }
         v4d acc[4];
         w.product((op == SPR_OUT ? (st[6] ? a.PTm : a.o.PT) : a.PTup) + slot * 4096, h, acc);      // P^T H'
         double u[16];
#pragma unroll
         for (int j = 0; j < 16; j++) u[j] = acc[j >> 2][j & 3];
         if (op == SPR_OUT) {
            const int vi = node - t.n_tips;
            spr_mfma_rescale(m, u, &ls);
            part_store(a.Ap + (part + (long)vi * (m.stride >> 4)) * 1024, lane, u);
            if (q == 0) a.SAp[sc + (long)vi * m.stride + p] = ls;
            continue;
         }
         spr_mfma_mul(m, w, a.pint_dn, a.ptip_dn, st[6] ? a.Lp : m.L, st[6] ? a.SLp : m.SL, k, g16, pc, node, u, &ls);      // W
         const double fk = grad_mfma_dot(u, ms);
         const long oi = nni_out_idx(a.o, k, st[7] - a.o.swap0, p);
         if (q == 0) { a.o.f[oi] = fk; a.o.sig[oi] = ls + ls_s; }
      }
   }
}
}  // namespace paml_amd

extern "C" int paml_amd_spr_list(int n_tips, int n_nodes, int root, const int *sons_ptr, const int *sons, int radius, int *moves, int cap)
{
   if (n_tips < 0) return PAML_AMD_EINVAL;
   const int n = spr_list(SprTreeView{n_tips, n_nodes, root, sons_ptr, sons}, radius, moves, cap);
   return n < 0 ? PAML_AMD_EINVAL : n;
}

namespace {

struct SprScratch : ScoreScratch {
   using ScoreScratch::ScoreScratch;
   DevBuf<double> Pup, Pdn, Pm, PTup, pint_dn, ptip_dn, pint_m, ptip_m, PTm, Lp, Ap, SLp, SAp;
   DevBuf<int> plan;
};

}  // namespace

extern "C" int paml_amd_spr_scores(paml_amd_engine *e, const double *branch, const double *gene_rate, int n_moves, const int *moves, double phi,
                                   double *lnL0, double *lnL, double *lnf)
{
   enter(e);
   spr_info = AncCallInfo{};
   const char *who = "spr_scores";
   if (!e || !branch || !moves || !lnL0 || !lnL) return fail(e, PAML_AMD_EINVAL, "spr_scores: null argument");
   if (n_moves < 1) return fail(e, PAML_AMD_EINVAL, "spr_scores: n_moves < 1");
   if (!(phi >= 0 && phi <= 1)) return fail(e, PAML_AMD_EINVAL, "spr_scores: phi = " + std::to_string(phi) + " is outside [0, 1]");
   if (int rc = score_begin(e, who, nullptr)) return rc;
   const TreeDesc &T = e->tree;
   const int nn = T.n_nodes, K = e->K, n_tips = e->n_tips;
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
   SprScratch w(spr_info);
   SprArgs a{};
   NniArgs &o = a.o;
   AncMargArgs &m = o.m;
   if (int rc = anc_tree_pack(e, who, w, &m.t)) return rc;
   {
      // one run of the builder per family; what the kernels need of it is kept before the next run
      std::vector<double> b(nn);
      for (int v = 0; v < nn; v++) b[v] = (1 - phi) * branch[v];
      if (int rc = anc_pmat_waited(e, who, b.data(), gene_rate, w)) return rc;
      if (int rc = anc_keep_pmat(e, nullptr, nullptr, &w.PTup, w.Pup)) return rc;
      for (int v = 0; v < nn; v++) b[v] = phi * branch[v];
      if (int rc = anc_pmat_waited(e, who, b.data(), gene_rate, w)) return rc;
      if (int rc = anc_keep_pmat(e, &w.pint_dn, &w.ptip_dn, nullptr, w.Pdn)) return rc;
      for (int v = 0; v < nn; v++) b[v] = branch[v] + (father[v] >= 0 && father[v] != T.root ? branch[father[v]] : 0.0);
      if (int rc = anc_pmat_waited(e, who, b.data(), gene_rate, w)) return rc;
      if (int rc = anc_keep_pmat(e, &w.pint_m, &w.ptip_m, &w.PTm, w.Pm)) return rc;
   }
   // the tree's own lengths last: what the passes read, and what the engine keeps
   if (int rc = score_present_pmat(e, who, branch, gene_rate, w, nullptr, true)) return rc;
   const size_t o_steps = plan.prunes.size(), o_factors = o_steps + plan.steps.size();
   {
      std::vector<int> pack(plan.prunes);
      pack.insert(pack.end(), plan.steps.begin(), plan.steps.end());
      pack.insert(pack.end(), plan.factors.begin(), plan.factors.end());
      pack.push_back(0);      // (a list without factors still has a buffer)
      HIPCHK(upload(w.plan, pack.data(), pack.size(), st));
      if (int rc = anc_pmat_wait(e, w)) return rc;      // (`pack` is on this stack)
   }
   e->pmat_valid = true;      // (d_rowmajor holds every branch's P(t) in the tree's own orientation, as after the gradient)

   // the workspace per pattern: the partials and the messages of the tree and of one prune, then (2 K + 1) doubles per row (the moves of a
   // group and the present tree).  The rows of a group by a rule of this call's own:
   const double fixed = 2 * score_fixed(e), per_row = (2.0 * K + 1) * 8;
   const double arena_mb = anc_arena_mb("PAML_AMD_SPR_ARENA_MB");
   int cap = n_moves;
   const double all_patt = (double)((n_patt + ANC_TILE - 1) / ANC_TILE * ANC_TILE);
   if ((fixed + per_row * (n_moves + 1)) * all_patt > arena_mb * 1048576.0)      // batches of patterns: the rows take no more of the workspace than
      cap = (int)std::min<double>(n_moves, std::max(1.0, floor(fixed / per_row) - 1));      // the partials do, so that a batch keeps the device busy
   if ((fixed + per_row * (cap + 1)) * ANC_TILE > arena_mb * 1048576.0)      // one tile with these rows does not fit: fewer
      cap = (int)std::min<double>(n_moves, std::max(1.0, floor((arena_mb * 1048576.0 / ANC_TILE - fixed) / per_row) - 1));
   cap = std::min(std::max(cap, plan.max_rows), 65534);      // (a prune is not split; the combining kernel has a grid row per row and one for the present tree)
   ScorePlan sp;
   if (int rc = score_plan(e, w, &sp, "PAML_AMD_SPR_ARENA_MB", per_row, n_moves, n_moves, 1, fixed, cap)) return rc;
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
   {
      const size_t rows = (size_t)K * (cap + 1);
      if (int rc = score_alloc(e, who, w, sp, {{&w.Lp, sp.part}, {&w.Ap, sp.part}, {&w.SLp, sp.sc}, {&w.SAp, sp.sc}, {&w.f, rows}, {&w.sig, rows}, {&w.lnf, (size_t)cap + 1}})) return rc;
   }
   score_fill(o, w, e, sp, n_moves);
   a.Pup = w.Pup.p; a.Pdn = w.Pdn.p; a.Pm = w.Pm.p; a.PTup = w.PTup.p; a.pint_dn = w.pint_dn.p; a.ptip_dn = w.ptip_dn.p;
   a.pint_m = w.pint_m.p; a.ptip_m = w.ptip_m.p; a.PTm = w.PTm.p;
   a.prunes = w.plan.p; a.steps = w.plan.p + o_steps; a.factors = w.plan.p + o_factors;
   a.Lp = w.Lp.p; a.Ap = w.Ap.p; a.SLp = w.SLp.p; a.SAp = w.SAp.p;
   auto lane_pass = [&](dim3 lanes, int pass) { anc_lanes(e->kk, [&](auto N) { hipLaunchKernelGGL(spr_lane_kernel<N()>, lanes, dim3(256), 0, st, a, pass); }); };
   auto group = [&](int gi) {      // the prunes group_first[gi] .. group_first[gi + 1] and their rows
      const int ip0 = group_first[gi], ip1 = group_first[gi + 1];
      a.prune0 = ip0; a.n_prunes = ip1 - ip0;
      o.swap0 = plan.prunes[SPR_PRUNE_INTS * ip0 + 3];
      o.n_group = (ip1 < plan.n_prunes() ? plan.prunes[SPR_PRUNE_INTS * ip1 + 3] : n_moves) - o.swap0;
   };
   if (int rc = anc_score_batches(
          e, w, o, sp.batch, (int)group_first.size() - 1,
          [&](int gi, dim3 tiles, dim3 lanes) {
             group(gi);
             if (mfma) hipLaunchKernelGGL(spr_mfma_kernel, tiles, dim3(256), 0, st, a);
             else lane_pass(lanes, 2);
          },
          [&](int gi, dim3 lanes) { hipLaunchKernelGGL(nni_combine_kernel, dim3(lanes.x, o.n_group + (gi == 0 ? 1 : 0)), dim3(256), 0, st, o); },
          [&](int, long h0, long nb) {      // the group's rows to the caller's [n_moves][n_patt], at the move's place in the caller's list
             return score_copy_rows(e, w.lnf.p, sp.batch, o.swap0, o.n_group, lnf, h0, nb, [&](long i) { return plan.order[i]; });
          },
          nullptr, lane_pass))
      return rc;
   return score_totals(e, w, sp, n_moves, plan.order.data(), lnL0, {lnL});
}

// engine_eval.hip — one likelihood evaluation: batched P(t) (Kernel A), the fused pruning kernel chosen for the problem (Kernel B:
// per-tree specialised, streamed or full interpreter), the reduction (Kernel C) and the exchange step over the ranks; and the
// entry points built on it (paml_amd_eval, _eval_batch, _eval_device, _eval_dirty, _eval_adg).
// Built for gfx950 only (one of the translation units of libpaml_amd.so, see engine_state.h).
#include "engine_state.h"
#include "kernels_pmat.h"
#include "kernels_prune.h"
#include "kernels_reduce.h"

namespace paml_amd {

int build_tiles(paml_amd_engine *e)
{
   std::vector<int2> tiles;
   for (int g = 0; g < e->n_genes; g++)
      for (int h = e->gene_off[g]; h < e->gene_off[g + 1]; h += e->tile_patt) tiles.push_back(make_int2(g, h));
   e->n_tiles = (int)tiles.size();
   HIPCHK(upload(e->d_tiles, tiles.data(), tiles.size(), e->stream));
   const int tf = e->kk == KK_MFMA64 ? GATHER_WAVES * 16 : 256;
   std::vector<int2> tfull;
   for (int g = 0; g < e->n_genes; g++)
      for (int h = e->gene_off[g]; h < e->gene_off[g + 1]; h += tf) tfull.push_back(make_int2(g, h));
   e->n_tiles_full = (int)tfull.size();
   HIPCHK(upload(e->d_tiles_full, tfull.data(), tfull.size(), e->stream));
   if (e->kk == KK_MFMA64) {      // where a tile's resident partials live: the groups of the 64-pattern tiles it covers (consecutive within a gene)
      std::vector<int> g0(tiles.size());
      size_t k = 0;
      int base = 0;                // 64-pattern tiles of the genes before
      for (int g = 0; g < e->n_genes; g++) {
         for (int h = e->gene_off[g]; h < e->gene_off[g + 1]; h += e->tile_patt) g0[k++] = (base + (h - e->gene_off[g]) / tf) * GATHER_WAVES;
         base += (e->gene_off[g + 1] - e->gene_off[g] + tf - 1) / tf;
      }
      HIPCHK(upload(e->d_tile_group0, g0.data(), g0.size(), e->stream));
   }
   if (e->kk == KK_MFMA64 && e->tile_patt >= 128 && e->d_z.p && e->d_weights.p) {   // code blocks of the specialised kernel
      // (trees of more than 207 tips: two halves per tile, the rows in the order the tree's walk consumes them — jit_zplan; the tree's
      //  program is known by the time a kernel with 128-pattern tiles has been chosen, and launch_eval comes back here when it changes)
      JitZPlan zp;
      const bool half = !e->prog.ops.empty() && (zp = jit_zplan(e->prog, e->n_tips, e->tile_patt)).half;
      e->zt_bytes = half ? zp.pieces * zp.ZP * 2048 : jit_zpieces(e->n_tips, e->tile_patt) * 2048;
      e->zt_key = half ? jit_program_key(e->prog, e->n_tips) : std::string();
      if (half) {      // (row -> tip, then row -> position in the block)
         std::vector<int> both(zp.tip_of);
         both.insert(both.end(), zp.row_at.begin(), zp.row_at.end());
         HIPCHK(upload(e->d_ztip_of, both.data(), both.size(), e->stream));
      }
      HIPCHK(e->d_ztiles.ensure((size_t)e->n_tiles * e->zt_bytes));
      hipLaunchKernelGGL(ztile_kernel, dim3(e->n_tiles), dim3(e->tile_patt), 0, e->stream, e->d_tiles.p, e->d_gene_off.p, e->d_z.p, (long)e->n_patt,
                         e->d_weights.p, e->n_tips, e->zt_bytes, e->d_ztiles.p, half ? (const int *)e->d_ztip_of.p : (const int *)nullptr,
                         half ? (const int *)e->d_ztip_of.p + (e->n_tips + 1) : (const int *)nullptr);
   }
   HIPCHK(hipStreamSynchronize(e->stream));
   e->tiles_built_for = e->tile_patt;
   return 0;
}

// The tile tables of the kernel about to run (21 .. 64 states): 128-pattern tiles with their code blocks (per-tree kernel, streaming
// interpreter) or 64-pattern ones.  A change of tile size swaps the current set with the stashed one (built once each, engine_state.h
// TileStash) — the resident partials have ONE layout whatever the tile size (PruneArgs::part_groups), they stay valid.
int select_tiles(paml_amd_engine *e, bool big_tiles, int want_waves, bool jit_ok)
{
   const bool change = big_tiles != e->mfma_dma || want_waves != e->mfma_waves;
   if (change) {
      e->swap_tile_stash();
      e->mfma_dma = big_tiles;
      e->mfma_waves = want_waves;
      e->tile_patt = e->mfma_waves * 16;
   }
   bool have = !change || (e->tiles_built_for == e->tile_patt && e->d_tiles.p);
   if (have && jit_ok && e->tile_patt >= 128 && (e->n_tips > 200 || !e->zt_key.empty())) {      // piece mode: the code blocks' rows follow the tree's program
      const JitZPlan zp = jit_zplan(e->prog, e->n_tips, e->tile_patt);
      have = (zp.half ? jit_program_key(e->prog, e->n_tips) : std::string()) == e->zt_key;
   }
   return have ? 0 : build_tiles(e);
}

// The full interpreters: gather (21..64 states), else one pattern per lane — the register-stack instantiation that fits the program, else
// the scratch one.
void launch_prune_full(paml_amd_engine *e, int max_stack, int n_blocks, const PruneArgs &pr, hipStream_t s)
{
   const dim3 g(n_blocks), b(256);
   switch (e->kk) {
   case KK_MFMA64: hipLaunchKernelGGL(prune_mfma64_gather<GATHER_WAVES>, g, dim3(GATHER_WAVES * 64), 0, s, pr); break;
   case KK_VALU4:
      if (max_stack <= 4) hipLaunchKernelGGL((prune_valu<4, 4, true>), g, b, 0, s, pr);
      else hipLaunchKernelGGL((prune_valu<4, VALU_MAXD_SMALL>), g, b, 0, s, pr);
      break;
   case KK_VALU5:
      if (max_stack <= 4) hipLaunchKernelGGL((prune_valu<5, 4, true>), g, b, 0, s, pr);
      else hipLaunchKernelGGL((prune_valu<5, VALU_MAXD_SMALL>), g, b, 0, s, pr);
      break;
   case KK_VALU20:      // a register stack costs > 256 VGPRs (one wave per SIMD) and measures 2x slower than scratch
      hipLaunchKernelGGL((prune_valu<20, VALU_MAXD_20>), g, b, 0, s, pr);
      break;
   }
}

// 21..64 states in the mfma64 layout, every eigen system a (U, V, Root) one: four workgroups per matrix on the matrix cores
// (pmat_mfma_kernel)
bool pmat_on_matrix_cores(const paml_amd_engine *e, const PmatArgs &pa)
{
   bool ok = e->kk == KK_MFMA64 && pa.layout == 1 && e->n_codes <= 256;
   for (const EigenHost &h : e->eigen) ok = ok && (h.kind == PAML_AMD_EIGEN_UVROOT || h.kind < 0);      // (< 0: an id never set, referred to by nothing)
   return ok;
}

void launch_pmat(const PmatArgs &pa, const InlineVec &iv, int n_nodes, int psets, bool small, hipStream_t s, bool mfma)
{
   const int gx = (n_nodes + std::max(pa.npb, 1) - 1) / std::max(pa.npb, 1);
   if (mfma) {
      if ((long)n_nodes * psets >= 128) hipLaunchKernelGGL(pmat_mfma_kernel<true>, dim3(n_nodes, psets, 4), dim3(256), 0, s, pa, iv);
      else hipLaunchKernelGGL(pmat_mfma_kernel<false>, dim3(n_nodes, psets, 4), dim3(256), 0, s, pa, iv);
   }
   else if (small) hipLaunchKernelGGL(pmat_small_kernel, dim3((n_nodes * psets + 7) / 8), dim3(256), 0, s, pa, iv);
   else if (pa.n <= 32 && pa.layout != 1) hipLaunchKernelGGL(pmat_kernel_t<32>, dim3(gx, psets), dim3(256), 2 * 32 * 32 * sizeof(double), s, pa, iv);
   else hipLaunchKernelGGL(pmat_kernel_t<64>, dim3(gx, psets), dim3(256), 2 * 4096 * sizeof(double), s, pa, iv);
}

void launch_zpm(const unsigned char *z, long z_stride, int n_tips, int n_patt, int zw, unsigned int *out, hipStream_t s)
{
   hipLaunchKernelGGL(zpm_kernel, dim3((n_patt + 255) / 256), dim3(256), 0, s, z, z_stride, n_tips, n_patt, zw, out);
}

// The one way to a per-tree kernel (declared in engine_state.h, which says what it promises).
int obtain_kernel(paml_amd_engine *e, paml_amd_engine::JitSlot &slot, JitKernel *dst, bool pooled, const std::string &key,
                  const std::function<std::string()> &gen, JitWait wait, const char *what, bool *have)
{
   *have = pooled ? e->jit_recall(key) : (dst->fn && dst->key == key);      // (the kernel in use, or one of this engine's other programs kept loaded)
   if (*have || slot.failed.count(key)) return 0;
   auto failed = [&](const std::string &why) {
      slot.failed.insert(key);
      e->err = std::string("jit (") + what + "): " + why;
      return e->env.jit_strict ? fail(e, PAML_AMD_EHIP, e->err) : 0;
   };
   auto load = [&](const std::vector<char> &code) {      // beside the kernel in use, which goes only when this one is there
      JitKernel nk;
      if (jit_load_code(code, &nk) != 0) {
         if (nk.mod) (void)hipModuleUnload(nk.mod);
         return failed("hipModuleLoadData failed");
      }
      if (pooled) e->jit_retire();
      else if (dst->mod) (void)hipModuleUnload(dst->mod);
      *dst = nk;
      dst->key = key;
      *have = true;
      return 0;
   };
   if (slot.job && slot.job->state.load() >= 2) {      // a finished worker: this key's, or an earlier tree's (dropped silently)
      const std::unique_ptr<paml_amd_engine::JitJob> job = std::move(slot.job);
      if (job->th.joinable()) job->th.join();
      if (job->key == key) return job->state.load() == 2 ? load(job->code) : failed(job->log);
   }
   // (a worker still compiling: a caller that does not wait goes on with the interpreter kernels; one that waits is not held up by
   //  another program's build and compiles its own)
   if (slot.job && wait == JIT_WAIT_WORKER) return 0;
   const std::string src = gen();
   if (!e->env.jit_dump.empty())
      if (FILE *f = fopen(e->env.jit_dump.c_str(), "w")) { fputs(src.c_str(), f); fclose(f); }
   std::vector<char> code;
   if (jit_cached_code(src, &code)) return load(code);      // a code object on disk is loaded at once
   if (wait == JIT_WAIT_CALLER) {
      std::string log;
      return jit_compile_code(src, &code, &log) == 0 ? load(code) : failed(log);
   }
   paml_amd_engine::JitJob *job = new paml_amd_engine::JitJob();
   slot.job.reset(job);
   job->key = key; job->src = src;
   job->state.store(1);
   job->th = std::thread([job]() { job->state.store(jit_compile_code(job->src, &job->code, &job->log) == 0 ? 2 : 3); });
   return 0;
}

// ---- the argument structures of P(t) and of the pruning kernels, filled in one place each (engine_state.h says what the sites add);
// to be called once the buffers have their size ----
PmatArgs pmat_args(const paml_amd_engine *e, int root, const int *label, int layout, double *pcol)
{
   PmatArgs pa{};
   pa.n = e->n; pa.n_nodes = e->tree.n_nodes; pa.root = root; pa.K = e->K; pa.n_genes = e->n_genes; pa.n_labels = e->n_labels;
   pa.n_codes = e->n_codes; pa.layout = layout; pa.pcol = pcol; pa.B = 1; pa.rate_gs = e->rate_per_gene ? e->K : 0;
   pa.label = label; pa.is_leaf = e->d_is_leaf.p; pa.branch = e->d_branch.p; pa.rate = e->d_rate.p;
   pa.gene_rate = e->d_gene_rate.p; pa.eigen_of = e->d_eigen_of.p; pa.qfactor = e->d_qfactor.p;
   pa.eigen = e->d_eigen.p; pa.n_chara = e->d_n_chara.p; pa.chara_map = e->d_chara_map.p; pa.plain_codes = e->plain_codes;
   pa.rowmajor = e->d_rowmajor.p; pa.pint = e->d_pint.p; pa.ptip = e->d_ptip.p; pa.tip_words = (long)tip_words(e);
   return pa;
}

// `prog` runs from `ops` over the tiles of the selected kernel or the 64-pattern / 256-pattern ones of the full interpreters, for K classes;
// keep-partials STOREs / LOADs and the scale factors go to `partials` / `scalef`.
PruneArgs prune_args(const paml_amd_engine *e, const Program &prog, int K, const Op *ops, bool full_tiles, int n_scale, bool keep, double *partials,
                     double *scalef, int overflow)
{
   const bool mfma = e->kk == KK_MFMA64;
   PruneArgs pr{};
   pr.ops = ops; pr.z = e->d_z.p; pr.z_stride = e->n_patt;
   pr.tiles = full_tiles ? e->d_tiles_full.p : e->d_tiles.p; pr.n_tiles = full_tiles ? e->n_tiles_full : e->n_tiles;
   pr.gene_off = e->d_gene_off.p; pr.weights = e->d_weights.p; pr.ztiles = e->d_ztiles.p; pr.zt_bytes = e->zt_bytes;
   pr.n = e->n; pr.n_tips = e->n_tips; pr.n_nodes = e->tree.n_nodes; pr.K = K; pr.n_genes = e->n_genes; pr.n_codes = e->n_codes;
   pr.cleandata = e->cleandata; pr.n_pi = e->n_pi; pr.mode = e->mode; pr.n_scale = n_scale; pr.keep = keep ? 1 : 0; pr.n_patt = e->n_patt;
   pr.pi = e->d_pi.p; pr.pint = mfma ? e->d_pint.p : e->d_rowmajor.p; pr.ptip = e->d_ptip.p;
   pr.fscale = e->d_fscale.p; pr.pcol = e->d_pcol.p;
   pr.fhK = e->d_fhK.p; pr.partials = partials; pr.scalef = scalef; pr.stack_scratch = e->d_stack.p;
   pr.stack_overflow_slots = overflow; pr.first_matmul = prog.first_matmul; pr.first_tip = prog.first_tip; pr.n_int = pr.n_nodes - e->n_tips;
   pr.tile_group0 = e->d_tile_group0.p; pr.part_groups = e->part_groups(); pr.code_mask = e->d_code_mask.p;
   pr.part_dump = (keep && mfma) ? partials + (size_t)K * pr.n_int * e->part_groups() * 1024 : nullptr;
   pr.stream = e->d_stream.p; pr.n_stream = (int)(e->prog.stream.size() / 2); pr.tip_words = (long)tip_words(e);
   pr.zpm = e->d_zpm.p; pr.zpm_words = e->zpm_words;
   return pr;
}

// ---- one evaluation, phase by phase (launch_eval, below, is the list) -----------------------------------------------------------------
namespace {

// The arguments of launch_eval and the locals its phases share; lives on launch_eval's stack.
struct Eval {
   const double *branch, *gene_rate;
   const unsigned char *clean; double *d_lnL_out; const BatchSpec *bs;
   bool want_lnf, want_pipe, want_fhk, slot_waited;
   int B, K, Km, G, psets;          // Km: classes of the model; K: classes the kernels see
   bool keep, new_prog, use_inline;
   bool pipe, dual, skip_entry;     // the fast path of consecutive eval_device calls; two pruning streams; nothing waits for this evaluation's entry event
   hipStream_t ms, ps;              // the stream of the pruning kernel and the partial sums; of the uploads and the P(t) kernel
   bool offload, side_total;        // the whole reduction / the (all-reduce and the) fixed-order total on the side stream `sc`
   int lane, slot;                  // two pruning streams: this evaluation's; its reduction slot
   int n_blocks, overflow;          // workgroups of the interpreters (tiles x classes); stack slots in global scratch
};

int begin_eval(paml_amd_engine *e, Eval &c)
{
   if (!(e->have_tips && e->have_tree && e->have_pi && e->have_classes))
      return fail(e, PAML_AMD_EINVAL, "eval before set_tips/set_tree/set_pi/set_classes");
   if (e->eigen.empty()) return fail(e, PAML_AMD_EINVAL, "eval before any set_eigen_*");
   c.keep = (e->flags & PAML_AMD_KEEP_PARTIALS) != 0;
   if (c.clean && (!c.keep || !e->partials_valid))
      return fail(e, PAML_AMD_EINVAL, "eval_dirty needs PAML_AMD_KEEP_PARTIALS and a previous full evaluation");
   c.B = c.bs ? c.bs->B : 1; c.Km = e->K; c.K = c.Km * c.B; c.G = e->n_genes; c.psets = c.G * c.K;
   if (c.B > 1 && (c.keep || c.clean)) return fail(e, PAML_AMD_EUNSUPPORTED, "eval_batch: not with PAML_AMD_KEEP_PARTIALS");
   // program (tree walk) — rebuilt when the tree or the clean set changes
   c.new_prog = !e->prog_valid || c.clean;
   if (c.new_prog) {
      e->prog = build_program(e->tree, c.keep, c.clean);
      e->prog_valid = (c.clean == nullptr);
      if (int rc = check_stack_depth(e, e->prog)) { e->prog_valid = false; return rc; }
   }
   return 0;
}

// The streams and events of a pipelined evaluation, and what its side stream has to wait for.
int setup_streams(paml_amd_engine *e, Eval &c)
{
   // the fast path of consecutive eval_device calls (see pipe_ok): nothing but branch lengths / gene rates may have changed
   // (worth its event traffic only where the pruning kernel is long: the 21..64-state kernels and the 20-state matrix-core kernel on
   //  >= 10^5 pattern-classes)
   c.want_pipe = c.want_pipe && (e->kk == KK_MFMA64 || (e->kk == KK_VALU20 && e->want_m20)) && (long)e->n_patt * e->K >= 100000;
   c.pipe = c.want_pipe && e->pipe_ok && !c.bs && !c.clean && !c.keep && !c.new_prog && !e->eigen_dirty;
   // Two pruning streams (paml_amd_engine::sb): from the second evaluation of such a run on, the evaluations alternate between the
   // engine's stream and `sb`, so that the persistent workgroups of evaluation i + 1 take the CUs as those of evaluation i leave
   // them — no kernel boundary, reduction or half-empty last round of tiles between two pruning kernels.  lane = reduction slot.
   c.dual = c.pipe && e->dual_ok && !e->profiling;
   c.lane = c.dual ? e->red_slot : 0;
   if (c.dual && c.lane && !e->sb[c.lane - 1]) HIPCHK(create_engine_stream(&e->sb[c.lane - 1]));
   if (c.dual)
      if (int rc = ensure_side_stream(e)) return rc;
   c.ms = c.lane ? e->sb[c.lane - 1] : e->stream;
   if (c.want_pipe && !e->s2) {
      for (DevEvent &ev : e->ev_setread) HIPCHK(ev.ensure(hipEventDisableTiming));
      for (int i = 0; i < paml_amd_engine::NPSET - 1; i++) e->spare[i].id = i + 1;
      HIPCHK(create_engine_stream(&e->s2));
      HIPCHK(e->ev_entry[0].ensure(hipEventDisableTiming));
      HIPCHK(e->ev_entry[1].ensure(hipEventDisableTiming));
      HIPCHK(e->ev_pmat.ensure(hipEventDisableTiming));
   }
   c.ps = e->stream;
   if (c.pipe) {
      // the side stream may overwrite the other P set once everything the main stream held in front of the PREVIOUS pruning
      // kernel is done: that set's last reader (the kernel before it), and the previous evaluation's own uploads and P(t)
      c.ps = e->s2;
      // (two pruning streams: only the run's first such evaluation — the uploads in front of the run; after that the side stream
      //  waits for nothing but the last reader of the set it is about to overwrite, four evaluations back)
      if (e->have_prev_entry && !(c.dual && e->dual_run)) HIPCHK(hipStreamWaitEvent(e->s2, e->ev_entry[e->entry_sel ^ 1], 0));
      const int nid = e->spare[e->spare_head].id;
      if (c.dual && e->setread_rec[nid]) HIPCHK(hipStreamWaitEvent(e->s2, e->ev_setread[nid], 0));
   }
   c.skip_entry = c.dual && e->dual_run;
   e->dual_run = c.dual;
   return 0;
}

// The small inputs: branch lengths and gene rates, the batch's class tables, the eigen table, the program.
int stage_inputs(paml_amd_engine *e, Eval &c, InlineVec &iv)
{
   const int B = c.B, Km = c.Km, G = c.G, nn = e->tree.n_nodes;
   const BatchSpec *const bs = c.bs;
   std::vector<EigenDev> tab;
   if (e->eigen_dirty)
      if (int rc = eigen_table(e, tab)) return rc;
   if (!(bs && bs->eigen_of))
      if (int rc = eigen_refs_ok(e, e->h_eigen_of.data(), e->h_eigen_of.size(), "eval")) return rc;

   // branch lengths and gene rates of a single evaluation ride in the kernel arguments of P(t) (InlineVec): no copy at all
   iv.n_branch = iv.n_rate = 0;
   c.use_inline = B == 1 && nn + G <= PMAT_INLINE_MAX;
   if (c.use_inline) {
      iv.n_branch = nn; iv.n_rate = G;
      memcpy(iv.v, c.branch, (size_t)nn * sizeof(double));
      for (int g = 0; g < G; g++) iv.v[nn + g] = c.gene_rate ? c.gene_rate[g] : 1.0;
   }
   // the other small inputs (and the batched ones) go through the pinned arena: async H2D, no host stall
   if (c.use_inline && !bs && tab.empty() && !c.new_prog) return 0;
   const size_t L = (size_t)e->n_labels;
   const size_t need = (size_t)B * nn * 8 + (size_t)B * G * 8 + tab.size() * sizeof(EigenDev) +
                       (bs ? (size_t)B * (G * Km * L * 4 + Km * L * 8 + 2 * Km * 8) + 64 : 0) +
                       (c.new_prog ? e->prog.ops.size() * sizeof(Op) + e->prog.stream.size() * sizeof(int) : 0) + 256;
   HIPCHK(e->stage.begin(need));
   DevBuf<double> &dbr = c.pipe ? e->d2_branch : e->d_branch, &dgr = c.pipe ? e->d2_gene_rate : e->d_gene_rate;   // (the side stream has its own)
   e->bl_gr_sent = false;
   HIPCHK(dbr.ensure((size_t)B * nn));
   HIPCHK(dgr.ensure((size_t)B * G));
   if (!c.use_inline) {
      const double *hb = e->stage.put(c.branch, (size_t)B * nn);
      HIPCHK(hipMemcpyAsync(dbr.p, hb, (size_t)B * nn * 8, hipMemcpyHostToDevice, c.ps));
      std::vector<double> gr((size_t)B * G, 1.0);
      if (c.gene_rate) gr.assign(c.gene_rate, c.gene_rate + (size_t)B * G);
      const double *hg = e->stage.put(gr.data(), gr.size());
      HIPCHK(hipMemcpyAsync(dgr.p, hg, gr.size() * 8, hipMemcpyHostToDevice, c.ps));
   }
   if (bs) {      // per-element class tables
      if (bs->eigen_of) {
         const size_t cnt = (size_t)B * G * Km * L;
         if (int rc = eigen_refs_ok(e, bs->eigen_of, cnt, "eval_batch")) return rc;
         HIPCHK(e->stage.send(e->d_b_eigen_of, bs->eigen_of, cnt, e->stream));
      }
      const double *src[3] = {bs->qfactor, bs->freqK, bs->rate};
      DevBuf<double> *dst[3] = {&e->d_b_qfactor, &e->d_b_freqK, &e->d_b_rate};
      const size_t cnt[3] = {(size_t)B * Km * L, (size_t)B * Km, (size_t)B * Km * (e->rate_per_gene ? G : 1)};
      for (int i = 0; i < 3; i++)
         if (src[i]) HIPCHK(e->stage.send(*dst[i], src[i], cnt[i], e->stream));
   }
   if (!tab.empty()) {
      HIPCHK(e->stage.send(e->d_eigen, tab.data(), tab.size(), e->stream));
      e->eigen_dirty = false;
   }
   if (c.new_prog) {
      HIPCHK(e->stage.send(e->d_ops, e->prog.ops.data(), e->prog.ops.size(), e->stream));
      HIPCHK(e->d_stream.ensure(e->prog.stream.size() + 2));
      if (!e->prog.stream.empty()) {
         const int *hs = e->stage.put(e->prog.stream.data(), e->prog.stream.size());
         HIPCHK(hipMemcpyAsync(e->d_stream.p, hs, e->prog.stream.size() * sizeof(int), hipMemcpyHostToDevice, e->stream));
      }
   }
   HIPCHK(e->stage.end(c.ps));
   return 0;
}

// Subtree tables (jit.h: SubtreeProgram): the classes of the tips + tree, the selection for this class count and these limits and what
// the builder and the walk read of it on the device — all of it only when one of them changed (Subtree::made_for: a handful of integers
// compared per evaluation), the classes only after set_tips / set_tree.  e->sub.sel is empty when nothing qualifies.
static std::string ckey_of(const paml_amd_engine *e, int K, int n, const std::string &pkey)
{
   return std::to_string(K) + "k" + std::to_string(n) + "m" + std::to_string(e->n_codes) + "c" + std::to_string(e->env.cherry_cap_mb) + ":" + pkey;
}
int ensure_subtree(paml_amd_engine *e, int K, int tp)
{
   paml_amd_engine::Subtree &sb = e->sub;
   // (cherry_gen: the cherry tables' own key — tree, class count, codes, their cap — changed)
   const paml_amd_engine::Subtree::Key key{e->tips_gen, e->tree_gen, e->cherry_gen, e->env.subtree_cap_mb, e->env.subtree_max_frac, K};
   if (sb.made_for == key) return 0;
   if (sb.d_nodes.p) HIPCHK(hipDeviceSynchronize());      // (a new selection: nothing may still read the previous one's tables and indices)
   const bool same_classes = sb.made_for.tips_gen == key.tips_gen && sb.made_for.tree_gen == key.tree_gen && sb.made_for.frac == key.frac;
   sb.made_for = key;
   sb.sel_gen++;
   const TreeDesc &t = e->tree;
   if (e->h_z.size() != (size_t)e->n_tips * e->n_patt) {      // (set_tips keeps the codes for the engines this form applies to)
      sb.sel.clear();
      sb.sp = SubtreeProgram();
      sb.made_for.tips_gen = -1;
      return 0;
   }
   if (!same_classes) {      // (the limit is part of the key: classes beyond it are not computed)
      const double lim_u = e->env.subtree_max_frac * (double)e->n_patt;
      SubtreeClasses sc = subtree_classes(e->n_tips, t.n_nodes, t.root, t.sons_ptr.data(), t.sons.data(), e->h_z.data(), (long)e->n_patt, (long)e->n_patt,
                                          e->n_codes, lim_u >= 4e9 ? ~0ull : (uint64_t)std::max(0.0, lim_u));
      sb.u.swap(sc.u); sb.done.swap(sc.done); sb.cls.swap(sc.cls); sb.son_cls.swap(sc.son_cls);
      for (int v = 0; v < t.n_nodes; v++)      // (a cherry's classes are ca * n_codes + cb: nothing reads the array again — 8 of the headline's 13)
         if (sc.cherry[v]) std::vector<unsigned int>().swap(sb.cls[v]);
      sb.n_computed++;
   }
   sb.sel = jit_subtree_select(t, e->cherry.tabs, sb.u, sb.done, e->n_patt, e->env.subtree_max_frac, (size_t)e->env.subtree_cap_mb << 20, K);
   sb.sp = SubtreeProgram();
   sb.rows = 0;
   for (int v : sb.sel)      // (what the builder reads per class: two son rows)
      if (sb.son_cls[v].size() != 2 * (size_t)sb.u[v]) { sb.sel.clear(); break; }
   if (sb.sel.empty()) return 0;
   sb.sp = jit_subtree_program(e->prog, e->cherry_n, t, sb.sel);
   if (sb.sp.top.empty() || !jit_subtree_zfits(e->n_tips, (int)sb.sp.top.size(), tp)) {      // (the index rows must leave room for two code blocks)
      sb.sel.clear();
      sb.sp = SubtreeProgram();
      return 0;
   }
   // the builder's nodes, level by level (sel keeps the order of the report: ascending u), and their classes' rows at the sons
   const int ns = (int)sb.sp.sub.size();
   std::vector<int> row0(ns), by_level;
   for (int i = 0; i < ns; i++) { row0[i] = (int)sb.rows; sb.rows += sb.u[sb.sp.sub[i].node]; }
   sb.level_first.clear();
   sb.level_tiles.clear();
   sb.level_small.clear();
   for (int l = 0; l < sb.sp.levels; l++) {
      sb.level_first.push_back((int)by_level.size());
      int tiles = 0;
      bool tip_son = false;
      for (int i = 0; i < ns; i++)
         if (sb.sp.sub[i].level == l) {
            by_level.push_back(i);
            tiles = std::max(tiles, (int)((sb.u[sb.sp.sub[i].node] + 127) / 128));
            tip_son = tip_son || sb.sp.sub[i].l.kind == 0 || sb.sp.sub[i].r.kind == 0;
         }
      sb.level_tiles.push_back(tiles);
      sb.level_small.push_back(tip_son ? 0 : 1);
   }
   sb.level_first.push_back((int)by_level.size());
   // rows in son order (unless PAML_AMD_SUBTREE_ROWS=0): class c of a table sits at the rank of (left son row, right son row) — sons
   // before fathers, so a father sorts by its sons' final rows — and a builder tile's gathers, and a sorted walk's, land on neighbouring
   // rows.  A row's bits do not depend on where it is stored; the classes themselves (sb.cls, the report) keep their numbering.
   sb.rowmap.assign(ns, std::vector<unsigned int>());
   std::vector<std::vector<unsigned int>> son_rows(ns);      // [2][u] by ROW of the table, the sons as rows of theirs
   for (int i = 0; i < ns; i++) {
      const SubtreeTab &st = sb.sp.sub[i];
      const size_t u = sb.u[st.node];
      const std::vector<unsigned int> &sc = sb.son_cls[st.node];
      std::vector<unsigned int> l(sc.begin(), sc.begin() + u), r(sc.begin() + u, sc.end());
      if (st.l.kind == 2 && !sb.rowmap[st.l.id].empty()) for (unsigned int &x : l) x = sb.rowmap[st.l.id][x];
      if (st.r.kind == 2 && !sb.rowmap[st.r.id].empty()) for (unsigned int &x : r) x = sb.rowmap[st.r.id][x];
      son_rows[i].resize(2 * u);
      if (e->env.subtree_rows) {
         std::vector<unsigned int> by(u);
         for (size_t c = 0; c < u; c++) by[c] = (unsigned int)c;
         std::sort(by.begin(), by.end(), [&](unsigned int a, unsigned int b) { return l[a] != l[b] ? l[a] < l[b] : (r[a] != r[b] ? r[a] < r[b] : a < b); });
         sb.rowmap[i].resize(u);
         for (size_t row = 0; row < u; row++) { sb.rowmap[i][by[row]] = (unsigned int)row; son_rows[i][row] = l[by[row]]; son_rows[i][u + row] = r[by[row]]; }
      }
      else { std::copy(l.begin(), l.end(), son_rows[i].begin()); std::copy(r.begin(), r.end(), son_rows[i].begin() + u); }
   }
   std::vector<SubtreeNodeDev> nodes(ns);
   std::vector<unsigned int> sidx;
   for (int k = 0; k < ns; k++) {
      const SubtreeTab &st = sb.sp.sub[by_level[k]];
      SubtreeNodeDev &nd = nodes[k];
      nd.node = st.node; nd.u = (int)sb.u[st.node]; nd.row0 = row0[by_level[k]];
      nd.lkind = st.l.kind; nd.lid = st.l.kind == 2 ? row0[st.l.id] : st.l.id;
      nd.rkind = st.r.kind; nd.rid = st.r.kind == 2 ? row0[st.r.id] : st.r.id;
      nd.pad = 0;
      nd.sidx = (long)sidx.size();
      sidx.insert(sidx.end(), son_rows[by_level[k]].begin(), son_rows[by_level[k]].end());      // [2][u]
   }
   std::vector<int> meta;
   for (int ti : sb.sp.top) { meta.push_back(row0[ti]); meta.push_back((int)sb.u[sb.sp.sub[ti].node]); }
   HIPCHK(upload(sb.d_nodes, nodes.data(), nodes.size(), e->stream));
   HIPCHK(upload(sb.d_sidx, sidx.data(), sidx.size(), e->stream));
   HIPCHK(upload(sb.d_meta, meta.data(), meta.size(), e->stream));
   HIPCHK(hipStreamSynchronize(e->stream));
   return 0;
}

// The tile blocks of the kernel with subtree tables: the current 128-pattern tile table's, with the class-index rows of the walk's lookups.
// Unless PAML_AMD_SUBTREE_ORDER=0 a tile holds the patterns order[first .. first + 127] of subtree_pattern_order (subtree_classes.h) over the
// classes of all the walk's lookups — subtree tables and cherry tables alike —, computed here once per selection, never per evaluation.
int ensure_subtree_ztiles(paml_amd_engine *e)
{
   paml_amd_engine::Subtree &sb = e->sub;
   if (sb.zt_sel_gen == sb.sel_gen && sb.zt_tiles == e->n_tiles && sb.zt_tile_patt == e->tile_patt) return 0;
   const int n_top = (int)sb.sp.top.size();
   std::vector<unsigned int> top((size_t)n_top * e->n_patt);
   for (int k = 0; k < n_top; k++) {
      const std::vector<unsigned int> &c = sb.cls[sb.sp.sub[sb.sp.top[k]].node], &rm = sb.rowmap[sb.sp.top[k]];
      if (rm.empty()) std::copy(c.begin(), c.end(), top.begin() + (size_t)k * e->n_patt);
      else for (long h = 0; h < e->n_patt; h++) top[(size_t)k * e->n_patt + h] = rm[c[h]];
   }
   sb.ordered = e->env.subtree_order != 0;
   if (sb.ordered && sb.order_sel_gen != sb.sel_gen) {
      const auto t0 = std::chrono::steady_clock::now();
      std::vector<const unsigned int *> keys;
      std::vector<unsigned int> bound;
      for (int k = 0; k < n_top; k++) { keys.push_back(top.data() + (size_t)k * e->n_patt); bound.push_back(sb.u[sb.sp.sub[sb.sp.top[k]].node]); }
      std::vector<std::vector<unsigned int>> cherry_cls;      // the walk's cherry lookups: row ca * n_codes + cb
      for (const Op &o : sb.sp.prog.ops)
         if (o.code == OP_LOOKUP && o.c < SUBTREE_TAB_BASE) {
            const CherryTab &ct = sb.sp.tabs[o.c];
            const unsigned char *za = e->h_z.data() + (size_t)ct.tip_a * e->n_patt, *zb = e->h_z.data() + (size_t)ct.tip_b * e->n_patt;
            cherry_cls.emplace_back(e->n_patt);
            for (long h = 0; h < e->n_patt; h++) cherry_cls.back()[h] = (unsigned int)za[h] * e->n_codes + zb[h];
         }
      for (const std::vector<unsigned int> &c : cherry_cls) { keys.push_back(c.data()); bound.push_back((unsigned int)(e->n_codes * e->n_codes)); }
      const std::vector<unsigned int> order = subtree_pattern_order(keys, bound, subtree_order_sequence(bound, e->env.subtree_order == 2), (long)e->n_patt);
      sb.order_host_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
      HIPCHK(upload(sb.d_order, (const int *)order.data(), order.size(), e->stream));
      HIPCHK(hipStreamSynchronize(e->stream));
      sb.h_order = order;      // (kept for the gathering walk's tiles, which are cut along it)
      sb.order_sel_gen = sb.sel_gen;
      sb.n_order_computed++;
   }
   sb.zt_bytes = jit_zpieces(jit_subtree_zrows(e->n_tips, n_top), e->tile_patt) * 2048;
   HIPCHK(upload(sb.d_top_cls, top.data(), top.size(), e->stream));
   HIPCHK(sb.d_ztiles.ensure((size_t)e->n_tiles * sb.zt_bytes));
   hipLaunchKernelGGL(sztile_kernel, dim3(e->n_tiles), dim3(e->tile_patt), 0, e->stream, e->d_tiles.p, e->d_gene_off.p, e->d_z.p, (long)e->n_patt, e->d_weights.p,
                      e->n_tips, sb.zt_bytes, sb.d_ztiles.p, n_top, sb.d_top_cls.p, sb.ordered ? sb.d_order.p : nullptr);
   HIPCHK(hipStreamSynchronize(e->stream));
   sb.d_top_cls.release();
   sb.zt_sel_gen = sb.sel_gen; sb.zt_tiles = e->n_tiles; sb.zt_tile_patt = e->tile_patt;
   return 0;
}

// The gathering walk (kernels_prune.h: gather_walk_kernel) serves a table form that is lookups, their multiplications into the stack slot
// and the root only: two to four lookups, no operand block, no rescaling.  PAML_AMD_GATHER_WALK=0 keeps the generated walk (read per
// evaluation: the tests flip it on one engine); the generated kernel is acquired either way.
static bool gather_walk_wanted()
{
   const char *v = getenv("PAML_AMD_GATHER_WALK");
   return !v || atoi(v) != 0;
}
static void gather_walk_plan(paml_amd_engine *e)
{
   paml_amd_engine::Subtree &sb = e->sub;
   if (sb.gw_plan_gen == sb.sel_gen) return;
   sb.gw_plan_gen = sb.sel_gen;
   sb.gw_ok = false;
   sb.gw_nlk = 0;
   const Program &p = sb.sp.prog;
   if (!p.stream.empty() || e->tree.n_scale || e->n_pi != 1 || e->n_genes != 1 || e->h_wflag.size() != (size_t)e->n_patt) return;
   // the shape: the first lookup is pushed to a stack slot; every later one pops that slot — jit_mul(lookup, slot) — and is pushed there
   // again, but the last, which stays the partial the root reads
   bool have_cur = false, rooted = false;
   int n = 0, slot = -1;
   for (const Op &o : p.ops) {
      if (o.code == OP_END) break;
      if (o.code == OP_ROOT) {
         if (!have_cur || rooted) return;
         rooted = true;
         continue;
      }
      if (o.code != OP_LOOKUP || rooted || have_cur || n == GATHER_MAX_LOOKUPS) return;
      const int pop = mm_pop_slot(o), push = mm_push_slot(o);
      if (n == 0 ? (pop >= 0 || push < 0) : (pop != slot || (push >= 0 && push != slot))) return;
      if (n == 0) slot = push;
      have_cur = push < 0;
      const bool sub = o.c >= SUBTREE_TAB_BASE;
      const long rows = sub ? (long)sb.u[sb.sp.sub[sb.sp.top[o.c - SUBTREE_TAB_BASE]].node] : (long)e->n_codes * e->n_codes;
      if (rows < 1 || rows * (long)CHERRY_ROW_BYTES >= (1L << 31)) return;      // (a row's byte offset is a 32-bit buffer offset)
      sb.gw_kind[n] = sub ? 0 : 1; sb.gw_id[n] = sub ? o.c - SUBTREE_TAB_BASE : o.c;
      n++;
   }
   if (!rooted || n < 2) return;
   sb.gw_nlk = n;
   sb.gw_ok = true;
}

// Its tiles (gather_tiles.h): cut along the pattern order the tile blocks of the generated walk use, laid out and uploaded once per
// selection — so only after set_tips, set_tree or a new selection —, when the switch first asks for them.
int ensure_gather_tiles(paml_amd_engine *e)
{
   paml_amd_engine::Subtree &sb = e->sub;
   gather_walk_plan(e);
   if (!sb.gw_ok) return 0;
   const int R = e->env.gather_R;
   if (sb.gw_sel_gen == sb.sel_gen && sb.gw_R == R && sb.gw_ordered == sb.ordered) return 0;
   if (sb.d_gw_desc.p) HIPCHK(hipDeviceSynchronize());      // (nothing may still read the previous selection's blocks)
   const auto t0 = std::chrono::steady_clock::now();
   const long np = e->n_patt;
   std::vector<std::vector<unsigned int>> cls(sb.gw_nlk, std::vector<unsigned int>(np));
   std::vector<const unsigned int *> keys;
   std::vector<unsigned int> bound;
   for (int k = 0; k < sb.gw_nlk; k++) {
      if (sb.gw_kind[k] == 0) {      // the pattern's class at the tabulated node, as a row of its table, clamped as jit_lookup_row clamps
         const int ti = sb.sp.top[sb.gw_id[k]];
         const std::vector<unsigned int> &c = sb.cls[sb.sp.sub[ti].node], &rm = sb.rowmap[ti];
         const unsigned int u = sb.u[sb.sp.sub[ti].node];
         for (long h = 0; h < np; h++) cls[k][h] = std::min(rm.empty() ? c[h] : rm[c[h]], u - 1);
         bound.push_back(u);
      }
      else {      // a cherry table's row ca * n_codes + cb, the codes clamped as jit_lookup_nc clamps them
         const CherryTab &ct = sb.sp.tabs[sb.gw_id[k]];
         const unsigned char *za = e->h_z.data() + (size_t)ct.tip_a * np, *zb = e->h_z.data() + (size_t)ct.tip_b * np;
         const unsigned int nc = (unsigned int)e->n_codes;
         for (long h = 0; h < np; h++) cls[k][h] = std::min((unsigned int)za[h], nc - 1) * nc + std::min((unsigned int)zb[h], nc - 1);
         bound.push_back(nc * nc);
      }
      keys.push_back(cls[k].data());
   }
   const bool ordered = sb.ordered && sb.h_order.size() == (size_t)np;
   const unsigned int *order = ordered ? sb.h_order.data() : nullptr;
   const GatherTiles g = gather_tiles(keys, bound, order, np, R);
   const std::vector<unsigned char> blocks = gather_tiles_pack(g, order, e->h_wflag.data(), np);
   sb.gw_host_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
   HIPCHK(upload(sb.d_gw_desc, blocks.data(), blocks.size(), e->stream));
   HIPCHK(hipStreamSynchronize(e->stream));
   sb.gw_tiles = (long)g.n_tiles(); sb.gw_rows = g.total_rows(); sb.gw_R = R; sb.gw_sel_gen = sb.sel_gen; sb.gw_ordered = sb.ordered;
   sb.gw_computed++;
   return 0;
}

// The pruning kernel of this evaluation: every obtain_kernel call of an evaluation and the tile tables.  Nonzero (*out untouched) only
// under PAML_AMD_JIT_STRICT or when the tile tables cannot be built.  21..64 states:
//   jit    — straight-line kernel specialised for this tree (jit.h), 128 patterns per workgroup
//   stream — the interpreter over the same operand stream (lean programs only), 128 patterns per workgroup
//   gather — the full interpreter (keep-partials STORE/LOAD, deep stacks, > MFMA_ZT tips, > 64 codes), 64 per workgroup
//   coop, coopjit — small data sets, below
int choose_kernel(paml_amd_engine *e, const Eval &c, PruneKernel *out)
{
   const int n = e->n, Km = c.Km, G = c.G;
   if (e->kk == KK_MFMA64) {
      bool lean = e->prog.max_stack <= MFMA_RS && e->n_tips <= MFMA_ZT && e->n_codes <= 64;
      // small data sets (at most a quarter of the CUs get a 128-pattern tile): the 64-pattern workgroups of the gather kernel —
      // one wave per SIMD, twice as many workgroups — finish a tile in 0.63 of the time (13 taxa x 79 codon patterns: 42 against 66 us,
      // a batched gradient of 25 evaluations 0.125 against 0.151 ms; profiles/r02_small_latency.jsonl)
      if ((e->n_patt + 127) / 128 <= e->n_cu / 4) lean = false;
      for (const Op &o : e->prog.ops)
         if (o.code == OP_PUSH || o.code == OP_SCALE || o.code == OP_STORE || o.code == OP_LOAD) lean = false;
      bool jit_ok = false;
      // waves per workgroup of the per-tree kernel: 8 (two per SIMD, 128 patterns per tile).  The three-per-SIMD variant (192-pattern
      // tiles, <= 168 VGPRs) measured SLOWER on MI355X (1.659 against 1.622 ms at C4, 4.73 against 4.63 ms with three classes — 40
      // spilled dwords and a third more LDS / DMA traffic per step) and was removed
      const int jw = 8;
      // (more than 64 codes: the per-tree kernel sums the rows of a code's states in ascending order — e->amb_ascending, set_tips — from
      //  the rows of the codes 0 .. n-1, which must be the single states — e->plain_codes >= n)
      // LOAD programs (paml_amd_eval_dirty: one per set of clean nodes) get a kernel too (round 6) — compiled on the worker thread from the
      // SECOND time a set is asked for (minbranches' walk repeats its sets cycle after cycle; a set seen once is not worth 0.5 s of compiler),
      // the interpreter serving meanwhile; code-block pieces follow one program's order, so trees beyond 207 tips keep the interpreter there
      bool has_load = false;
      for (const Op &o : e->prog.ops) has_load = has_load || o.code == OP_LOAD;
      e->n_ctab = 0;
      e->n_stab = 0;
      if (e->jit_enabled && !(has_load && e->n_tips > 207) && (e->n_codes <= 64 || (e->amb_ascending && e->plain_codes >= n)) && jit_supported(e->prog, e->n_tips, e->n_codes, e->n_pi, 6, jw * 16, true)) {
         const std::string pkey = jit_program_key(e->prog, e->n_tips);
         std::string key = "m" + std::to_string(n) + "c" + std::to_string(e->n_codes) + "w" + std::to_string(jw) + ":" + pkey;
         // Cherry tables (jit.h: OP_LOOKUP): one gene and frequency vector, single evaluations of the whole tree, enough patterns for the
         // builder's launch to pay (EnvCfg), as many cherries, in program order, as the cap on table bytes leaves room for
         int n_tab = 0;
         if (e->env.cherry_tables != 0 && G == 1 && e->n_pi == 1 && c.B == 1 && !c.keep && !c.clean && !has_load &&
             (e->env.cherry_tables == 1 || e->n_patt >= e->env.cherry_min_patt)) {
            const std::string ckey = ckey_of(e, c.K, n, pkey);
            if (e->cherry_key != ckey) {      // (a new tree, class count or code table: the count and the table form once)
               e->cherry_n = jit_cherry_count(e->prog, e->n_tips, n, e->n_codes, c.K, (size_t)e->env.cherry_cap_mb << 20, jw * 16);
               e->cherry = e->cherry_n ? jit_cherry_program(e->prog, e->cherry_n) : CherryProgram();
               e->cherry_key = ckey;
               e->cherry_gen++;
            }
            n_tab = e->cherry_n;
         }
         // Subtree tables above them (jit.h: SubtreeProgram): wherever cherry tables run, unless PAML_AMD_SUBTREE_TABLES=0
         if (n_tab && e->env.subtree_tables != 0) {
            if (int r = ensure_subtree(e, c.K, jw * 16)) return r;
            if (!e->sub.sel.empty()) {
               std::string skey = "s";
               for (int v : e->sub.sel) skey += std::to_string(v) + ".";
               skey += "t" + std::to_string(n_tab) + key;
               const bool ordered = e->env.subtree_order != 0;      // (the walk stores at order[position]: another kernel)
               if (ordered) skey = "o" + skey;
               bool ok = false;
               const int n_top = (int)e->sub.sp.top.size();
               if (int r = obtain_kernel(e, e->jit_slot, &e->jit, true, skey, [&]() { return jit_generate(e->sub.sp.prog, e->n_tips, n, e->n_codes, &e->sub.sp.tabs, n_top, ordered); },
                                         (e->prog.ops.size() > 120 && !e->jit_forced && !e->env.jit_sync) ? JIT_WAIT_WORKER : JIT_WAIT_CALLER, "tree, subtree tables", &ok)) return r;
               if (ok) { jit_ok = true; e->n_ctab = n_tab; e->n_stab = (int)e->sub.sel.size(); }
            }
         }
         if (n_tab && !jit_ok) {
            const std::string tkey = "t" + std::to_string(n_tab) + key;
            bool ok = false;
            if (int r = obtain_kernel(e, e->jit_slot, &e->jit, true, tkey, [&]() { return jit_generate(e->cherry.prog, e->n_tips, n, e->n_codes, &e->cherry.tabs); },
                                      (e->prog.ops.size() > 120 && !e->jit_forced && !e->env.jit_sync) ? JIT_WAIT_WORKER : JIT_WAIT_CALLER, "tree, cherry tables", &ok)) return r;
            if (ok) { jit_ok = true; e->n_ctab = n_tab; }
         }
         // Large trees (> 120 ops: roughly more than 35 taxa): tens of thousands of instructions, many seconds of compiler time.  Unless the
         // caller asked to wait (PAML_AMD_JIT flag / PAML_AMD_JIT_SYNC), the kernel is built on a worker thread while the interpreter kernels
         // serve, and the engine changes over when the code object is there; one found on disk is loaded at once.  Round 5: the generator
         // cuts such a walk into basic blocks (jit_split_mode), which is what the hardware wants and makes the full build as quick as the
         // build without the three passes that are quadratic on one giant block — the two-stage build of rounds before (a quick kernel at
         // 0.63 of the FP64 peak first, the full one after) went with that.
         const bool big = e->prog.ops.size() > 120;
         const bool background = (big || has_load) && !e->jit_forced && !e->env.jit_sync;
         const bool wanted = !has_load || e->jit_forced || e->env.jit_sync || e->jit_recall(key) || e->jit_count_request(key) >= 2;
         if (wanted && !jit_ok)      // (also while the table form is still being compiled, or when it could not be)
            if (int r = obtain_kernel(e, e->jit_slot, &e->jit, true, key, [&]() { return jit_generate(e->prog, e->n_tips, n, e->n_codes); },
                                      background ? JIT_WAIT_WORKER : JIT_WAIT_CALLER, "tree", &jit_ok)) return r;
      }
      const bool big_tiles = jit_ok || lean;
      const int want_waves = jit_ok ? jw : (lean ? DMA_WAVES : GATHER_WAVES);
      if (int r = select_tiles(e, big_tiles, want_waves, jit_ok)) return r;
      if (e->n_stab)
         if (int r = ensure_subtree_ztiles(e)) return r;
      if (e->n_stab && jit_ok && gather_walk_wanted() && e->env.prof_ops.empty() && !e->env.prof_tiles)
         if (int r = ensure_gather_tiles(e)) return r;
      if (jit_ok || e->mfma_dma) {
         *out = jit_ok ? PK_MFMA64_JIT : PK_MFMA64_STREAM;
         return 0;
      }
      // Small data sets on the 21..64-state interpreters: every 16-pattern group can have a CU (ONE round: the kernels' LDS leaves room for
      // one workgroup per CU, and two rounds of a 25 us walk lose to one round of the gather kernel's 39) — four waves per group
      // (prune_mfma64_coop), and once the tree's own kernel is there, that one with the reduction inside (jit_generate_coop: one launch
      // after P(t) per evaluation).  Single engines only: with pattern shards the chunk sums go through the exchange step.
      bool coop = !c.keep && !c.clean && !e->env.no_coop && e->tile_patt == 64 && e->prog.max_stack <= COOP_SLOTS &&
                  (long)e->n_tiles * 4 * c.K <= (long)e->n_cu && !e->env.prof_ops.size();
      bool coopj = false;
      for (const Op &o : e->prog.ops) coop = coop && o.code != OP_STORE && o.code != OP_LOAD && o.code != OP_EXPORT;
      if (coop && e->coopj_enabled && !e->comm && e->nb_global == (e->n_patt + e->chunk - 1) / e->chunk && e->first_chunk == 0 &&
          jit_coop_supported(e->prog, e->n_tips, e->n_codes)) {
         const std::string key = "cj" + std::to_string(n <= 32 ? n : 64) + ":" + jit_program_key(e->prog, e->n_tips);
         if (int r = obtain_kernel(e, e->coop_slot, &e->jit_coop, false, key, [&]() { return jit_generate_coop(e->prog, e->n_tips, n); },
                                   (e->jit_forced || e->env.jit_sync) ? JIT_WAIT_CALLER : JIT_WAIT_WORKER, "coop", &coopj)) return r;
      }
      *out = coopj ? PK_MFMA64_COOPJIT : (coop ? PK_MFMA64_COOP : PK_MFMA64_GATHER);
      return 0;
   }
   // 4 / 5 / 20 states: the interpreter unrolled for this tree
   bool jit_ok = false, second = false;      // second: the fused form (4 / 5 states), the matrix-core form (20)
   // (20 states: the unrolled walk needs > 256 VGPRs and runs at one wave per SIMD, slower than the interpreter)
   if (e->jit_enabled && !c.keep && n <= 5 && jit_valu_supported(e->prog)) {
      // the fused form (classes inside, LDS tip tables, reduction in the epilogue) when the model fits it
      const ValuFusedPlan pl = jit_valu_fused_plan(e->prog, n, e->n_tips, e->n_codes, Km, e->chunk);
      // Several genes (round 6): the fused form exists (jit_generate_valu_fused with G > 1: one gene's tables at a time, refilled where a
      // workgroup's chunks cross into the next gene; same bits) and is NOT the default: on MI355X it measures no faster than the unfused
      // kernel + reduce_stage1, which serve genes for free — a workgroup is one (tile, class) there — 32 taxa x 10^5 patterns x Gamma-4 in 4
      // genes: one evaluation 0.050 ms fused against 0.030 unfused, a gradient's 122 evaluations in one launch 1.77 against 1.77 ms (one
      // gene, fused: 0.029 / 1.33).  Why the several-genes form of the same inner loop runs 1.6 x slower than the one-gene form OUTSIDE
      // the profiler (within 4 % of it under rocprofv3, equal instruction counts) was bisected to the table fill living inside the
      // chunk loop and not resolved: profiles/r06_genes_4state.txt.  PAML_AMD_VF_GENES=1 switches it on (tests, measurements).
      const bool vf_genes = getenv("PAML_AMD_VF_GENES") && atoi(getenv("PAML_AMD_VF_GENES")) != 0;      // (read per call: tests switch it)
      if (pl.ok && (G == 1 ? e->n_pi == 1 : (vf_genes && (e->n_pi == 1 || e->n_pi == G))) && e->d_zpm.p && G <= 64) {
         // (4 states: a matrix-core form (v_mfma_f64_4x4x4) was correct but slower, 0.32 of peak against 0.64: profiles/r02_valu_fused_shapes.txt)
         int r = obtain_kernel(e, e->jit_slot, &e->jit, true, std::string("vf") + std::to_string(n) + "c" + std::to_string(e->n_codes) + "k" + std::to_string(Km) + "r" + std::to_string(pl.R) + "w" +
                                     std::to_string(pl.CW) + (pl.cherry ? "y" : "n") + (G > 1 ? "g" + std::to_string(G) + ":" : ":") + jit_program_key(e->prog, e->n_tips),
                               [&]() { return jit_generate_valu_fused(e->prog, n, e->n_tips, e->n_codes, Km, e->chunk, G); }, JIT_WAIT_CALLER, "valu fused", &jit_ok);
         if (r) return r;
         second = jit_ok;
         e->fused_threads = 256 * pl.CW;
      }
      if (!jit_ok) {
         int r = obtain_kernel(e, e->jit_slot, &e->jit, true, "v" + std::to_string(n) + ":" + jit_program_key(e->prog, e->n_tips),
                               [&]() { return jit_generate_valu(e->prog, n); }, JIT_WAIT_CALLER, "valu", &jit_ok);
         if (r) return r;
      }
   }
   if (e->want_m20 && !c.clean && jit_m20_supported(e->prog, e->n_tips, G)) {
      int r = obtain_kernel(e, e->jit_slot, &e->jit, true, std::string("m20c") + std::to_string(e->n_codes) + (G > 1 ? "g:" : ":") + jit_program_key(e->prog, e->n_tips),
                            [&]() { return jit_generate_m20(e->prog, e->n_tips, e->n_codes, G > 1 ? 2 : 1); }, JIT_WAIT_CALLER, "m20", &jit_ok);
      if (r) return r;
      second = jit_ok;
   }
   *out = PruneKernel(3 * e->kk + (second ? 2 : (jit_ok ? 1 : 0)));
   return 0;
}

// The buffers whose size follows from the choice: P(t) (pipelined: the set the previous evaluation did not use), class likelihoods,
// the resident partials of a keep-partials engine, the overflow stack of deep trees.
int ensure_buffers(paml_amd_engine *e, Eval &c)
{
   if (c.pipe) {
      paml_amd_engine::PSet &sp = e->spare[e->spare_head];      // the set used longest ago
      std::swap(e->d_rowmajor, sp.rowmajor); std::swap(e->d_pint, sp.pint); std::swap(e->d_ptip, sp.ptip); std::swap(e->d_pcol, sp.pcol);
      std::swap(e->d_ctab, sp.ctab);
      std::swap(e->d_stab, sp.stab);
      std::swap(e->pset, sp.id);
      e->spare_head = (e->spare_head + 1) % (paml_amd_engine::NPSET - 1);
   }
   if (int rc = ensure_pmat_buffers(e, c.psets, e->kk == KK_VALU20 && e->want_m20, e->kk == KK_MFMA64)) return rc;
   if (e->kernel != PK_MFMA64_JIT) e->n_ctab = e->n_stab = 0;
   e->last_stab_n = e->n_stab;
   e->last_stab_bytes = e->n_stab ? (long)((size_t)c.K * e->sub.rows * CHERRY_ROW_BYTES) : 0;
   e->last_stab_blocks = e->n_stab ? (long)(e->sub.sp.prog.stream.size() / 2) : -1;
   if (e->n_stab) HIPCHK(e->d_stab.ensure((size_t)e->last_stab_bytes / sizeof(double)));
   e->last_ctab_n = e->n_ctab;
   e->last_ctab_bytes = (long)((size_t)c.K * e->n_ctab * cherry_table_bytes(e->n_codes));
   if (e->n_ctab) HIPCHK(e->d_ctab.ensure((size_t)e->last_ctab_bytes / sizeof(double)));
   HIPCHK(e->d_fhK.ensure((size_t)c.K * e->n_patt));
   c.n_blocks = e->n_tiles * c.K;
   if (c.keep) {
      const int n_int = e->tree.n_nodes - e->n_tips;
      size_t words = e->kk == KK_MFMA64 ? (size_t)c.K * n_int * e->part_groups() * 1024 + (size_t)std::max(e->mfma_waves, 8) * 1024      // (+ PruneArgs::part_dump: a row per wave)
                                        : (size_t)c.K * n_int * e->n_patt * e->n;
      HIPCHK(e->d_partials.ensure(words));
      HIPCHK(e->d_scalef.ensure((size_t)c.K * std::max(1, e->tree.n_scale) * e->n_patt));
   }
   return stack_overflow(e, e->prog, c.n_blocks, e->mfma_waves, &c.overflow);
}

// Kernel A: batched P(t), and the events that order the pruning kernel behind it.
int run_pmat(paml_amd_engine *e, Eval &c, const InlineVec &iv)
{
   const int B = c.B, Km = c.Km, G = c.G, nn = e->tree.n_nodes;
   const BatchSpec *const bs = c.bs;
   // (layout 2 — 20 states on the matrix cores: operand-order copies beside the row-major matrices)
   PmatArgs pa = pmat_args(e, e->tree.root, e->d_label.p, e->kk == KK_MFMA64 ? 1 : (e->kernel == PK_MFMA4X20_JIT ? 2 : 0),
                           e->kk == KK_MFMA64 ? e->d_pcol.p : nullptr);
   if (c.pipe) { pa.branch = e->d2_branch.p; pa.gene_rate = e->d2_gene_rate.p; }
   pa.B = B; pa.branch_bs = nn; pa.gene_rate_bs = G;
   if (bs && bs->eigen_of) { pa.eigen_of = e->d_b_eigen_of.p; pa.eigen_of_bs = (long)G * Km * e->n_labels; }
   if (bs && bs->qfactor) { pa.qfactor = e->d_b_qfactor.p; pa.qfactor_bs = (long)Km * e->n_labels; }
   // (several nodes per workgroup in a run of evaluations: 20 states no faster, 61 states slower, 0.211 against 0.203 ms at the 8-GPU shard size)
   pa.npb = 1;
   if (bs && bs->rate) { pa.rate = e->d_b_rate.p; pa.rate_bs = e->rate_per_gene ? (long)G * Km : Km; }
   const bool pmat_mfma = pmat_on_matrix_cores(e, pa);
   // ... on the matrix cores in the mfma64 layout nobody reads the row-major copy (paml_amd_get_pmat rebuilds P from the operand-order ones)
   if (pmat_mfma && pa.layout == 1) pa.rowmajor = nullptr;
   e->rowmajor_valid = pa.rowmajor != nullptr;
   e->pmat_B = B;
   // ... and single evaluations get label -> eigen_of -> eigen set -> U / V / Root resolved on the host (PmatArgs::res)
   if (pmat_mfma && !bs && c.use_inline && !e->rate_per_gene && !e->eigen.empty()) {
      if (!e->pres_valid) {
         std::vector<PmatRes> res((size_t)c.psets * nn);
         for (int g = 0; g < G; g++)
            for (int ir = 0; ir < Km; ir++)
               for (int v = 0; v < nn; v++) {
                  const int lab = e->tree.label.empty() ? 0 : e->tree.label[v];
                  const EigenHost &h = e->eigen[e->h_eigen_of[((size_t)g * Km + ir) * e->n_labels + lab]];
                  res[((size_t)g * Km + ir) * nn + v] = PmatRes{h.U.p, h.V.p, h.Root.p, e->class_rate[ir], e->h_qfactor[(size_t)ir * e->n_labels + lab],
                                                                e->tree.is_leaf(v) ? 1 : 0, 0};
               }
         HIPCHK(e->d_pres.ensure(res.size()));
         // (pageable source: staged by the runtime before the call returns; in stream order in front of the P(t) kernel)
         HIPCHK(hipMemcpyAsync(e->d_pres.p, res.data(), res.size() * sizeof(PmatRes), hipMemcpyHostToDevice, c.ps));
         e->pres_valid = true;
      }
      pa.res = e->d_pres.p;
   }
   mark_on(e, c.ps);
   bool small_pmat = e->kk != KK_MFMA64 && e->n <= 5;
   for (const EigenHost &h : e->eigen) small_pmat = small_pmat && h.kind != PAML_AMD_EIGEN_QMAT;      // (ids never set: kind < 0, fine)
   launch_pmat(pa, iv, nn, c.psets, small_pmat, c.ps, pmat_mfma);
   if (e->n_ctab) {      // the cherry tables of this P(t): behind it, on its stream
      CherryTabArgs ca{};
      ca.n_codes = e->n_codes; ca.n_nodes = nn; ca.n_tabs = e->n_ctab; ca.tip_words = (long)tip_words(e);
      ca.pint = e->d_pint.p; ca.ptip = e->d_ptip.p; ca.pcol = e->d_pcol.p; ca.ctab = e->d_ctab.p;
      for (int i = 0; i < e->n_ctab; i++) { ca.tabs[3 * i] = e->cherry.tabs[i].tip_a; ca.tabs[3 * i + 1] = e->cherry.tabs[i].tip_b; ca.tabs[3 * i + 2] = e->cherry.tabs[i].node; }
      const size_t lds = (size_t)(3 * 4096 + 64) * sizeof(double);
      if (!e->ctab_attr_set) {
         HIPCHK(hipFuncSetAttribute((const void *)cherry_table_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
         HIPCHK(hipFuncSetAttribute((const void *)cherry_table_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
         HIPCHK(hipFuncSetAttribute((const void *)cherry_table_kernel<false, 15>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
         e->ctab_attr_set = true;
      }
      const dim3 g((e->n_codes * e->n_codes + 127) / 128, e->n_ctab, c.K);
      if (e->n == 61) hipLaunchKernelGGL(cherry_table_kernel<true>, g, dim3(512), lds, c.ps, ca);
      else if (e->n == 60) hipLaunchKernelGGL((cherry_table_kernel<false, 15>), g, dim3(512), lds, c.ps, ca);      // (jit_cherry_count: 60 .. 64 states)
      else hipLaunchKernelGGL(cherry_table_kernel<false>, g, dim3(512), lds, c.ps, ca);
   }
   if (e->n_stab) {      // the subtree tables: level by level behind the cherry builder (a level reads the cherry tables and the levels before)
      const paml_amd_engine::Subtree &sb = e->sub;
      SubtreeTabArgs sa{};
      sa.n_codes = e->n_codes; sa.n_nodes = nn; sa.n_ctab = e->n_ctab; sa.tip_words = (long)tip_words(e); sa.stab_rows = sb.rows;
      sa.pint = e->d_pint.p; sa.ptip = e->d_ptip.p; sa.pcol = e->d_pcol.p; sa.ctab = e->d_ctab.p;
      sa.nodes = sb.d_nodes.p; sa.sidx = sb.d_sidx.p; sa.stab = e->d_stab.p;
      // (a level none of whose nodes has a tip son: the P block and the column table only, several workgroups per CU)
      const size_t lds_full = (size_t)(3 * 4096 + 64) * sizeof(double), lds_small = (size_t)(4096 + 64) * sizeof(double);
      if (!e->stab_attr_set) {
         HIPCHK(hipFuncSetAttribute((const void *)subtree_table_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_full));
         HIPCHK(hipFuncSetAttribute((const void *)subtree_table_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_full));
         HIPCHK(hipFuncSetAttribute((const void *)subtree_table_kernel<false, 15>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_full));
         e->stab_attr_set = true;
      }
      for (int l = 0; l < sb.sp.levels; l++) {
         sa.first = sb.level_first[l];
         sa.small = sb.level_small[l] ? 1 : 0;
         const size_t lds = sa.small ? lds_small : lds_full;
         const dim3 g(sb.level_tiles[l], sb.level_first[l + 1] - sb.level_first[l], c.K);
         if (e->n == 61) hipLaunchKernelGGL(subtree_table_kernel<true>, g, dim3(512), lds, c.ps, sa);
         else if (e->n == 60) hipLaunchKernelGGL((subtree_table_kernel<false, 15>), g, dim3(512), lds, c.ps, sa);
         else hipLaunchKernelGGL(subtree_table_kernel<false>, g, dim3(512), lds, c.ps, sa);
      }
   }
   mark_on(e, c.ps);
   if (c.pipe) {      // the pruning kernel (main stream) starts when this P(t) is there
      HIPCHK(hipEventRecord(e->ev_pmat, e->s2));
      HIPCHK(hipStreamWaitEvent(c.ms, e->ev_pmat, 0));
   }
   if (c.want_pipe && !c.skip_entry) {      // "everything on the main stream in front of this pruning kernel": what the next pipelined evaluation waits for
      HIPCHK(hipEventRecord(e->ev_entry[e->entry_sel], c.ms));
      e->entry_sel ^= 1;
      e->have_prev_entry = true;
   }
   e->n_pmat += (long)c.psets * (nn - 1);
   return 0;
}

// This evaluation's stream: the reduction that last read its slot (two evaluations ago) is done.  Once per evaluation, whoever
// asks first: a kernel that writes the slot's class likelihoods or partial sums itself, else the reduction.
int wait_slot(paml_amd_engine *e, Eval &c)
{
   if (c.slot_waited) return 0;
   c.slot_waited = true;
   if (e->done_pending[c.slot]) {
      e->done_pending[c.slot] = false;
      // (the caller's stream, once joined to that total by flush / enter, is already behind it; any other stream waits here)
      if (c.ms != e->stream || e->join_pending[c.slot]) {
         const int si = (int)(e->st_count % paml_amd_engine::NSTAT);
         if (e->comm_stats) HIPCHK(hipEventRecord(e->st_w0[si], c.ms));
         HIPCHK(hipStreamWaitEvent(c.ms, e->ev_done[c.slot], 0));
         if (e->comm_stats) { HIPCHK(hipEventRecord(e->st_w1[si], c.ms)); e->st_waited[si] = true; }
         if (c.ms == e->stream) e->join_pending[c.slot] = false;
      }
   }
   return 0;
}

// Where the reduction runs and the slot (class likelihoods, partial sums) it uses; the buffers of the reduction.
int prepare_slot(paml_amd_engine *e, Eval &c)
{
   const int B = c.B, nbg = e->nb_global;
   // PAML_AMD_OFFLOAD=1 (experiment): in a run of paml_amd_eval_device calls the whole reduction of evaluation i (mixture + log +
   // chunk sums, the exchange step, the fixed-order total) runs on the engine's side stream while the main stream goes straight on
   // to the pruning kernel of evaluation i + 1, two slots of class likelihoods alternating.  Measured on MI355X at the 8-GPU shard
   // size (profiles/r03_comm_overhead.txt): 0.2351 ms per evaluation against 0.2281 with the two small kernels left on the main
   // stream — the event record / wait pairs that order the streams cost what the kernel boundaries they remove did.  Not the default;
   // with a communicator only the all-reduce and the total go to the side stream.
   c.offload = c.want_pipe && !pk_forms_reduction(e->kernel) && !c.keep && !c.clean && !c.bs && !c.want_lnf && !e->tree.n_scale && e->env.offload;
   c.side_total = e->comm || c.dual;
   if (!c.offload && !c.side_total)
      if (int rc = join_comm(e)) return rc;
   c.slot = (c.side_total || c.offload) ? e->red_slot : 0;
   if (e->comm_stats && !e->st_part[0])
      for (int i = 0; i < paml_amd_engine::NSTAT; i++) {
         HIPCHK(e->st_part[i].ensure()); HIPCHK(e->st_done[i].ensure());
         HIPCHK(e->st_w0[i].ensure()); HIPCHK(e->st_w1[i].ensure());
      }
   if (e->comm_stats) e->st_waited[e->st_count % paml_amd_engine::NSTAT] = false;
   DevBuf<double> &dpart = e->part_slot(c.slot);
   if ((size_t)nbg * B > dpart.cap) {
      if (e->sc) HIPCHK(hipStreamSynchronize(e->sc));      // (reallocation: nothing may still be reading the old buffer)
      HIPCHK(dpart.ensure((size_t)nbg * B));
      HIPCHK(hipMemsetAsync(dpart.p, 0, dpart.cap * sizeof(double), c.ms));
   }
   e->last_fhk = (c.offload || c.dual) ? c.slot : 0;      // the slot's class likelihoods
   if (e->last_fhk) HIPCHK(e->fhk_slot(e->last_fhk).ensure((size_t)c.K * e->n_patt));
   c.slot_waited = false;
   if (c.offload) {
      if (int rc = ensure_side_stream(e)) return rc;
      if (int rc = wait_slot(e, c)) return rc;      // (the pruning kernel writes this slot's class likelihoods)
   }
   if ((size_t)B * RED_TICKET_WORDS > e->d_red_counter.cap) {
      HIPCHK(e->d_red_counter.ensure((size_t)std::max(B, 64) * RED_TICKET_WORDS));
      HIPCHK(hipMemsetAsync(e->d_red_counter.p, 0, e->d_red_counter.cap * sizeof(int), c.ms));
   }
   HIPCHK(e->d_out.ensure(B));
   if (c.want_lnf) HIPCHK(e->d_lnf.ensure((size_t)B * e->n_patt));
   return 0;
}

// Kernel B: fused pruning — the kernel choose_kernel named.
int run_prune(paml_amd_engine *e, Eval &c)
{
   const PruneKernel k = e->kernel;
   const int B = c.B, K = c.K, G = c.G, n_blocks = c.n_blocks;
   const BatchSpec *const bs = c.bs;
   if (pk_module(k) && e->tree.n_scale) HIPCHK(e->d_fscale.ensure((size_t)K * e->n_patt));
   PruneArgs pr = prune_args(e, e->prog, K, e->d_ops.p, false, e->tree.n_scale, c.keep, e->d_partials.p, e->d_scalef.p, c.overflow);
   if (k == PK_MFMA4X20_JIT) { pr.pint = e->d_pint.p; pr.pcol = e->d_rowmajor.p; }      // (operand-order P(t); the row-major copies for the all-4x4x4 experiment)
   pr.fhK = e->fhk_slot(e->last_fhk).p;
   if (k == PK_MFMA64_JIT && e->n_ctab) { pr.ctab = e->d_ctab.p; pr.n_ctab = e->n_ctab; }      // (this P set's cherry tables)
   if (k == PK_MFMA64_JIT && e->n_stab) {      // (... its subtree tables, and the tile blocks with the class-index rows)
      pr.stab = e->d_stab.p; pr.stab_rows = e->sub.rows; pr.stab_meta = e->sub.d_meta.p;
      pr.ztiles = e->sub.d_ztiles.p; pr.zt_bytes = e->sub.zt_bytes;
      pr.order = e->sub.ordered ? e->sub.d_order.p : nullptr;
   }
   // the gathering walk in the generated walk's place, where the table form is lookups and the root only and its tiles are laid out for
   // this selection (choose_kernel); everything around the launch stays
   const paml_amd_engine::Subtree &gsb = e->sub;
   const bool gather = k == PK_MFMA64_JIT && e->n_stab && !bs && gather_walk_wanted() && e->env.prof_ops.empty() && !e->env.prof_tiles && gsb.gw_ok &&
                       gsb.gw_sel_gen == gsb.sel_gen && gsb.gw_ordered == gsb.ordered && gsb.gw_tiles > 0 && gsb.d_gw_desc.p;
   e->last_gw = gather;
   if (gather) {
      pr.gw_desc = gsb.d_gw_desc.p; pr.gw_tiles = (int)gsb.gw_tiles; pr.gw_desc_bytes = gather_desc_bytes(gsb.gw_R); pr.gw_R = gsb.gw_R;
      for (int i = 0; i < 4; i++) { pr.gw_kind[i] = gsb.gw_kind[i]; pr.gw_id[i] = gsb.gw_id[i]; }
   }
   const int nb = (e->n_patt + e->chunk - 1) / e->chunk;      // the reduction's geometry: chunks of this engine
   if (pk_forms_reduction(k)) {      // (the others leave the partial sums to reduce_stage1)
      pr.Km = c.Km; pr.chunk = e->chunk; pr.first_chunk = e->first_chunk; pr.nb_stride = e->nb_global;
      pr.want_fhk = (c.want_fhk || e->tree.n_scale) ? 1 : 0;
      pr.freqK = (bs && bs->freqK) ? e->d_b_freqK.p : e->d_freqK.p; pr.freqK_bs = (bs && bs->freqK) ? c.Km : 0;
      pr.lnf = c.want_lnf ? e->d_lnf.p : nullptr;
      pr.red_partial = e->part_slot(c.slot).p; pr.red_out = c.d_lnL_out ? c.d_lnL_out : e->d_out.p; pr.nb_local = nb;
      if (int rc = wait_slot(e, c)) return rc;      // (this kernel writes the partial sums itself)
      // the total: a one-block stage-2 launch — but the cooperative per-tree kernel: always the last workgroup, of each batch element
      pr.red_counter = k == PK_MFMA64_COOPJIT ? e->d_red_counter.p : nullptr;
   }
   if (!e->env.prof_ops.empty()) {      // experiments only
      // per-op stamps: a fresh buffer and a dump after every launch; the workgroup timeline: one buffer, overwritten by every
      // launch and written out when the engine goes (nothing between the launches, so that the clock is the production clock)
      const int prof_stride = std::max((int)e->prog.ops.size() + 3, e->env.prof_tiles ? 96 : 0);
      const size_t words = (size_t)3 * n_blocks * prof_stride;
      if (!e->env.prof_tiles || words != e->prof_words) {
         if (e->d_prof) (void)hipFree(e->d_prof);
         e->d_prof = nullptr;
         HIPCHK(hipMalloc((void **)&e->d_prof, paml_amd_engine::MAXL * words * 8));      // (pruning streams: one timeline per lane)
         HIPCHK(hipMemsetAsync(e->d_prof, 0, paml_amd_engine::MAXL * words * 8, c.ms));
         e->prof_words = words; e->prof_blocks = n_blocks; e->prof_stride = prof_stride;
      }
      pr.prof = e->d_prof + (size_t)c.lane * words;
      pr.prof_stride = prof_stride;
      pr.prof_tid = e->env.prof_tid;
   }
   mark(e);
   // CUs of the persistent kernels.  One pruning stream inside a communicator: a few stay free for the collective (engine_state.h,
   // comm_cus).  Runs of evaluations on two pruning streams: all of them — CUs left free by one kernel are taken at once by the
   // first workgroups of the next, so a reservation reserves nothing there and only costs tiles per CU (measured, 16 taxa x 10^6
   // codon patterns: 1.524-1.526 ms per evaluation on 256 CUs against 1.534-1.542 on 254; the same at the 8-GPU shard size, with
   // and without a communicator); the small kernels run when workgroups retire.
   const bool two_streams = c.want_pipe && e->env.dual && !e->profiling;
   const int cus = (e->comm && !two_streams) ? std::max(1, e->n_cu - e->comm_cus) : e->n_cu;
   void *params[] = {&pr};
   hipStream_t const ms = c.ms;
   switch (k) {
   case PK_MFMA64_JIT:      // persistent: one 130 KB-LDS workgroup per CU walks the tiles
      if (gather) {
         const size_t lds = gather_walk_lds_bytes(pr.gw_R);
         if (!e->gw_attr_set) {
            HIPCHK(hipFuncSetAttribute((const void *)gather_walk_kernel<2>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)gather_walk_lds_bytes(128)));
            HIPCHK(hipFuncSetAttribute((const void *)gather_walk_kernel<3>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)gather_walk_lds_bytes(128)));
            HIPCHK(hipFuncSetAttribute((const void *)gather_walk_kernel<4>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)gather_walk_lds_bytes(128)));
            e->gw_attr_set = true;
         }
         const dim3 gg(std::min(pr.gw_tiles * K, cus)), gb(512);
         if (gsb.gw_nlk == 2) hipLaunchKernelGGL(gather_walk_kernel<2>, gg, gb, lds, ms, pr);
         else if (gsb.gw_nlk == 3) hipLaunchKernelGGL(gather_walk_kernel<3>, gg, gb, lds, ms, pr);
         else hipLaunchKernelGGL(gather_walk_kernel<4>, gg, gb, lds, ms, pr);
         break;
      }
      HIPCHK(hipModuleLaunchKernel(e->jit.fn, std::min(n_blocks, cus), 1, 1, e->mfma_waves * 64, 1, 1, 0, ms, params, nullptr));
      break;
   case PK_MFMA64_STREAM:
      if (!e->stream_attr_set) {
         HIPCHK(hipFuncSetAttribute((const void *)prune_mfma64_stream, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
         e->stream_attr_set = true;
      }
      hipLaunchKernelGGL(prune_mfma64_stream, dim3(n_blocks), dim3(512), (size_t)4 * 4096 * sizeof(double) + (size_t)e->n_tips * 128, ms, pr);
      break;
   // small data sets — every 16-pattern group can have a CU (ONE round: the kernel's 90 KB of LDS leave room for one workgroup
   // per CU, and two rounds of its 25 us walks lose to one round of the gather kernel's 39): four waves per group (prune_mfma64_coop)
   case PK_MFMA64_COOPJIT:
      HIPCHK(hipModuleLaunchKernel(e->jit_coop.fn, e->n_tiles * 4 * K, 1, 1, 256, 1, 1, 0, ms, params, nullptr));
      break;
   case PK_MFMA64_COOP:
      hipLaunchKernelGGL(prune_mfma64_coop, dim3(e->n_tiles * 4 * K), dim3(256), 0, ms, pr);
      break;
   case PK_VALU4_FUSED_JIT: case PK_VALU5_FUSED_JIT: {
      // single evaluations: one workgroup per chunk; batched ones: about two resident workgroups per CU in all, each walking every
      // gx-th chunk of its element (the LDS tables of an element's P(t) are filled once per workgroup, not once per 256 patterns)
      const int gx = B > 1 ? std::max(1, std::min(nb, 2 * e->n_cu / B)) : nb;
      HIPCHK(hipModuleLaunchKernel(e->jit.fn, gx, B, 1, e->fused_threads, 1, 1, 0, ms, params, nullptr));
      break;
   }
   case PK_MFMA4X20_JIT: {      // persistent: a multiple of the class count, every workgroup keeps its class's P(t) in LDS
      int grid = std::min(std::max(K, cus / K * K), e->n_tiles * K);
      // Runs of evaluations on two pruning streams: the small kernels beside this one (partial sums, the next P(t)) are
      // dispatched to shader engines in turn, and a workgroup sent to an engine whose CUs all hold a persistent workgroup
      // waits for the end of this kernel even if the engine next door has room (measured: both then end WITH this kernel and
      // the next pruning kernel, which needs them, cannot be queued ahead).  7/8 of the CUs leave every shader engine one
      // free; taken when it costs this kernel nothing, i.e. when a wave still walks the same number of 32-pattern units
      // (10^5 patterns x 4 classes: 7 at 56 workgroups per class as at 63).  0.1885 -> 0.182 ms per evaluation (32 taxa).
      if (two_streams && G == 1) {
         const int units = std::min(e->n_tiles * 8, (e->n_patt + 31) / 32), g78 = e->n_cu * 7 / 8 / K * K;
         auto rounds = [&](int g) { return ((units + g / K - 1) / (g / K) + 7) / 8; };
         if (g78 >= K && g78 < grid && rounds(g78) == rounds(grid)) grid = g78;
      }
      // (several genes: a workgroup serves one (gene, class); the kernel deals a class's workgroups to the genes, at least one each)
      HIPCHK(hipModuleLaunchKernel(e->jit.fn, std::max(grid / K, G > 1 ? G : 1) * K, 1, 1, 512, 1, 1, 0, ms, params, nullptr));
      break;
   }
   case PK_VALU4_JIT: case PK_VALU5_JIT: case PK_VALU20_JIT:
      HIPCHK(hipModuleLaunchKernel(e->jit.fn, n_blocks, 1, 1, 256, 1, 1, 0, ms, params, nullptr));
      break;
   case PK_MFMA64_GATHER: case PK_VALU4: case PK_VALU5: case PK_VALU20:      // the full interpreters
      launch_prune_full(e, e->prog.max_stack, n_blocks, pr, ms);
      break;
   }
   mark(e);
   if (c.want_pipe && e->env.dual) {      // this P set's last reader so far
      HIPCHK(hipEventRecord(e->ev_setread[e->pset], ms));
      e->setread_rec[e->pset] = true;
   }
   return 0;
}

// PAML_AMD_PROF_OPS without PAML_AMD_PROF_TILES: the per-op stamps of the launch just queued, written out (a host synchronisation).
int dump_op_stamps(paml_amd_engine *e, const Eval &c)
{
   if (e->env.prof_ops.empty() || e->env.prof_tiles) return 0;
   std::vector<unsigned long long> hp((size_t)3 * e->prof_blocks * e->prof_stride);
   HIPCHK(hipMemcpyAsync(hp.data(), e->d_prof, hp.size() * 8, hipMemcpyDeviceToHost, c.ms));
   HIPCHK(hipStreamSynchronize(c.ms));
   if (FILE *f = fopen(e->env.prof_ops.c_str(), "wb")) {
      int hdr[2] = {e->prof_blocks, e->prof_stride};
      fwrite(hdr, sizeof(int), 2, f);
      std::vector<int> codes;
      for (auto &o : e->prog.ops) codes.push_back(o.code);
      codes.resize(e->prof_stride - 3, 0);
      fwrite(codes.data(), sizeof(int), codes.size(), f);
      fwrite(hp.data(), 8, hp.size(), f);
      fclose(f);
   }
   return 0;
}

// Kernel C: mixture + log + weighted sum.  Stage 1 leaves one partial sum per chunk of patterns at the chunk's global
// position; with a communicator the ranks' (disjoint, zero elsewhere) arrays are summed over RCCL — adding zeros is exact,
// so every rank then holds the same array whatever the number of ranks — and stage 2 adds it up in a fixed order.
int reduce(paml_amd_engine *e, Eval &c)
{
   const PruneKernel k = e->kernel;
   const int B = c.B, Km = c.Km, slot = c.slot, nbg = e->nb_global, nb = (e->n_patt + e->chunk - 1) / e->chunk;
   const BatchSpec *const bs = c.bs;
   DevBuf<double> &dpart = e->part_slot(slot);
   ReduceArgs ra{};
   ra.fhK = e->fhk_slot(e->last_fhk).p; ra.weights = e->d_weights.p; ra.freqK = e->d_freqK.p; ra.lnf = c.want_lnf ? e->d_lnf.p : nullptr;
   ra.partial = dpart.p; ra.out = c.d_lnL_out ? c.d_lnL_out : e->d_out.p;
   ra.raw = pk_leaves_log(k) ? 1 : 0; ra.fscale = e->d_fscale.p;
   ra.n_patt = e->n_patt; ra.K = Km; ra.mode = e->mode; ra.n_scale = e->tree.n_scale; ra.chunk = e->chunk;
   ra.first_chunk = e->first_chunk; ra.nb_stride = nbg;
   // (measured on MI355X, 32 taxa x 10^5 nucleotide patterns: 28.2 us per evaluation with the separate one-block launch against
   //  30.2 with tickets — the agent-scope store + two atomics + coherent reads cross the XCDs' L2s and cost more than a launch)
   if (bs && bs->freqK) { ra.freqK = e->d_b_freqK.p; ra.freqK_bs = Km; }
   hipStream_t rs = c.ms;      // the stream of the reduction
   if (c.offload) {
      HIPCHK(hipEventRecord(e->ev_part[slot], c.ms));
      HIPCHK(hipStreamWaitEvent(e->sc, e->ev_part[slot], 0));
      rs = e->sc;
   }
   mark_on(e, rs);
   if (int rc = wait_slot(e, c)) return rc;
   if (!pk_forms_reduction(k)) hipLaunchKernelGGL(reduce_stage1, dim3(nb, B), dim3(256), 0, rs, ra);
   if (c.side_total) {
      // the exchange step, off the pruning stream: the side stream takes over when this evaluation's partial sums are there
      // (ev_part), all-reduces them into the slot's second buffer and forms the fixed-order total; the next evaluation's P(t) and
      // pruning kernel follow on the main stream without waiting for any of it
      DevBuf<double> &dtot = e->comm ? e->tot_slot(slot) : dpart;      // (one GPU, two pruning streams: only the total moves to `sc`)
      if (e->comm && (size_t)nbg * B > dtot.cap) {
         HIPCHK(hipStreamSynchronize(e->sc));
         HIPCHK(dtot.ensure((size_t)nbg * B));
      }
      if (!c.offload) {
         HIPCHK(hipEventRecord(e->ev_part[slot], c.ms));
         HIPCHK(hipStreamWaitEvent(e->sc, e->ev_part[slot], 0));
      }
      if (e->comm_stats) HIPCHK(hipEventRecord(e->st_part[e->st_count % paml_amd_engine::NSTAT], e->sc));      // (on `sc`, behind the wait: "partial sums ready")
      if (e->comm) {
         const ncclResult_t nr = rccl().AllReduce(dpart.p, dtot.p, (size_t)nbg * B, ncclDouble, ncclSum, e->comm, e->sc);
         if (nr != ncclSuccess) return fail(e, PAML_AMD_EHIP, std::string("ncclAllReduce: ") + rccl().GetErrorString(nr));
      }
      hipLaunchKernelGGL(reduce_stage2, dim3(B), dim3(256), 0, e->sc, (const double *)dtot.p, nbg, ra.out);
   }
   else if (nbg > 1 && k != PK_MFMA64_COOPJIT) hipLaunchKernelGGL(reduce_stage2, dim3(B), dim3(256), 0, rs, (const double *)dpart.p, nbg, ra.out);      // (one block per element: stage 1 wrote the total)
   if (c.side_total || c.offload) {
      if (e->comm_stats && c.side_total) { HIPCHK(hipEventRecord(e->st_done[e->st_count % paml_amd_engine::NSTAT], e->sc)); e->st_count++; }
      HIPCHK(hipEventRecord(e->ev_done[slot], e->sc));
      e->done_pending[slot] = true;
      e->join_pending[slot] = true;
      e->last_slot = slot;
      e->red_slot = (slot + 1) % e->n_lanes;
   }
   mark_on(e, rs);
   HIPCHK(hipGetLastError());
   if (e->profiling) e->prof_evals++;
   e->n_eval++;
   if (c.keep && !c.clean) e->partials_valid = true;
   e->pmat_valid = true;
   e->pipe_ok = c.want_pipe;      // (every other entry point clears it)
   // two pruning streams from the next call on: persistent kernels only (they are what holds every CU to its end), nothing shared
   // between consecutive evaluations but the two slots (class likelihoods, partial sums, P sets)
   e->dual_ok = c.want_pipe && e->env.dual && !e->env.offload && pk_persistent(k) && !c.overflow &&
                !e->tree.n_scale && !c.keep && !c.clean && !bs && !c.want_lnf && nbg > 1 && (e->env.prof_ops.empty() || e->env.prof_tiles);
   return 0;
}

}  // namespace

int launch_eval(paml_amd_engine *e, const double *branch, const double *gene_rate, const unsigned char *clean,
                double *d_lnL_out, bool want_lnf, const BatchSpec *bs, bool want_pipe, bool want_fhk)
{
   Eval c{branch, gene_rate, clean, d_lnL_out, bs, want_lnf, want_pipe, want_fhk};
   InlineVec iv;      // (branch lengths and gene rates inside the arguments of P(t))
   if (int rc = begin_eval(e, c)) return rc;              // the call is valid; the tree's program
   if (int rc = setup_streams(e, c)) return rc;           // pipelined and two-stream runs
   if (int rc = stage_inputs(e, c, iv)) return rc;        // small inputs, uploaded
   if (int rc = choose_kernel(e, c, &e->kernel)) return rc;
   if (int rc = ensure_buffers(e, c)) return rc;
   if (int rc = run_pmat(e, c, iv)) return rc;            // Kernel A
   if (int rc = prepare_slot(e, c)) return rc;
   if (int rc = run_prune(e, c)) return rc;               // Kernel B
   if (int rc = dump_op_stamps(e, c)) return rc;
   return reduce(e, c);                                   // Kernel C, the exchange step, the total
}

}  // namespace paml_amd

extern "C" {

int paml_amd_eval(paml_amd_engine *e, const double *branch, const double *gene_rate, double *lnL, double *lnf,
                  double *fhK)
{
   enter(e);
   if (!e || !branch || !lnL) return fail(e, PAML_AMD_EINVAL, "eval: null argument");
   int r = ensure_hout(e, 1);
   if (r) return r;
   r = launch_eval(e, branch, gene_rate, nullptr, e->h_out, lnf != nullptr, nullptr, false, fhK != nullptr);
   if (r) return r;
   if (lnf) HIPCHK(hipMemcpyAsync(lnf, e->d_lnf.p, (size_t)e->n_patt * sizeof(double), hipMemcpyDeviceToHost, e->stream));
   if (fhK)
      HIPCHK(hipMemcpyAsync(fhK, e->d_fhK.p, (size_t)e->K * e->n_patt * sizeof(double), hipMemcpyDeviceToHost, e->stream));
   if (int rc = join_comm(e)) return rc;
   HIPCHK(hipStreamSynchronize(e->stream));
   if (int rc = eigen_fail_check(e)) return rc;
   *lnL = e->h_out[0];
   return 0;
}

int paml_amd_eval_batch(paml_amd_engine *e, int n_batch, const double *branch, const double *gene_rate, const int *eigen_of,
                        const double *qfactor, const double *freqK, const double *rate, double *lnL, double *lnf)
{
   enter(e);
   if (!e || !branch || !lnL || n_batch < 1) return fail(e, PAML_AMD_EINVAL, "eval_batch: bad arguments");
   if ((long)n_batch * e->K * e->n_genes > 65535) return fail(e, PAML_AMD_EINVAL, "eval_batch: n_batch * K * n_genes > 65535");
   BatchSpec bs{n_batch, eigen_of, qfactor, freqK, rate};
   int r = ensure_hout(e, n_batch);
   if (r) return r;
   r = launch_eval(e, branch, gene_rate, nullptr, e->h_out, lnf != nullptr, &bs, false, false);
   if (r) return r;
   if (lnf)
      HIPCHK(hipMemcpyAsync(lnf, e->d_lnf.p, (size_t)n_batch * e->n_patt * sizeof(double), hipMemcpyDeviceToHost, e->stream));
   if (int rc = join_comm(e)) return rc;
   HIPCHK(hipStreamSynchronize(e->stream));
   if (int rc = eigen_fail_check(e)) return rc;
   memcpy(lnL, e->h_out, (size_t)n_batch * sizeof(double));
   return 0;
}

int paml_amd_eval_adg(paml_amd_engine *e, const double *branch, const double *gene_rate, const double *MK, const int *pose, int ls,
                      double *lnL)
{
   enter(e);
   if (!e || !branch || !MK || !pose || !lnL || ls < 1) return fail(e, PAML_AMD_EINVAL, "eval_adg: bad arguments");
   if (e->mode != PAML_AMD_MODE_LFUNDG) return fail(e, PAML_AMD_EINVAL, "eval_adg: needs the lfundG class mode");
   // With pattern shards pose[] holds GLOBAL pattern indices, the same on every rank: the class likelihoods are computed
   // on the shards, gathered over the ranks, and every rank runs the (sequential, short) chain over the sites itself.
   const bool sharded = e->comm && e->world > 1;
   const int K = e->K, npl = e->n_patt;
   const long np = sharded ? e->n_patt_global : npl;
   for (int i = 0; i < ls; i++)
      if (pose[i] < 0 || pose[i] >= np) return fail(e, PAML_AMD_EINVAL, "eval_adg: pose entry out of range");
   int r = launch_eval(e, branch, gene_rate, nullptr, nullptr, false);      // fx_r on the device
   if (r) return r;
   if (int rc = join_comm(e)) return rc;
   std::vector<double> fhK((size_t)K * np), w(np), b1(K), b2(K);
   const double *src = e->fhk_slot(e->last_fhk).p;
   if (sharded) {
      // the gather: every rank puts its columns into a zeroed [K + 1][n_patt_global] table (class likelihoods, then the weights) and
      // the tables are added — x + 0 is exact, so every rank ends with the bits a single engine would hold
      HIPCHK(e->d_adg_all.ensure((size_t)(K + 1) * np));
      HIPCHK(hipMemsetAsync(e->d_adg_all.p, 0, (size_t)(K + 1) * np * sizeof(double), e->stream));
      HIPCHK(hipMemcpy2DAsync(e->d_adg_all.p + e->first_patt, (size_t)np * sizeof(double), src, (size_t)npl * sizeof(double),
                              (size_t)npl * sizeof(double), (size_t)K, hipMemcpyDeviceToDevice, e->stream));
      HIPCHK(hipMemcpyAsync(e->d_adg_all.p + (size_t)K * np + e->first_patt, e->d_weights.p, (size_t)npl * sizeof(double),
                            hipMemcpyDeviceToDevice, e->stream));
      HIPCHK(hipEventRecord(e->ev_part[0], e->stream));
      HIPCHK(hipStreamWaitEvent(e->sc, e->ev_part[0], 0));
      const ncclResult_t nr = rccl().AllReduce(e->d_adg_all.p, e->d_adg_all.p, (size_t)(K + 1) * np, ncclDouble, ncclSum, e->comm, e->sc);
      if (nr != ncclSuccess) return fail(e, PAML_AMD_EHIP, std::string("eval_adg: ncclAllReduce: ") + rccl().GetErrorString(nr));
      HIPCHK(hipEventRecord(e->ev_done[0], e->sc));
      HIPCHK(hipStreamWaitEvent(e->stream, e->ev_done[0], 0));
      HIPCHK(hipMemcpyAsync(fhK.data(), e->d_adg_all.p, fhK.size() * sizeof(double), hipMemcpyDeviceToHost, e->stream));
      HIPCHK(hipMemcpyAsync(w.data(), e->d_adg_all.p + (size_t)K * np, w.size() * sizeof(double), hipMemcpyDeviceToHost, e->stream));
   } else {
      HIPCHK(hipMemcpyAsync(fhK.data(), src, fhK.size() * sizeof(double), hipMemcpyDeviceToHost, e->stream));
      HIPCHK(hipMemcpyAsync(w.data(), e->d_weights.p, w.size() * sizeof(double), hipMemcpyDeviceToHost, e->stream));
   }
   HIPCHK(hipStreamSynchronize(e->stream));
   if (int rc = eigen_fail_check(e)) return rc;
   // the chain over sites in their original order is sequential: host (treesub.c:7456-7492)
   double l = 0;
   if (e->tree.n_scale)
      for (long h = 0; h < np; h++) {
         const double fh = fhK[h];
         if (!(w[h] > 0)) continue;
         l += fh * w[h];
         fhK[h] = 1;
         for (int ir = 1; ir < K; ir++) fhK[(size_t)ir * np + h] = exp(fhK[(size_t)ir * np + h] - fh);
      }
   for (int il = 0; il < ls; il++) {
      const int h = pose[il];
      if (il == 0)
         for (int ir = 0; ir < K; ir++) b1[ir] = fhK[(size_t)ir * np + h];
      else {
         for (int ir = 0; ir < K; ir++) {
            double fh = 0;
            for (int j = 0; j < K; j++) fh += MK[ir * K + j] * b1[j];
            b2[ir] = fh * fhK[(size_t)ir * np + h];
         }
         b1 = b2;
      }
      double fh = 0;
      for (int ir = 0; ir < K; ir++) fh += b1[ir];
      if (fh < 1e-90) fh = 1e-300;
      for (int ir = 0; ir < K; ir++) b1[ir] /= fh;
      l += log(fh);
   }
   std::vector<double> fk(K);
   HIPCHK(hipMemcpy(fk.data(), e->d_freqK.p, K * sizeof(double), hipMemcpyDeviceToHost));
   double fh = 0;
   for (int ir = 0; ir < K; ir++) fh += fk[ir] * b1[ir];
   *lnL = l + log(fh);
   return 0;
}

int paml_amd_eval_device(paml_amd_engine *e, const double *branch, const double *gene_rate, double *d_lnL)
{
   if (!e || !branch || !d_lnL) return fail(e, PAML_AMD_EINVAL, "eval_device: null argument");
   return launch_eval(e, branch, gene_rate, nullptr, d_lnL, false, nullptr, true, false);
}

int paml_amd_flush(paml_amd_engine *e)
{
   if (!e) return PAML_AMD_EINVAL;
   if (int rc = join_comm(e)) return rc;
   // (no host synchronisation here: a decomposition that has ALREADY reported its sweep limit is returned now, one still running is
   //  caught by the next synchronous entry point — paml_amd_eigen_status waits for it)
   return eigen_fail_check(e);
}

int paml_amd_eigen_status(paml_amd_engine *e)
{
   if (!e) return PAML_AMD_EINVAL;
   if (int rc = join_comm(e)) return rc;
   HIPCHK(hipStreamSynchronize(e->stream));
   return eigen_fail_check(e);
}

int paml_amd_eval_dirty(paml_amd_engine *e, const double *branch, const double *gene_rate, const unsigned char *clean,
                        double *lnL)
{
   enter(e);
   if (!e || !branch || !lnL || !clean) return fail(e, PAML_AMD_EINVAL, "eval_dirty: null argument");
   int r = ensure_hout(e, 1);
   if (r) return r;
   r = launch_eval(e, branch, gene_rate, clean, e->h_out, false);
   if (r) return r;
   if (int rc = join_comm(e)) return rc;
   HIPCHK(hipStreamSynchronize(e->stream));
   if (int rc = eigen_fail_check(e)) return rc;
   *lnL = e->h_out[0];
   return 0;
}

}  // extern "C"

// engine_jitdbg.hip — the tree-walk program and the per-tree kernel generators without an engine: what the tests inspect, and the
// build-time prebuild of the benchmark configurations' kernels (hiprtc needs no GPU).
// Built for gfx950 only (one of the translation units of libpaml_amd.so, see engine_state.h).
#include "engine_state.h"

// PAML_AMD_PREBUILD_GENES=G (G > 1): the several-genes form of the 4- / 5-state fused kernel and of the 20-state matrix-core kernel
static int prebuild_genes() { const char *v = getenv("PAML_AMD_PREBUILD_GENES"); return v && atoi(v) > 1 ? atoi(v) : 1; }

// The tree of the entry points below, from its sons in CSR form; false: the arguments do not describe one
static bool tree_from_csr(int n_tips, int n_nodes, int root, const int *sons_ptr, const int *sons, const unsigned char *scale_node, TreeDesc *out)
{
   if (!sons_ptr || !sons || n_nodes <= 0 || root < 0 || root >= n_nodes) return false;
   TreeDesc &t = *out;
   t.n_tips = n_tips; t.n_nodes = n_nodes; t.root = root;
   t.sons_ptr.assign(sons_ptr, sons_ptr + n_nodes + 1);
   t.sons.assign(sons, sons + sons_ptr[n_nodes]);
   t.label.assign(n_nodes, 0);
   t.scale_node.assign(n_nodes, 0);
   t.scale_slot.assign(n_nodes, -1);
   if (scale_node)
      for (int i = 0; i < n_nodes; i++)
         if (scale_node[i]) { t.scale_node[i] = 1; t.scale_slot[i] = t.n_scale++; }
   return true;
}

extern "C" {

int paml_amd_debug_program(int n_tips, int n_nodes, int root, const int *sons_ptr, const int *sons,
                           const unsigned char *scale_node, int keep_partials, const unsigned char *clean,
                           int *ops_out, int cap, int *max_stack)
{
   TreeDesc t;
   if (!tree_from_csr(n_tips, n_nodes, root, sons_ptr, sons, scale_node, &t)) return PAML_AMD_EINVAL;
   Program p = build_program(t, keep_partials != 0, clean);
   if (max_stack) *max_stack = p.max_stack;
   if (ops_out)
      for (int i = 0; i < (int)p.ops.size() && i < cap; i++) {
         ops_out[4 * i] = p.ops[i].code; ops_out[4 * i + 1] = p.ops[i].a;
         ops_out[4 * i + 2] = p.ops[i].b; ops_out[4 * i + 3] = p.ops[i].c;
      }
   return (int)p.ops.size();
}

int paml_amd_debug_branch_plan(int n_tips, int n_nodes, int root, const int *sons_ptr, const int *sons, const unsigned char *scale_node,
                               int n_calls, const int *node_b, const double *branch, int *ends_out, int *up_out, unsigned char *clean_out,
                               int *ops_out, int cap)
{
   TreeDesc T;
   if (!tree_from_csr(n_tips, n_nodes, root, sons_ptr, sons, scale_node, &T) || n_calls < 1 || !node_b || !branch || !ends_out || !up_out || !clean_out)
      return PAML_AMD_EINVAL;
   const Adjacency adj = adjacency(T);
   BranchCache bc;
   Program prog;
   for (int i = 0; i < n_calls; i++) {
      const double *br = branch + (size_t)i * n_nodes;
      BranchPlan p;
      if (node_b[i] < 0 || node_b[i] >= n_nodes || node_b[i] == root || !branch_ends(T, adj, node_b[i], p)) return PAML_AMD_EINVAL;
      reset_if_stale(bc, n_nodes, 1, std::vector<double>(1, 1.0));
      invalidate(bc, T, adj, br);
      orient(bc, T, adj, p);
      tree_seen_from(T, adj, br, p);
      ends_out[2 * i] = p.A; ends_out[2 * i + 1] = p.Bn;
      std::copy(p.up.begin(), p.up.end(), up_out + (size_t)i * n_nodes);
      std::copy(p.clean.begin(), p.clean.end(), clean_out + (size_t)i * n_nodes);
      if (i == n_calls - 1) {
         std::vector<int> roots;
         for (int rt : {p.A, p.Bn})
            if (!T.is_leaf(rt) && !p.clean[rt]) roots.push_back(rt);
         prog = forest_program(p.tr, roots, p.clean.data(), true);
      }
      commit(bc, p, n_tips);
   }
   if (ops_out)
      for (int i = 0; i < (int)prog.ops.size() && i < cap; i++) {
         ops_out[4 * i] = prog.ops[i].code; ops_out[4 * i + 1] = prog.ops[i].a;
         ops_out[4 * i + 2] = prog.ops[i].b; ops_out[4 * i + 3] = prog.ops[i].c;
      }
   return (int)prog.ops.size();
}

int paml_amd_debug_code_order(int n_states, int n_codes, const int *n_chara, const unsigned char *chara_map, const unsigned char *z,
                              long nz, int *order_out)
{
   if (n_states < 1 || n_states > 64 || n_codes < 1 || n_codes > 256 || !n_chara || !chara_map || (!z && nz > 0) || !order_out)
      return PAML_AMD_EINVAL;
   for (int c = 0; c < n_codes; c++) {
      if (n_chara[c] < 0 || n_chara[c] > n_states) return PAML_AMD_EINVAL;
      for (int k = 0; k < n_chara[c]; k++)
         if (chara_map[(size_t)c * n_states + k] >= n_states) return PAML_AMD_EINVAL;
   }
   std::vector<long> cnt(n_codes, 0);
   for (long i = 0; i < nz; i++) {
      if (z[i] >= n_codes) return PAML_AMD_EINVAL;
      cnt[z[i]]++;
   }
   const std::vector<int> order = code_order(n_states, n_codes, n_chara, chara_map, cnt.data());
   std::copy(order.begin(), order.end(), order_out);
   return n_codes;
}

int paml_amd_debug_jit(int n_tips, int n_nodes, int root, const int *sons_ptr, const int *sons,
                       const unsigned char *scale_node, char *text_out, int cap, int compile)
{
   TreeDesc t;
   if (!tree_from_csr(n_tips, n_nodes, root, sons_ptr, sons, scale_node, &t)) return PAML_AMD_EINVAL;
   Program p = build_program(t, false, nullptr);
   const int fusedK = (compile & 2) ? (compile >> 16) & 0xff : 0, fusedNC = (compile >> 24) & 0xff;      // bit 1: the fused 4 / 5-state kernel
   int n_states = (compile >> 8) & 0xff;    // 0: the 61-state kernel; 4 / 5 / 20: the one-pattern-per-lane kernels;
   const int compile_all = compile;         // 64 + n: the MFMA kernel trimmed to n states
   compile &= 1;
   std::string text;
   if (n_states > 64) {
      if (!jit_supported(p, n_tips, 61)) return PAML_AMD_EUNSUPPORTED;
      text = jit_generate(p, n_tips, n_states - 64, n_states - 64);
   }
   else if (fusedK && n_states == 20) {
      if (!jit_m20_supported(p, n_tips, prebuild_genes())) return PAML_AMD_EUNSUPPORTED;
      text = jit_generate_m20(p, n_tips, fusedNC, prebuild_genes());
   }
   else if (fusedK) {
      const int chunk = (compile_all >> 2) & 0x3f ? ((compile_all >> 2) & 0x3f) * 256 : 256;      // bits 2..7: reduction chunk / 256
      if (!jit_valu_fused_plan(p, n_states, n_tips, fusedNC, fusedK, chunk).ok) return PAML_AMD_EUNSUPPORTED;
      text = jit_generate_valu_fused(p, n_states, n_tips, fusedNC, fusedK, chunk, prebuild_genes());
   }
   else if (n_states == 4 || n_states == 5 || n_states == 20) {
      if (!jit_valu_supported(p)) return PAML_AMD_EUNSUPPORTED;
      text = jit_generate_valu(p, n_states);
   }
   else {
      if (!jit_supported(p, n_tips, 61)) return PAML_AMD_EUNSUPPORTED;
      text = jit_generate(p, n_tips, 61, 64);
   }
   int rc = (int)text.size();
   if (compile) {
      std::vector<char> code;
      std::string log;
      // PAML_AMD_JIT_SHIP=dir: keep the code object there (the library's read-only lib/jit directory is filled this way at build time)
      if (jit_compile_code(text, &code, &log, getenv("PAML_AMD_JIT_SHIP")) != 0) {
         text = log;
         rc = PAML_AMD_EHIP;
      }
   }
   if (text_out && cap > 0) {
      const size_t ncp = std::min((size_t)cap - 1, text.size());
      memcpy(text_out, text.data(), ncp);
      text_out[ncp] = 0;
   }
   return rc;
}

// The table form (jit.h: OP_LOOKUP) of the 61-state kernel for a tree, at most max_tabs cherries tabulated: its source, the operand
// stream it is left with ((is_tip, node) pairs) and the tabulated cherries ((tip a, tip b, node) triples).  Returns the number of
// cherries tabulated (0: the table form does not apply); *n_stream the number of pairs.
int paml_amd_debug_jit_tables(int n_tips, int n_nodes, int root, const int *sons_ptr, const int *sons, const unsigned char *scale_node,
                              int max_tabs, char *text_out, int cap, int *stream_out, int stream_cap, int *n_stream, int *tabs_out, int tabs_cap)
{
   TreeDesc t;
   if (!tree_from_csr(n_tips, n_nodes, root, sons_ptr, sons, scale_node, &t)) return PAML_AMD_EINVAL;
   const Program p = build_program(t, false, nullptr);
   if (!jit_supported(p, n_tips, 61)) return PAML_AMD_EUNSUPPORTED;
   const int n_tab = jit_cherry_count(p, n_tips, 61, 61, 1, (size_t)std::max(max_tabs, 0) * cherry_table_bytes(61));
   if (n_stream) *n_stream = 0;
   if (text_out && cap > 0) text_out[0] = 0;
   if (!n_tab) return 0;
   const CherryProgram cp = jit_cherry_program(p, n_tab);
   const std::string text = jit_generate(cp.prog, n_tips, 61, 61, &cp.tabs);
   if (text_out && cap > 0) {
      const size_t ncp = std::min((size_t)cap - 1, text.size());
      memcpy(text_out, text.data(), ncp);
      text_out[ncp] = 0;
   }
   if (n_stream) *n_stream = (int)cp.prog.stream.size() / 2;
   if (stream_out)
      for (int i = 0; i < (int)cp.prog.stream.size() && i < stream_cap; i++) stream_out[i] = cp.prog.stream[i];
   if (tabs_out)
      for (int i = 0; i < n_tab && 3 * i + 2 < tabs_cap; i++) { tabs_out[3 * i] = cp.tabs[i].tip_a; tabs_out[3 * i + 1] = cp.tabs[i].tip_b; tabs_out[3 * i + 2] = cp.tabs[i].node; }
   return n_tab;
}

// The classes of subtree_classes.h for a tree and tip codes z[n_tips][n_patt], without an engine: u_out[n_nodes] (0: tips, the root),
// cls_out[n_nodes][n_patt] (optional; rows of nodes without classes are left alone).
int paml_amd_debug_subtree_classes(int n_tips, int n_nodes, int root, const int *sons_ptr, const int *sons, const unsigned char *z, long n_patt,
                                   int n_codes, unsigned int *u_out, unsigned int *cls_out)
{
   TreeDesc t;
   if (!z || n_patt < 1 || n_codes < 1 || !tree_from_csr(n_tips, n_nodes, root, sons_ptr, sons, nullptr, &t)) return PAML_AMD_EINVAL;
   for (long i = 0; i < (long)n_tips * n_patt; i++)
      if (z[i] >= n_codes) return PAML_AMD_EINVAL;
   const SubtreeClasses sc = subtree_classes(n_tips, n_nodes, root, t.sons_ptr.data(), t.sons.data(), z, n_patt, n_patt, n_codes);
   for (int v = 0; v < n_nodes; v++) {
      if (u_out) u_out[v] = sc.u[v];
      if (cls_out && sc.done[v]) memcpy(cls_out + (long)v * n_patt, sc.cls[v].data(), (size_t)n_patt * sizeof(unsigned int));
   }
   return 0;
}

// subtree_pattern_order (subtree_classes.h) for n_keys class arrays keys[n_keys][n_patt] with bound[k] > every entry of keys[k]: the
// engine's sequence of the keys (largest_first: the other one), or the keys in the order given (as_given).  order_out[n_patt].
int paml_amd_debug_subtree_order(int n_keys, const unsigned int *keys, const unsigned int *bound, long n_patt, int largest_first, int as_given,
                                 unsigned int *order_out)
{
   if (n_keys < 0 || n_patt < 1 || (n_keys && (!keys || !bound)) || !order_out) return PAML_AMD_EINVAL;
   std::vector<const unsigned int *> k(n_keys);
   std::vector<unsigned int> b(n_keys);
   std::vector<int> seq(n_keys);
   for (int i = 0; i < n_keys; i++) { k[i] = keys + (long)i * n_patt; b[i] = bound[i]; seq[i] = i; }
   for (long i = 0; i < (long)n_keys * n_patt; i++)
      if (keys[i] >= bound[i / n_patt]) return PAML_AMD_EINVAL;
   if (!as_given) seq = subtree_order_sequence(b, largest_first != 0);
   const std::vector<unsigned int> order = subtree_pattern_order(k, b, seq, n_patt);
   memcpy(order_out, order.data(), (size_t)n_patt * sizeof(unsigned int));
   return 0;
}

// gather_tiles + gather_tiles_pack (gather_tiles.h) for n_keys row arrays keys[n_keys][n_patt] below bound[n_keys]: the kernel's blocks.
int paml_amd_debug_gather_tiles(int n_keys, const unsigned int *keys, const unsigned int *bound, const unsigned int *order, const unsigned char *wflag,
                                long n_patt, int R, unsigned char *blocks_out, long cap_bytes, long *n_tiles, long *n_rows)
{
   if (n_keys < 1 || n_keys > GATHER_MAX_LOOKUPS || n_patt < 1 || !keys || !bound || R < n_keys || R > GATHER_R_MAX) return PAML_AMD_EINVAL;
   std::vector<const unsigned int *> k(n_keys);
   std::vector<unsigned int> b(bound, bound + n_keys);
   for (int i = 0; i < n_keys; i++) k[i] = keys + (long)i * n_patt;
   for (long i = 0; i < (long)n_keys * n_patt; i++)
      if (keys[i] >= bound[i / n_patt]) return PAML_AMD_EINVAL;
   if (order) {      // a permutation
      std::vector<char> seen(n_patt, 0);
      for (long i = 0; i < n_patt; i++) {
         if (order[i] >= (unsigned long)n_patt || seen[order[i]]) return PAML_AMD_EINVAL;
         seen[order[i]] = 1;
      }
   }
   const GatherTiles g = gather_tiles(k, b, order, n_patt, R);
   const std::vector<unsigned char> ones(wflag ? 0 : n_patt, 1);
   const std::vector<unsigned char> blocks = gather_tiles_pack(g, order, wflag ? wflag : ones.data(), n_patt);
   if (n_tiles) *n_tiles = (long)g.n_tiles();
   if (n_rows) *n_rows = g.total_rows();
   if (blocks_out) memcpy(blocks_out, blocks.data(), std::min((size_t)std::max(0L, cap_bytes), blocks.size()));
   return gather_desc_bytes(R);
}

// The nodes an engine of these sizes (one gene, K classes, the switches of the environment) tabulates above the cherries for tip codes
// z[n_tips][n_patt]: the classes, then jit_subtree_select with the engine's limits.  Returns their number (sel_out: the first `cap`).
int paml_amd_debug_subtree_select(int n_tips, int n_nodes, int root, const int *sons_ptr, const int *sons, const unsigned char *scale_node, int n_states,
                                  int n_codes, int K, const unsigned char *z, long n_patt, int *sel_out, int cap)
{
   TreeDesc t;
   if (!z || n_patt < 1 || !tree_from_csr(n_tips, n_nodes, root, sons_ptr, sons, scale_node, &t)) return PAML_AMD_EINVAL;
   const Program p = build_program(t, false, nullptr);
   if (!jit_supported(p, n_tips, n_codes)) return 0;
   EnvCfg env;
   env.read();
   const int n_tab = env.subtree_tables != 0 ? jit_cherry_count(p, n_tips, n_states, n_codes, K, (size_t)env.cherry_cap_mb << 20) : 0;
   if (!n_tab) return 0;
   const CherryProgram cp = jit_cherry_program(p, n_tab);
   const double lim_u = env.subtree_max_frac * (double)n_patt;
   const SubtreeClasses sc = subtree_classes(n_tips, n_nodes, root, t.sons_ptr.data(), t.sons.data(), z, n_patt, n_patt, n_codes,
                                             lim_u >= 4e9 ? ~0ull : (uint64_t)std::max(0.0, lim_u));
   const std::vector<int> sel = jit_subtree_select(t, cp.tabs, sc.u, sc.done, n_patt, env.subtree_max_frac, (size_t)env.subtree_cap_mb << 20, K);
   for (int i = 0; i < (int)sel.size() && i < cap; i++)
      if (sel_out) sel_out[i] = sel[i];
   return (int)sel.size();
}

// The per-tree 60..64-state kernel with the subtree tables of the nodes sel[n_sel] (sons before fathers: the engine's selection order; the
// source depends on the node set, not on the data) beside the cherry tables an engine with K classes builds: its source, compiled for
// gfx950 when `compile` (into `dir` when given: the library's lib/jit at build time).  *blocks_left: operand blocks left per tile.
// Returns the length of the source; 0 when the table form does not apply to the tree or a node of sel cannot be tabulated.
int paml_amd_debug_jit_subtree(int n_tips, int n_nodes, int root, const int *sons_ptr, const int *sons, const unsigned char *scale_node, int n_states,
                               int n_codes, int K, const int *sel, int n_sel, int compile, const char *dir, char *text_out, int cap, int *blocks_left)
{
   TreeDesc t;
   if (!sel || n_sel < 1 || !tree_from_csr(n_tips, n_nodes, root, sons_ptr, sons, scale_node, &t)) return PAML_AMD_EINVAL;
   const Program p = build_program(t, false, nullptr);
   if (!jit_supported(p, n_tips, n_codes)) return PAML_AMD_EUNSUPPORTED;
   EnvCfg env;
   env.read();
   const int n_tab = jit_cherry_count(p, n_tips, n_states, n_codes, K, (size_t)env.cherry_cap_mb << 20);
   if (text_out && cap > 0) text_out[0] = 0;
   if (!n_tab) return 0;
   // the rules of jit_subtree_select without the data: every node of sel within limits
   const CherryProgram cp = jit_cherry_program(p, n_tab);
   std::vector<unsigned int> u(n_nodes, 0);
   std::vector<char> done(n_nodes, 0);
   for (int i = 0; i < n_sel; i++) {
      if (sel[i] < n_tips || sel[i] >= n_nodes) return PAML_AMD_EINVAL;
      u[sel[i]] = 1 + i;
      done[sel[i]] = 1;
   }
   const std::vector<int> ok = jit_subtree_select(t, cp.tabs, u, done, 1L << 30, 1.0, ~(size_t)0 >> 8, 1);
   if ((int)ok.size() != n_sel) return 0;
   const SubtreeProgram sp = jit_subtree_program(p, n_tab, t, ok);
   if (sp.top.empty() || !jit_subtree_zfits(n_tips, (int)sp.top.size())) return 0;
   if (blocks_left) *blocks_left = (int)sp.prog.stream.size() / 2;
   std::string text = jit_generate(sp.prog, n_tips, n_states, n_codes, &sp.tabs, (int)sp.top.size(), env.subtree_order != 0);      // (the engine's form)
   int rc = (int)text.size();
   if (compile) {
      std::vector<char> code;
      std::string log;
      if (jit_compile_code(text, &code, &log, (dir && *dir) ? dir : nullptr) != 0) {
         text = log;
         rc = PAML_AMD_EHIP;
      }
   }
   if (text_out && cap > 0) {
      const size_t ncp = std::min((size_t)cap - 1, text.size());
      memcpy(text_out, text.data(), ncp);
      text_out[ncp] = 0;
   }
   return rc;
}

int paml_amd_jit_prebuild(int n_states, int n_tips, int n_codes, int K, long n_patt_global, int n_nodes, int root, const int *sons_ptr,
                          const int *sons, const unsigned char *scale_node, const char *dir, char *log_out, int log_cap)
{
   TreeDesc t;
   if (!dir || n_states < 2 || n_states > 64 || !tree_from_csr(n_tips, n_nodes, root, sons_ptr, sons, scale_node, &t)) return PAML_AMD_EINVAL;
   // (PAML_AMD_PREBUILD_KEEP=1: the kernel of a PAML_AMD_KEEP_PARTIALS engine, every internal node's partial stored)
   const Program p = build_program(t, n_states > 20 && getenv("PAML_AMD_PREBUILD_KEEP") != nullptr, nullptr);
   std::string text;
   // the same choices launch_eval makes for an engine of these sizes
   // (PAML_AMD_PREBUILD_COOP=1: the cooperative per-tree kernel of small data sets, whatever the number of states from 20 to 64)
   if (getenv("PAML_AMD_PREBUILD_COOP")) {
      if (!jit_coop_supported(p, n_tips, n_codes)) return PAML_AMD_EUNSUPPORTED;
      text = jit_generate_coop(p, n_tips, n_states);
   }
   else if (n_states == 20 && jit_m20_supported(p, n_tips, prebuild_genes())) text = jit_generate_m20(p, n_tips, n_codes, prebuild_genes());
   else if (n_states <= 5) {
      if (!jit_valu_supported(p)) return PAML_AMD_EUNSUPPORTED;
      const int chunk = red_chunk(n_patt_global);
      text = !jit_valu_fused_plan(p, n_states, n_tips, n_codes, K, chunk).ok ? jit_generate_valu(p, n_states)
                                                                               : jit_generate_valu_fused(p, n_states, n_tips, n_codes, K, chunk, prebuild_genes());
   }
   else {
      if (!jit_supported(p, n_tips, n_codes)) return PAML_AMD_EUNSUPPORTED;
      text = jit_generate(p, n_tips, n_states, n_codes);
      // ... and the table form an engine of these sizes (one gene, one frequency vector) runs by default: choose_kernel's conditions
      EnvCfg env;
      env.read();
      const bool keep = getenv("PAML_AMD_PREBUILD_KEEP") != nullptr;
      const int n_tab = (env.cherry_tables != 0 && !keep && (env.cherry_tables == 1 || n_patt_global >= env.cherry_min_patt))
                           ? jit_cherry_count(p, n_tips, n_states, n_codes, K, (size_t)env.cherry_cap_mb << 20) : 0;
      if (n_tab) {
         const CherryProgram cp = jit_cherry_program(p, n_tab);
         std::vector<char> code;
         std::string log;
         if (jit_compile_code(jit_generate(cp.prog, n_tips, n_states, n_codes, &cp.tabs), &code, &log, dir) != 0) {
            if (log_out && log_cap > 0) { strncpy(log_out, log.c_str(), log_cap - 1); log_out[log_cap - 1] = 0; }
            return PAML_AMD_EHIP;
         }
      }
   }
   if (const char *dump = getenv("PAML_AMD_JIT_DUMP")) {
      FILE *f = fopen(dump, "w");
      if (f) { fputs(text.c_str(), f); fclose(f); }
   }
   std::vector<char> code;
   std::string log;
   const int rc = jit_compile_code(text, &code, &log, dir);
   if (log_out && log_cap > 0) { strncpy(log_out, log.c_str(), log_cap - 1); log_out[log_cap - 1] = 0; }
   return rc ? PAML_AMD_EHIP : 0;
}

}  // extern "C"

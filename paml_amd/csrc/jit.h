// jit.h — per-tree specialised pruning kernels: the generators (host C++: a program in, a source text out; jit_cache.h compiles it).
//
// The interpreter kernels (kernels_prune.h) pay for their generality on every op: a switch dispatch, scalar
// loads of the op and stream tables, and — worst on CDNA4, where FP64 MFMA and VALU share the SIMD's
// issue — dozens of v_mov per op that the compiler needs to merge the loop-carried partials.  For a fixed
// tree the op sequence is known when paml_amd_set_tree returns, so this header unrolls it: it emits one
// straight-line HIP kernel (a few dozen calls into the hand-written building blocks of device_common.h,
// every block index, ring slot, wait count and register array a literal), compiled for gfx950 with
// hiprtc and cached as a module.  Partials are renamed instead of copied: each MFMA result is a fresh
// v4d[4] that *is* the next partial.  Same arithmetic, same operand stream, same LDS ring as
// prune_mfma64_stream; the interpreter remains the fallback (deep stacks, > 64 codes, > 128 tips, no hiprtc).
#pragma once
#include <algorithm>
#include <cstdlib>
#include <sstream>
#include <string>
#include <vector>

#include "program.h"

namespace paml_amd {

// Stack slots of the 61-state kernel that live in register arrays (each 32 VGPRs); deeper slots are spilled to global scratch.
// MFMA_RS (the interpreter's register slots) sizes the scratch: the engine allocates max_stack - MFMA_RS slots per workgroup.
constexpr int JIT_REG_SLOTS = 4;
constexpr int JIT_SCRATCH_BASE = 2;      // = MFMA_RS (checked in engine_state.h): scratch slot k holds stack slot k + 2

// Which programs the generator covers.
inline int jit_zpieces(int n_tips, int tp = 128) { return ((n_tips + 1) * tp + 2047) / 2048; }   // 2 KB units of a tile's code block (tp patterns per tile)

// LDS: ring, zb code blocks, pi, column tables, dump slot.  Two code blocks fit up to 95 tips, one up to 207.
inline bool jit_lds_fits(int n_tips, int zb, int tp = 128) { return 4 * 32768 + zb * jit_zpieces(n_tips, tp) * 2048 + 4 * 64 * 8 + (4 * 64 + 32) * 8 + 1024 <= 160 * 1024; }
inline int jit_zbuffers(int n_tips, int tp = 128) { return jit_lds_fits(n_tips, 2, tp) ? 2 : 1; }

// (STORE — every internal node's partial kept, PAML_AMD_KEEP_PARTIALS — is part of the tree's one program.  LOAD programs differ with the
//  set of clean nodes: a kernel per set would be compiled again and again, so they go to the interpreter unless `allow_load`.)
// Where a tile's tip codes live in LDS.  Up to 95 tips two blocks (the next tile's arrive while this one is walked), up to 207 one
// (replaced between tiles); beyond that the block is cut into PIECES by order of use: the rows (one per tip, then the weight flags) are
// laid out in the order the walk consumes them — every tip is read exactly once —, a piece is resident while the walk uses it and the
// next replaces it at the crossing (one wait for the DMA per tile and piece: nothing beside a tile's hundreds of products).  Round 5
// had two pieces (up to ~413 tips); round 6: as many as the tree needs (the reference's limit is NS 5000, codeml.c:19).
constexpr int JIT_ZP_MAX = 13;      // 2 KB units of LDS left for ONE code buffer beside the ring (27 392 bytes): 208 rows of 128 patterns
struct JitZPlan {
   int bufs = 2;             // LDS buffers (2: double-buffered; 1: one block or one piece)
   bool half = false;        // piece mode (the name is round 5's, when there were two)
   int pieces = 1;           // ... so many
   int ZP = 0;               // 2 KB units per buffer
   std::vector<int> row;     // tip (or n_tips: the flags) -> row in its piece
   std::vector<int> piece;   // tip (or n_tips) -> its piece
   std::vector<int> tip_of;  // row (over all pieces, in order of use) -> tip
   std::vector<int> row_at;  // row (over all pieces) -> row position in the tile's block: piece x (rows a buffer holds) + row in the piece
};
inline JitZPlan jit_zplan(const Program &p, int n_tips, int tp = 128)
{
   JitZPlan z;
   z.row.resize(n_tips + 1);
   z.piece.assign(n_tips + 1, 0);
   z.tip_of.resize(n_tips + 1);
   z.row_at.resize(n_tips + 1);
   for (int t = 0; t <= n_tips; t++) z.row[t] = z.tip_of[t] = z.row_at[t] = t;
   z.ZP = jit_zpieces(n_tips, tp);
   if (jit_lds_fits(n_tips, 2, tp)) { z.bufs = 2; return z; }
   z.bufs = 1;
   if (jit_lds_fits(n_tips, 1, tp)) return z;
   // pieces: rows in order of use, cut at op boundaries (the rows of one op — a cherry has two — stay together)
   z.half = true;
   std::vector<int> order;
   std::vector<char> seen(n_tips + 1, 0);
   std::vector<int> op_start;      // index into `order` where each tip-reading op starts
   for (const Op &o : p.ops) {
      const bool one = o.code == OP_SET_TIP || o.code == OP_MUL_TIP || o.code == OP_INIT_TIP, two = o.code == OP_SET_TIP2 || o.code == OP_MUL_TIP2;
      if (!one && !two) continue;
      op_start.push_back((int)order.size());
      if (!seen[o.a]) { seen[o.a] = 1; order.push_back(o.a); }
      if (two && !seen[o.b]) { seen[o.b] = 1; order.push_back(o.b); }
   }
   for (int t = 0; t < n_tips; t++)
      if (!seen[t]) order.push_back(t);      // (tips the program never reads: rows nobody looks at)
   order.push_back(n_tips);                  // the weight flags: read by ROOT, last
   const int total = n_tips + 1, cap = JIT_ZP_MAX * 2048 / tp;      // rows a buffer holds at most
   const int npc = std::max(2, (total + cap - 1) / cap);
   const int want = (total + npc - 1) / npc;      // even pieces (two: the halves of round 5), each cut moved up to the next op boundary
   std::vector<int> first(1, 0);      // first row of every piece
   while (total - first.back() > (first.size() == 1 && npc == 2 ? want : std::min(cap, std::max(want, 1)))) {
      int cut = first.back() + want;
      int at = -1;
      for (int st : op_start)
         if (st >= cut) { at = st; break; }
      if (at < 0 || at - first.back() > cap) {      // no boundary at or after the even cut within the buffer: the last one before it
         at = -1;
         for (int st : op_start)
            if (st > first.back() && st <= first.back() + cap) at = st;
         if (at < 0) at = std::min(total - 1, first.back() + cap);      // (cannot happen: an op has at most two rows)
      }
      if (at >= total) break;
      first.push_back(at);
   }
   first.push_back(total);
   z.pieces = (int)first.size() - 1;
   int rows_max = 0;
   for (int k = 0; k < z.pieces; k++) rows_max = std::max(rows_max, first[k + 1] - first[k]);
   z.ZP = (rows_max * tp + 2047) / 2048;
   const int rows_buf = z.ZP * 2048 / tp;
   for (int k = 0; k < z.pieces; k++)
      for (int r = first[k]; r < first[k + 1]; r++) {
         z.tip_of[r] = order[r];
         z.row[order[r]] = r - first[k];
         z.piece[order[r]] = k;
         z.row_at[r] = k * rows_buf + (r - first[k]);
      }
   return z;
}
inline bool jit_zfits(const Program &p, int n_tips, int tp = 128)
{
   const JitZPlan z = jit_zplan(p, n_tips, tp);
   return 4 * 32768 + z.bufs * z.ZP * 2048 + 4 * 64 * 8 + (4 * 64 + 32) * 8 + 1024 <= 160 * 1024;
}

inline bool jit_supported(const Program &p, int n_tips, int n_codes, int n_pi = 1, int max_arrays = 6, int tp = 128, bool allow_load = false)
{
   if (n_codes > 256 || p.ops.size() > 8000 || n_pi > 4) return false;      // (more than 64 codes: JIT_AMB_OVERFLOW, device_common.h)
   if (!jit_zfits(p, n_tips, tp)) return false;
   if (p.stream.size() / 2 < 4) return false;                       // trees this small go to the interpreter
   for (const Op &o : p.ops)
      if (o.code == OP_LOAD && !allow_load) return false;
   (void)max_arrays;      // stack slots beyond JIT_REG_SLOTS register arrays go to global scratch
   return true;
}

// (61 states: rows 48..60 of every product without the padded rows 61..63: no faster, 1.573 against 1.569 ms, profiles/r04_61state.txt)

inline std::string jit_program_key(const Program &p, int n_tips)
{
   std::ostringstream k;
   k << n_tips << ":";
   for (const Op &o : p.ops) k << o.code << "," << o.a << "," << o.b << ";";
   return k.str();
}

// ---- cherry tables (60..64 states) ------------------------------------------------------------------------------------
// A cherry's partial tipA[:,ca] o tipB[:,cb] takes at most n_codes^2 values over the whole alignment, and so does its product with
// P(t_cherry).  cherry_table_kernel (kernels_pmat.h) forms T_c[ca][cb] = P(t_c) . (tipA[:,ca] o tipB[:,cb]) once per evaluation, right
// behind P(t), with the walk's own building blocks (same bits), and the walk gathers the finished 64-vector: `SET_TIP2 a b` directly
// followed by the MATMUL / MATMUL_POP of the cherry's node becomes one OP_LOOKUP, and its three operand blocks leave the stream.
// Only the per-tree kernel sees this form: it is derived from the tree's program, which the interpreters keep.
constexpr int OP_LOOKUP = 100;           // a: the cherry's node, b: as MATMUL (pop / push slots), c: its table's number
constexpr int JIT_LOOKAHEAD = 2;         // lookups whose rows are requested before the one being consumed is awaited
struct CherryTab { int tip_a, tip_b, node; };
struct CherryProgram {
   Program prog;
   std::vector<CherryTab> tabs;
};
constexpr int CHERRY_MAX_TABS = 48;           // cherries of a tree whose tip codes fit two LDS blocks (<= 95 tips): what CherryTabArgs carries
constexpr size_t CHERRY_ROW_BYTES = 512;      // one (ca, cb) pair: [piece i of 8][q of 4][16 bytes] — the four q-lanes of a pattern read 64 contiguous bytes
inline size_t cherry_table_bytes(int n_codes) { return (size_t)n_codes * n_codes * CHERRY_ROW_BYTES; }

inline CherryProgram jit_cherry_program(const Program &p, int max_tabs)
{
   CherryProgram cp;
   cp.prog.max_stack = p.max_stack;
   const std::vector<Op> &o = p.ops;
   for (size_t i = 0; i < o.size(); i++) {
      const bool mm = i + 1 < o.size() && (o[i + 1].code == OP_MATMUL || o[i + 1].code == OP_MATMUL_POP);
      if (o[i].code == OP_SET_TIP2 && mm && (int)cp.tabs.size() < max_tabs) {
         cp.prog.ops.push_back({OP_LOOKUP, o[i + 1].a, o[i + 1].b, (int)cp.tabs.size()});
         cp.tabs.push_back({o[i].a, o[i].b, o[i + 1].a});
         i++;
         continue;
      }
      cp.prog.ops.push_back(o[i]);
      if (o[i].code == OP_MATMUL || o[i].code == OP_MATMUL_POP) cp.prog.n_matmul++;
   }
   finish_program(cp.prog);      // (the stream without the tabulated cherries' blocks; OP_LOOKUP is none of its cases)
   return cp;
}

// Cherries to tabulate: in program order while the tables of all K classes stay within `cap_bytes`, and none where the table form does
// not apply (more than 64 codes, LOAD / STORE programs, trees whose tip codes do not fit two LDS blocks) or would leave the ring fewer
// than four operand blocks per tile.
inline int jit_cherry_count(const Program &p, int n_tips, int n_states, int n_codes, int K, size_t cap_bytes, int tp = 128)
{
   if (n_states < 60 || n_states > 64 || n_codes > 64 || n_codes < 1 || K < 1) return 0;
   if (jit_zplan(p, n_tips, tp).bufs != 2) return 0;
   for (const Op &o : p.ops)
      if (o.code == OP_LOAD || o.code == OP_STORE) return 0;
   int want = (int)std::min<size_t>(cap_bytes / ((size_t)K * cherry_table_bytes(n_codes)), (size_t)CHERRY_MAX_TABS);
   for (; want > 0; want--) {
      const CherryProgram cp = jit_cherry_program(p, want);
      if ((int)cp.tabs.size() < want) { want = (int)cp.tabs.size() + 1; continue; }      // (fewer cherries than the cap allows)
      if (cp.prog.stream.size() / 2 >= 4) return want;
   }
   return 0;
}

// ---- subtree tables (60..64 states): repeated patterns above the cherries -------------------------------------------------------
// What holds for a cherry holds one and two levels up, not over all tuples of codes but over the tuples the alignment contains
// (subtree_classes.h: u_v classes at node v).  subtree_table_kernel (kernels_pmat.h) forms T_v[c] = P(t_v) . (row_l o row_r) for every
// class c of a selected node v from its sons' rows — a tip's column, a cherry table's row, a subtree table's row —, level by level behind
// the cherry builder, and the walk's whole op run of v (its sons' steps and lookups and its MATMUL / MATMUL_POP) becomes ONE OP_LOOKUP
// whose row number is the pattern's class at v.  Only the topmost selected nodes appear in the walk; all cherries are still tabulated
// (the level above reads them).  Selection and the table form depend on the node set only; the u_v are data and reach the kernels as
// arguments (PruneArgs::stab_meta), so one compiled kernel serves every alignment with the same selected set.
constexpr int SUBTREE_TAB_BASE = 1 << 16;      // OP_LOOKUP with c >= this: lookup c - SUBTREE_TAB_BASE of the walk reads a subtree table
struct SubtreeSon { int kind = 0, id = 0; };      // kind 0: tip `id`; 1: cherry table `id`; 2: subtree table `id` (index into SubtreeProgram::sub)
struct SubtreeTab { int node = 0, level = 0; SubtreeSon l, r; };
struct SubtreeProgram {
   Program prog;                    // the table form: cherries and top-level selected nodes as OP_LOOKUPs
   std::vector<CherryTab> tabs;     // the cherry tables, as jit_cherry_program numbers them (all built)
   std::vector<SubtreeTab> sub;     // every selected node, sons before fathers
   std::vector<int> top;            // lookup t of the walk -> index into sub
   int levels = 0;
};

// Nodes to tabulate beside the cherries `tabs`: exactly two sons, each a tip or tabulated, no rescaling at the node, not the root; in
// ascending u (u_father >= u_son, ties broken by height) while u <= frac x n_patt and K x rows x 512 bytes stay within cap_bytes.
inline std::vector<int> jit_subtree_select(const TreeDesc &t, const std::vector<CherryTab> &tabs, const std::vector<unsigned int> &u,
                                           const std::vector<char> &done, long n_patt, double frac, size_t cap_bytes, int K)
{
   std::vector<int> sel, cand, height(t.n_nodes, 0), tab_of(t.n_nodes, -1), is_sel(t.n_nodes, 0);
   for (size_t i = 0; i < tabs.size(); i++) {
      const int v = tabs[i].node;
      if (t.sons_ptr[v + 1] - t.sons_ptr[v] == 2 && t.sons[t.sons_ptr[v]] == tabs[i].tip_a && t.sons[t.sons_ptr[v] + 1] == tabs[i].tip_b) tab_of[v] = (int)i;
   }
   {  // heights, sons first
      std::vector<int> order, st(1, t.root);
      while (!st.empty()) {
         const int v = st.back();
         st.pop_back();
         order.push_back(v);
         for (int j = t.sons_ptr[v]; j < t.sons_ptr[v + 1]; j++) st.push_back(t.sons[j]);
      }
      for (size_t k = order.size(); k-- > 0;)
         for (int j = t.sons_ptr[order[k]]; j < t.sons_ptr[order[k] + 1]; j++) height[order[k]] = std::max(height[order[k]], height[t.sons[j]] + 1);
   }
   // (never a cherry: one that the cherry tables left out — their cap, or their rule of four operand blocks — stays a product, and so
   //  does everything above it; its class numbers are not dense and it has no son rows)
   auto cherry = [&](int v) { return t.sons[t.sons_ptr[v]] < t.n_tips && t.sons[t.sons_ptr[v] + 1] < t.n_tips; };
   for (int v = t.n_tips; v < t.n_nodes; v++)
      if (v != t.root && done[v] && tab_of[v] < 0 && t.sons_ptr[v + 1] - t.sons_ptr[v] == 2 && !cherry(v) && !(v < (int)t.scale_node.size() && t.scale_node[v]) &&
          (double)u[v] <= frac * (double)n_patt)
         cand.push_back(v);
   std::sort(cand.begin(), cand.end(), [&](int a, int b) { return u[a] != u[b] ? u[a] < u[b] : (height[a] != height[b] ? height[a] < height[b] : a < b); });
   size_t rows = 0;
   for (int v : cand) {
      bool ok = true;
      for (int j = t.sons_ptr[v]; j < t.sons_ptr[v + 1]; j++) {
         const int s = t.sons[j];
         ok = ok && (s < t.n_tips || tab_of[s] >= 0 || is_sel[s]);
      }
      if (!ok || (rows + u[v]) * CHERRY_ROW_BYTES * (size_t)K > cap_bytes || u[v] >= (1u << 24)) continue;      // (a class index travels as three bytes)
      rows += u[v];
      is_sel[v] = 1;
      sel.push_back(v);
   }
   return sel;
}

// The table form of `p` with the cherries of jit_cherry_program(p, max_tabs) and the nodes `sel` (jit_subtree_select's order) tabulated.
inline SubtreeProgram jit_subtree_program(const Program &p, int max_tabs, const TreeDesc &t, const std::vector<int> &sel)
{
   SubtreeProgram sp;
   const std::vector<Op> &o = p.ops;
   // the cherry tables, by the op that starts them — jit_cherry_program's scan
   std::vector<int> cherry_at(o.size(), -1), tab_of(t.n_nodes, -1), sub_of(t.n_nodes, -1), father(t.n_nodes, -1);
   for (size_t i = 0; i + 1 < o.size(); i++)
      if (o[i].code == OP_SET_TIP2 && (o[i + 1].code == OP_MATMUL || o[i + 1].code == OP_MATMUL_POP) && (int)sp.tabs.size() < max_tabs) {
         cherry_at[i] = (int)sp.tabs.size();
         tab_of[o[i + 1].a] = (int)sp.tabs.size();
         sp.tabs.push_back({o[i].a, o[i].b, o[i + 1].a});
      }
   for (int v = 0; v < t.n_nodes; v++)
      for (int j = t.sons_ptr[v]; j < t.sons_ptr[v + 1]; j++) father[t.sons[j]] = v;
   for (int v : sel) {
      SubtreeTab st;
      st.node = v;
      SubtreeSon *son[2] = {&st.l, &st.r};
      for (int j = 0; j < 2; j++) {
         const int s = t.sons[t.sons_ptr[v] + j];
         if (s < t.n_tips) *son[j] = {0, s};
         else if (tab_of[s] >= 0) *son[j] = {1, tab_of[s]};
         else { *son[j] = {2, sub_of[s]}; st.level = std::max(st.level, sp.sub[sub_of[s]].level + 1); }
      }
      sp.levels = std::max(sp.levels, st.level + 1);
      sub_of[v] = (int)sp.sub.size();
      sp.sub.push_back(st);
   }
   // the op run of every node's product: from the op that starts the partial its MATMUL multiplies to that MATMUL
   std::vector<int> run_end(o.size(), -1), run_node(o.size(), -1);      // by first op, for the topmost selected nodes
   {
      int cur_start = -1;
      std::vector<int> slot_start(256, -1);
      for (size_t i = 0; i < o.size(); i++) {
         switch (o[i].code) {
         case OP_INIT_ONES: case OP_INIT_TIP: case OP_SET_TIP: case OP_SET_TIP2: case OP_LOAD: cur_start = (int)i; break;
         case OP_PUSH: slot_start[o[i].b & 255] = cur_start; cur_start = -1; break;
         case OP_MATMUL: case OP_MATMUL_POP: {
            const int v = o[i].a, pop = mm_pop_slot(o[i]), push = mm_push_slot(o[i]);
            if (sub_of[v] >= 0 && cur_start >= 0 && (father[v] < 0 || sub_of[father[v]] < 0)) { run_end[cur_start] = (int)i; run_node[cur_start] = v; }
            if (pop >= 0) cur_start = slot_start[pop];      // (the father's partial began where the popped one did)
            if (push >= 0) { slot_start[push] = cur_start; cur_start = -1; }
         } break;
         default: break;
         }
      }
   }
   int max_slot = -1;
   for (size_t i = 0; i < o.size(); i++) {
      if (run_end[i] >= 0) {
         const Op &mm = o[run_end[i]];
         sp.prog.ops.push_back({OP_LOOKUP, mm.a, mm.b, SUBTREE_TAB_BASE + (int)sp.top.size()});
         sp.top.push_back(sub_of[run_node[i]]);
         max_slot = std::max(max_slot, mm_push_slot(mm));
         i = run_end[i];
         continue;
      }
      if (cherry_at[i] >= 0) {
         sp.prog.ops.push_back({OP_LOOKUP, o[i + 1].a, o[i + 1].b, cherry_at[i]});
         max_slot = std::max(max_slot, mm_push_slot(o[i + 1]));
         i++;
         continue;
      }
      sp.prog.ops.push_back(o[i]);
      if (o[i].code == OP_MATMUL || o[i].code == OP_MATMUL_POP) { sp.prog.n_matmul++; max_slot = std::max(max_slot, mm_push_slot(o[i])); }
      if (o[i].code == OP_PUSH) max_slot = std::max(max_slot, o[i].b & 255);
   }
   sp.prog.max_stack = std::min(p.max_stack, max_slot + 1);      // (the collapsed runs held the deep slots)
   finish_program(sp.prog);
   return sp;
}
// the rows of a tile's code block with the class indices of n_top lookups behind the weight flags; they must leave room for two blocks
inline int jit_subtree_zrows(int n_tips, int n_top) { return n_tips + 3 * n_top; }
inline bool jit_subtree_zfits(int n_tips, int n_top, int tp = 128) { return jit_lds_fits(jit_subtree_zrows(n_tips, n_top), 2, tp); }

// ---- what the generators share -------------------------------------------------------------------------------------------
// The profiling switches of the kernel experiments, read once per generation (build() and the tests change them between calls).
struct JitProf {
   const bool tiles = getenv("PAML_AMD_PROF_TILES") != nullptr;            // s_memrealtime (100 MHz) at workgroup start and at the end of each of its tiles (tools/prof_tiles.py)
   const bool ops = !tiles && getenv("PAML_AMD_PROF_OPS") != nullptr;      // s_memtime stamp at every op
   const int every = getenv("PAML_AMD_PROF_EVERY") ? std::max(1, atoi(getenv("PAML_AMD_PROF_EVERY"))) : 1;      // ... at every n-th op only
   const std::string tid = getenv("PAML_AMD_PROF_TID") ? getenv("PAML_AMD_PROF_TID") : "0";                      // the thread that stamps the tiles (20 states)
};

// A partial's place: an array of the pool (A<i>), one of the 61-state kernel's arrays outside it — AS, the next tile's first cherry, and
// AL<i>, the rows of its first lookups, both filled under the predecessor's last product — or stack slot i spilled to global scratch.
struct JitArr {
   enum Kind { NONE, POOL, NEXT_CHERRY, NEXT_LOOKUP, SPILLED } kind = NONE;
   int i = -1;
   std::string name() const { return kind == NEXT_CHERRY ? "AS" : (kind == NEXT_LOOKUP ? "AL" : "A") + std::to_string(i); }
};

// Register arrays and stack slots of a walk.  Partials are renamed, not copied: a product's result is a fresh array of the pool — a free
// list, last released first out, on which the arrays' names in the generated text depend — and `cur` names the partial under construction.
struct JitRegs {
   enum Step { MUL, MUL_MEM, SPILL };      // what finish_product asks `emit` to write: out *= in;  out *= scratch slot in.i;  scratch slot in.i = out
   std::vector<int> free_list;
   std::vector<JitArr> slot = std::vector<JitArr>(256);      // stack slot -> its partial
   JitArr cur;
   const int reg_slots;         // stack slots from this one on are spilled (the 61-state kernel)
   bool exhausted = false;      // more arrays wanted than declared: the generator returns jit_exhausted_source(), not undefined behaviour here
   explicit JitRegs(int n_arrays, int reg_slots_ = 256) : reg_slots(reg_slots_)
   {
      for (int i = n_arrays - 1; i >= 0; i--) free_list.push_back(i);
   }
   JitArr alloc()
   {
      if (free_list.empty()) { exhausted = true; return {JitArr::POOL, 0}; }
      const int r = free_list.back();
      free_list.pop_back();
      return {JitArr::POOL, r};
   }
   void release(const JitArr &r) { if (r.kind == JitArr::POOL) free_list.push_back(r.i); }
   // An op that starts a partial.  One of the pool that is still held is written over: a forest of subtrees (the branch-local refill,
   // engine_branch.hip) — the previous subtree's root was stored and is done.  (Not AS: the tile's last product fills it for the NEXT tile
   // while this tile's later partials would still live in it.)
   void start_partial() { if (cur.kind != JitArr::POOL) cur = alloc(); }
   void end_partial() { release(cur); cur = JitArr(); }      // ROOT: the partial is used up
   template <class Emit> void push(int s, Emit emit) { finish_product(cur, -1, s, emit); }
   // The tail of a product (or lookup) whose result is in `out`: multiply the popped slot in, then push — to the slot, or spilled — or keep as cur
   template <class Emit> void finish_product(const JitArr &out, int pop, int push, Emit emit)
   {
      if (pop >= 0) {
         emit(slot[pop].kind == JitArr::SPILLED ? MUL_MEM : MUL, out, slot[pop]);
         release(slot[pop]);
         slot[pop] = JitArr();
      }
      if (push >= reg_slots) {
         slot[push] = {JitArr::SPILLED, push};
         emit(SPILL, out, slot[push]);
         release(out);
      }
      else if (push >= 0) slot[push] = out;
      cur = push >= 0 ? JitArr() : out;
   }
};
inline std::string jit_exhausted_source() { return "#error \"jit register arrays exhausted\"\n"; }

// The static model of a thread's vector-memory queue (vmcnt): what was issued and is not yet known to have landed, oldest first, in
// pieces = vector-memory instructions.  Every JIT_WAIT(N) of the 61-state walk is computed here.  The ring's DMA pieces, the tip-code
// blocks, the eight 1 KB wave stores / loads of a STORE / LOAD and the eight gathers of a lookup are entries of the ONE list because the
// hardware counts them in one counter, in order of issue: a wait computed without the stores would make every block step wait for their
// completion in HBM.  (At a tile's start the list lacks the previous tile's last stores: those waits are stricter than needed, never laxer.)
struct JitItem {
   enum Kind { RING, CODES, MEM, LOOKUP } kind;      // operand block i of the tile (>= nblk: the next tile's), a code block, a store / load, lookup i
   int i;
   bool operator==(const JitItem &o) const { return kind == o.kind && i == o.i; }
};
struct JitInFlight {
   struct Entry { JitItem item; int pieces; };
   std::vector<Entry> fl;
   void issue(JitItem it, int pieces) { fl.push_back({it, pieces}); }
   // a piece issued on its own (the deferred refill): an item whose pieces are interleaved with others' has several entries
   void add_piece(JitItem it)
   {
      if (!fl.empty() && fl.back().item == it) fl.back().pieces++;
      else fl.push_back({it, 1});
   }
   // pieces that may stay in flight once `it` has to be complete (-1: already covered by an earlier wait); everything up to its LAST entry is dropped
   int wait_for(JitItem it)
   {
      int pos = -1, nfl = 0;
      for (size_t i = 0; i < fl.size(); i++)
         if (fl[i].item == it) pos = (int)i;
      if (pos < 0) return -1;
      for (size_t i = pos + 1; i < fl.size(); i++) nfl += fl[i].pieces;
      fl.erase(fl.begin(), fl.begin() + pos + 1);
      return nfl;
   }
   void clear() { fl.clear(); }
   // between the code in front of the loop and the loop body: the blocks requested there are blocks 0.. of the tile the loop starts with
   void renumber_blocks(int by)
   {
      for (Entry &e : fl)
         if (e.item.kind == JitItem::RING) e.item.i += by;
   }
};

// ---- the 61-state walk: one straight-line kernel for one program ------------------------------------------------------------
//
// Schedule (all static): the program's operand blocks are consumed in stream order through a ring of four LDS buffers
// that runs on across tiles (JIT2_* in device_common.h).  Every block step is  s_waitcnt vmcnt(N) + barrier  with N =
// the DMA pieces issued after the block, then the ring is refilled up to three blocks ahead — inside the MFMA loop of
// the step's matmul where there is one.  A cherry (SET_TIP2) that follows a pushed matmul is gathered under that
// matmul's second half; the first cherry of the NEXT tile is gathered under the current tile's last matmul (the tile's
// own first cherry was done that way by its predecessor; the first tile's is peeled in front of the loop).
// A tile's walk is one straight line of code — several hundred KB for a large tree — and the hardware runs such a line several times
// slower than the same instructions with a branch every few ops (230 tips, 256 tiles per launch: 5.8 ms against 1.03 ms; an `s_branch` to
// the next instruction does as well as a compiler-visible one: profiles/r05_big_tree_split.txt).  Programs of more than JIT_SPLIT_OPS ops
// get a never-taken uniform branch (JIT_SPLIT) every eighth op; the compiler then also works on blocks of a few thousand instructions
// instead of one of 10^5 (192 taxa: 28 s instead of 130 on this container's core), so one full build serves: no quick build in front of it.
// Small programs get the compiler-visible form too: no front-end effect there (a bare s_branch changes nothing at 16 taxa), but the
// compiler's schedule of the shorter blocks measures 0.6 % faster (kernel 1.554 -> 1.544 ms at 16 taxa x 10^6 patterns, two runs each).
static const size_t JIT_SPLIT_OPS = 8;
inline bool jit_split_mode(size_t nops) { return nops > JIT_SPLIT_OPS; }
// One generation of the 61-state walk: `first` = operand blocks of a tile already requested when the loop body starts (the body's last
// step leaves the same number of the next tile's in flight; first_out reports it so that jit_generate can make the two agree).
struct JitWalk {
   const Program &p;
   const int n_tips, n_states, n_codes, first;
   const std::vector<CherryTab> *const tabs;
   const JitProf &prof;
   const int n_top;      // subtree tables: lookups of the walk that read one (their class indices are rows of the tile's code block)
   const bool ordered;   // ... and the tiles hold the patterns in the order PruneArgs::order: the root stores at order[position]
   static constexpr int waves = 8, TP = waves * 16;
   const int nblk = (int)p.stream.size() / 2;
   const size_t nops = p.ops.size();
   const JitZPlan zpl = jit_zplan(p, n_tips, TP);
   const int ZP = n_top ? jit_zpieces(jit_subtree_zrows(n_tips, n_top), TP) : zpl.ZP, ZR = (ZP * 8 + waves - 1) / waves;      // code block (or piece): 2 KB units; DMA rounds per wave
   // fewer than four operand blocks left per tile (subtree tables: the headline tree keeps none): the ring never runs more than one tile
   // ahead, nothing of the next tile is started early, and a tile ends with everything it requested landed — see tile_tail
   const bool short_form = n_top > 0 && nblk < 4;
   // states beyond n are zero padding: only RB row blocks and KB k-blocks of every P take part (4 and 16 at 61 states)
   const int RB = (n_states + 15) / 16, KB = (n_states + 3) / 4, KB2 = (KB + 1) / 2, NPc = KB2;   // NPc: 16-byte pieces per tip-table row
   const bool fuse_tips = KB2 >= 2;   // cherries gathered under the preceding matmul
   const int MID = KB2 / 2;           // ... from this k-block pair on (jit_matvec_tip2)
   // chunks of a tip table that hold codes of this data set (two codes per 1 KB chunk)
   const int TCH = (n_codes + 1) / 2 >= 31 ? 32 : (n_codes + 1) / 2;
   // DMA rounds per block: a P has chunks pair * 4 + row block (< KB2 * 4 used), a tip table TCH chunks; `waves` chunks per round
   const int P_ROUNDS = (KB2 * 4 + waves - 1) / waves, T_ROUNDS = (TCH + waves - 1) / waves;
   // 61 states: the last k-block of P is the single column 60 — its rank-1 term goes through the vector pipe (a 512-byte
   // column table travels with every P block as a fifth DMA piece) and the k-block's four MFMAs are dropped
   const bool tail61 = n_states == 61;
   const bool amb_over = n_codes > 64;      // codes beyond the 64 a ring block has rows for: summed from the rows of their states (device_common.h)
   const std::string ambarg = amb_over ? ", amb" : "";
   const int last_mm = [&] {
      int at = -1;
      for (size_t i = 0; i < nops; i++)
         if (p.ops[i].code == OP_MATMUL || p.ops[i].code == OP_MATMUL_POP) at = (int)i;
      return at;
   }();
   // the next tile's first cherry rides under this tile's last matmul
   // (only when that matmul is the tile's last consumer of operand blocks: the ring has no room for more)
   const bool tail_blocks = [&] {
      for (size_t i = last_mm + 1; i < nops; i++)
         if (p.ops[i].code == OP_SET_TIP || p.ops[i].code == OP_MUL_TIP || p.ops[i].code == OP_SET_TIP2 || p.ops[i].code == OP_MUL_TIP2) return true;
      return false;
   }();
   // one code block only (large trees): it is replaced between tiles, so nothing of the next tile can start early
   const bool zsingle = zpl.bufs == 1, zhalf = zpl.half;
   const bool peel = fuse_tips && nops > 2 && p.ops[0].code == OP_SET_TIP2 && last_mm > 1 && p.ops[1].code != OP_MUL_TIP &&
                     p.ops[1].code != OP_MUL_TIP2 && !tail_blocks && !zsingle && !short_form;      // the tile's first cherry is produced by its predecessor, into AS
   // cherry tables (OP_LOOKUP): the rows of a lookup are requested LA lookups ahead of their use, so that a product lies between request
   // and use; those of a tile's first lookups under the previous tile's last product (or, in front of the loop, for the first tile),
   // into arrays of their own
   const std::vector<int> lk_op = [&] {      // the program's lookups, in order: op index
      std::vector<int> at;
      for (size_t i = 0; i < nops; i++)
         if (p.ops[i].code == OP_LOOKUP) at.push_back((int)i);
      return at;
   }();
   const int nlk = (int)lk_op.size();
   const bool lk_cross = nlk > 0 && !peel && !zsingle && !short_form;      // the first lookups of a tile are requested by its predecessor
   // (trees that keep three or more partials stacked in registers: one lookup ahead — with two the 23-taxon random tree of the tests
   //  spills 18 VGPRs)
   const int LA = std::min(p.max_stack, JIT_REG_SLOTS) >= 3 ? 1 : JIT_LOOKAHEAD;
   const int lk_ncross = lk_cross ? std::min(nlk, LA) : 0;
   const int NA = std::min(p.max_stack, JIT_REG_SLOTS) + 2 + (fuse_tips ? 1 : 0) + (nlk ? LA : 0);      // arrays of the pool
   const bool resident = [&] {      // the program stores or loads resident partials (keep-partials mode)
      for (const Op &o : p.ops)
         if (o.code == OP_STORE || o.code == OP_LOAD) return true;
      return false;
   }();
   const bool split_mode = jit_split_mode(nops);      // a branch every `split_every` ops, see jit_split_mode
   static constexpr int split_every = 8;

   std::ostringstream s;
   JitRegs regs{NA, JIT_REG_SLOTS};
   JitInFlight fl;
   int issued = 0, consumed = 0;             // operand blocks requested / used so far
   int cur_piece = 0;                        // (piece mode) the piece of the tile's codes that is in LDS
   bool z_pending = false;                   // the next tile's code block still has to be requested in this tile
   std::vector<std::string> pend_store;      // the pieces of a STORE that ride under the product that follows it (see step_side)
   std::vector<std::pair<int, std::string>> pend_lookup;      // (lookup, text): the next tile's, requested in the last iteration of the product that follows
   std::vector<JitArr> lk_arr = std::vector<JitArr>(nlk);     // lookup -> its array
   int lk_issued = 0, lk_seen = 0;           // lookups of this tile requested / consumed so far
   bool lk_next_done = false;                // the next tile's first lookups are requested

   JitWalk(const Program &p_, int n_tips_, int n_states_, int n_codes_, int first_, const std::vector<CherryTab> *tabs_, const JitProf &prof_, int n_top_ = 0, bool ordered_ = false)
      : p(p_), n_tips(n_tips_), n_states(n_states_), n_codes(n_codes_), first(first_), tabs(tabs_), prof(prof_), n_top(n_top_), ordered(ordered_ && n_top_ > 0) {}

   // ---- text of the operands ----
   int n_rounds(int blk) const { return p.stream[2 * (blk % nblk)] ? T_ROUNDS : P_ROUNDS; }
   int n_pieces(int blk) const { return n_rounds(blk) + ((tail61 && !p.stream[2 * (blk % nblk)]) ? 1 : 0); }
   std::string piece(int blk, int c4) const      // one DMA piece of block blk (the last one of a P: the column table)
   {
      const bool nx = blk >= nblk;
      const int loc = blk % nblk, is_tip = p.stream[2 * loc], node = p.stream[2 * loc + 1];
      if (c4 == n_rounds(blk)) return std::string("JIT2_PIECE_") + (nx ? "NPC(" : "PC(") + std::to_string(blk) + ", " + std::to_string(node) + ");";
      return std::string("JIT2_PIECE_") + (nx ? "N" : "") + (is_tip ? "T(" : "P(") + std::to_string(blk) + ", " + std::to_string(node) + ", " +
             std::to_string(c4) + ");";
   }
   std::string code(int tip, bool next = false) const { return (next ? "JIT2_NCODE(" : "JIT2_CODE(") + std::to_string(ZP) + ", " + std::to_string(zpl.row[tip]) + ")"; }
   std::string buf(int blk) const { return "JIT2_BUF(" + std::to_string(blk) + ")"; }
   std::string colarg(int blk) const { return tail61 ? ", JIT2_COL(" + std::to_string(blk) + "), x60" : std::string(); }
   std::string issue_z() const { return zhalf ? "JIT2_ISSUE_ZH(" + std::to_string(ZP) + ", n_tile, 0)" : "JIT2_ISSUE_Z(" + std::to_string(ZP) + ")"; }
   static std::string spill_ptr(int slot_no) { return "JIT_SPILL_PTR(" + std::to_string(slot_no - JIT_SCRATCH_BASE) + ")"; }
   // the rows of lookup k into array `arr`: of this tile, or (next) of the tile after it, into its AL array
   std::string lookup_text(int k, bool next) const
   {
      const Op &o = p.ops[lk_op[k]];
      if (o.c >= SUBTREE_TAB_BASE) {      // a subtree table: the row is the pattern's class, from the index rows behind the weight flags
         const int tn = o.c - SUBTREE_TAB_BASE;
         return "jit_lookup_row(" + (next ? JitArr{JitArr::NEXT_LOOKUP, k} : lk_arr[k]).name() + ", JIT_STAB(" + (next ? "n_iclass" : "iclass") + ", " + std::to_string(tn) + "), " +
                (next ? "JIT2_NIDX(" : "JIT2_IDX(") + std::to_string(ZP) + ", " + std::to_string(n_tips + 1 + 3 * tn) + "), JIT_STAB_U(" + std::to_string(tn) + "), q);";
      }
      const CherryTab &t = (*tabs)[o.c];
      return "jit_lookup(" + (next ? JitArr{JitArr::NEXT_LOOKUP, k} : lk_arr[k]).name() + ", JIT_CTAB(" + (next ? "n_iclass" : "iclass") + ", " + std::to_string(o.c) +
             "), " + code(t.tip_a, next) + ", " + code(t.tip_b, next) + ", q);";
   }

   // ---- the schedule ----
   // the ring is refilled up to three blocks ahead, and never beyond the next tile's blocks (whose P set is the one known)
   int ahead() const { return std::min(consumed + 4, 2 * nblk); }
   void issue_now()
   {
      s << "  ";
      for (int c4 = 0; c4 < n_pieces(issued); c4++) s << " " << piece(issued, c4);
      s << "\n";
      fl.issue({JitItem::RING, issued}, n_pieces(issued));
      issued++;
   }
   // make the next c blocks visible: wait for them, barrier, and (once per tile, behind its first barrier) request the next tile's codes
   void arrive(int c)
   {
      // (a step whose blocks the ring has not been asked for yet — a cherry right after the tile's first one, as the forests of the branch-local
      //  refill have them: the top-up of the step before stopped short of it.  Every wave is done with the slots they go to after a barrier.)
      if (issued < consumed + c) {
         s << "   JIT_SYNC();\n";
         while (issued < consumed + c) issue_now();
      }
      const int nw = fl.wait_for({JitItem::RING, consumed + c - 1});
      if (nw >= 0) s << "   JIT_WAIT(" << nw << ");";
      s << "   JIT_SYNC();\n";
      if (z_pending) {
         s << "   JIT2_ISSUE_Z(" << ZP << ")\n";
         fl.issue({JitItem::CODES, 0}, ZR);
         z_pending = false;
      }
   }
   // a block step of an op without a product: arrive, then top the ring up at once, to three blocks ahead
   void step(int c)
   {
      arrive(c);
      if (!pend_store.empty()) {
         s << "  ";
         for (const std::string &st : pend_store) s << " " << st;
         s << "\n";
         fl.issue({JitItem::MEM, 0}, (int)pend_store.size());
         pend_store.clear();
      }
      while (issued < ahead()) issue_now();
   }
   // a product's block step: arrive, and the refill as a `side` functor that spreads its pieces over the first `iters` k-block pairs
   // of the matmul that follows
   std::string step_side(int iters)
   {
      arrive(1);
      struct Piece { JitItem item; std::string text; };
      std::vector<Piece> pieces;
      for (; issued < ahead(); issued++)
         for (int c4 = 0; c4 < n_pieces(issued); c4++) pieces.push_back({{JitItem::RING, issued}, piece(issued, c4)});
      if (pieces.empty() && pend_store.empty() && pend_lookup.empty()) return "JitNoSide()";
      const int per = pieces.empty() ? 1 : ((int)pieces.size() + iters - 1) / iters;
      std::vector<std::vector<Piece>> at(iters);
      for (size_t i = 0; i < pieces.size(); i++) at[i / per].push_back(pieces[i]);
      // a STORE waiting for this product (keep-partials mode: the partial it multiplies): its eight 1 KB wave stores go out one per
      // k-block pair, under the MFMAs — issued together they hold the CU's store path for ~5 000 cycles during which no wave of the
      // workgroup gets to its MFMAs (measured: 2.2 ms per evaluation at 16 taxa x 10^6 codon patterns against 1.56 without the stores).
      for (size_t i = 0; i < pend_store.size(); i++) at[i * iters / pend_store.size()].push_back({{JitItem::MEM, 0}, pend_store[i]});
      pend_store.clear();
      // the next tile's lookups: behind every DMA piece of this step — the order the code in front of the loop issues them in
      for (const std::pair<int, std::string> &lk : pend_lookup)
         for (int i = 0; i < 8; i++) at[iters - 1].push_back({{JitItem::LOOKUP, lk.first}, i ? std::string() : lk.second});
      pend_lookup.clear();
      // the in-flight list records every piece where it is issued
      std::string f = "[&](int kb2) {";
      for (int i = 0; i < iters; i++) {
         if (at[i].empty()) continue;
         f += " if (kb2 == " + std::to_string(i) + ") {";
         for (const Piece &pc : at[i]) {
            f += " " + pc.text;
            fl.add_piece(pc.item);
         }
         f += " }";
      }
      return f + " }";
   }
   void stamp(size_t iop)
   {
      if (prof.ops && iop % prof.every == 0)
         s << "   if (a.prof && tid == a.prof_tid && ptile) a.prof[(long)blockIdx.x * a.prof_stride + 1 + " << iop
           << "] = __builtin_amdgcn_s_memtime();\n";
      else if (!prof.ops && split_mode && iop && iop % split_every == 0)
         s << "   JIT_SPLIT()\n";
   }
   // (piece mode) rows of a later piece are needed from here on: every wave is done with the piece in LDS, the next comes over it
   void cross_if(std::initializer_list<int> tips)
   {
      if (!zhalf) return;
      int need = cur_piece;
      for (int t : tips) need = std::max(need, zpl.piece[t]);
      while (cur_piece < need) {
         cur_piece++;
         s << "   __syncthreads();\n   JIT2_ISSUE_ZH(" << ZP << ", cur_tile, " << cur_piece << ")\n   JIT_WAIT(0); __syncthreads();\n";
         fl.clear();
      }
   }
   void issue_lookup(int k)
   {
      lk_arr[k] = regs.alloc();
      s << "   " << lookup_text(k, false) << "\n";
      fl.issue({JitItem::LOOKUP, k}, 8);
   }
   void issue_next_lookups()      // (behind every operand block the tile requests: the order the code in front of the loop has)
   {
      for (int k = 0; k < lk_ncross; k++) {
         s << "   " << lookup_text(k, true) << "\n";
         fl.issue({JitItem::LOOKUP, k}, 8);
      }
      lk_next_done = true;
   }
   void finish_product(const JitArr &out, int pop, int push)
   {
      regs.finish_product(out, pop, push, [&](JitRegs::Step st, const JitArr &o, const JitArr &in) {
         if (st == JitRegs::MUL) s << "   jit_mul(" << o.name() << ", " << in.name() << ");\n";
         else s << (st == JitRegs::SPILL ? "   jit_spill(" : "   jit_mul_mem(") << o.name() << ", " << spill_ptr(in.i) << ");\n";
      });
   }

   // ---- the stages ----
   void defines_and_prologue()
   {
      s << "#define JIT_KB2 " << KB2 << "\n#define JIT_RB " << RB << "\n#define JIT_TCH " << TCH << "\n#define JIT_WAVES " << waves << "\n";
      if (zsingle) s << "#define JIT_ZB 1\n";
      if (zhalf) s << "#define JIT_ZPIECES " << zpl.pieces << "\n";
      if (amb_over) s << "#define JIT_AMB_OVERFLOW 1\n";
      if (nlk) s << "#define JIT_NC " << n_codes << "\n";
      s << "#include \"device_common.h\"\nusing namespace paml_amd;\n";
      s << "extern \"C\" __global__ __launch_bounds__(" << waves * 64 << ", " << waves / 4 << ") void prune_jit(PruneArgs a)\n{\n";
      s << "   JIT2_PROLOGUE(" << ZP << ")\n";
      if (amb_over) {      // the state sets of the codes 64 .. : into the three quarters of sPi a single frequency vector leaves unused (192 x 8 bytes)
         s << "   if (a.n_pi == 1) for (int i = tid; i < a.n_codes - 64; i += JIT_WAVES * 64) ((unsigned long long *)sPi)[64 + i] = a.code_mask[64 + i];\n";
         s << "   const JitAmb amb{a.code_mask, (__attribute__((address_space(3))) const unsigned long long *)(sPi + 64), a.n_pi == 1};\n";
      }
      s << "   roff = " << ((4 - nblk % 4) & 3) << ";\n";
      for (int i = 0; i < NA; i++) s << "   v4d A" << i << "[4];\n";
      if (peel) s << "   v4d AS[4];\n";
      for (int k = 0; k < lk_ncross; k++) s << "   v4d AL" << k << "[4];\n";
   }
   // in front of the loop: the first tile is the "next" tile of an empty predecessor
   void front_of_loop()
   {
      s << "   JIT2_NEXT_SET()\n   " << issue_z() << "\n";
      fl.issue({JitItem::CODES, 0}, ZR);
      issued = nblk;                           // numbered as the blocks after the (empty) predecessor's
      for (int i = 0; i < first; i++) issue_now();
      if (peel) {
         const int nw = fl.wait_for({JitItem::RING, nblk + 1});
         s << "   JIT_WAIT(" << nw << "); __syncthreads();\n";
         s << "   jit_tip2_set<" << NPc << ">(AS, " << buf(nblk) << ", " << code(p.ops[0].a, true) << ", " << buf(nblk + 1) << ", " << code(p.ops[0].b, true) << ", q, lane" << ambarg << ");\n";
      }
      if (lk_ncross) {      // (the first tile's codes have to be there; the list keeps its items: the waits of later trips need them)
         s << "   JIT_WAIT(0); __syncthreads();\n";
         issue_next_lookups();
      }
      if (zsingle || short_form) {      // everything requested so far has to be there when the loop starts: the same state the loop's end leaves
         s << "   JIT_WAIT(0); __syncthreads();\n";
         fl.clear();
      }
      fl.renumber_blocks(-nblk);
      issued = first;
      consumed = peel ? 2 : 0;
   }
   void tile_head()
   {
      if (prof.tiles) s << "   int ptc = 0; if (a.prof && tid == 0) { a.prof[(long)blockIdx.x * a.prof_stride] = __builtin_amdgcn_s_memrealtime(); a.prof[(long)blockIdx.x * a.prof_stride + a.prof_stride - 2] = __builtin_amdgcn_s_memtime(); }\n";
      s << "   int ptile = 1;\n   for (;; ptile = 0) {\n";
      s << "   JIT2_ADVANCE(" << nblk << ")\n";
      if (ordered) s << "   JIT2_ORDER()\n";
      // (n_tile is still this tile's number here; the groups of a tile's waves that start past its gene's end belong to nobody: not stored)
      if (resident) s << "   const int tg0 = as_const(a.tile_group0)[n_tile];\n   const bool wave_in = h0 + wave * 16 < hend;\n";
      if (zhalf) s << "   const int cur_tile = n_tile;\n";
      s << "   work += gridDim.x;\n   JIT2_NEXT_SET()\n";
      z_pending = !zsingle;
      if (short_form) {      // (every tile ends behind a barrier with nothing in flight: the other code buffer is free from here on)
         s << "   JIT2_ISSUE_Z(" << ZP << ")\n";
         fl.issue({JitItem::CODES, 0}, ZR);
         z_pending = false;
      }
      if (peel) regs.cur = {JitArr::NEXT_CHERRY, 0};
      if (prof.ops) s << "   if (a.prof && tid == a.prof_tid && ptile) a.prof[(long)blockIdx.x * a.prof_stride] = __builtin_amdgcn_s_memtime();\n";
      lk_issued = lk_ncross;
      lk_next_done = !lk_cross;
      for (int k = 0; k < lk_ncross; k++) lk_arr[k] = {JitArr::NEXT_LOOKUP, k};
      if (nlk && !lk_cross)
         while (lk_issued < std::min(nlk, LA)) issue_lookup(lk_issued++);
   }
   void tile_tail()
   {
      if (!lk_next_done) issue_next_lookups();
      // programs whose steps never came by a barrier after the tile switch (no operand blocks): request the codes here
      if (z_pending) {
         s << "   __syncthreads();\n   JIT2_ISSUE_Z(" << ZP << ")\n";
         fl.issue({JitItem::CODES, 0}, ZR);
      }
      if (short_form) {      // the next tile's codes (its lookups read them at its start) and whatever of its blocks is on the way: landed, for every wave
         s << "   JIT_WAIT(0); __syncthreads();\n";
         fl.clear();
      }
      if (zsingle) {      // all waves are done with this tile's codes: fetch the next tile's (first piece) over them, and wait (once per tile)
         s << "   __syncthreads();\n   " << issue_z() << "\n   JIT_WAIT(0); __syncthreads();\n";
         fl.clear();
      }
      if (prof.tiles) s << "   if (a.prof && tid == 0 && ptc < a.prof_stride - 4) { a.prof[(long)blockIdx.x * a.prof_stride + 1 + ptc] = __builtin_amdgcn_s_memrealtime(); a.prof[(long)blockIdx.x * a.prof_stride + a.prof_stride - 1] = __builtin_amdgcn_s_memtime(); }\n   ptc++;\n";
      s << "   if (!has_next) break;\n   }\n   JIT_WAIT(0);\n}\n";
   }

   // ---- the ops ----
   void op_init(const Op &o)
   {
      regs.start_partial();
      if (o.code == OP_INIT_TIP) cross_if({o.a});
      if (o.code == OP_INIT_TIP) s << "   jit_init_tip(" << regs.cur.name() << ", " << code(o.a) << ", q, a.cleandata);\n";
      else s << "   jit_init_ones(" << regs.cur.name() << ", q, n);\n";
   }
   void op_tip(const Op &o)      // SET_TIP, MUL_TIP
   {
      if (o.code == OP_SET_TIP) regs.start_partial();
      cross_if({o.a});
      step(1);
      s << "   " << (o.code == OP_SET_TIP ? "jit_tip_set<" : "jit_tip_mul<") << NPc << ">(" << regs.cur.name() << ", " << buf(consumed) << ", " << code(o.a) << ", q, lane" << ambarg << ");\n";
      consumed += 1;
   }
   void op_tip2(const Op &o)      // SET_TIP2, MUL_TIP2
   {
      if (o.code == OP_SET_TIP2 || regs.cur.kind == JitArr::NONE) regs.start_partial();
      cross_if({o.a, o.b});
      step(2);
      s << "   " << (o.code == OP_SET_TIP2 ? "jit_tip2_set<" : "jit_tip2_mul<") << NPc << ">(" << regs.cur.name() << ", " << buf(consumed) << ", " << code(o.a)
        << ", " << buf(consumed + 1) << ", " << code(o.b) << ", q, lane" << ambarg << ");\n";
      consumed += 2;
   }
   void op_lookup(const Op &o)
   {
      const int j = lk_seen++;
      while (lk_issued < nlk && lk_issued <= j + LA) issue_lookup(lk_issued++);
      regs.release(regs.cur);
      const int nw = fl.wait_for({JitItem::LOOKUP, j});
      if (nw >= 0) s << "   JIT_WAIT(" << nw << ");\n";
      if (lk_arr[j].kind == JitArr::NEXT_LOOKUP) {      // (the predecessor's array is wanted again under this tile's last product)
         const JitArr own = regs.alloc();
         s << "   jit_copy(" << own.name() << ", " << lk_arr[j].name() << ");\n";
         lk_arr[j] = own;
      }
      finish_product(lk_arr[j], mm_pop_slot(o), mm_push_slot(o));
   }
   // wait, barrier, refill (as the product's side functor), product, pop / push
   void op_product(size_t &iop)
   {
      const Op &o = p.ops[iop];
      const int pop = mm_pop_slot(o), push = mm_push_slot(o);
      const JitArr in = regs.cur, out = regs.alloc();
      const Op *const after = iop + 1 < nops && p.ops[iop + 1].code == OP_SET_TIP2 ? &p.ops[iop + 1] : nullptr;
      // a cherry right after a pushed matmul: its two tip gathers ride under this matmul's second half
      // (piece mode: a cherry whose codes lie in the NEXT piece is not folded under this product — the crossing then happens at the cherry's
      //  own step; there are at most pieces - 1 of them per tile.  The folded form gave a wrong lnL once on the 1 000-tip tree of
      //  tests/test_engine_gpu.py, cause not found, and was removed.)
      const bool crossing_cherry = zhalf && after && std::max(zpl.piece[after->a], zpl.piece[after->b]) > cur_piece;
      const bool fuse = fuse_tips && push >= 0 && after && !crossing_cherry;
      const bool fuse_next = peel && (int)iop == last_mm;     // ... or the next tile's first cherry under the last matmul
      if (fuse) cross_if({after->a, after->b});
      // (tip tables the ring could not hold earlier are requested in the first k-block pairs and awaited at the midpoint)
      // (the cross-lane read of x[60] is issued before the step's wait + barrier so that its latency hides there)
      if (tail61) s << "   { const double x60 = jit_x60(" << in.name() << ", lane);\n";
      // the next tile's first lookups: under this, the tile's last, product — once this tile has consumed its own (a cherry that is a
      // son of the root comes AFTER the last product and still lives in its AL array: then they are requested in front of ROOT)
      if (lk_cross && (int)iop == last_mm && !tail_blocks && !fuse && !fuse_next && lk_seen >= lk_ncross) {
         for (int k = 0; k < lk_ncross; k++) pend_lookup.push_back({k, lookup_text(k, true)});
         lk_next_done = true;
      }
      const std::string side = step_side((fuse || fuse_next) ? MID : KB2);
      JitArr tgt;
      if (fuse || fuse_next) {
         const Op &nx = fuse ? *after : p.ops[0];
         tgt = fuse ? regs.alloc() : JitArr{JitArr::NEXT_CHERRY, 0};
         const int mid = fl.wait_for({JitItem::RING, consumed + 2});
         s << "   jit_matvec_tip2<" << (mid < 0 ? 63 : mid) << (tail61 ? ", true, " : ", false, ") << RB << ", " << KB << ">(" << buf(consumed) << ", lane, " << in.name()
           << ", " << out.name() << ", " << buf(consumed + 1) << ", " << code(nx.a, !fuse) << ", " << buf(consumed + 2) << ", "
           << code(nx.b, !fuse) << ", q, " << tgt.name() << ", " << side << colarg(consumed) << (amb_over ? (tail61 ? ", amb" : ", nullptr, 0.0, amb") : "") << ");"
           << (tail61 ? " }" : "") << "\n";
         consumed += 3;
      }
      else {
         s << "   jit_matvec<" << (tail61 ? "true" : "false") << ", " << RB << ", " << KB << ">(" << buf(consumed) << ", lane, " << in.name() << ", "
           << out.name() << ", "
           << side << colarg(consumed) << ");" << (tail61 ? " }" : "") << "\n";
         consumed += 1;
      }
      regs.release(in);
      finish_product(out, pop, push);
      if (fuse) {      // the SET_TIP2 is done
         regs.cur = tgt;
         stamp(++iop);
      }
   }
   void op_scale(const Op &o)
   {
      s << "   { const double fac = jit_scale(" << regs.cur.name() << ", q, n); lnscale += fac;\n"
        << "     if (a.keep && q == 0 && valid) a.scalef[((long)iclass * a.n_scale + " << o.b << ") * a.n_patt + h] = fac; }\n";
   }
   // STORE / LOAD: eight vector-memory operations per wave, entered in the in-flight list like the ring's DMA pieces (see JitInFlight)
   void op_store(size_t iop)
   {
      const Op &o = p.ops[iop];
      const bool under_product = iop + 1 < nops && (p.ops[iop + 1].code == OP_MATMUL || p.ops[iop + 1].code == OP_MATMUL_POP) && p.ops[iop + 1].a == o.a;
      if (under_product)      // (the product that follows reads this very array and leaves it alone: see step_side)
         for (int i = 0; i < 8; i++)
            pend_store.push_back("JIT_STORE_PIECE(" + regs.cur.name() + ", JIT_PART_DST(" + std::to_string(o.a) + "), " + std::to_string(i) + ");");
      else {
         s << "   jit_store(" << regs.cur.name() << ", JIT_PART_DST(" << o.a << "), lane);\n";
         fl.issue({JitItem::MEM, 0}, 8);
      }
   }
   void op_load(const Op &o)
   {
      regs.start_partial();
      s << "   jit_load(" << regs.cur.name() << ", JIT_PART_PTR(" << o.a << "), lane);\n";
      fl.issue({JitItem::MEM, 0}, 8);
   }
   void op_root()
   {
      cross_if({n_tips});      // (the weight flags: the last row)
      if (!lk_next_done) issue_next_lookups();
      // keep-partials mode with scaling nodes: the factors of clean subtrees were stored by earlier evaluations — all of them are
      // summed from memory in slot order, as the interpreter kernels do (MFMA_ROOT_CASE; treesub.c:7746-7747)
      if (resident)
         s << "   if (a.keep && a.n_scale) { lnscale = 0; if (valid) for (int k_ = 0; k_ < a.n_scale; k_++) lnscale += a.scalef[((long)iclass * a.n_scale + k_) * a.n_patt + h]; }\n";
      s << "   jit_root_lds(a, " << regs.cur.name() << ", lnscale, sPi + (a.n_pi > 1 ? gene : 0) * 64, " << code(n_tips)
        << ", iclass, q, " << (ordered ? "hs" : "h") << ", valid);\n";
      regs.end_partial();
   }

   std::string generate(int *first_out)
   {
      defines_and_prologue();
      front_of_loop();
      tile_head();
      for (size_t iop = 0; iop < nops; iop++) {
         const Op &o = p.ops[iop];
         stamp(iop);
         if (iop == 0 && peel) continue;      // done by the predecessor
         switch (o.code) {
         case OP_INIT_ONES: case OP_INIT_TIP: op_init(o); break;
         case OP_SET_TIP: case OP_MUL_TIP: op_tip(o); break;
         case OP_SET_TIP2: case OP_MUL_TIP2: op_tip2(o); break;
         case OP_LOOKUP: op_lookup(o); break;
         case OP_PUSH: regs.push(o.b, [&](JitRegs::Step, const JitArr &c, const JitArr &to) { s << "   jit_spill(" << c.name() << ", " << spill_ptr(to.i) << ");\n"; }); break;
         case OP_MATMUL: case OP_MATMUL_POP: op_product(iop); break;
         case OP_SCALE: op_scale(o); break;
         case OP_STORE: op_store(iop); break;
         case OP_LOAD: op_load(o); break;
         case OP_ROOT: op_root(); break;
         default: break;
         }
      }
      tile_tail();
      *first_out = issued - nblk;
      return regs.exhausted ? jit_exhausted_source() : s.str();
   }
};

// (`tabs`: p is the table form of the tree's program — jit_cherry_program — and these are its tables)
// (n_top: p is the table form with subtree tables — jit_subtree_program — and so many of its lookups read one; ordered: its tiles hold the
//  patterns in the order PruneArgs::order)
inline std::string jit_generate(const Program &p, int n_tips, int n_states = 61, int n_codes = 64, const std::vector<CherryTab> *tabs = nullptr, int n_top = 0,
                                bool ordered = false)
{
   const JitProf prof;
   int first = std::min(3, (int)p.stream.size() / 2), got = first;
   std::string src = JitWalk(p, n_tips, n_states, n_codes, first, tabs, prof, n_top, ordered).generate(&got);
   if (got != first) {
      first = got;
      src = JitWalk(p, n_tips, n_states, n_codes, first, tabs, prof, n_top, ordered).generate(&got);
   }
   if (got != first) return std::string("#error \"jit schedule does not close\"\n");
   return src;
}

// The one-pattern-per-lane kernels (4 / 5 / 20 states) specialised the same way: the op interpreter of prune_valu<N>
// unrolled into straight-line code over renamed register arrays.
inline bool jit_valu_supported(const Program &p, int max_arrays = 8)
{
   if (p.ops.size() > 600) return false;
   for (const Op &o : p.ops)
      if (o.code == OP_STORE || o.code == OP_LOAD || o.code == OP_EXPORT) return false;
   return p.max_stack + 2 <= max_arrays;
}

inline std::string jit_generate_valu(const Program &p, int N)
{
   std::ostringstream s;
   s << "#include \"device_common.h\"\nusing namespace paml_amd;\n";
   s << "extern \"C\" __global__ __launch_bounds__(256) void prune_jit(PruneArgs a)\n{\n   JV_PROLOGUE(" << N << ")\n";
   const int NA = p.max_stack + 2;
   for (int i = 0; i < NA; i++) s << "   double A" << i << "[N];\n";
   JitRegs regs(NA);
   const JitArr &cur = regs.cur;
   const char *LOOP = "_Pragma(\"unroll\") for (int j = 0; j < N; j++) ";
   auto mul_popped = [&](JitRegs::Step, const JitArr &out, const JitArr &in) { s << "   " << LOOP << out.name() << "[j] = " << in.name() << "[j] * " << out.name() << "[j];\n"; };
   for (const Op &o : p.ops) {
      switch (o.code) {
      case OP_INIT_ONES:
         regs.start_partial();
         s << "   " << LOOP << cur.name() << "[j] = 1.0;\n";
         break;
      case OP_INIT_TIP:
         regs.start_partial();
         s << "   { const int c = JV_CODE(" << o.a << "); " << LOOP << cur.name() << "[j] = (a.cleandata && j == c) ? 1.0 : 0.0; }\n";
         break;
      case OP_SET_TIP: case OP_MUL_TIP:
         regs.start_partial();
         s << "   { const double *r = JV_ROW(" << o.a << ", JV_CODE(" << o.a << ")); " << LOOP << cur.name()
           << (o.code == OP_SET_TIP ? "[j] = r[j]; }\n" : "[j] *= r[j]; }\n");
         break;
      case OP_SET_TIP2: case OP_MUL_TIP2:
         regs.start_partial();
         s << "   { const double *r1 = JV_ROW(" << o.a << ", JV_CODE(" << o.a << ")), *r2 = JV_ROW(" << o.b << ", JV_CODE(" << o.b << ")); "
           << LOOP << cur.name() << (o.code == OP_SET_TIP2 ? "[j] = r1[j] * r2[j]; }\n" : "[j] = (" + cur.name() + "[j] * r1[j]) * r2[j]; }\n");
         break;
      case OP_PUSH: regs.push(o.b, mul_popped); break;
      case OP_MATMUL: case OP_MATMUL_POP: {
         const JitArr in = cur, out = regs.alloc();
         s << "   jv_matvec<N>(Pint + " << (long)o.a * N * N << ", " << in.name() << ", " << out.name() << ");\n";
         regs.release(in);
         regs.finish_product(out, mm_pop_slot(o), mm_push_slot(o), mul_popped);
      } break;
      case OP_SCALE:
         s << "   { const double fac = jv_scale<N>(" << cur.name() << "); lnscale += fac;\n"
           << "     if (a.keep && valid) a.scalef[((long)iclass * a.n_scale + " << o.b << ") * a.n_patt + h] = fac; }\n";
         break;
      case OP_ROOT:
         s << "   jv_root<N>(a, " << cur.name() << ", lnscale, gene, iclass, h, valid);\n";
         regs.end_partial();
         break;
      default: break;
      }
   }
   s << "}\n";
   return regs.exhausted ? jit_exhausted_source() : s.str();
}

// ---- fused variant (4 / 5 states): classes as the inner loop, tip factors from LDS tables, reduction in the epilogue --------
// Specialised on the program, the number of states N, of character codes NC, of classes K and on the shape below.
// See the block comment at jvf_row_set (device_common.h) for the design.
//   R  = patterns per lane (1 or 2): with two, every P(t) entry fetched through the scalar cache feeds two FMAs and the
//        waits on those fetches come half as often — the big-problem shape;
//   CW = class groups per workgroup (1, 2 or 4): the workgroup has 256 x CW threads, group g walks the classes g, g + CW, ...
//        of the chunk's 256 patterns and the mixture is summed (in class order) by group 0 from an LDS exchange — the
//        small-problem shape: a data set of 10^5 patterns is only ~1.5 waves per SIMD otherwise.
struct ValuFusedPlan {
   bool ok = false;
   bool cherry = false;      // product tables for SET_TIP2 cherries
   int n_cherry = 0, R = 1, CW = 1;
   size_t lds_bytes = 0;
};

inline ValuFusedPlan jit_valu_fused_plan(const Program &p, int N, int n_tips, int n_codes, int K, int chunk)
{
   ValuFusedPlan pl;
   if (!jit_valu_supported(p) || (N != 4 && N != 5) || n_tips > 255 || K < 1) return pl;
   for (const Op &o : p.ops)
      if (o.code == OP_SET_TIP2) pl.n_cherry++;
   // shape: a function of the (global) chunk size only, so that every rank of a sharded evaluation picks the same kernel
   // (measured on MI355X, 32 taxa x Gamma-4: two class groups beat one and four at 10^5 and at 4 x 10^6 patterns — more waves to
   //  hide the scalar-cache latency of the P(t) fetches than one group, a smaller P(t) working set than four; two patterns per
   //  lane cost more in registers than they save: profiles/r02_valu_fused_shapes.txt)
   (void)chunk;
   pl.CW = K >= 2 ? 2 : 1;
   pl.R = 1;
   const size_t rows = (size_t)K * n_tips * n_codes * N * 8;
   const size_t ch = (size_t)K * pl.n_cherry * n_codes * n_codes * N * 8;
   const size_t xch = pl.CW > 1 ? (size_t)K * 256 * 8 : 0;
   if (rows + xch > 60 * 1024) return pl;               // (the unfused kernel, gathering from L2, takes such models)
   pl.ok = true;
   pl.cherry = pl.n_cherry > 0 && n_codes <= 8 && rows + ch + xch <= 56 * 1024;
   pl.lds_bytes = rows + (pl.cherry ? ch : 0) + xch;
   return pl;
}

// Several genes (option G: com.posG / com.rgene / com.piG; G > 1 here): a gene has its own P(t) — gene rate, per Mgene also its own
// eigen system and frequencies — so the LDS tables are one gene's.  A chunk is walked gene segment by gene segment: the tables are
// refilled where the gene changes (a workgroup's chunks ascend, so at most G + 1 times), and the 256-pattern sub-tile a boundary falls
// into is walked once per gene with the other gene's lanes switched off — every pattern keeps the lane and the turn it has in
// reduce_stage1's order, so the chunk sums keep their bits.  With G == 1 the generated text is the single-gene kernel's, unchanged.
inline std::string jit_generate_valu_fused(const Program &p, int N, int n_tips, int n_codes, int K, int chunk, int G = 1)
{
   const ValuFusedPlan pl = jit_valu_fused_plan(p, N, n_tips, n_codes, K, chunk);
   const bool MG = G > 1;
   std::ostringstream s;
   const int R = MG ? 1 : pl.R, CW = pl.CW;
   const int NC = n_codes, ROWW = n_tips * NC * N, CHW = pl.cherry ? pl.n_cherry * NC * NC * N : 0, TABW = ROWW + CHW;   // doubles per class
   const int ZW = ((n_tips + 3) / 4 + 3) / 4 * 4;      // dwords of packed codes per pattern
   const int NTH = 256 * CW;
   s << "#include \"device_common.h\"\nusing namespace paml_amd;\n";
   // the LDS tables: the tips are nodes 0 .. NT-1, so a class's rows are one contiguous run of pmat's output; for a cherry the products of
   // its two tips' rows.  Several genes: the fill is needed inside the loop over the chunks, where — inlined — the compiler computes its
   // thirty-odd loop-invariant addresses once, in front of that loop, and keeps them in registers through the whole walk (142 VGPRs
   // instead of 111: one workgroup per CU instead of two); it is a function of its own there, called where the gene changes.
   std::ostringstream fill;      // the body, in terms of `ptip0` (the tables of the element's class 0) and `cstride` (doubles per class)
   {
      fill << "   for (int ir = 0; ir < K; ir++) {\n"
           << "      const double *src = ptip0 + ir * cstride;\n"
           << "      for (int i = threadIdx.x; i < ROWW; i += NTH) sTab[ir * TABW + i] = src[i];\n"
           << "   }\n   __syncthreads();\n";
      if (pl.cherry) {
         int c = 0;
         fill << "   for (int i = threadIdx.x; i < K * NC * NC * N; i += NTH) {\n"
              << "      const int ir = i / (NC * NC * N), r = i % (NC * NC * N), ca = r / (NC * N), cb = (r / N) % NC, j = r % N;\n"
              << "      const double *rw = sTab + ir * TABW;\n";
         for (const Op &o : p.ops)
            if (o.code == OP_SET_TIP2) {
               fill << "      sTab[ir * TABW + ROWW + " << c * NC * NC * N << " + r] = rw[(" << o.a << " * NC + ca) * N + j] * rw[(" << o.b << " * NC + cb) * N + j];\n";
               c++;
            }
         fill << "   }\n   __syncthreads();\n";
      }
   }
   const std::string consts = "constexpr int N = " + std::to_string(N) + ", NC = " + std::to_string(NC) + ", K = " + std::to_string(K) + ", NT = " + std::to_string(n_tips) +
                              ", ROWW = " + std::to_string(ROWW) + ", TABW = " + std::to_string(TABW) + ", ZW = " + std::to_string(ZW) + ", CW = " + std::to_string(CW) +
                              ", NTH = " + std::to_string(NTH) + ";\n";
   if (MG) {
      s << consts << "__shared__ __attribute__((aligned(16))) double sTab[K * TABW];\n";
      s << "__device__ __attribute__((noinline)) void vf_fill(const double *ptip0, long cstride)\n{\n" << fill.str() << "}\n";
   }
   s << "extern \"C\" __global__ __launch_bounds__(" << NTH << (R > 1 ? ", 2" : "") << ") void prune_jit(PruneArgs a)\n{\n";
   if (!MG) {
      s << "   " << consts << "   (void)NT;\n";
      s << "   __shared__ __attribute__((aligned(16))) double sTab[K * TABW];\n";
   }
   if (CW > 1) s << "   __shared__ double sF[K * 256];\n";
   s << "   const int tid = threadIdx.x & 255, cw = __builtin_amdgcn_readfirstlane(threadIdx.x >> 8), bat = blockIdx.y;\n   (void)cw;\n";
   s << "   const long cls0 = (long)bat * K;\n";
   auto emit_fill = [&](const char *ind, const char *pset0) {      // pset0: parameter set of the batch element's class 0 (gene x all classes + cls0)
      if (MG) s << ind << "vf_fill(a.ptip + (" << pset0 << ") * a.n_nodes * a.tip_words, (long)a.n_nodes * a.tip_words);\n";
      else s << "   { const double *ptip0 = a.ptip + (" << pset0 << ") * a.n_nodes * a.tip_words; const long cstride = (long)a.n_nodes * a.tip_words;\n" << fill.str() << "   }\n";
   };
   if (!MG) emit_fill("   ", "cls0");
   s << "   const CONST_AS double *fK = as_const(a.freqK + bat * a.freqK_bs);\n";
   if (!MG) s << "   const CONST_AS double *pi = as_const(a.pi);\n";
   else {
      // the G + 1 gene offsets sit in scalar registers for the whole launch (independent loads, one round trip): finding a chunk's
      // gene is a chain of scalar compares — a search through memory cost every chunk a string of dependent scalar loads with
      // nothing to overlap them (measured: the batched 4-gene launch 14 % slower than the one-gene one, a single evaluation 13 us)
      s << "   int tab_gene = -1;\n   const CONST_AS int *goff = as_const(a.gene_off);\n";
      for (int g = 0; g <= G; g++) s << "   const long go" << g << " = " << "goff[" << g << "];\n";
   }
   // the workgroup's chunks: its own (gridDim.x = number of chunks: single evaluations), or every gridDim.x-th one (batched
   // evaluations: fewer, longer workgroups per element, so that the tables above are filled once per ~100 chunks)
   s << "   for (int cb = blockIdx.x; cb < a.nb_local; cb += gridDim.x) {\n";
   s << "   const long c_lo = (long)cb * a.chunk, c_hi = (c_lo + a.chunk < (long)a.n_patt) ? c_lo + a.chunk : (long)a.n_patt;\n";
   s << "   double acc = 0;\n";
   if (MG) {
      s << "   int gene = 0; long g_lo = go0, g_hi = go1;\n";
      for (int g = 1; g < G; g++) s << "   if (c_lo >= go" << g << ") { gene = " << g << "; g_lo = go" << g << "; g_hi = go" << g + 1 << "; }\n";
      s << "   for (;;) {\n";
      s << "   const long seg_lo = g_lo > c_lo ? g_lo : c_lo, seg_hi = g_hi < c_hi ? g_hi : c_hi;\n";
      s << "   if (seg_lo < seg_hi) {\n";
      s << "   const long gset0 = (long)gene * a.K + cls0;\n";
      s << "   const CONST_AS double *pi = as_const(a.pi + (a.n_pi > 1 ? gene : 0) * N);\n";
      s << "   for (long h0 = c_lo + (seg_lo - c_lo) / 256 * 256; h0 < seg_hi; h0 += 256) {\n";
   }
   else s << "   for (long h0 = c_lo; h0 < c_hi; h0 += " << 256 * R << ") {\n";
   auto sfx = [&](int r) { return R > 1 ? "_" + std::to_string(r) : std::string(); };
   for (int r = 0; r < R; r++) {
      const std::string x = sfx(r);
      if (MG)
         s << "      const long h" << x << " = h0 + " << 256 * r << " + tid;\n      const bool valid" << x << " = h" << x << " >= seg_lo && h" << x << " < seg_hi;\n      const long hc" << x
           << " = h" << x << " < c_hi ? h" << x << " : c_hi - 1;\n";      // (any pattern of the chunk: its codes are loaded before the gene's tables are known to be there)
      else
      s << "      const long h" << x << " = h0 + " << 256 * r << " + tid;\n      const bool valid" << x << " = h" << x << " < c_hi;\n      const long hc" << x
        << " = valid" << x << " ? h" << x << " : c_hi - 1;\n";
      s << "      unsigned int zw" << x << "[ZW];\n";
      s << "      { const uint4 *zp = (const uint4 *)(a.zpm + hc" << x << " * ZW);\n";
      for (int i = 0; i < ZW / 4; i++)
         s << "        { const uint4 t = zp[" << i << "]; zw" << x << "[" << 4 * i << "] = t.x; zw" << x << "[" << 4 * i + 1 << "] = t.y; zw" << x << "[" << 4 * i + 2
           << "] = t.z; zw" << x << "[" << 4 * i + 3 << "] = t.w; }\n";
      s << "      }\n";
      s << "      const double wt" << x << " = a.weights[hc" << x << "];\n";
      if (MG) {      // the tables of this segment's gene (the codes and the weight above are already on their way)
         s << "      if (gene != tab_gene) {\n         __syncthreads();\n";
         emit_fill("         ", "gset0");
         s << "         tab_gene = gene;\n      }\n";
      }
      // per-pattern table offsets (in doubles), formed once and used by every class
      s << "#define zw zw" << x << "\n";
      int c = 0;
      std::vector<char> seen(n_tips, 0);
      for (const Op &o : p.ops)
         if (o.code == OP_SET_TIP2 && pl.cherry) {
            s << "      const int oc" << c << x << " = ROWW + " << c * NC * NC * N << " + (JVF_CODE(" << o.a << ") * NC + JVF_CODE(" << o.b << ")) * N;\n";
            seen[o.a] = seen[o.b] = 1;
            c++;
         }
      for (const Op &o : p.ops) {
         auto tipoff = [&](int t) {
            if (!seen[t]) { s << "      const int ot" << t << x << " = (" << t << " * NC + JVF_CODE(" << t << ")) * N;\n"; seen[t] = 2; }
         };
         switch (o.code) {
         case OP_SET_TIP: case OP_MUL_TIP: tipoff(o.a); break;
         case OP_MUL_TIP2: tipoff(o.a); tipoff(o.b); break;
         case OP_SET_TIP2: if (!pl.cherry) { tipoff(o.a); tipoff(o.b); } break;
         case OP_INIT_TIP: s << "      const int ci" << o.a << x << " = JVF_CODE(" << o.a << ");\n"; break;
         default: break;
         }
      }
      s << "#undef zw\n";
      s << "      double fh" << x << " = 0, v" << x << " = 0;\n";
   }
   s << "      _Pragma(\"unroll 1\") for (int ir = " << (CW > 1 ? "cw" : "0") << "; ir < K; ir += CW) {\n";
   s << "         const double *Pint = a.pint + (" << (MG ? "gset0" : "cls0") << " + ir) * a.n_nodes * (N * N);\n";
   s << "         const double *tab = sTab + ir * TABW;\n";
   const int NA = p.max_stack + 2;
   for (int r = 0; r < R; r++) {
      s << "         double lnscale" << sfx(r) << " = 0;\n         (void)lnscale" << sfx(r) << ";\n";
      for (int i = 0; i < NA; i++) s << "         double A" << i << sfx(r) << "[N];\n";
   }
   JitRegs regs(NA);
   auto name = [&](const JitArr &a, int r) { return a.name() + sfx(r); };
   int ich = 0;
   const char *LOOP = "_Pragma(\"unroll\") for (int j = 0; j < N; j++) ";
   auto mul_popped = [&](JitRegs::Step, const JitArr &out, const JitArr &in) {
      for (int r = 0; r < R; r++) s << "         " << LOOP << name(out, r) << "[j] = " << name(in, r) << "[j] * " << name(out, r) << "[j];\n";
   };
   for (const Op &o : p.ops) {
      if (o.code == OP_INIT_ONES || o.code == OP_INIT_TIP || o.code == OP_SET_TIP || o.code == OP_SET_TIP2) regs.start_partial();
      const bool mm = o.code == OP_MATMUL || o.code == OP_MATMUL_POP;
      const JitArr curin = regs.cur, out = mm ? regs.alloc() : JitArr();
      for (int r = 0; r < R; r++) {
         const std::string x = sfx(r), C = name(curin, r);
         switch (o.code) {
         case OP_INIT_ONES: s << "         " << LOOP << C << "[j] = 1.0;\n"; break;
         case OP_INIT_TIP: s << "         " << LOOP << C << "[j] = (a.cleandata && j == ci" << o.a << x << ") ? 1.0 : 0.0;\n"; break;
         case OP_SET_TIP: s << "         jvf_row_set<N>(" << C << ", tab + ot" << o.a << x << ");\n"; break;
         case OP_MUL_TIP: s << "         jvf_row_mul<N>(" << C << ", tab + ot" << o.a << x << ");\n"; break;
         case OP_SET_TIP2:
            if (pl.cherry) s << "         jvf_row_set<N>(" << C << ", tab + oc" << ich << x << ");\n";
            else
               s << "         { const double *r1 = tab + ot" << o.a << x << ", *r2 = tab + ot" << o.b << x << "; " << LOOP << C << "[j] = r1[j] * r2[j]; }\n";
            break;
         case OP_MUL_TIP2:
            s << "         { const double *r1 = tab + ot" << o.a << x << ", *r2 = tab + ot" << o.b << x << "; " << LOOP << C << "[j] = (" << C << "[j] * r1[j]) * r2[j]; }\n";
            break;
         case OP_MATMUL:
         case OP_MATMUL_POP:
            s << "         jv_matvec<N>(Pint + " << (long)o.a * N * N << ", " << C << ", " << name(out, r) << ");\n";
            break;
         case OP_SCALE: s << "         lnscale" << x << " += jv_scale<N>(" << C << ");\n"; break;
         case OP_ROOT:
            // fx_r treesub.c:7728-7749 / lfun 7780-7798, then this class's term of lfundG's mixture (7632-7652)
            s << "         { double f = 0;\n            " << LOOP << "f = fma(pi[j], " << C << "[j], f);\n"
              << "            if (a.mode == PAML_AMD_MODE_LFUN) { if (f <= 0) f = 1e-80; v" << x << " = log(f) + lnscale" << x << "; if (a.want_fhk && valid" << x
              << ") a.fhK[(cls0 + ir) * a.n_patt + h" << x << "] = wt" << x << " > 0 ? v" << x << " : 0.0; }\n"
              << "            else {\n"
              << "               if (f <= 0) f = 1e-300;\n"
              << "               if (a.n_scale) { if (valid" << x << ") a.fhK[(cls0 + ir) * a.n_patt + h" << x << "] = wt" << x << " > 0 ? log(f) + lnscale" << x << " : 0.0; }\n"
              << "               else {\n";
            if (CW > 1) s << "                  sF[ir * 256 + tid] = f;\n";
            else s << "                  fh" << x << " += fK[ir] * f;\n";
            s << "                  if (a.want_fhk && valid" << x << ") a.fhK[(cls0 + ir) * a.n_patt + h" << x << "] = wt" << x << " > 0 ? f : 0.0; }\n"
              << "            } }\n";
            break;
         default: break;
         }
      }
      switch (o.code) {
      case OP_SET_TIP2: if (pl.cherry) ich++; break;
      case OP_PUSH: regs.push(o.b, mul_popped); break;
      case OP_MATMUL: case OP_MATMUL_POP:
         regs.release(curin);
         regs.finish_product(out, mm_pop_slot(o), mm_push_slot(o), mul_popped);
         break;
      case OP_ROOT: regs.end_partial(); break;
      default: break;
      }
   }
   s << "      }\n";      // classes
   if (CW > 1) s << "      __syncthreads();\n";
   for (int r = 0; r < R; r++) {
      const std::string x = sfx(r);
      s << "      if (a.mode != PAML_AMD_MODE_LFUN" << (CW > 1 ? " && cw == 0" : "") << ") {\n"
           "         if (a.n_scale) {      /* log-sum-exp around the first maximum (treesub.c:7640-7649) */\n"
           "            const double *fk = a.fhK + cls0 * a.n_patt + hc" << x << ";\n"
           "            int it = 0;\n"
           "            for (int ir = 1; ir < K; ir++) if (fk[(long)ir * a.n_patt] > fk[(long)it * a.n_patt]) it = ir;\n"
           "            const double t = fk[(long)it * a.n_patt];\n"
           "            double fh = 0;\n"
           "            for (int ir = 0; ir < K; ir++) fh += fK[ir] * exp(fk[(long)ir * a.n_patt] - t);\n"
           "            v" << x << " = t + log(fh);\n"
           "         }\n"
           "         else {\n";
      if (CW > 1) s << "            for (int ir = 0; ir < K; ir++) fh" << x << " += fK[ir] * sF[ir * 256 + tid];\n";
      s << "            if (fh" << x << " <= 0) fh" << x << " = 1e-300;\n            v" << x << " = log(fh" << x << ");\n         }\n      }\n";
      s << "      if (!(valid" << x << " && wt" << x << " > 0)) v" << x << " = 0;\n";
      s << "      if (valid" << x << (CW > 1 ? " && cw == 0" : "") << ") { acc += v" << x << " * wt" << x << "; if (a.lnf) a.lnf[(long)bat * a.n_patt + h" << x << "] = v" << x << "; }\n";
   }
   if (CW > 1) s << "      __syncthreads();\n";      // sF is reused by the next sub-tile
   s << "   }\n";      // sub-tiles
   if (MG) {      // on to the chunk's next gene segment
      s << "   }\n   if (g_hi >= c_hi || gene + 1 >= " << G << ") break;\n   gene++; g_lo = g_hi;\n   g_hi = ";
      for (int g = 1; g < G - 1; g++) s << "gene == " << g << " ? go" << g + 1 << " : ";
      s << "go" << G << ";\n   }\n";
   }
   if (CW > 1) s << "   if (cw > 0) acc = 0;\n";
   s << "   red_block_finish<" << CW << ">(acc, a.red_partial + (long)bat * a.nb_stride, a.first_chunk + cb, a.nb_stride, a.red_out + bat, a.red_counter ? a.red_counter + bat * RED_TICKET_WORDS : nullptr);\n";
   s << "   }\n}\n";
   return regs.exhausted ? jit_exhausted_source() : s.str();
}

// ---- 20 states on v_mfma_f64_4x4x4 (m20_* in device_common.h) -----------------------------------------------------------------
// One class per workgroup (grid = a multiple of the class count, persistent over the 256-pattern tiles of its class): the
// row-major P(t) of every internal branch of that class sits in LDS (3 200 bytes each) for the whole launch; 8 waves x 2 groups
// of 16 patterns; tip rows are gathered from pmat's tables (L1 / L2 resident); fx_r's value per class goes to fhK and the usual
// reduction kernel does the mixture.  One gene; trees whose internal branches fit in LDS (<= 46).
inline bool jit_m20_supported(const Program &p, int n_tips, int n_genes, int *n_slots = nullptr)
{
   (void)n_genes;      // (several genes, round 6: a workgroup serves one (gene, class) — jit_generate_m20)
   if (!jit_valu_supported(p, 64) || n_tips > 64) return false;      // (tip codes: one 16-byte word per lane, 4 lanes per pattern)
   int nmm = 0;
   for (const Op &o : p.ops) {
      if (o.code == OP_MATMUL || o.code == OP_MATMUL_POP) nmm++;
      if (o.code == OP_INIT_TIP) return false;
   }
   if (n_slots) *n_slots = nmm;
   // (trees with more internal branches than LDS holds P(t) blocks for — M20_LDS_NODES — read the others' operands from global memory)
   return nmm >= 1 && nmm <= 200 && p.max_stack + 2 <= 9;
}
constexpr int M20_LDS_NODES = 46;      // P(t) blocks (3 200 bytes each) kept in LDS for the whole launch

// Several genes (G > 1): a gene has its own P(t), so a persistent workgroup serves one (gene, class): the workgroups of a class are dealt
// to the genes in proportion to their 32-pattern units (at least one each), and a gene's workgroups cut ITS units into contiguous ranges.
inline std::string jit_generate_m20(const Program &p, int n_tips, int n_codes, int G = 1, const JitProf &prof = JitProf())
{
   std::ostringstream s;
   const bool MG = G > 1;
   int nmm = 0;
   std::vector<int> mm_nodes;
   for (const Op &o : p.ops)
      if (o.code == OP_MATMUL || o.code == OP_MATMUL_POP) { mm_nodes.push_back(o.a); nmm++; }
   s << "#include \"device_common.h\"\nusing namespace paml_amd;\n";
   const int NTH = 512;
   s << "extern \"C\" __global__ __launch_bounds__(" << NTH << ") void prune_jit(PruneArgs a)\n{\n";
   // tip tables: as many as fit beside the P(t) blocks go to LDS (in order of use), the others are gathered from L1 / L2
   const int tip_bytes = n_codes * 168;      // rows padded to 21 doubles in LDS: with 20, codes c and c + 8 share all their banks
   // 16x16x4 + 4x4x4 (m20h_matvec2)
   const int NL = std::min(nmm, M20_LDS_NODES);      // products 0 .. NL - 1: operands in LDS; the others: in global memory, operand order
   const int room = 158 * 1024 - NL * 3200;
   const int n_lds_max = std::max(0, room / tip_bytes);
   std::vector<int> lds_slot(n_tips, -1);
   int n_lds = 0;
   for (const Op &o : p.ops) {
      auto take = [&](int t) { if (t >= 0 && t < n_tips && lds_slot[t] < 0 && n_lds < n_lds_max) lds_slot[t] = n_lds++; };
      if (o.code == OP_SET_TIP || o.code == OP_MUL_TIP) take(o.a);
      if (o.code == OP_SET_TIP2 || o.code == OP_MUL_TIP2) { take(o.a); take(o.b); }
   }
   s << "   constexpr int NMM = " << std::max(1, NL) << ", NC = " << n_codes << ", NLT = " << std::max(1, n_lds) << ";\n";
   s << "   __shared__ __attribute__((aligned(16))) double sP[NMM * 400];\n";
   s << "   __shared__ __attribute__((aligned(16))) double sT[NLT * NC * 21];\n";
   s << "   __shared__ int sTicket;\n";
   s << "   const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, st = lane >> 4, col = lane & 15;\n";
   if (prof.tiles) s << "   if (a.prof && tid == 0) a.prof[(long)blockIdx.x * a.prof_stride + a.prof_stride - 3] = __builtin_amdgcn_s_memrealtime();      /* kernel entry, before the LDS fill */\n";
   if (!MG) s << "   const int iclass = blockIdx.x % a.K, first = blockIdx.x / a.K, stride = gridDim.x / a.K;\n   constexpr int gene = 0, tile0 = 0;\n   const int hbeg = 0;\n   (void)hbeg;\n";
   else {
      // gene g's workgroups (of this class): [g + rest * cum(g) / tot, g + 1 + rest * cum(g + 1) / tot), cum = units of the genes before,
      // rest = workgroups per class beyond one per gene (the host launches at least G per class)
      s << "   const int iclass = blockIdx.x % a.K, wgc = blockIdx.x / a.K, W = gridDim.x / a.K;\n";
      s << "   int gene = 0, first = 0, stride = 1, tile0 = 0;\n";
      s << "   { const CONST_AS int *go = as_const(a.gene_off);\n";
      s << "     long tot = 0; for (int g = 0; g < a.n_genes; g++) tot += (go[g + 1] - go[g] + 31) / 32;\n";
      s << "     if (tot < 1) tot = 1;\n";
      s << "     const long rest = W - a.n_genes; long cu = 0; int t0 = 0;\n";
      s << "     for (int g = 0; g < a.n_genes; g++) {\n";
      s << "        const long ug = (go[g + 1] - go[g] + 31) / 32;\n";
      s << "        const int lo = g + (int)(rest * cu / tot), hi = g + 1 + (int)(rest * (cu + ug) / tot);\n";
      s << "        if (wgc >= lo && wgc < hi) { gene = g; first = wgc - lo; stride = hi - lo; tile0 = t0; }\n";
      s << "        cu += ug; t0 += (go[g + 1] - go[g] + 255) / 256;\n";
      s << "     } }\n";
      s << "   const int hbeg = as_const(a.gene_off)[gene];\n";
      s << "   if (as_const(a.gene_off)[gene + 1] <= hbeg) return;      /* (a shard that holds nothing of this gene) */\n";
   }
   // (a.pint: the branches' P(t) in operand order — [kb][lane] <- P[lane & 15][4 kb + (lane >> 4)], then [kb][k][i] <- P[16 + i][4 kb + k],
   //  written so by pmat_kernel_t<32> in layout 2)
   s << "   const double *Pall = " << "a.pint" << " + ((long)gene * a.K + iclass) * a.n_nodes * 400;\n";
   s << "   const double *Ptip = a.ptip + ((long)gene * a.K + iclass) * a.n_nodes * a.tip_words;\n";
   for (int k = 0; k < NL; k++)
      s << "   for (int i = tid; i < 400; i += " << NTH << ") sP[" << k * 400 << " + i] = Pall[" << (long)mm_nodes[k] * 400 << " + i];\n";
   for (int t = 0; t < n_tips; t++)
      if (lds_slot[t] >= 0)
         s << "   for (int i = tid; i < NC * 20; i += " << NTH << ") sT[" << lds_slot[t] << " * NC * 21 + (i / 20) * 21 + i % 20] = Ptip[(long)" << t << " * a.tip_words + i];\n";
   s << "   __syncthreads();\n";
   s << "   const int aoff = (lane & 3) * 20 + (lane >> 4);      /* A operand: lane 16 k + 4 b + i <- P[4I + i][4K + k] */\n";
   s << "   double pis[5];\n   _Pragma(\"unroll\") for (int m = 0; m < 5; m++) pis[m] = a.pi[(a.n_pi > 1 ? gene : 0) * 20 + 4 * m + st];\n";
   // tip codes: pattern-major, four per dword (PruneArgs::zpm); the NEXT tile's are fetched while this tile is walked, so that no
   // tip row's address waits on a global load
   // (round 6: the four state-quarter lanes of a pattern used to hold the same ZW dwords each — 64 VGPRs for the two groups of a unit and
   //  the next unit's at 60 taxa, and the walk spilled; now lane (st, col) holds the pattern's 16-byte word number st, the codes of tips
   //  16 st .. 16 st + 15, and a tip step fetches its dword from the owner lane with one ds_bpermute_b32: 16 VGPRs whatever the tree)
   const int ZW = ((n_tips + 3) / 4 + 3) / 4 * 4;
   s << "   constexpr int ZW = " << ZW << ";\n";
   s << "   const int hend = as_const(a.gene_off)[gene + 1];\n";
   s << "   const int zq = st < ZW / 4 ? st : ZW / 4 - 1, bp0 = col * 4;\n";
   s << "   unsigned int zn_0[4], zn_1[4];\n";
   // Work inside a workgroup is handed out per wave by an LDS ticket, in units of 32 patterns (two 16-pattern groups share every
   // operand fetch): the two waves of a SIMD do not advance at the same pace (the older wave wins the MFMA arbitration, 7 units
   // against 5-6), and with fixed slots the kernel ended 20 % after its fastest waves had finished.  The LAST units of a
   // workgroup's range are handed out as half units — one 16-pattern group, a second copy of the walk without the other group's
   // instructions: when the tickets run out a wave is at most half a unit from its end instead of a whole one
   // (profiles/r03_20state.txt: the tail was 6 % of the span).  Ticket t < nfull: the full unit ubase + t; else the half
   // (t - nfull) & 1 of unit ubase + nfull + (t - nfull) / 2.  A wave's first ticket is its own number; the next one is drawn a
   // unit ahead, so that its tip codes arrive while the current unit is walked.
   const int SPLIT = 8;
   s << "#define M20_UNIT_OF(T) ((T) < nfull ? ubase + (T) : ubase + nfull + (((T) - nfull) >> 1))\n";
   s << "#define M20_HALF_OF(T) ((T) < nfull ? -1 : (((T) - nfull) & 1))\n";
   s << "#define M20_FETCH_CODES(T) { int tn_ = (T) < nt ? (T) : nt - 1; tn_ = tn_ < 0 ? 0 : tn_; const int un_ = M20_UNIT_OF(tn_), hf_ = M20_HALF_OF(tn_); \\\n"
        "      const int h0n = as_const(a.tiles)[tile0 + (un_ >> 3)].y + (un_ & 7) * 32 + (hf_ > 0 ? 16 : 0); \\\n"
        "      long hn = h0n + col; if (hn >= hend) hn = hend - 1; const uint4 *zp = (const uint4 *)(a.zpm + hn * ZW); \\\n"
        "      { const uint4 t = zp[zq]; zn_0[0] = t.x; zn_0[1] = t.y; zn_0[2] = t.z; zn_0[3] = t.w; } \\\n"
        "      hn = h0n + 16 + col; if (hn >= hend) hn = hend - 1; zp = (const uint4 *)(a.zpm + hn * ZW); \\\n"
        "      { const uint4 t = zp[zq]; zn_1[0] = t.x; zn_1[1] = t.y; zn_1[2] = t.z; zn_1[3] = t.w; } }\n";
   s << "#define M20_TICKET() __builtin_amdgcn_readfirstlane(lane == 0 ? __hip_atomic_fetch_add(&sTicket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) : 0)\n";
   if (NL > 0) s << "   double Acol[5], AsN[5] = {0, 0, 0, 0, 0};\n   (void)AsN;\n   m20h_read_big(m20_lds_addr(sP), lane, Acol);      /* the first product's big operands (a unit's last product fetches them for the next unit) */\n   (void)aoff;\n";
   else      // (no P(t) block in LDS: the first product's operands come from global memory like every other's)
      s << "   double Acol[5], AsN[5];\n   { const double *Pn_ = Pall + " << (long)mm_nodes[0] * 400 << "; _Pragma(\"unroll\") for (int i = 0; i < 5; i++) { Acol[i] = Pn_[i * 64 + lane]; AsN[i] = Pn_[320 + i * 16 + ((lane >> 4) << 2) + (lane & 3)]; } }\n   (void)aoff; (void)sP;\n";
   const std::string &pt = prof.tid;
   if (prof.tiles) s << "   int ptc = 0; if (a.prof && tid == " << pt << ") { a.prof[(long)blockIdx.x * a.prof_stride] = __builtin_amdgcn_s_memrealtime(); a.prof[(long)blockIdx.x * a.prof_stride + a.prof_stride - 2] = __builtin_amdgcn_s_memtime(); }\n";
   // the class's units (32 patterns each, numbered through its 256-pattern tiles) are cut into one contiguous range per workgroup:
   // 10^5 patterns over 64 workgroups are 48 or 49 units each, where whole tiles were 48 or 56
   s << "   const int total_units = " << (MG ? "(hend - hbeg + 31) / 32" : "min(a.n_tiles * 8, (hend + 31) / 32)") << ";\n";
   s << "   const int ubase = (int)((long)first * total_units / stride), uend = (int)((long)(first + 1) * total_units / stride);\n";
   s << "   const int nfull = max(0, (uend - ubase) - " << SPLIT << "), nt = nfull + 2 * ((uend - ubase) - nfull);\n";
   s << "   if (threadIdx.x == 0) sTicket = " << NTH / 64 << ";      /* the first tickets are the waves' own */\n   __syncthreads();\n";
   s << "   int u = wv, unext = M20_TICKET();\n";
   s << "   M20_FETCH_CODES(u)\n";
   s << "   while (u < nt) {\n";
   s << "      const int unit = M20_UNIT_OF(u), half = M20_HALF_OF(u);\n";
   s << "      const int h0 = as_const(a.tiles)[tile0 + (unit >> 3)].y + (unit & 7) * 32 + (half > 0 ? 16 : 0);\n";
   s << "      unsigned int zw_0[4], zw_1[4];\n";
   s << "      _Pragma(\"unroll\") for (int i = 0; i < 4; i++) { zw_0[i] = zn_0[i]; zw_1[i] = zn_1[i]; }\n";
   s << "      M20_FETCH_CODES(unext)\n";
   s << "      const int unext2 = M20_TICKET();\n";
   bool exhausted = false;
   auto emit_body = [&](const int G) {      // the walk over one unit: G = 2 pattern groups, or (half units) group 0 alone
   for (int g = 0; g < G; g++) {
      s << "      const long h_" << g << " = h0 + " << 16 * g << " + col;\n      const bool valid_" << g << " = h_" << g << " < hend;\n";
      s << "      double lnscale_" << g << " = 0;\n      (void)lnscale_" << g << ";\n";
   }
   const int NA = p.max_stack + 2;
   for (int g = 0; g < G; g++)
      for (int i = 0; i < NA; i++) s << "      double A" << i << "_" << g << "[5];\n";
   JitRegs regs(NA);
   auto name = [&](const JitArr &a, int g) { return a.name() + "_" + std::to_string(g); };
   const char *LOOP = "_Pragma(\"unroll\") for (int m = 0; m < 5; m++) ";
   auto mul_popped = [&](JitRegs::Step, const JitArr &out, const JitArr &in) {
      for (int g = 0; g < G; g++) s << "      " << LOOP << name(out, g) << "[m] = " << name(in, g) << "[m] * " << name(out, g) << "[m];\n";
   };
   // Tip rows are gathered from global memory: the loads of the tip steps that follow a matrix product are issued BEFORE that
   // product (its 50 MFMAs cover their latency) and nothing else is allowed to move across a step (sched_barrier): left to
   // itself the compiler hoists every tip load of the tile to the top and spills.
   const size_t nops = p.ops.size();
   auto is_tip = [&](const Op &o) { return o.code == OP_SET_TIP || o.code == OP_MUL_TIP || o.code == OP_SET_TIP2 || o.code == OP_MUL_TIP2; };
   auto is_mm = [&](const Op &o) { return o.code == OP_MATMUL || o.code == OP_MATMUL_POP; };
   std::vector<char> loaded(nops, 0);
   auto tip_src = [&](int t) {
      return lds_slot[t] >= 0 ? "sT + " + std::to_string(lds_slot[t]) + " * NC * 21, 21" : "Ptip + (long)" + std::to_string(t) + " * a.tip_words, 20";
   };
   auto emit_loads = [&](size_t i) {      // the rows of tip step i -> T<i>a_<g>, T<i>b_<g>
      const Op &o = p.ops[i];
      const bool two = o.code == OP_SET_TIP2 || o.code == OP_MUL_TIP2;
      for (int g = 0; g < G; g++) {
         auto codeof = [&](int t) {
            return "(int)(((unsigned)__builtin_amdgcn_ds_bpermute(bp0 + " + std::to_string((t >> 4) * 64) + ", (int)zw_" + std::to_string(g) + "[" + std::to_string((t >> 2) & 3) + "]) >> " +
                   std::to_string((t & 3) * 8) + ") & 0xffu)";
         };
         s << "      double T" << i << "a_" << g << "[5]; m20_tip(" << tip_src(o.a) << ", " << codeof(o.a) << ", st, T" << i << "a_" << g << ");\n";
         if (two) s << "      double T" << i << "b_" << g << "[5]; m20_tip(" << tip_src(o.b) << ", " << codeof(o.b) << ", st, T" << i << "b_" << g << ");\n";
      }
      loaded[i] = 1;
   };
   // loads run TWO products ahead of their use
   std::vector<size_t> mm_at;
   for (size_t i = 0; i < nops; i++)
      if (is_mm(p.ops[i])) mm_at.push_back(i);
   // ... rows gathered from L1 / L2 run TWO products ahead of their use, rows in LDS one (their latency is a fraction of a
   // product, and every step in flight holds 20 - 40 registers)
   auto all_lds = [&](const Op &o) {
      const bool two = o.code == OP_SET_TIP2 || o.code == OP_MUL_TIP2;
      return lds_slot[o.a] >= 0 && (!two || lds_slot[o.b] >= 0);
   };
   auto emit_loads_after = [&](int k, int which) {      // the tip steps between product k and product k + 1 (k = -1: in front of the first); which: 1 = LDS rows, 2 = the others, 3 = all
      const size_t lo = k < 0 ? 0 : (k < (int)mm_at.size() ? mm_at[k] + 1 : nops), hi = k + 1 < (int)mm_at.size() ? mm_at[k + 1] : nops;
      for (size_t j = lo; j < hi; j++)
         if (is_tip(p.ops[j]) && !loaded[j] && (which & (all_lds(p.ops[j]) ? 1 : 2))) emit_loads(j);
   };
   emit_loads_after(-1, 3);
   emit_loads_after(0, 2);
   int imm = 0;
   for (size_t iop = 0; iop < nops; iop++) {
      const Op &o = p.ops[iop];
      if (o.code == OP_INIT_ONES || o.code == OP_SET_TIP || o.code == OP_SET_TIP2) regs.start_partial();
      const JitArr curin = regs.cur, out = is_mm(o) ? regs.alloc() : JitArr();
      switch (o.code) {
      case OP_INIT_ONES:
         for (int g = 0; g < G; g++) s << "      " << LOOP << name(curin, g) << "[m] = 1.0;\n";
         break;
      case OP_SET_TIP:
         for (int g = 0; g < G; g++) s << "      " << LOOP << name(curin, g) << "[m] = T" << iop << "a_" << g << "[m];\n";
         break;
      case OP_MUL_TIP:
         for (int g = 0; g < G; g++) s << "      " << LOOP << name(curin, g) << "[m] *= T" << iop << "a_" << g << "[m];\n";
         break;
      case OP_SET_TIP2:
         for (int g = 0; g < G; g++) s << "      " << LOOP << name(curin, g) << "[m] = T" << iop << "a_" << g << "[m] * T" << iop << "b_" << g << "[m];\n";
         break;
      case OP_MUL_TIP2:
         for (int g = 0; g < G; g++)
            s << "      " << LOOP << name(curin, g) << "[m] = (" << name(curin, g) << "[m] * T" << iop << "a_" << g << "[m]) * T" << iop << "b_" << g << "[m];\n";
         break;
      case OP_PUSH: regs.push(o.b, mul_popped); break;
      case OP_MATMUL: case OP_MATMUL_POP:
         emit_loads_after(imm, 1);
         emit_loads_after(imm + 1, 2);
         s << "      __builtin_amdgcn_sched_barrier(0);\n";
         {
            const int nxt = (imm + 1) % nmm;
            auto opnd = [&](int k) { return k < NL ? "sP + " + std::to_string(k * 400) : "Pall + " + std::to_string((long)mm_nodes[k] * 400); };
            const std::string tpl = std::string("<") + (imm >= NL ? "true" : "false") + ", " + (nxt >= NL ? "true" : "false") + ">";
            if (G == 2)
               s << "      m20h_matvec2x" << tpl << "(" << opnd(imm) << ", " << opnd(nxt) << ", lane, Acol, AsN, " << name(curin, 0) << ", " << name(out, 0) << ", "
                 << name(curin, 1) << ", " << name(out, 1) << ");\n";
            else
               s << "      m20h_matvec1x" << tpl << "(" << opnd(imm) << ", " << opnd(nxt) << ", lane, Acol, AsN, " << name(curin, 0) << ", " << name(out, 0) << ");\n";
         }
         s << "      __builtin_amdgcn_sched_barrier(0);\n";
         imm++;
         regs.release(curin);
         regs.finish_product(out, mm_pop_slot(o), mm_push_slot(o), mul_popped);
         break;
      case OP_SCALE:
         for (int g = 0; g < G; g++)
            s << "      { const double fac = m20_scale(" << name(curin, g) << "); lnscale_" << g << " += fac;\n"
              << "        if (a.keep && st == 0 && valid_" << g << ") a.scalef[((long)iclass * a.n_scale + " << o.b << ") * a.n_patt + h_" << g << "] = fac; }\n";
         break;
      case OP_ROOT:
         for (int g = 0; g < G; g++)
            s << "      m20_root(a, " << name(curin, g) << ", pis, lnscale_" << g << ", iclass, h_" << g << ", st == 0 && valid_" << g << ");\n";
         regs.end_partial();
         break;
      default: break;
      }
   }
   exhausted = exhausted || regs.exhausted;
   };      // emit_body
   s << "      if (half < 0) {\n";
   emit_body(2);
   s << "      } else {\n";
   emit_body(1);
   s << "      }\n";
   if (prof.tiles) s << "      if (a.prof && tid == " << pt << " && ptc < a.prof_stride - 4) { a.prof[(long)blockIdx.x * a.prof_stride + 1 + ptc] = __builtin_amdgcn_s_memrealtime(); a.prof[(long)blockIdx.x * a.prof_stride + a.prof_stride - 1] = __builtin_amdgcn_s_memtime(); }\n      ptc++;\n";
   s << "      u = unext; unext = unext2;\n";
   s << "   }\n}\n";
   return exhausted ? jit_exhausted_source() : s.str();
}

// ---- small data sets: the cooperative kernel (prune_mfma64_coop) unrolled for one tree, reduction inside (device_common.h, COOPJ_*) ----
// Every operand of the walk is requested straight into registers as far ahead as `budget` VGPRs allow (a product's A operands 32,
// a tip's two row pieces 8): the generator walks the program once, keeping a list of the operands in order of use, and emits a
// request whenever the registers of the requests still open fit the budget — at the top of the kernel until it is full, then
// after every step that consumed one.
inline bool jit_coop_supported(const Program &p, int n_tips, int n_codes)
{
   if (p.ops.size() > 260 || n_tips > 96 || n_codes > 256) return false;
   for (const Op &o : p.ops)
      if (o.code == OP_STORE || o.code == OP_LOAD || o.code == OP_EXPORT) return false;
   return p.max_stack <= 12;
}

inline std::string jit_generate_coop(const Program &p, int n_tips, int n_states = 61, int budget = 380)
{
   std::ostringstream s;
   // k-blocks of four states that hold states of the model, in pairs (a 16-byte word of the operand order): the rest of the padded
   // 64 x 64 matrices is zeros and is neither fetched nor multiplied (20 states: 5 k-blocks instead of 16)
   const int KB = n_states <= 32 ? (n_states + 3) / 4 : 16, NP = (KB + 1) / 2, pcost = 4 * NP;
   s << "#define COOPJ_NP " << NP << "\n#define COOPJ_KB " << KB << "\n";
   s << "#include \"device_common.h\"\nusing namespace paml_amd;\n";
   s << "extern \"C\" __global__ __launch_bounds__(256) void prune_jit(PruneArgs a)\n{\n   COOPJ_PROLOGUE\n";
   s << "   const int cj_bat = iclass / a.Km, cj_nwg = a.n_tiles * 4 * a.Km;\n";
   s << "   if (!empty) {\n";
   // the operands in order of use
   struct Req { bool tip; int id; int cost; };      // id: tip number, or index of the product
   std::vector<Req> reqs;
   std::vector<int> req_of_op_a(p.ops.size(), -1), req_of_op_b(p.ops.size(), -1);
   int n_prod = 0;
   for (size_t i = 0; i < p.ops.size(); i++) {
      const Op &o = p.ops[i];
      switch (o.code) {
      case OP_MATMUL: case OP_MATMUL_POP: req_of_op_a[i] = (int)reqs.size(); reqs.push_back({false, n_prod++, pcost}); break;
      case OP_SET_TIP: case OP_MUL_TIP: req_of_op_a[i] = (int)reqs.size(); reqs.push_back({true, o.a, 8}); break;
      case OP_SET_TIP2: case OP_MUL_TIP2:
         req_of_op_a[i] = (int)reqs.size(); reqs.push_back({true, o.a, 8});
         req_of_op_b[i] = (int)reqs.size(); reqs.push_back({true, o.b, 8});
         break;
      default: break;
      }
   }
   // the character codes of this lane's pattern, every tip (one byte load each, all in flight together)
   std::vector<char> used(n_tips, 0);
   for (const Op &o : p.ops) {
      if (o.code == OP_SET_TIP || o.code == OP_MUL_TIP || o.code == OP_INIT_TIP) used[o.a] = 1;
      if (o.code == OP_SET_TIP2 || o.code == OP_MUL_TIP2) used[o.a] = used[o.b] = 1;
   }
   for (int t = 0; t < n_tips; t++)
      if (used[t]) s << "   const int c" << t << " = (int)a.z[(long)" << t << " * a.z_stride + hc];\n";
   // product k: node of its branch
   std::vector<int> prod_node;
   for (const Op &o : p.ops)
      if (o.code == OP_MATMUL || o.code == OP_MATMUL_POP) prod_node.push_back(o.a);
   size_t next_req = 0;
   int open_cost = 0;
   auto top_up = [&]() {
      bool any = false;
      while (next_req < reqs.size() && (open_cost + reqs[next_req].cost <= budget || open_cost == 0)) {
         const Req &r = reqs[next_req];
         if (r.tip) s << "   COOPJ_T(T" << next_req << ", " << r.id << ", c" << r.id << ")\n";
         else s << "   COOPJ_P(P" << r.id << ", " << prod_node[r.id] << ")\n";
         open_cost += r.cost;
         next_req++;
         any = true;
      }
      if (any) s << "   __builtin_amdgcn_sched_barrier(0);\n";
   };
   auto consumed = [&](int req) {
      // (requests are consumed in the order they were made)
      open_cost -= reqs[req].cost;
   };
   top_up();
   const int NA = p.max_stack + 2;
   for (int i = 0; i < NA; i++) s << "   double A" << i << "[4];\n";
   JitRegs regs(NA);
   const JitArr &cur = regs.cur;
   auto name = [](const JitArr &a) { return a.name(); };
   int xb = 0;
   const char *LOOP = "_Pragma(\"unroll\") for (int r = 0; r < 4; r++) ";
   auto mul_popped = [&](JitRegs::Step, const JitArr &out, const JitArr &in) { s << "   " << LOOP << name(out) << "[r] = " << name(in) << "[r] * " << name(out) << "[r];\n"; };
   for (size_t iop = 0; iop < p.ops.size(); iop++) {
      const Op &o = p.ops[iop];
      const int ra = req_of_op_a[iop], rb = req_of_op_b[iop];
      switch (o.code) {
      case OP_INIT_ONES:
         regs.start_partial();
         s << "   " << LOOP << name(cur) << "[r] = (4 * (4 * wave + r) + q < n) ? 1.0 : 0.0;\n";
         break;
      case OP_INIT_TIP:
         regs.start_partial();
         s << "   " << LOOP << name(cur) << "[r] = (a.cleandata && 4 * (4 * wave + r) + q == c" << o.a << ") ? 1.0 : 0.0;\n";
         break;
      case OP_SET_TIP:
         regs.start_partial();
         s << "   " << name(cur) << "[0] = T" << ra << "a.x; " << name(cur) << "[1] = T" << ra << "a.y; " << name(cur) << "[2] = T" << ra << "b.x; " << name(cur) << "[3] = T" << ra << "b.y;\n";
         consumed(ra);
         break;
      case OP_MUL_TIP:
         s << "   " << name(cur) << "[0] *= T" << ra << "a.x; " << name(cur) << "[1] *= T" << ra << "a.y; " << name(cur) << "[2] *= T" << ra << "b.x; " << name(cur) << "[3] *= T" << ra << "b.y;\n";
         consumed(ra);
         break;
      case OP_SET_TIP2:
         regs.start_partial();
         s << "   " << name(cur) << "[0] = T" << ra << "a.x * T" << rb << "a.x; " << name(cur) << "[1] = T" << ra << "a.y * T" << rb << "a.y; "
           << name(cur) << "[2] = T" << ra << "b.x * T" << rb << "b.x; " << name(cur) << "[3] = T" << ra << "b.y * T" << rb << "b.y;\n";
         consumed(ra); consumed(rb);
         break;
      case OP_MUL_TIP2:
         s << "   " << name(cur) << "[0] = (" << name(cur) << "[0] * T" << ra << "a.x) * T" << rb << "a.x; " << name(cur) << "[1] = (" << name(cur) << "[1] * T" << ra << "a.y) * T" << rb << "a.y; "
           << name(cur) << "[2] = (" << name(cur) << "[2] * T" << ra << "b.x) * T" << rb << "b.x; " << name(cur) << "[3] = (" << name(cur) << "[3] * T" << ra << "b.y) * T" << rb << "b.y;\n";
         consumed(ra); consumed(rb);
         break;
      case OP_PUSH: regs.push(o.b, mul_popped); break;
      case OP_MATMUL: case OP_MATMUL_POP: {
         const JitArr in = cur, out = regs.alloc();
         s << "   COOPJ_MATVEC(P" << reqs[ra].id << ", " << name(in) << ", " << name(out) << ", " << xb << ")\n";
         xb ^= 1;
         consumed(ra);
         regs.release(in);
         regs.finish_product(out, mm_pop_slot(o), mm_push_slot(o), mul_popped);
      } break;
      case OP_SCALE:
         s << "   COOPJ_SCALE(" << name(cur) << ")\n";
         break;
      case OP_ROOT:
         s << "   COOPJ_ROOT(" << name(cur) << ", " << xb << ")\n";
         xb ^= 1;
         regs.end_partial();
         break;
      default: break;
      }
      if (ra >= 0) top_up();
   }
   s << "   }\n   coopj_finish(a, cj_bat, (int)blockIdx.x - cj_bat * cj_nwg, cj_nwg);\n}\n";
   return regs.exhausted ? jit_exhausted_source() : s.str();
}

}  // namespace paml_amd

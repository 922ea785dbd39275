// branch_plan.h — host side of the branch-local evaluation (paml_amd_eval_branch, engine_branch.hip): which resident partials are still
// current, the orientation towards the branch, the tree seen from it, the program of its dirty subtrees.  No device call: every
// function is a pure function of its arguments, and paml_amd_debug_branch_plan (engine_jitdbg.hip) plays them without an engine.
//
// The message cache: what updateconP (treesub.c:7982) + com.oldconP (treespace.c:250) save the reference.  Every internal node v keeps
// one partial M[v]: the likelihood of everything on v's side of the edge (v, up[v]).  With all up[] pointing towards the branch being
// worked on, M[A] and M[B] are the two partials across it.  Moving to another branch re-orients only the nodes on the path between the
// two branches; a changed branch length invalidates only the partials that look across it.  Nothing else is recomputed.
#pragma once
#include "program.h"

namespace paml_amd {

// resident partials on both sides of every edge, re-used from call to call (eval_branch)
struct BranchCache {
   bool valid = false;
   int K = 0;
   std::vector<int> up;            // up[v]: the neighbour v's stored partial looks away from
   std::vector<char> ok;           // the stored partial of internal node v is current
   std::vector<double> br, gr;     // branch lengths (by lower node) and gene rates the partials were formed with
   // eigen-basis form (kernels_branch.h): the coefficients c_k of the branch `coef_node` are in d_bl_coef, formed from the current
   // partials of its two ends — further trial lengths on that branch need no matrix product
   bool coef_ok = false;
   int coef_node = -1;
   std::vector<char> frag_ok;      // per branch label: V / U^T diag(pi) in operand order and the tips' z rows are in d_bl_efrag / d_bl_ztab
};

// The tree as set, undirected.  (The order of nbr[v] fixes the order of the sons in the tree seen from a branch, so the order of the
// products and the bits.)
struct Adjacency {
   std::vector<int> father;
   std::vector<std::vector<int>> nbr;
};
inline Adjacency adjacency(const TreeDesc &T)
{
   Adjacency a{std::vector<int>(T.n_nodes, -1), std::vector<std::vector<int>>(T.n_nodes)};
   for (int i = 0; i < T.n_nodes; i++)
      for (int j = T.sons_ptr[i]; j < T.sons_ptr[i + 1]; j++) {
         a.father[T.sons[j]] = i;
         a.nbr[i].push_back(T.sons[j]);
         a.nbr[T.sons[j]].push_back(i);
      }
   return a;
}

// What one call works with: the two ends of the branch, the orientation towards it, what is still current, the tree seen from it.
struct BranchPlan {
   int A = -1, Bn = -1;               // the end that may be a tip is "b"
   bool b_tip = false, any_dirty = false;
   std::vector<int> up;
   std::vector<unsigned char> clean;  // internal node v: its stored partial is current and looks the way this call needs
   TreeDesc tr;                       // sons = neighbours other than up[]; the edge data of (v, up[v]) sits at index v
   std::vector<double> br_eff;
   std::vector<int> lab_eff;
};

// The two ends of node_b's branch (the contraction is symmetric for reversible models: pi_i P_ij = pi_j P_ji); false: both are tips
inline bool branch_ends(const TreeDesc &T, const Adjacency &adj, int node_b, BranchPlan &p)
{
   p.A = adj.father[node_b]; p.Bn = node_b;
   if (T.is_leaf(p.A)) std::swap(p.A, p.Bn);
   p.b_tip = T.is_leaf(p.Bn);
   return !T.is_leaf(p.A);
}

// Start over when the cache is invalid or was formed for another node count, K or gene rates; true: it was.
inline bool reset_if_stale(BranchCache &bc, int nn, int K, const std::vector<double> &gr)
{
   if (bc.valid && (int)bc.up.size() == nn && bc.K == K && bc.gr == gr) return false;
   bc.up.assign(nn, -2); bc.ok.assign(nn, 0); bc.br.assign(nn, -1.0); bc.gr = gr; bc.K = K;
   bc.valid = true;
   bc.coef_ok = false;
   bc.frag_ok.clear();
   return true;
}

// Branch lengths that changed since the partials were formed: taken into bc.br, and every stored partial dropped whose side of
// (v, up[v]) holds a changed edge with both ends inside.
inline void invalidate(BranchCache &bc, const TreeDesc &T, const Adjacency &adj, const double *branch)
{
   const int nn = T.n_nodes;
   std::vector<int> changed;
   for (int x = 0; x < nn; x++)
      if (x != T.root && branch[x] != bc.br[x]) { changed.push_back(x); bc.br[x] = branch[x]; }
   if (changed.empty()) return;
   std::vector<char> in(nn);
   std::vector<int> stack;
   for (int v = T.n_tips; v < nn; v++) {
      if (!bc.ok[v]) continue;
      std::fill(in.begin(), in.end(), 0);      // v's side of the edge (v, up[v])
      stack.assign(1, v);
      in[v] = 1;
      while (!stack.empty()) {
         const int u = stack.back();
         stack.pop_back();
         for (int w : adj.nbr[u])
            if (!in[w] && !(u == v && w == bc.up[v])) { in[w] = 1; stack.push_back(w); }
      }
      for (int x : changed)
         if (in[x] && in[adj.father[x]]) { bc.ok[v] = 0; break; }
   }
}

// Orientation towards the branch (p.A, p.Bn), and which stored partials serve it as they are
inline void orient(const BranchCache &bc, const TreeDesc &T, const Adjacency &adj, BranchPlan &p)
{
   const int nn = T.n_nodes;
   std::vector<int> queue;
   p.up.assign(nn, -1);
   p.up[p.A] = p.Bn; p.up[p.Bn] = p.A;
   queue.push_back(p.A); queue.push_back(p.Bn);
   for (size_t qi = 0; qi < queue.size(); qi++) {
      const int u = queue[qi];
      for (int w : adj.nbr[u])
         if (w != p.up[u] && p.up[w] < 0) { p.up[w] = u; queue.push_back(w); }
   }
   p.clean.assign(nn, 0);
   p.any_dirty = false;
   for (int v = T.n_tips; v < nn; v++) {
      p.clean[v] = bc.ok[v] && bc.up[v] == p.up[v];
      p.any_dirty = p.any_dirty || !p.clean[v];
   }
}

// The tree seen from the branch, rooted at A, with the lengths and labels re-indexed (an edge of the tree as set is named by its lower
// node).  The nodes SetNodeScale marked keep their scale slots.
inline void tree_seen_from(const TreeDesc &T, const Adjacency &adj, const double *branch, BranchPlan &p)
{
   const int nn = T.n_nodes;
   TreeDesc &tr = p.tr;
   tr = TreeDesc();
   tr.n_tips = T.n_tips; tr.n_nodes = nn; tr.root = p.A;
   tr.sons_ptr.assign(nn + 1, 0);
   p.br_eff.assign(nn, 0.0);
   p.lab_eff.assign(nn, 0);
   for (int v = 0; v < nn; v++) {
      for (int w : adj.nbr[v])
         if (w != p.up[v]) tr.sons.push_back(w);
      tr.sons_ptr[v + 1] = (int)tr.sons.size();
      if (v != p.A && v != p.Bn) { const int x = adj.father[v] == p.up[v] ? v : p.up[v]; p.br_eff[v] = branch[x]; p.lab_eff[v] = T.label[x]; }
   }
   tr.label = p.lab_eff;
   tr.scale_node.assign(nn, 0);
   tr.scale_slot.assign(nn, -1);
   if (T.n_scale > 0)
      for (int i = 0; i < nn; i++)
         if (T.scale_node[i] && !tr.is_leaf(i)) { tr.scale_node[i] = 1; tr.scale_slot[i] = T.scale_slot[i]; tr.n_scale = T.n_scale; }
}

// The dirty subtrees below `roots`, one program: build_program for each root without its OP_ROOT / OP_END, then OP_END and the prefetch
// links of the whole (every MATMUL names the next one).  An empty forest gives an empty program, or OP_END alone with `end_if_empty`.
inline Program forest_program(const TreeDesc &tr, const std::vector<int> &roots, const unsigned char *clean, bool end_if_empty)
{
   Program prog;
   TreeDesc t = tr;
   for (int rt : roots) {
      t.root = rt;
      const Program ps = build_program(t, true, clean);
      for (const Op &o : ps.ops)
         if (o.code != OP_ROOT && o.code != OP_END) prog.ops.push_back(o);
      prog.max_stack = std::max(prog.max_stack, ps.max_stack);
   }
   if (prog.ops.empty() && !end_if_empty) return prog;
   prog.ops.push_back({OP_END, 0, 0, -1});
   int next = -1;
   for (int i = (int)prog.ops.size() - 1; i >= 0; i--)
      if (prog.ops[i].code == OP_MATMUL || prog.ops[i].code == OP_MATMUL_POP) { prog.ops[i].c = next; next = prog.ops[i].a; }
   prog.first_matmul = next;
   return prog;
}

// The kernels that form the dirty partials are queued: every internal node's partial is current and looks along up[].  Returns how
// many were formed.
inline long commit(BranchCache &bc, const BranchPlan &p, int n_tips)
{
   for (int v = n_tips; v < (int)p.up.size(); v++) { bc.up[v] = p.up[v]; bc.ok[v] = 1; }
   return (long)std::count(p.clean.begin() + n_tips, p.clean.end(), 0);
}

}  // namespace paml_amd

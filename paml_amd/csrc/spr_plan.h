// spr_plan.h — the host side of paml_amd_spr_scores that needs no device: which moves are valid, the canonical list, and the lists of
// steps the kernels of kernels_spr.h walk per pruned s (the definition is at the top of that header).  Plain C++: engine_spr.hip and
// tools/spr_host_check.cpp both include it.
#pragma once
#include <algorithm>
#include <string>
#include <vector>

namespace paml_amd {

struct SprTreeView {
   int n_tips, n_nodes, root;
   const int *sons_ptr, *sons;      // CSR son lists
   int n_sons(int v) const { return sons_ptr[v + 1] - sons_ptr[v]; }
};

// a step: eight ints
//   [0] op          SPR_UP: L'_node of a path node;  SPR_OUT: A'_node of a node off the path;  SPR_TARGET: the score of target node
//   [1] node
//   [2] head kind   SPR_HEAD_ONES;  SPR_HEAD_PRESENT: A of [3] in the present tree (the root: pi);  SPR_HEAD_SCRATCH: A'_[3] of this prune
//   [3] head node
//   [4] first factor, [5] number of factors: the messages multiplied in, in son-list order of the tree without s and f
//   [6] SPR_OUT: 1 when the node is c (its branch is the merged one);  SPR_TARGET: 1 when L'_node is this prune's (a path node)
//   [7] SPR_TARGET: the move's row in the sorted list
// a factor: two ints, (kind, node): SPR_FAC_PRESENT: P_node L_node;  SPR_FAC_MERGED: P_c(t_c + t_f) L_c;  SPR_FAC_PATH: P_node L'_node
enum { SPR_UP = 0, SPR_OUT = 1, SPR_TARGET = 2 };
enum { SPR_HEAD_ONES = 0, SPR_HEAD_PRESENT = 1, SPR_HEAD_SCRATCH = 2 };
enum { SPR_FAC_PRESENT = 0, SPR_FAC_MERGED = 1, SPR_FAC_PATH = 2 };
#define SPR_STEP_INTS 8
#define SPR_PRUNE_INTS 4      // s, first step, number of steps, first row

struct SprPlan {
   std::vector<int> prunes, steps, factors;
   std::vector<int> order;      // [row of the sorted list] the move's place in the caller's list
   int max_rows = 0;            // the most targets one s has
   int n_prunes() const { return (int)prunes.size() / SPR_PRUNE_INTS; }
};

// father[] of every node; false when a son is out of range
inline bool spr_fathers(const SprTreeView &t, std::vector<int> &father)
{
   father.assign(t.n_nodes, -1);
   for (int v = 0; v < t.n_nodes; v++)
      for (int j = t.sons_ptr[v]; j < t.sons_ptr[v + 1]; j++) {
         if (t.sons[j] < 0 || t.sons[j] >= t.n_nodes) return false;
         father[t.sons[j]] = v;
      }
   return true;
}

// why s cannot be pruned; empty: it can
inline std::string spr_check_prune(const SprTreeView &t, const std::vector<int> &father, int s)
{
   if (s < 0 || s >= t.n_nodes) return "node " + std::to_string(s) + " is out of range";
   if (s == t.root || father[s] < 0) return "node " + std::to_string(s) + " is the root";
   const int f = father[s];
   if (f == t.root || father[f] < 0) return "the father of " + std::to_string(s) + " is the root";
   if (t.n_sons(f) != 2) return "the father of " + std::to_string(s) + " does not have exactly two sons";
   return "";
}

inline int spr_sibling(const SprTreeView &t, const std::vector<int> &father, int s)
{
   const int f = father[s], a = t.sons[t.sons_ptr[f]];
   return a == s ? t.sons[t.sons_ptr[f] + 1] : a;
}

// why (s, x) is not a move; empty: it is one
inline std::string spr_check_move(const SprTreeView &t, const std::vector<int> &father, int s, int x)
{
   std::string why = spr_check_prune(t, father, s);
   if (!why.empty()) return why;
   if (x < 0 || x >= t.n_nodes) return "node " + std::to_string(x) + " is out of range";
   if (x == t.root || father[x] < 0) return "node " + std::to_string(x) + " is the root";
   if (x == father[s]) return "node " + std::to_string(x) + " is the father of " + std::to_string(s);
   if (x == spr_sibling(t, father, s)) return "node " + std::to_string(x) + " is the sibling of " + std::to_string(s) + ": the same topology";
   for (int u = x; u >= 0; u = father[u])
      if (u == s) return "node " + std::to_string(x) + " lies in the subtree below " + std::to_string(s);
   return "";
}

// The canonical list: every valid (s, x) whose target branch lies within `radius` branches of the merged branch above c in the tree
// without s and f (radius <= 0: no limit), s in node order and x in node order within s.  Returns the length (moves null: that only),
// -1 when the arrays are not a tree or the list is longer than cap.
inline int spr_list(const SprTreeView &t, int radius, int *moves, int cap)
{
   std::vector<int> father;
   if (t.n_nodes < 1 || t.root < 0 || t.root >= t.n_nodes || !t.sons_ptr || !t.sons || !spr_fathers(t, father)) return -1;
   const int nn = t.n_nodes;
   int count = 0;
   std::vector<int> dist(nn), queue;
   std::vector<char> below(nn);
   for (int s = 0; s < nn; s++) {
      if (!spr_check_prune(t, father, s).empty()) continue;
      const int f = father[s], g = father[f], c = spr_sibling(t, father, s);
      std::fill(below.begin(), below.end(), 0);
      queue.assign(1, s);
      for (size_t qi = 0; qi < queue.size() && queue.size() <= (size_t)nn; qi++) {
         below[queue[qi]] = 1;
         for (int j = t.sons_ptr[queue[qi]]; j < t.sons_ptr[queue[qi] + 1]; j++) queue.push_back(t.sons[j]);
      }
      // the nodes' distances from the merged branch (its ends g and c: 0) in the tree without s and f
      std::fill(dist.begin(), dist.end(), nn + 1);
      dist[g] = dist[c] = 0;
      queue.assign({g, c});
      for (size_t qi = 0; qi < queue.size(); qi++) {
         const int u = queue[qi];
         auto reach = [&](int v) {
            if (v < 0 || v == f || below[v] || dist[v] <= dist[u] + 1) return;
            dist[v] = dist[u] + 1;
            queue.push_back(v);
         };
         reach(u == c ? g : father[u]);
         for (int j = t.sons_ptr[u]; j < t.sons_ptr[u + 1]; j++) reach(t.sons[j] == f ? c : t.sons[j]);
      }
      for (int x = 0; x < nn; x++) {
         if (x == t.root || father[x] < 0 || x == f || x == c || below[x]) continue;
         if (radius > 0 && std::min(dist[father[x]], dist[x]) + 1 > radius) continue;
         if (moves) {
            if (count >= cap) return -1;
            moves[2 * count] = s; moves[2 * count + 1] = x;
         }
         count++;
      }
   }
   return count;
}

// The steps of a list of valid moves: the moves sorted by s (the caller's order within one s), per s the products up the path, the
// outward chain over the nodes that lead to its targets, then the targets.  What is computed for one (s, x) does not depend on the
// other moves: a node's L' and A' are the same whichever targets ask for them.
inline void spr_plan(const SprTreeView &t, const std::vector<int> &father, int n_moves, const int *moves, SprPlan &plan)
{
   const int nn = t.n_nodes;
   plan = SprPlan();
   plan.order.resize(n_moves);
   for (int i = 0; i < n_moves; i++) plan.order[i] = i;
   std::stable_sort(plan.order.begin(), plan.order.end(), [&](int a, int b) { return moves[2 * a] < moves[2 * b]; });
   std::vector<int> pre, stack(1, t.root);      // pre-order of the present tree: also one of the tree without s and f
   while (!stack.empty()) {
      const int v = stack.back();
      stack.pop_back();
      pre.push_back(v);
      for (int j = t.sons_ptr[v + 1] - 1; j >= t.sons_ptr[v]; j--) stack.push_back(t.sons[j]);
   }
   std::vector<char> onpath(nn), need(nn);
   for (int r0 = 0; r0 < n_moves;) {
      const int s = moves[2 * plan.order[r0]];
      int r1 = r0;
      while (r1 < n_moves && moves[2 * plan.order[r1]] == s) r1++;
      const int f = father[s], g = father[f], c = spr_sibling(t, father, s);
      auto father2 = [&](int u) { return u == c ? g : father[u]; };
      // (head, factors) of node u of the tree without s and f: A' of its father and its siblings' messages
      auto around = [&](int u, int *head_kind, int *head_node, int *fac0, int *n_fac) {
         const int fu = father2(u);
         *head_kind = onpath[fu] ? SPR_HEAD_PRESENT : SPR_HEAD_SCRATCH;
         *head_node = fu;
         *fac0 = (int)plan.factors.size() / 2;
         for (int j = t.sons_ptr[fu]; j < t.sons_ptr[fu + 1]; j++) {
            const int v = t.sons[j] == f ? c : t.sons[j];
            if (v == u) continue;
            plan.factors.push_back(v == c ? SPR_FAC_MERGED : onpath[v] ? SPR_FAC_PATH : SPR_FAC_PRESENT);
            plan.factors.push_back(v);
         }
         *n_fac = (int)plan.factors.size() / 2 - *fac0;
      };
      std::fill(onpath.begin(), onpath.end(), 0);
      std::fill(need.begin(), need.end(), 0);
      const int step0 = (int)plan.steps.size() / SPR_STEP_INTS;
      for (int a = g; a != t.root; a = father[a]) onpath[a] = 1;
      for (int a = g; a != t.root; a = father[a]) {      // up the path (nobody reads L' of the root)
         const int fac0 = (int)plan.factors.size() / 2;
         for (int j = t.sons_ptr[a]; j < t.sons_ptr[a + 1]; j++) {
            const int v = t.sons[j] == f ? c : t.sons[j];
            plan.factors.push_back(v == c ? SPR_FAC_MERGED : onpath[v] ? SPR_FAC_PATH : SPR_FAC_PRESENT);
            plan.factors.push_back(v);
         }
         const int st[SPR_STEP_INTS] = {SPR_UP, a, SPR_HEAD_ONES, 0, fac0, (int)plan.factors.size() / 2 - fac0, 0, 0};
         plan.steps.insert(plan.steps.end(), st, st + SPR_STEP_INTS);
      }
      onpath[t.root] = 1;      // (the root's message is the present tree's too: pi)
      for (int r = r0; r < r1; r++)
         for (int u = father2(moves[2 * plan.order[r] + 1]); !onpath[u]; u = father2(u)) need[u] = 1;
      for (int u : pre)
         if (need[u]) {
            int st[SPR_STEP_INTS] = {SPR_OUT, u, 0, 0, 0, 0, u == c ? 1 : 0, 0};
            around(u, &st[2], &st[3], &st[4], &st[5]);
            plan.steps.insert(plan.steps.end(), st, st + SPR_STEP_INTS);
         }
      for (int r = r0; r < r1; r++) {
         const int x = moves[2 * plan.order[r] + 1];
         int st[SPR_STEP_INTS] = {SPR_TARGET, x, 0, 0, 0, 0, onpath[x] ? 1 : 0, r};
         around(x, &st[2], &st[3], &st[4], &st[5]);
         plan.steps.insert(plan.steps.end(), st, st + SPR_STEP_INTS);
      }
      const int pr[SPR_PRUNE_INTS] = {s, step0, (int)plan.steps.size() / SPR_STEP_INTS - step0, r0};
      plan.prunes.insert(plan.prunes.end(), pr, pr + SPR_PRUNE_INTS);
      plan.max_rows = std::max(plan.max_rows, r1 - r0);
      r0 = r1;
   }
}

}  // namespace paml_amd

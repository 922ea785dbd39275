// hessian_plan.h — the host side of paml_amd_hessian that needs no device: which node of a pair is its source, the check of the caller's
// list, and the lists of steps the kernels of kernels_hessian.h walk per source u (the definition is at the top of that header).  Plain
// C++: engine_hessian.hip and tools/hessian_host_check.cpp both include it.
#pragma once
#include <algorithm>
#include <string>
#include <vector>

namespace paml_amd {

struct HessTreeView {
   int n_tips, n_nodes, root;
   const int *sons_ptr, *sons;      // CSR son lists
};

// a step: eight ints
//   [0] op          HESS_UP: L'_node of a path node;  HESS_OUT: A'_node of a node off the path;  HESS_TARGET: m_{u,node}
//   [1] node
//   [2] head kind   HESS_HEAD_ONES;  HESS_HEAD_PRESENT: A of [3] in the present tree (the root: pi);  HESS_HEAD_SCRATCH: A'_[3] of this source
//   [3] head node
//   [4] first factor, [5] number of factors: the messages multiplied in, in son-list order
//   [6] HESS_TARGET: 1 when the node is a path node (dP_node meets L'_node of this source, not L_node)
//   [7] HESS_TARGET: the pair's row in the plan's list
// a factor: two ints, (kind, node): HESS_FAC_PRESENT: P_node L_node;  HESS_FAC_SOURCE: D_u = dP_node L_node (node = u);  HESS_FAC_PATH: P_node L'_node
enum { HESS_UP = 0, HESS_OUT = 1, HESS_TARGET = 2 };
enum { HESS_HEAD_ONES = 0, HESS_HEAD_PRESENT = 1, HESS_HEAD_SCRATCH = 2 };
enum { HESS_FAC_PRESENT = 0, HESS_FAC_SOURCE = 1, HESS_FAC_PATH = 2 };
#define HESS_STEP_INTS 8
#define HESS_SOURCE_INTS 4      // u, first step, number of steps, first row

struct HessPlan {
   std::vector<int> sources, steps, factors;
   std::vector<int> pairs;      // [row] (source, target)
   int max_rows = 0;            // the most targets one source has
   int n_sources() const { return (int)sources.size() / HESS_SOURCE_INTS; }
   int n_pairs() const { return (int)pairs.size() / 2; }
};

// father[] of every node and the pre-order of the tree; false when a son is out of range
inline bool hess_fathers(const HessTreeView &t, std::vector<int> &father, std::vector<int> &pre)
{
   father.assign(t.n_nodes, -1);
   for (int v = 0; v < t.n_nodes; v++)
      for (int j = t.sons_ptr[v]; j < t.sons_ptr[v + 1]; j++) {
         if (t.sons[j] < 0 || t.sons[j] >= t.n_nodes) return false;
         father[t.sons[j]] = v;
      }
   pre.clear();
   std::vector<int> stack(1, t.root);
   while (!stack.empty() && pre.size() <= (size_t)t.n_nodes) {
      const int v = stack.back();
      stack.pop_back();
      pre.push_back(v);
      for (int j = t.sons_ptr[v + 1] - 1; j >= t.sons_ptr[v]; j--) stack.push_back(t.sons[j]);
   }
   return pre.size() == (size_t)t.n_nodes;
}

// why the list cannot be served; empty: it can
inline std::string hess_check_nodes(const HessTreeView &t, const int *nodes, int n_list)
{
   std::vector<char> seen(t.n_nodes, 0);
   for (int i = 0; i < n_list; i++) {
      const int v = nodes[i];
      if (v < 0 || v >= t.n_nodes) return "nodes[" + std::to_string(i) + "] = " + std::to_string(v) + " is out of range";
      if (v == t.root) return "nodes[" + std::to_string(i) + "] = " + std::to_string(v) + " is the root";
      if (seen[v]) return "nodes[" + std::to_string(i) + "] = " + std::to_string(v) + " is repeated";
      seen[v] = 1;
   }
   return "";
}

inline bool hess_is_ancestor(const std::vector<int> &father, int a, int v)      // a lies on the way from v to the root (a != v)
{
   for (int x = father[v]; x >= 0; x = father[x])
      if (x == a) return true;
   return false;
}

// The source of the pair {u, v}, a rule of the pair and the tree alone: the lower node when one lies below the other (its path to the
// root passes the other), otherwise the node with the smaller number.
inline int hess_source_of(const std::vector<int> &father, int u, int v)
{
   if (hess_is_ancestor(father, u, v)) return v;
   if (hess_is_ancestor(father, v, u)) return u;
   return std::min(u, v);
}

// The steps of the listed nodes' pairs: the sources in node order, per source the products up the path as far as a target needs them,
// the outward chain over the nodes that lead to its targets (pre-order), then the targets in node order.  What is computed for one
// pair does not depend on the other pairs: a node's L' and A' are the same whichever targets ask for them.
inline void hess_plan(const HessTreeView &t, const std::vector<int> &father, const std::vector<int> &pre, int n_list, const int *nodes, HessPlan &plan)
{
   const int nn = t.n_nodes;
   plan = HessPlan();
   std::vector<char> listed(nn, 0), onpath(nn), need(nn);
   for (int i = 0; i < n_list; i++) listed[nodes[i]] = 1;
   std::vector<int> pathson(nn), depth(nn), targets;
   for (int u = 0; u < nn; u++) {
      if (!listed[u]) continue;
      targets.clear();
      for (int v = 0; v < nn; v++)
         if (v != u && listed[v] && hess_source_of(father, u, v) == u) targets.push_back(v);
      if (targets.empty()) continue;
      std::fill(onpath.begin(), onpath.end(), 0);
      std::fill(need.begin(), need.end(), 0);
      std::fill(pathson.begin(), pathson.end(), -1);
      std::vector<int> chain;      // father(u), ..., the root
      for (int c = u, a = father[u]; a >= 0; c = a, a = father[a]) {
         onpath[a] = 1;
         pathson[a] = c;
         depth[a] = (int)chain.size();
         chain.push_back(a);
      }
      int need_up = -1;      // L' is needed of chain[0 .. need_up]
      for (int v : targets) {
         if (onpath[v]) { need_up = std::max(need_up, depth[v]); continue; }
         int x = father[v];
         for (; !onpath[x]; x = father[x]) need[x] = 1;
         if (pathson[x] != u) need_up = std::max(need_up, depth[pathson[x]]);
      }
      auto factor = [&](int s) {
         plan.factors.push_back(s == u ? HESS_FAC_SOURCE : (onpath[s] ? HESS_FAC_PATH : HESS_FAC_PRESENT));
         plan.factors.push_back(s);
      };
      // (head, factors) of node x: A or A' of its father and its siblings' messages
      auto around = [&](int x, int *st) {
         const int fx = father[x];
         st[2] = onpath[fx] ? HESS_HEAD_PRESENT : HESS_HEAD_SCRATCH;
         st[3] = fx;
         st[4] = (int)plan.factors.size() / 2;
         for (int j = t.sons_ptr[fx]; j < t.sons_ptr[fx + 1]; j++)
            if (t.sons[j] != x) factor(t.sons[j]);
         st[5] = (int)plan.factors.size() / 2 - st[4];
      };
      const int step0 = (int)plan.steps.size() / HESS_STEP_INTS, row0 = plan.n_pairs();
      for (int i = 0; i <= need_up; i++) {
         const int a = chain[i], fac0 = (int)plan.factors.size() / 2;
         for (int j = t.sons_ptr[a]; j < t.sons_ptr[a + 1]; j++) factor(t.sons[j]);
         const int st[HESS_STEP_INTS] = {HESS_UP, a, HESS_HEAD_ONES, 0, fac0, (int)plan.factors.size() / 2 - fac0, 0, 0};
         plan.steps.insert(plan.steps.end(), st, st + HESS_STEP_INTS);
      }
      for (int x : pre)
         if (need[x]) {
            int st[HESS_STEP_INTS] = {HESS_OUT, x, 0, 0, 0, 0, 0, 0};
            around(x, st);
            plan.steps.insert(plan.steps.end(), st, st + HESS_STEP_INTS);
         }
      for (int v : targets) {
         int st[HESS_STEP_INTS] = {HESS_TARGET, v, 0, 0, 0, 0, onpath[v] ? 1 : 0, plan.n_pairs()};
         around(v, st);
         plan.steps.insert(plan.steps.end(), st, st + HESS_STEP_INTS);
         plan.pairs.push_back(u);
         plan.pairs.push_back(v);
      }
      const int sr[HESS_SOURCE_INTS] = {u, step0, (int)plan.steps.size() / HESS_STEP_INTS - step0, row0};
      plan.sources.insert(plan.sources.end(), sr, sr + HESS_SOURCE_INTS);
      plan.max_rows = std::max(plan.max_rows, (int)targets.size());
   }
}

}  // namespace paml_amd

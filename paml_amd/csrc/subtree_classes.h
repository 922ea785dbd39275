// subtree_classes.h — host side of the subtree tables (jit.h: OP_LOOKUP above the cherries; kernels_pmat.h: subtree_table_kernel): which
// patterns repeat below a node.  No device call and no engine: pure functions of their arguments (a tree as son lists, the tip codes),
// so that tools/subtree_classes_check.cpp runs them under the host sanitizers and paml_amd_debug_subtree_classes plays them for the tests.
//
// The partial of an internal node v for a pattern depends on the codes of the tips below v only, so it takes as many values over the
// alignment as there are distinct tuples of those codes: u_v.  The class of a pattern at v is the dense rank, in order of first
// occurrence, of the tuple of its sons' classes (a tip's class is its code) — except at a cherry, whose class is ca * n_codes + cb: the
// row number the cherry tables already use.  Both are injective in the tuple of tip codes below v, which is all the ranks above need.
// The alignment is fixed for a whole search and the tree between two paml_amd_set_tree calls: the engine computes this once per (tips,
// tree), never per evaluation.
#pragma once
#include <cstdint>
#include <utility>
#include <vector>

namespace paml_amd {

struct SubtreeClasses {
   // per node (tips and the root: empty / 0)
   std::vector<uint32_t> u;                           // number of classes; a cherry: distinct (ca, cb) pairs that occur (its class numbers are NOT dense)
   std::vector<std::vector<uint32_t>> cls;            // [n_patt]: the pattern's class
   std::vector<std::vector<uint32_t>> son_cls;        // [n_sons][u]: class c's index at every son, son-major (cherries: empty, the index says it)
   std::vector<char> cherry, done;                    // the node is a cherry; its classes were computed
};

namespace detail {
// (key -> dense rank) by open addressing: 10^6 patterns per node make std::unordered_map the whole cost
struct RankTable {
   std::vector<uint64_t> key;
   std::vector<uint32_t> val;
   uint64_t mask;
   uint32_t n = 0;
   explicit RankTable(size_t expect)
   {
      size_t cap = 16;
      while (cap < 2 * expect + 2) cap <<= 1;
      key.assign(cap, ~0ull);
      val.assign(cap, 0);
      mask = cap - 1;
   }
   uint32_t rank(uint64_t k)      // k != ~0
   {
      uint64_t h = k * 0x9E3779B97F4A7C15ull;
      h ^= h >> 29;
      for (uint64_t i = h & mask;; i = (i + 1) & mask) {
         if (key[i] == k) return val[i];
         if (key[i] == ~0ull) { key[i] = k; val[i] = n; return n++; }
      }
   }
};
}  // namespace detail

// z: [n_tips][z_stride] codes < n_codes.  Nodes whose class count exceeds `u_limit` are left undone together with everything above them
// (u_parent >= u_son: they cannot be tabulated either) — the engine passes frac x n_patt, the checks no limit.
inline SubtreeClasses subtree_classes(int n_tips, int n_nodes, int root, const int *sons_ptr, const int *sons, const unsigned char *z, long z_stride,
                                      long n_patt, int n_codes, uint64_t u_limit = ~0ull)
{
   SubtreeClasses sc;
   sc.u.assign(n_nodes, 0);
   sc.cls.resize(n_nodes);
   sc.son_cls.resize(n_nodes);
   sc.cherry.assign(n_nodes, 0);
   sc.done.assign(n_nodes, 0);
   if (n_patt <= 0) return sc;
   // post-order without recursion (caterpillars of thousands of tips)
   std::vector<int> order, st(1, root);
   while (!st.empty()) {
      const int v = st.back();
      st.pop_back();
      order.push_back(v);
      for (int j = sons_ptr[v]; j < sons_ptr[v + 1]; j++) st.push_back(sons[j]);
   }
   auto class_of = [&](int s, long h) -> uint32_t { return s < n_tips ? (uint32_t)z[(long)s * z_stride + h] : sc.cls[s][h]; };
   for (size_t k = order.size(); k-- > 0;) {
      const int v = order[k], ns = sons_ptr[v + 1] - sons_ptr[v];
      if (v == root || v < n_tips || ns == 0) continue;
      const int *sv = sons + sons_ptr[v];
      bool ready = true, tips_only = true;
      for (int j = 0; j < ns; j++) {
         if (sv[j] >= n_tips) { tips_only = false; ready = ready && sc.done[sv[j]]; }
      }
      if (!ready) continue;
      std::vector<uint32_t> &cv = sc.cls[v];
      cv.resize(n_patt);
      if (tips_only && ns == 2) {
         sc.cherry[v] = 1;
         std::vector<char> seen((size_t)n_codes * n_codes, 0);
         const unsigned char *za = z + (long)sv[0] * z_stride, *zb = z + (long)sv[1] * z_stride;
         for (long h = 0; h < n_patt; h++) {
            const uint32_t c = (uint32_t)za[h] * n_codes + zb[h];
            cv[h] = c;
            if (!seen[c]) { seen[c] = 1; sc.u[v]++; }
         }
         sc.done[v] = 1;
         continue;
      }
      // fold the sons in: (rank so far, next son's class) -> rank; the last fold's ranks are the node's classes
      std::vector<uint32_t> acc(n_patt), first;      // first[c]: the first pattern of class c
      for (long h = 0; h < n_patt; h++) acc[h] = class_of(sv[0], h);
      uint32_t u = 0;
      if (ns == 1) {
         detail::RankTable t(n_patt);
         for (long h = 0; h < n_patt; h++) {
            const uint32_t r = t.rank(acc[h]);
            if (r == first.size()) first.push_back((uint32_t)h);
            acc[h] = r;
         }
         u = t.n;
      }
      for (int j = 1; j < ns; j++) {
         detail::RankTable t(n_patt);
         first.clear();
         for (long h = 0; h < n_patt; h++) {
            const uint32_t r = t.rank(((uint64_t)acc[h] << 32) | class_of(sv[j], h));
            if (r == first.size()) first.push_back((uint32_t)h);
            acc[h] = r;
         }
         u = t.n;
      }
      if ((uint64_t)u > u_limit) { cv.clear(); cv.shrink_to_fit(); continue; }
      cv.swap(acc);
      sc.u[v] = u;
      sc.son_cls[v].resize((size_t)ns * u);
      for (int j = 0; j < ns; j++)
         for (uint32_t c = 0; c < u; c++) sc.son_cls[v][(size_t)j * u + c] = class_of(sv[j], first[c]);
      sc.done[v] = 1;
   }
   return sc;
}

// The order the tabulated walk visits the patterns in (kernels_prune.h: sztile_kernel; jit.h: the table form's root).  The walk gathers one
// table row per lookup and pattern; patterns of one class read the same row, so neighbours in this order should share classes.  keys[k]
// [n_patt] are the class arrays of the walk's lookups, bound[k] > every entry of keys[k]; the result is the lexicographic sort of the
// patterns by (keys[seq[0]], keys[seq[1]], ...), ties broken by the pattern number: order[position] = pattern, a permutation of
// 0 .. n_patt - 1 and a function of its arguments alone.  One stable counting sort per key, the last of the sequence first.
inline std::vector<uint32_t> subtree_pattern_order(const std::vector<const uint32_t *> &keys, const std::vector<uint32_t> &bound, const std::vector<int> &seq,
                                                   long n_patt)
{
   std::vector<uint32_t> order(n_patt > 0 ? n_patt : 0), next(order.size());
   for (long h = 0; h < n_patt; h++) order[h] = (uint32_t)h;
   for (size_t s = seq.size(); s-- > 0;) {
      const uint32_t *key = keys[seq[s]];
      std::vector<uint32_t> start((size_t)bound[seq[s]] + 1, 0);
      for (long h = 0; h < n_patt; h++) start[(size_t)key[h] + 1]++;
      for (size_t c = 1; c < start.size(); c++) start[c] += start[c - 1];
      for (long i = 0; i < n_patt; i++) next[start[key[order[i]]]++] = order[i];
      order.swap(next);
   }
   return order;
}

// The sequence of the keys: by ascending number of classes (the smallest table first: its rows change least often along the order, the
// largest table's rows are then met in runs inside every run of the others), equal counts in the order given; `largest_first` reverses it.
inline std::vector<int> subtree_order_sequence(const std::vector<uint32_t> &n_classes, bool largest_first = false)
{
   std::vector<int> seq(n_classes.size());
   for (size_t i = 0; i < seq.size(); i++) seq[i] = (int)i;
   for (size_t i = 1; i < seq.size(); i++)      // (insertion sort: a handful of keys, stable)
      for (size_t j = i; j > 0 && (largest_first ? n_classes[seq[j]] > n_classes[seq[j - 1]] : n_classes[seq[j]] < n_classes[seq[j - 1]]); j--)
         std::swap(seq[j], seq[j - 1]);
   return seq;
}

}  // namespace paml_amd

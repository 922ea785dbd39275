// The class computation of the subtree tables (paml_amd/csrc/subtree_classes.h) against a brute-force count, under the host sanitizers:
//     g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all tools/subtree_classes_check.cpp -o subtree_classes_check
//     ./subtree_classes_check            (exit status 0 and an "ok" line per case when everything agrees)
// The cases are made here: random trees (binary, with a polytomy, rooted at a tip) and small random alignments over few codes, so that
// tuples repeat; one pattern; a limit on the class count.  The reference collects, per node, the tuples of the tip codes below it
// (std::map, first occurrence order kept beside it) and holds u_v, the per-pattern class (up to the cherry numbering) and every class's
// son indices against it.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <vector>

#include "../paml_amd/csrc/subtree_classes.h"

using namespace paml_amd;

static unsigned long long rng_state = 88172645463325252ull;
static unsigned rnd(unsigned n)      // xorshift64: the same cases on every run
{
   rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
   return (unsigned)((rng_state >> 11) % n);
}

struct Tree {
   int n_tips = 0, nn = 0, root = 0;
   std::vector<int> sons_ptr, sons;
};

// joins random pairs (or, once, a triple: the polytomy) of the roots of a forest until `top` are left, which become the root's sons
static Tree make_tree(int n_tips, bool polytomy, bool tip_root, int top)
{
   std::vector<std::vector<int>> s(n_tips);
   std::vector<int> forest;
   for (int i = tip_root ? 1 : 0; i < n_tips; i++) forest.push_back(i);
   bool poly_done = !polytomy;
   while ((int)forest.size() > top) {
      const int k = (!poly_done && forest.size() >= (size_t)top + 2) ? 3 : 2;
      poly_done = poly_done || k == 3;
      std::vector<int> kids;
      for (int j = 0; j < k; j++) {
         const unsigned at = rnd((unsigned)forest.size());
         kids.push_back(forest[at]);
         forest.erase(forest.begin() + at);
      }
      s.push_back(kids);
      forest.push_back((int)s.size() - 1);
   }
   Tree t;
   t.n_tips = n_tips;
   if (tip_root) { t.root = 0; s[0] = forest; }
   else { s.push_back(forest); t.root = (int)s.size() - 1; }
   t.nn = (int)s.size();
   t.sons_ptr.push_back(0);
   for (int v = 0; v < t.nn; v++) {
      for (int x : s[v]) t.sons.push_back(x);
      t.sons_ptr.push_back((int)t.sons.size());
   }
   return t;
}

static void tips_below(const Tree &t, int v, std::vector<int> &out)
{
   if (v < t.n_tips && v != t.root) { out.push_back(v); return; }
   for (int j = t.sons_ptr[v]; j < t.sons_ptr[v + 1]; j++) tips_below(t, t.sons[j], out);
}

static int fails = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); fails++; } } while (0)

static void run_case(const char *name, int n_tips, long n_patt, int n_codes, bool polytomy, bool tip_root, int top, unsigned long long limit = ~0ull)
{
   const Tree t = make_tree(n_tips, polytomy, tip_root, top);
   std::vector<unsigned char> z((size_t)n_tips * n_patt);
   for (auto &c : z) c = (unsigned char)rnd(n_codes);
   const SubtreeClasses sc = subtree_classes(n_tips, t.nn, t.root, t.sons_ptr.data(), t.sons.data(), z.data(), n_patt, n_patt, n_codes, limit);
   int n_checked = 0;
   for (int v = 0; v < t.nn; v++) {
      const int ns = t.sons_ptr[v + 1] - t.sons_ptr[v];
      if (v == t.root || ns == 0) { CHECK(!sc.done[v] && sc.u[v] == 0); continue; }
      std::vector<int> below;
      tips_below(t, v, below);
      std::map<std::vector<unsigned char>, unsigned> rank;
      std::vector<unsigned> ref(n_patt);
      std::vector<long> first;
      for (long h = 0; h < n_patt; h++) {
         std::vector<unsigned char> key;
         for (int tip : below) key.push_back(z[(size_t)tip * n_patt + h]);
         auto it = rank.find(key);
         if (it == rank.end()) { it = rank.emplace(key, (unsigned)rank.size()).first; first.push_back(h); }
         ref[h] = it->second;
      }
      if (!sc.done[v]) {      // only beyond the limit, or above a node beyond it
         bool over = rank.size() > limit;
         for (int j = t.sons_ptr[v]; j < t.sons_ptr[v + 1]; j++) over = over || (t.sons[j] >= t.n_tips && !sc.done[t.sons[j]]);
         CHECK(over);
         continue;
      }
      n_checked++;
      CHECK(sc.u[v] == rank.size());
      CHECK((long)sc.cls[v].size() == n_patt);
      const bool cherry = ns == 2 && t.sons[t.sons_ptr[v]] < t.n_tips && t.sons[t.sons_ptr[v] + 1] < t.n_tips;
      CHECK(cherry == (bool)sc.cherry[v]);
      for (long h = 0; h < n_patt; h++) {
         if (cherry) CHECK(sc.cls[v][h] == (unsigned)z[(size_t)t.sons[t.sons_ptr[v]] * n_patt + h] * n_codes + z[(size_t)t.sons[t.sons_ptr[v] + 1] * n_patt + h]);
         else CHECK(sc.cls[v][h] == ref[h]);      // dense ranks in order of first occurrence
      }
      if (cherry) continue;
      CHECK(sc.son_cls[v].size() == (size_t)ns * sc.u[v]);
      for (int j = 0; j < ns; j++) {
         const int s = t.sons[t.sons_ptr[v] + j];
         for (unsigned c = 0; c < sc.u[v]; c++) {
            const long h = first[c];
            const unsigned want = s < t.n_tips ? z[(size_t)s * n_patt + h] : sc.cls[s][h];
            CHECK(sc.son_cls[v][(size_t)j * sc.u[v] + c] == want);
         }
      }
   }
   printf("%s %s: %d tips, %ld patterns, %d nodes with classes\n", fails ? "FAILED" : "ok", name, n_tips, n_patt, n_checked);
}

int main()
{
   run_case("binary", 9, 700, 3, false, false, 3);
   run_case("binary, two root sons", 12, 2000, 2, false, false, 2);
   run_case("polytomy", 11, 900, 3, true, false, 3);
   run_case("tip root", 8, 500, 4, false, true, 2);
   run_case("one pattern", 7, 1, 5, true, false, 3);
   run_case("many codes", 16, 3000, 61, false, false, 3);
   run_case("limit", 10, 1500, 3, false, false, 3, 40);
   return fails ? 1 : 0;
}

// The pattern order of the walk with subtree tables (paml_amd/csrc/subtree_classes.h: subtree_pattern_order, subtree_order_sequence) against
// a brute-force sort, under the host sanitizers:
//     g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all tools/subtree_order_check.cpp -o subtree_order_check
//     ./subtree_order_check            (exit status 0 and an "ok" line per case when everything agrees)
// The cases are made here: skewed class arrays (a few large classes, many of one pattern) of one to four keys, with both sequences of the
// keys; one pattern; no key; a key with one class; bounds far above the classes that occur.  The reference is std::sort over (key tuple,
// pattern); the order must equal it and be a permutation.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "../paml_amd/csrc/subtree_classes.h"

using namespace paml_amd;

static unsigned long long rng_state = 88172645463325252ull;
static unsigned rnd(unsigned n)      // xorshift64: the same cases on every run
{
   rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
   return (unsigned)((rng_state >> 11) % n);
}

static int fails = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); fails++; } } while (0)

static void run_case(const char *name, long n_patt, const std::vector<uint32_t> &bound, bool largest_first)
{
   const int nk = (int)bound.size();
   std::vector<std::vector<uint32_t>> key(nk, std::vector<uint32_t>(n_patt));
   std::vector<const uint32_t *> kp(nk);
   for (int k = 0; k < nk; k++) {
      for (long h = 0; h < n_patt; h++) {      // the smaller of two draws, twice: skewed towards the low classes
         const uint32_t a = rnd(bound[k]), b = rnd(bound[k]), c = rnd(bound[k]);
         key[k][h] = std::min(a, std::min(b, c));
      }
      kp[k] = key[k].data();
   }
   const std::vector<int> seq = subtree_order_sequence(bound, largest_first);
   CHECK((int)seq.size() == nk);
   for (int i = 1; i < nk; i++) {
      CHECK(largest_first ? bound[seq[i - 1]] >= bound[seq[i]] : bound[seq[i - 1]] <= bound[seq[i]]);
      if (bound[seq[i - 1]] == bound[seq[i]]) CHECK(seq[i - 1] < seq[i]);
   }
   const std::vector<uint32_t> order = subtree_pattern_order(kp, bound, seq, n_patt);
   CHECK((long)order.size() == n_patt);
   std::vector<uint32_t> ref(n_patt);
   for (long h = 0; h < n_patt; h++) ref[h] = (uint32_t)h;
   std::sort(ref.begin(), ref.end(), [&](uint32_t a, uint32_t b) {
      for (int s : seq)
         if (key[s][a] != key[s][b]) return key[s][a] < key[s][b];
      return a < b;
   });
   std::vector<char> seen(n_patt, 0);
   bool same = order.size() == ref.size();
   for (long i = 0; same && i < n_patt; i++) {
      same = order[i] == ref[i] && order[i] < n_patt && !seen[order[i]];
      if (same) seen[order[i]] = 1;
   }
   CHECK(same);
   CHECK(subtree_pattern_order(kp, bound, seq, n_patt) == order);      // a function of its arguments
   printf("%s %s: %ld patterns, %d keys, %s first\n", fails ? "FAILED" : "ok", name, n_patt, nk, largest_first ? "largest" : "smallest");
}

int main()
{
   for (int lf = 0; lf < 2; lf++) {
      run_case("three tables", 5000, {900, 40, 3721}, lf != 0);
      run_case("one table", 3000, {500}, lf != 0);
      run_case("four tables, two of a size", 2000, {30, 200, 30, 7}, lf != 0);
      run_case("one pattern", 1, {5, 3}, lf != 0);
      run_case("no key", 100, {}, lf != 0);
      run_case("one class", 300, {1, 50}, lf != 0);
      run_case("sparse bounds", 400, {1000000, 70000}, lf != 0);
      run_case("partial last tile", 128 * 3 + 37, {37, 12}, lf != 0);
   }
   return fails ? 1 : 0;
}

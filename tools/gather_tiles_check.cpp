// The tiles of the gathering walk (paml_amd/csrc/gather_tiles.h: gather_tiles, gather_tiles_pack) against a brute-force recount, under the
// host sanitizers:
//     g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all tools/gather_tiles_check.cpp -o gather_tiles_check
//     ./gather_tiles_check            (exit status 0 and an "ok" line per case when everything agrees)
// The cases are made here: 1, 127, 128, 129 and 128 * 5 + 37 patterns; a table with one row; every row distinct (tiles cut by R); R = 8, which
// cuts everywhere; with and without a pattern order.  Checked: every position appears exactly once and in order; no tile has more than 128
// patterns or more than R rows; every slot points at the pattern's own row; no list holds a row twice; the cut is the greedy one (the
// pattern behind a tile would not have fitted); and the blocks the kernel reads say the same.
#include <algorithm>
#include <cstdio>
#include <set>
#include <vector>

#include "../paml_amd/csrc/gather_tiles.h"

using namespace paml_amd;

static unsigned long long rng_state = 88172645463325252ull;
static unsigned rnd(unsigned n)      // xorshift64: the same cases on every run
{
   rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
   return (unsigned)((rng_state >> 11) % n);
}

static int fails = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); fails++; } } while (0)

// kind 0: skewed draws below the bound; 1: every row distinct (row = pattern)
static void run_case(const char *name, long n_patt, const std::vector<uint32_t> &bound, int R, bool ordered, int kind = 0)
{
   const int before = fails;
   const int nk = (int)bound.size();
   std::vector<std::vector<uint32_t>> key(nk, std::vector<uint32_t>(n_patt));
   std::vector<const uint32_t *> kp(nk);
   for (int k = 0; k < nk; k++) {
      for (long h = 0; h < n_patt; h++) key[k][h] = kind == 1 ? (uint32_t)h : std::min(rnd(bound[k]), std::min(rnd(bound[k]), rnd(bound[k])));
      kp[k] = key[k].data();
   }
   std::vector<uint32_t> order(n_patt);
   for (long h = 0; h < n_patt; h++) order[h] = (uint32_t)h;
   if (ordered) {
      for (long h = n_patt - 1; h > 0; h--) std::swap(order[h], order[rnd((unsigned)h + 1)]);      // any permutation will do for the cut
      std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return key[0][a] < key[0][b]; });
   }
   std::vector<unsigned char> wflag(n_patt);
   for (long h = 0; h < n_patt; h++) wflag[h] = rnd(5) != 0;
   const uint32_t *op = ordered ? order.data() : nullptr;
   const GatherTiles g = gather_tiles(kp, bound, op, n_patt, R);
   CHECK(g.n_lookups == nk && g.R == R);
   CHECK(g.list_at.size() == g.n_tiles() * nk + 1 && g.list_at.back() == g.rows.size());
   long next = 0;
   for (size_t t = 0; t < g.n_tiles(); t++) {
      CHECK((long)g.first[t] == next);      // every position once, in order
      CHECK(g.count[t] >= 1 && g.count[t] <= (uint32_t)GATHER_TILE_PATT);
      int distinct = 0;
      std::vector<std::set<uint32_t>> want(nk);
      for (int k = 0; k < nk; k++) {
         const uint32_t b = g.list_at[t * nk + k], e = g.list_at[t * nk + k + 1];
         std::set<uint32_t> in_list(g.rows.begin() + b, g.rows.begin() + e);
         CHECK(in_list.size() == e - b);      // no row twice
         for (uint32_t i = 0; i < g.count[t]; i++) {
            const long pos = (long)g.first[t] + i, h = order[pos];
            const uint32_t s = g.slot[(size_t)k * n_patt + pos];
            CHECK(s < e - b && g.rows[b + s] == key[k][h]);      // the slot points at the pattern's own row
            want[k].insert(key[k][h]);
         }
         CHECK(want[k] == in_list);      // ... and the list holds nothing else
         distinct += (int)in_list.size();
      }
      CHECK(distinct <= R);
      next += g.count[t];
      if (next < n_patt && g.count[t] < (uint32_t)GATHER_TILE_PATT) {      // greedy: the next pattern would have taken the tile past R
         int fresh = 0;
         for (int k = 0; k < nk; k++) fresh += !want[k].count(key[k][order[next]]);
         CHECK(distinct + fresh > R);
      }
   }
   CHECK(next == n_patt);
   // the blocks
   const std::vector<unsigned char> blk = gather_tiles_pack(g, op, wflag.data(), n_patt);
   const int DB = gather_desc_bytes(R);
   CHECK(blk.size() == g.n_tiles() * (size_t)DB && DB % 256 == 0 && gather_desc_off_patt(R) + 4 * GATHER_TILE_PATT <= DB);
   for (size_t t = 0; t < g.n_tiles() && blk.size() == g.n_tiles() * (size_t)DB; t++) {
      const unsigned char *d = blk.data() + t * (size_t)DB;
      const int32_t *head = (const int32_t *)d;
      const uint32_t *rows = (const uint32_t *)(d + 32);
      const int32_t *patt = (const int32_t *)(d + gather_desc_off_patt(R));
      const int start[5] = {0, head[2], head[3], head[4], head[5]};
      CHECK(head[0] == (int32_t)g.first[t] && head[1] == (int32_t)g.count[t]);
      CHECK(head[5] % 2 == 0 && head[5] <= gather_desc_slots(R));
      for (int k = 0; k < GATHER_MAX_LOOKUPS; k++) CHECK(start[k] % 2 == 0 && start[k] <= start[k + 1]);
      for (int k = nk; k < GATHER_MAX_LOOKUPS; k++) CHECK(start[k] == head[5]);
      for (int k = 0; k < nk; k++) {
         const uint32_t b = g.list_at[t * nk + k], n = g.list_at[t * nk + k + 1] - b;
         CHECK(start[k + 1] - start[k] == (int)((n + 1) & ~1u));
         for (uint32_t i = 0; i < n; i++) CHECK(rows[start[k] + i] == g.rows[b + i]);
         if (n & 1) CHECK(rows[start[k] + n] == g.rows[b + n - 1]);      // the odd list's last row once more
         for (int i = 0; i < GATHER_TILE_PATT; i++) {
            const int s = d[gather_desc_off_slot(R) + k * GATHER_TILE_PATT + i];
            if ((uint32_t)i < g.count[t]) CHECK(s >= start[k] && s < start[k] + (int)n && rows[s] == key[k][order[g.first[t] + i]]);
            else CHECK(s == start[k]);
         }
      }
      for (int i = 0; i < GATHER_TILE_PATT; i++) {
         const bool in = (uint32_t)i < g.count[t];
         const uint32_t h = order[g.first[t] + (in ? i : 0)];
         CHECK(patt[i] == (int32_t)h);
         CHECK(d[gather_desc_off_flag(R) + i] == (in ? wflag[h] : 0));
      }
   }
   printf("%s %s: %ld patterns, %d lookups, R = %d, %s, %zu tiles, %ld rows\n", fails == before ? "ok" : "FAILED", name, n_patt, nk, R,
          ordered ? "ordered" : "alignment order", g.n_tiles(), g.total_rows());
}

int main()
{
   for (int ord = 0; ord < 2; ord++) {
      for (long n : {1L, 127L, 128L, 129L, 128L * 5 + 37}) {
         run_case("three tables", n, {900, 40, 3721}, 128, ord != 0);
         run_case("three tables", n, {900, 40, 3721}, 96, ord != 0);
         run_case("cuts everywhere", n, {900, 40, 3721}, 8, ord != 0);
      }
      run_case("a table with one row", 128 * 5 + 37, {1, 50}, 128, ord != 0);
      run_case("one row each", 300, {1, 1}, 128, ord != 0);
      run_case("every row distinct", 128 * 5 + 37, {128 * 5 + 37, 128 * 5 + 37, 128 * 5 + 37}, 128, ord != 0, 1);
      run_case("every row distinct, four lookups", 300, {300, 300, 300, 300}, 160, ord != 0, 1);
      run_case("R = lookups", 200, {30, 30, 30}, 3, ord != 0);
      run_case("one lookup", 1000, {77}, 128, ord != 0);
   }
   {  // fewer rows than lookups allowed: nothing, not a crash
      const std::vector<uint32_t> k(10, 0);
      const GatherTiles g = gather_tiles({k.data(), k.data()}, {1, 1}, nullptr, 10, 1);
      CHECK(g.n_tiles() == 0);
      printf("%s R below the lookups\n", g.n_tiles() == 0 ? "ok" : "FAILED");
   }
   return fails ? 1 : 0;
}

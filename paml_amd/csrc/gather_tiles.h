// gather_tiles.h — host side of the gathering walk (kernels_prune.h: gather_walk_kernel): the tiles of the tabulated walk with the distinct
// table rows each of them reads.  No device call and no engine: pure functions of their arguments, so that tools/gather_tiles_check.cpp
// runs them under the host sanitizers and paml_amd_debug_gather_tiles plays them for the tests.
//
// The walk reads one 512-byte table row per lookup and pattern; patterns of one class read the same row, and the pattern order
// (subtree_classes.h: subtree_pattern_order) puts them side by side.  A tile is a run of at most GATHER_TILE_PATT positions of that
// order whose distinct rows, all lookups together, number at most R: the kernel fetches every one of them once into LDS, and a pattern
// finds its row of lookup k through a one-byte slot into the tile's list k.  The lists do not depend on the class of the model (it only
// moves the tables' base), so they are computed once per (tips, tree, selection), never per evaluation.
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

namespace paml_amd {

constexpr int GATHER_TILE_PATT = 128;      // patterns per tile at most: 8 waves x 16
constexpr int GATHER_MAX_LOOKUPS = 4;
constexpr int GATHER_R_MAX = 160;          // (a slot is one byte; the kernel's LDS holds two row buffers of R <= 128)

struct GatherTiles {
   int n_lookups = 0, R = 0;
   std::vector<uint32_t> first, count;      // per tile: first position of the order, patterns
   std::vector<uint32_t> list_at;           // [tile * n_lookups + k]: where list k of the tile starts in `rows`; one entry more at the end
   std::vector<uint32_t> rows;              // the lists one behind the other: table-relative row numbers, in order of first use
   std::vector<uint8_t> slot;               // [k][position]: the position's row of lookup k is entry `slot` of its tile's list k
   size_t n_tiles() const { return first.size(); }
   long total_rows() const { return (long)rows.size(); }
};

// cls[k][pattern] < bound[k]: the (row-mapped, clamped) row of lookup k; order[position] = pattern (null: the identity).  Tiles are cut
// greedily along the order: a position joins the open tile unless that would give it more than GATHER_TILE_PATT patterns or more than R
// distinct rows.  n_lookups <= R is required (a tile of one pattern must fit).
inline GatherTiles gather_tiles(const std::vector<const uint32_t *> &cls, const std::vector<uint32_t> &bound, const uint32_t *order, long n_patt, int R)
{
   GatherTiles g;
   g.n_lookups = (int)cls.size();
   g.R = R;
   const int nk = g.n_lookups;
   if (n_patt <= 0 || nk < 1 || R < nk) return g;
   g.slot.assign((size_t)nk * n_patt, 0);
   std::vector<std::vector<uint32_t>> seen_in(nk);      // row -> 1 + the last tile that lists it
   std::vector<std::vector<uint8_t>> slot_of(nk);       // ... and its slot there
   for (int k = 0; k < nk; k++) { seen_in[k].assign(bound[k], 0); slot_of[k].assign(bound[k], 0); }
   std::vector<std::vector<uint32_t>> open(nk);         // the open tile's lists
   uint32_t tile_first = 0, tile_count = 0;
   int distinct = 0;
   auto close = [&]() {
      g.first.push_back(tile_first);
      g.count.push_back(tile_count);
      for (int k = 0; k < nk; k++) {
         g.list_at.push_back((uint32_t)g.rows.size());
         g.rows.insert(g.rows.end(), open[k].begin(), open[k].end());
         open[k].clear();
      }
      distinct = 0;
      tile_count = 0;
   };
   for (long pos = 0; pos < n_patt; pos++) {
      const long h = order ? (long)order[pos] : pos;
      const uint32_t tile_id = (uint32_t)g.first.size() + 1;
      int fresh = 0;
      for (int k = 0; k < nk; k++) fresh += seen_in[k][cls[k][h]] != tile_id;
      if (tile_count && (tile_count == (uint32_t)GATHER_TILE_PATT || distinct + fresh > R)) close();
      if (!tile_count) tile_first = (uint32_t)pos;
      const uint32_t id = (uint32_t)g.first.size() + 1;
      for (int k = 0; k < nk; k++) {
         const uint32_t r = cls[k][h];
         if (seen_in[k][r] != id) {
            seen_in[k][r] = id;
            slot_of[k][r] = (uint8_t)open[k].size();
            open[k].push_back(r);
            distinct++;
         }
         g.slot[(size_t)k * n_patt + pos] = slot_of[k][r];
      }
      tile_count++;
   }
   if (tile_count) close();
   g.list_at.push_back((uint32_t)g.rows.size());
   return g;
}

// ---- what the kernel reads of it: one block of gather_desc_bytes(R) per tile ---------------------------------------------------------
//   int   head[8]   first position, patterns, first slot of the lists 1, 2, 3, slots in all (an even number), 0, 0
//   uint  rows[R + 4]   the lists one behind the other, each starting at an EVEN slot (a wave instruction fetches the rows of two
//                       neighbouring slots from ONE table); an odd list is followed by its last row once more
//   uchar slot[4][128]  per lookup and pattern of the tile: its slot (counted from the block's first); past the tile's end: the list's first
//   uchar flag[128]     weight > 0
//   int   patt[128]     order[position]; past the tile's end: the tile's first pattern
// Lists of lookups the walk does not have start at `slots in all`.  (constexpr: the kernel uses the same functions)
constexpr int gather_desc_slots(int R) { return R + GATHER_MAX_LOOKUPS; }
constexpr int gather_desc_off_slot(int R) { return 32 + 4 * gather_desc_slots(R); }
constexpr int gather_desc_off_flag(int R) { return gather_desc_off_slot(R) + GATHER_MAX_LOOKUPS * GATHER_TILE_PATT; }
constexpr int gather_desc_off_patt(int R) { return gather_desc_off_flag(R) + GATHER_TILE_PATT; }
constexpr int gather_desc_bytes(int R) { return (gather_desc_off_patt(R) + 4 * GATHER_TILE_PATT + 255) / 256 * 256; }

inline std::vector<unsigned char> gather_tiles_pack(const GatherTiles &g, const uint32_t *order, const unsigned char *wflag, long n_patt)      // wflag[pattern]: weight > 0
{
   const int R = g.R, nk = g.n_lookups, DB = gather_desc_bytes(R);
   std::vector<unsigned char> out(g.n_tiles() * (size_t)DB, 0);
   for (size_t t = 0; t < g.n_tiles(); t++) {
      unsigned char *d = out.data() + t * (size_t)DB;
      int32_t head[8] = {(int32_t)g.first[t], (int32_t)g.count[t], 0, 0, 0, 0, 0, 0};
      uint32_t *rows = (uint32_t *)(d + 32);
      int at = 0, start[GATHER_MAX_LOOKUPS] = {0, 0, 0, 0};
      for (int k = 0; k < nk; k++) {
         start[k] = at;
         const uint32_t b = g.list_at[t * nk + k], e = g.list_at[t * nk + k + 1];
         for (uint32_t i = b; i < e; i++) rows[at++] = g.rows[i];
         if (at & 1) { rows[at] = rows[at - 1]; at++; }
      }
      for (int k = nk; k < GATHER_MAX_LOOKUPS; k++) start[k] = at;
      head[2] = start[1]; head[3] = start[2]; head[4] = start[3]; head[5] = at;
      memcpy(d, head, sizeof head);
      unsigned char *slot = d + gather_desc_off_slot(R), *flag = d + gather_desc_off_flag(R);
      int32_t *patt = (int32_t *)(d + gather_desc_off_patt(R));
      const long h_first = order ? (long)order[g.first[t]] : (long)g.first[t];
      for (int i = 0; i < GATHER_TILE_PATT; i++) {
         const bool in = (uint32_t)i < g.count[t];
         const long pos = (long)g.first[t] + i, h = in ? (order ? (long)order[pos] : pos) : h_first;
         for (int k = 0; k < nk; k++) slot[k * GATHER_TILE_PATT + i] = (unsigned char)(start[k] + (in ? g.slot[(size_t)k * n_patt + pos] : 0));
         flag[i] = in && wflag[h] ? 1 : 0;
         patt[i] = (int32_t)h;
      }
   }
   return out;
}

}  // namespace paml_amd

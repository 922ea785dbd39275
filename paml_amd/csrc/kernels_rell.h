// RELL / SH bootstrap replicates on the device (the resampling loop of rell(), treesub.c:5844-6009).
//
//   rep[r][t] = sum over the ls draws of replicate r of lnf[t][pattern(draw)],   sites drawn with replacement inside each gene.
//
// Draws are counter-based: no generator state lives anywhere.  With
//     GAMMA   = 0x9E3779B97F4A7C15
//     mix(z)  : z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;  z = (z ^ z >> 27) * 0x94D049BB133111EB;  return z ^ z >> 31
//               (the SplitMix64 finaliser; all arithmetic modulo 2^64)
//     stream(seed, r, g) = mix(seed + GAMMA * ((r << 32 | g) + 1))            r = replicate, g = gene (empty genes keep their number)
//     u(seed, r, g, j)   = mix(stream(seed, r, g) + GAMMA * (j + 1))          = output j of SplitMix64 started at stream(seed, r, g)
//     site               = first site of gene g + ((u * lgene) >> 64)         the high 64 bits of the 64 x 64-bit product
// draw j of gene g of replicate r is a pure function of (seed, r, g, j): the same for every n_rep, grid, batch and device.
//
// Summation order, fixed: the ls draws of a replicate, genes one after the other, are numbered d = 0 .. ls - 1 and cut into chunks
// of RELL_CHUNK = 4096 consecutive draws.  One wave owns one (replicate, chunk): lane l adds the draws d0 + l, d0 + l + 64,
// d0 + l + 128, ... in that order into its own accumulator, then the 64 lane sums are combined by the xor butterfly 32, 16, 8, 4, 2, 1
// (a + b commutes, so every lane ends with the same bits).  rell_sum_chunks then adds a replicate's chunk sums in chunk order.
// No floating-point atomics.
//
// Layout: lnf is transposed once to tab[pattern][T_pad], T_pad = n_trees rounded up to a power of two >= 2, padding = 0: one draw is
// one contiguous 16 / 32 / 64-byte read.  Above T_pad = RELL_TREE_BLOCK = 8 the trees are walked in blocks of 8 (blockIdx.y), each
// block re-deriving the draws.  The site -> pattern map is the expanded site list int[ls], built from the integer weights by an
// inclusive scan (end[h]) and a fill (site s belongs to the first pattern with end[h] > s: patterns of weight 0 never appear).
//
// What bounds it: per draw two dependent random reads (4 bytes of the site list, then one row of the table) against about 40 integer
// instructions for the hash — latency / sector-bound gathers out of L2 and the Infinity Cache; four draws per lane are in flight at
// a time and the kernel runs at full occupancy to hide them.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels_rng.h"      // rell_mix, rell_stream, RELL_GAMMA: shared with kernels_simulate.h

namespace paml_amd {

#define RELL_CHUNK 4096           // draws per (replicate, chunk) = per wave
#define RELL_TREE_BLOCK 8         // trees per pass over the draws
#define RELL_THREADS 256
#define RELL_SCAN_TILE 2048

// ---- site list: inclusive scan of the integer weights, then one thread per site ----
__global__ __launch_bounds__(RELL_THREADS) void rell_tile_sums(const int *w, int n, int *sums)
{
   __shared__ int s[RELL_THREADS];
   int t = 0;
   const int base = blockIdx.x * RELL_SCAN_TILE;
   for (int r = 0; r < RELL_SCAN_TILE / RELL_THREADS; r++) {
      const int e = base + r * RELL_THREADS + threadIdx.x;
      if (e < n) t += w[e];
   }
   s[threadIdx.x] = t;
   __syncthreads();
   for (int st = RELL_THREADS / 2; st >= 1; st >>= 1) {
      if (threadIdx.x < st) s[threadIdx.x] += s[threadIdx.x + st];
      __syncthreads();
   }
   if (threadIdx.x == 0) sums[blockIdx.x] = s[0];
}

// exclusive scan of the m tile sums in place, one block
__global__ __launch_bounds__(1024) void rell_scan_tiles(int *v, int m)
{
   __shared__ int s[1024];
   const int per = (m + 1023) / 1024, lo = min((int)threadIdx.x * per, m), hi = min(lo + per, m);
   int sum = 0;
   for (int i = lo; i < hi; i++) sum += v[i];
   s[threadIdx.x] = sum;
   __syncthreads();
   for (int off = 1; off < 1024; off <<= 1) {
      const int t = (int)threadIdx.x >= off ? s[threadIdx.x - off] : 0;
      __syncthreads();
      s[threadIdx.x] += t;
      __syncthreads();
   }
   int run = s[threadIdx.x] - sum;
   for (int i = lo; i < hi; i++) { const int x = v[i]; v[i] = run; run += x; }
}

// end[h] = w[0] + ... + w[h]
__global__ __launch_bounds__(RELL_THREADS) void rell_tile_scan(const int *w, const int *tile_off, int n, int *end)
{
   __shared__ int s[RELL_THREADS];
   constexpr int PER = RELL_SCAN_TILE / RELL_THREADS;      // 8 consecutive patterns per thread
   const int base = blockIdx.x * RELL_SCAN_TILE + threadIdx.x * PER;
   int loc[PER], t = 0;
   for (int k = 0; k < PER; k++) { loc[k] = base + k < n ? w[base + k] : 0; t += loc[k]; }
   s[threadIdx.x] = t;
   __syncthreads();
   for (int off = 1; off < RELL_THREADS; off <<= 1) {
      const int v = (int)threadIdx.x >= off ? s[threadIdx.x - off] : 0;
      __syncthreads();
      s[threadIdx.x] += v;
      __syncthreads();
   }
   int run = tile_off[blockIdx.x] + s[threadIdx.x] - t;
   for (int k = 0; k < PER; k++) {
      if (base + k >= n) break;
      run += loc[k];
      end[base + k] = run;
   }
}

// site[s] = the first pattern h with end[h] > s
__global__ __launch_bounds__(RELL_THREADS) void rell_fill_sites(const int *end, int n_patt, int ls, int *site)
{
   const int s = blockIdx.x * RELL_THREADS + threadIdx.x;
   if (s >= ls) return;
   int lo = 0, hi = n_patt - 1;      // end[n_patt - 1] = ls > s
   while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (end[mid] > s) hi = mid; else lo = mid + 1;
   }
   site[s] = lo;
}

// tab[h][t] = lnf[t][h], zero in the padding columns
__global__ __launch_bounds__(RELL_THREADS) void rell_transpose(const double *lnf, int n_trees, int n_patt, int t_pad, double *tab)
{
   const int h = blockIdx.x * RELL_THREADS + threadIdx.x;
   if (h >= n_patt) return;
   for (int t = 0; t < t_pad; t++) tab[(size_t)h * t_pad + t] = t < n_trees ? lnf[(size_t)t * n_patt + h] : 0.0;
}

struct RellArgs {
   const double *tab;      // [n_patt][t_pad]
   const int *site;        // [ls] site -> pattern
   const int *soff;        // [n_genes + 1] first site of every gene; soff[n_genes] = ls
   double *part;           // [n_rep_batch][n_chunks][t_pad] chunk sums
   unsigned long long seed;
   int ls, n_genes, n_chunks, t_pad;
   int rep0;               // first replicate of this batch
   long n_items;           // n_rep_batch * n_chunks
};

template <int TB> struct RellRow { double v[TB]; };

template <int TB> __device__ __forceinline__ RellRow<TB> rell_load_row(const double *p)
{
   RellRow<TB> r;
   const double2 *q = reinterpret_cast<const double2 *>(p);      // rows are 16-byte aligned: t_pad is even
#pragma unroll
   for (int k = 0; k < TB / 2; k++) { const double2 x = q[k]; r.v[2 * k] = x.x; r.v[2 * k + 1] = x.y; }
   return r;
}

// one wave per (replicate, chunk); blockIdx.y = block of TB trees
template <int TB> __global__ __launch_bounds__(RELL_THREADS) void rell_chunk_sums(RellArgs a)
{
   const int lane = threadIdx.x & 63;
   const long item = (long)blockIdx.x * (RELL_THREADS / 64) + (threadIdx.x >> 6);
   if (item >= a.n_items) return;      // wave-uniform
   const int rl = (int)(item / a.n_chunks), c = (int)(item - (long)rl * a.n_chunks);
   const unsigned r = (unsigned)(a.rep0 + rl);
   const int d0 = c * RELL_CHUNK, d1 = min(d0 + RELL_CHUNK, a.ls);      // c * RELL_CHUNK < ls < 2^31
   const double *tab = a.tab + (size_t)blockIdx.y * TB;
   double acc[TB];
#pragma unroll
   for (int k = 0; k < TB; k++) acc[k] = 0.0;
   // the gene of this lane's first draw; later draws only move forward
   int g = 0;
   {  int lo = 0, hi = a.n_genes - 1;
      const int d = min(d0 + lane, a.ls - 1);
      while (lo < hi) {      // the last g with soff[g] <= d
         const int mid = (lo + hi + 1) >> 1;
         if (a.soff[mid] <= d) lo = mid; else hi = mid - 1;
      }
      g = lo; }
   int g0 = a.soff[g], g1 = a.soff[g + 1];
   unsigned long long st = rell_stream(a.seed, r, (unsigned)g);
   constexpr int U = 4;      // draws of one lane in flight
   for (long d = d0 + lane; d < d1; d += 64 * U) {      // long: d + 64 u may pass 2^31 at the end of the longest alignment
      int pat[U];
      bool ok[U];
#pragma unroll
      for (int u = 0; u < U; u++) {
         const long du = d + 64 * u;
         ok[u] = du < d1;
         pat[u] = 0;
         if (ok[u]) {
            while (du >= g1) { g++; g0 = g1; g1 = a.soff[g + 1]; st = rell_stream(a.seed, r, (unsigned)g); }      // empty genes: g1 == g0, passed over
            const unsigned long long x = rell_mix(st + RELL_GAMMA * ((unsigned long long)(du - g0 + 1)));
            pat[u] = a.site[g0 + (int)__umul64hi(x, (unsigned long long)(g1 - g0))];
         }
      }
      RellRow<TB> row[U];
#pragma unroll
      for (int u = 0; u < U; u++) row[u] = rell_load_row<TB>(tab + (size_t)pat[u] * a.t_pad);      // pattern 0 for the lanes past the end: in bounds, not added
#pragma unroll
      for (int u = 0; u < U; u++)
         if (ok[u]) {
#pragma unroll
            for (int k = 0; k < TB; k++) acc[k] += row[u].v[k];
         }
   }
#pragma unroll
   for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
      for (int k = 0; k < TB; k++) acc[k] += __shfl_xor(acc[k], off, 64);
   }
   if (lane == 0) {
      double *o = a.part + (size_t)item * a.t_pad + (size_t)blockIdx.y * TB;
#pragma unroll
      for (int k = 0; k < TB; k++) o[k] = acc[k];
   }
}

// rep[r][t] = the chunk sums of replicate r in chunk order
__global__ __launch_bounds__(RELL_THREADS) void rell_sum_chunks(const double *part, int n_rep, int n_chunks, int t_pad, int n_trees, double *rep)
{
   const long i = (long)blockIdx.x * RELL_THREADS + threadIdx.x;
   if (i >= (long)n_rep * n_trees) return;
   const int r = (int)(i / n_trees), t = (int)(i - (long)r * n_trees);
   const double *p = part + (size_t)r * n_chunks * t_pad + t;
   double s = 0.0;
   for (int c = 0; c < n_chunks; c++) s += p[(size_t)c * t_pad];
   rep[i] = s;
}

}  // namespace paml_amd

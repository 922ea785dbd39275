// Simulation of alignments under the engine's model on the device (the role of Evolve / Simulate, evolver.c:737-805 and 818).
//
// One site is drawn independently of every other: a site class, a state at the root, then along every branch, from the root down, the
// state at the branch's lower end given the state at its upper end.  The definition, all of it part of the contract (tests/simulate_ref.py
// restates it in numpy and the device's bytes equal that restatement's):
//
// Random numbers.  Counter-based, the SplitMix64 finaliser of kernels_rng.h (rell_mix, rell_stream, GAMMA = RELL_GAMMA; written out in kernels_rell.h).  For replicate
// r, gene 0 and the GLOBAL site index j (0-based over the whole request: first_site + the site's position in the call), draw number d of
// the site is
//     u64 = mix(stream(seed, r, 0) + GAMMA * (j * (n_nodes + 2) + d + 1))        (all arithmetic modulo 2^64)
//     u   = (u64 >> 11) * 2^-53                                                   in [0, 1)
//     d = 0          the site class
//     d = 1          the state at the root
//     d = 2 + node   the state at the lower end of the branch above `node`
// A site is a pure function of (seed, r, j): the same bytes for every n_sites, first_site, batch size, grid and device.
//
// Inverse CDF.  The class is drawn from freqK[0..K), the root state from pi[0..n), the state of a child from the row
// P(t)[parent's state][.] of the matrix of the site's class and the child's branch — row-major P[from * n + to], exactly as an
// evaluation builds it (kernels_pmat.h: branch length x class rate x gene rate x Qfactor, the eigen set of eigen_of[class][label]).
// In every case c_k = max(p_0, 0) + ... + max(p_k, 0), summed sequentially in double in ascending index order (PMatCijk does not clamp:
// negative entries count as 0), and the drawn value is the first k with u < c_k.  If rounding leaves u >= c_last, the drawn value is the
// last index whose entry is positive (the last index of all if none is).  K = 1 still consumes draw 0.
//
// The walk.  Pre-order from the engine's root over the engine's own tree (any number of sons per node, any number of internal nodes, a
// root that is a tip: its drawn state is then that tip's sequence).
//
// Kernels.  sim_cdf_kernel: one lane per row of every P(t) (and one each for pi and freqK) forms the cumulative row sequentially — a
// parallel scan would change the association and the bits.  sim_walk_kernel: a workgroup owns a tile of SIM_TILE consecutive sites, one
// per lane, and walks the tree node-outer: for each node in pre-order the node's tables of all classes are staged in LDS when they fit
// (K n^2 <= SIM_LDS_CDF doubles: 61 states at K = 1 do, M8's 11 classes do not and are read from L2), every lane reads its parent's
// state byte, searches its row (binary search, ceil(log2 n) + 1 steps; n <= 5: the row's thresholds in registers and one compare each) and
// writes one byte.  A tile's node states live in LDS while the tree fits (n_nodes <= SIM_LDS_NODES), otherwise the parent's byte is
// read back from the output array [n_nodes][batch], which the same lane wrote.  Ordinary byte stores only; no atomics.
//
// What bounds it: per site n_nodes - 1 dependent gathers of ceil(log2 n) + 1 doubles out of a table row chosen by a random byte, about 40
// integer instructions of hash per draw, and n_nodes bytes written: latency-bound random reads out of LDS (or L2), hidden by
// occupancy; the HBM traffic is the n_nodes output bytes per site.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels_rng.h"

namespace paml_amd {

#define SIM_TILE 256            // sites per workgroup, one per lane
#define SIM_LDS_CDF 4096        // doubles of LDS for one node's tables of all classes (32 KB)
#define SIM_LDS_NODES 64        // nodes whose states a tile keeps in LDS (16 KB)

// Row r < n_rows: the cumulative form of P's row r (r = (class * n_nodes + node) * n + from; the root's rows are skipped: there is no
// branch above it).  Row n_rows: pi.  Row n_rows + 1: freqK.  last[row] = the last index with a positive entry.
__global__ __launch_bounds__(256) void sim_cdf_kernel(const double *P, const double *pi, const double *freqK, int n, int K, int n_nodes, int root,
                                                      double *cdf, unsigned char *last)
{
   const long n_rows = (long)K * n_nodes * n, r = (long)blockIdx.x * 256 + threadIdx.x;
   if (r >= n_rows + 2) return;
   const double *src;
   int len = n;
   if (r < n_rows) {
      if ((int)((r / n) % n_nodes) == root) return;
      src = P + r * n;
   }
   else if (r == n_rows) src = pi;
   else { src = freqK; len = K; }
   double *dst = cdf + (r <= n_rows ? r * n : n_rows * n + n);
   double c = 0;
   int lp = len - 1;
   for (int k = 0; k < len; k++) {
      const double p = src[k];
      if (p > 0) { c += p; lp = k; }
      dst[k] = c;
   }
   last[r] = (unsigned char)lp;
}

struct SimArgs {
   const double *cdf;            // [K][n_nodes][n][n], then pi's [n], then freqK's [K]
   const unsigned char *last;    // [K * n_nodes * n + 2]
   const int2 *order;            // [n_nodes - 1] (node, parent) in pre-order
   unsigned char *state;         // [n_nodes][stride] the batch's states
   unsigned char *cls;           // [stride]
   unsigned long long stream;    // rell_stream(seed, replicate, 0)
   long site0;                   // global index of the batch's first site
   long n_sites, stride;         // sites of this batch; row stride of `state`
   int n, K, n_nodes, root;
   int lds_cdf, lds_state;       // the node's tables / the tile's states are kept in LDS
};

__device__ __forceinline__ double sim_u(unsigned long long base, int d)
{
   const unsigned long long x = rell_mix(base + RELL_GAMMA * (unsigned long long)(d + 1));
   return (double)(x >> 11) * 0x1.0p-53;
}

// the first k in [0, len) with u < c[k]; `fallback` if there is none
template <bool SMALL> __device__ __forceinline__ int sim_search(const double *c, int len, double u, const unsigned char *fallback)
{
   int k;
   if (SMALL) {      // len <= 5: c is non-decreasing, so the first k with u < c[k] is the number of k with u >= c[k]
      double t[5];
#pragma unroll
      for (int i = 0; i < 5; i++) t[i] = i < len ? c[i] : 2.0;
      k = 0;
#pragma unroll
      for (int i = 0; i < 5; i++) k += u >= t[i] ? 1 : 0;
   }
   else {
      int lo = 0, hi = len;
      while (lo < hi) {
         const int mid = (lo + hi) >> 1;
         if (u < c[mid]) hi = mid; else lo = mid + 1;
      }
      k = lo;
   }
   return k < len ? k : (int)*fallback;
}

template <bool SMALL> __global__ __launch_bounds__(SIM_TILE) void sim_walk_kernel(SimArgs a)
{
   extern __shared__ __attribute__((aligned(16))) double sim_lds[];
   const int tid = threadIdx.x, n = a.n, K = a.K, nn = a.n_nodes, n2 = n * n;
   double *sC = sim_lds;
   unsigned char *sS = (unsigned char *)(sim_lds + (a.lds_cdf ? K * n2 : 0));
   const long s = (long)blockIdx.x * SIM_TILE + tid;
   const bool on = s < a.n_sites;      // (lanes past the end keep to the barriers and touch no memory)
   const unsigned long long base = a.stream + RELL_GAMMA * ((unsigned long long)(a.site0 + s) * (unsigned long long)(nn + 2));
   const long n_rows = (long)K * nn * n;
   int cl = 0;
   if (on) {
      cl = sim_search<false>(a.cdf + n_rows * n + n, K, sim_u(base, 0), a.last + n_rows + 1);
      if (a.cls) a.cls[s] = (unsigned char)cl;
      const int st = sim_search<SMALL>(a.cdf + n_rows * n, n, sim_u(base, 1), a.last + n_rows);
      a.state[(long)a.root * a.stride + s] = (unsigned char)st;
      if (a.lds_state) sS[a.root * SIM_TILE + tid] = (unsigned char)st;
   }
   for (int i = 0; i < nn - 1; i++) {
      const int2 np = a.order[i];
      const int node = np.x, parent = np.y;
      if (a.lds_cdf) {      // this node's tables of all classes
         __syncthreads();      // (the previous node's are no longer read)
         for (int c = 0; c < K; c++) {
            const double *src = a.cdf + ((long)c * nn + node) * n2;
            for (int idx = tid; idx < n2; idx += SIM_TILE) sC[c * n2 + idx] = src[idx];
         }
         __syncthreads();
      }
      if (on) {
         const int ps = a.lds_state ? sS[parent * SIM_TILE + tid] : a.state[(long)parent * a.stride + s];
         const long row = ((long)cl * nn + node) * n + ps;
         const double *c = a.lds_cdf ? sC + (cl * n + ps) * n : a.cdf + row * n;
         const int st = sim_search<SMALL>(c, n, sim_u(base, 2 + node), a.last + row);
         a.state[(long)node * a.stride + s] = (unsigned char)st;
         if (a.lds_state) sS[node * SIM_TILE + tid] = (unsigned char)st;
      }
   }
}

}  // namespace paml_amd

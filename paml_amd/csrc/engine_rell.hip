// engine_rell.hip — bootstrap replicates of the tree comparison (rell() treesub.c:5844-6009) on the device; kernels, the generator
// and the summation order in kernels_rell.h.  Stand-alone: no engine.  Built for gfx950 only.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/paml_amd.h"
#include "dev_buf.h"
#include "kernels_rell.h"

using namespace paml_amd;

// the calling thread's last failure of a stand-alone entry: what paml_amd_last_error(NULL) returns (engine_core.hip)
static std::string &standalone_error() { static thread_local std::string s; return s; }
extern "C" const char *paml_amd_standalone_error(void) { return standalone_error().c_str(); }

static thread_local int rell_last_batches = 0;
static thread_local double rell_last_kernel_ms = 0;      // HIP events around the replicate kernels of every batch, summed

static int rell_fail(int code, const char *fmt, long a = 0, double b = 0)
{
   char buf[256];
   snprintf(buf, sizeof(buf), fmt, a, b);
   standalone_error() = buf;
   return code;
}

extern "C" void paml_amd_rell_info(int *chunk, int *tree_block, int *last_batches, double *last_kernel_ms)
{
   if (last_kernel_ms) *last_kernel_ms = rell_last_kernel_ms;
   if (chunk) *chunk = RELL_CHUNK;
   if (tree_block) *tree_block = RELL_TREE_BLOCK;
   if (last_batches) *last_batches = rell_last_batches;
}

extern "C" int paml_amd_rell_replicates(int n_trees, int n_patt, const double *w, const double *lnf, int n_genes, const int *gene_off, int n_rep,
                                        unsigned long long seed, double *rep)
{
   standalone_error().clear();
   rell_last_batches = 0;
   rell_last_kernel_ms = 0;
   if (n_trees < 1) return rell_fail(PAML_AMD_EINVAL, "rell_replicates: n_trees = %ld < 1", n_trees);
   if (n_patt < 1) return rell_fail(PAML_AMD_EINVAL, "rell_replicates: n_patt = %ld < 1", n_patt);
   if (n_rep < 1) return rell_fail(PAML_AMD_EINVAL, "rell_replicates: n_rep = %ld < 1", n_rep);
   if (!w || !lnf || !rep) return rell_fail(PAML_AMD_EINVAL, "rell_replicates: null argument");
   if (!gene_off) n_genes = 1;
   else {
      if (n_genes < 1) return rell_fail(PAML_AMD_EINVAL, "rell_replicates: n_genes = %ld < 1", n_genes);
      if (gene_off[0] != 0 || gene_off[n_genes] != n_patt) return rell_fail(PAML_AMD_EINVAL, "rell_replicates: gene_off does not run from 0 to n_patt = %ld", n_patt);
      for (int g = 0; g < n_genes; g++)
         if (gene_off[g + 1] < gene_off[g]) return rell_fail(PAML_AMD_EINVAL, "rell_replicates: gene_off decreases at gene %ld", g);
   }
   std::vector<int> wi((size_t)n_patt), soff((size_t)n_genes + 1);
   long ls = 0;
   for (int h = 0, g = 0; h <= n_patt; h++) {
      while (g <= n_genes && (gene_off ? gene_off[g] : g * n_patt) == h) soff[g++] = (int)ls;      // ls < 2^31 here: checked below as it grows
      if (h == n_patt) break;
      const double x = w[h];
      if (!(x >= 0)) return rell_fail(PAML_AMD_EINVAL, "rell_replicates: weight of pattern %ld is negative (%g)", h, x);
      if (x != std::floor(x)) return rell_fail(PAML_AMD_EINVAL, "rell_replicates: weight of pattern %ld is not an integer (%g)", h, x);
      if (x >= 2147483648.0) return rell_fail(PAML_AMD_EINVAL, "rell_replicates: weight of pattern %ld is 2^31 or more (%g)", h, x);
      wi[h] = (int)x;
      ls += wi[h];
      if (ls >= 2147483648L) return rell_fail(PAML_AMD_EINVAL, "rell_replicates: more than 2^31 - 1 sites at pattern %ld", h);
   }
   if (ls == 0) return rell_fail(PAML_AMD_EINVAL, "rell_replicates: no sites (ls = 0: every weight is zero)");
   int ndev = 0;
   if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return rell_fail(PAML_AMD_EHIP, "rell_replicates: no HIP device visible");

   int t_pad = 2;
   while (t_pad < n_trees) t_pad <<= 1;
   const int tb = t_pad < RELL_TREE_BLOCK ? t_pad : RELL_TREE_BLOCK, n_tb = t_pad / tb;
   const int n_chunks = (int)((ls + RELL_CHUNK - 1) / RELL_CHUNK), n_tiles = (n_patt + RELL_SCAN_TILE - 1) / RELL_SCAN_TILE;
   // replicates per batch: what the workspace of chunk sums holds (default 256 MiB; PAML_AMD_RELL_ARENA_MB gives another size), at
   // most 2^30 (replicate, chunk) items per launch, at least one replicate
   double arena_mb = 256;
   if (const char *s = getenv("PAML_AMD_RELL_ARENA_MB")) { const double v = atof(s); if (v > 0) arena_mb = v; }
   const double per_rep = (double)n_chunks * t_pad * sizeof(double);
   long batch = (long)(arena_mb * 1048576.0 / per_rep);
   if (batch > (1L << 30) / n_chunks) batch = (1L << 30) / n_chunks;
   if (batch > n_rep) batch = n_rep;
   if (batch < 1) batch = 1;

   DevBuf<double> d_lnf, d_tab, d_part, d_rep;
   DevBuf<int> d_w, d_end, d_sums, d_site, d_soff;
   DevEvent ev0, ev1;
#define RELLCHK(call) do { if ((call) != hipSuccess) return rell_fail(PAML_AMD_EHIP, "rell_replicates: HIP error at line %ld", __LINE__); } while (0)
#define RELLMEM(call, what) do { if ((call) != hipSuccess) { (void)hipGetLastError(); return rell_fail(PAML_AMD_ENOMEM, "rell_replicates: no device memory for " what); } } while (0)
   RELLMEM(d_tab.ensure((size_t)n_patt * t_pad), "the lnf table");
   RELLMEM(d_site.ensure((size_t)ls), "the site list");
   RELLMEM(d_w.ensure((size_t)n_patt), "the weights");
   RELLMEM(d_end.ensure((size_t)n_patt), "the weights");
   RELLMEM(d_sums.ensure((size_t)n_tiles), "the weights");
   RELLMEM(d_soff.ensure((size_t)n_genes + 1), "the gene offsets");
   RELLMEM(d_lnf.ensure((size_t)n_patt * n_trees), "lnf");
   RELLCHK(hipMemcpy(d_lnf.p, lnf, (size_t)n_patt * n_trees * sizeof(double), hipMemcpyHostToDevice));
   RELLCHK(hipMemcpy(d_w.p, wi.data(), (size_t)n_patt * sizeof(int), hipMemcpyHostToDevice));
   RELLCHK(hipMemcpy(d_soff.p, soff.data(), ((size_t)n_genes + 1) * sizeof(int), hipMemcpyHostToDevice));
   hipLaunchKernelGGL(rell_transpose, dim3((n_patt + RELL_THREADS - 1) / RELL_THREADS), dim3(RELL_THREADS), 0, 0, d_lnf.p, n_trees, n_patt, t_pad, d_tab.p);
   hipLaunchKernelGGL(rell_tile_sums, dim3(n_tiles), dim3(RELL_THREADS), 0, 0, d_w.p, n_patt, d_sums.p);
   hipLaunchKernelGGL(rell_scan_tiles, dim3(1), dim3(1024), 0, 0, d_sums.p, n_tiles);
   hipLaunchKernelGGL(rell_tile_scan, dim3(n_tiles), dim3(RELL_THREADS), 0, 0, d_w.p, d_sums.p, n_patt, d_end.p);
   hipLaunchKernelGGL(rell_fill_sites, dim3((unsigned)((ls + RELL_THREADS - 1) / RELL_THREADS)), dim3(RELL_THREADS), 0, 0, d_end.p, n_patt, (int)ls, d_site.p);
   RELLCHK(hipGetLastError());
   RELLCHK(hipDeviceSynchronize());
   d_lnf.release();
   // the workspace: halve the batch until it fits
   for (;;) {
      if (d_part.ensure((size_t)batch * n_chunks * t_pad) == hipSuccess && d_rep.ensure((size_t)batch * n_trees) == hipSuccess) break;
      (void)hipGetLastError();
      d_part.release();
      if (batch == 1) return rell_fail(PAML_AMD_ENOMEM, "rell_replicates: no device memory for the chunk sums of one replicate");
      batch = (batch + 1) / 2;
   }
   RELLCHK(ev0.ensure()); RELLCHK(ev1.ensure());
   for (long r0 = 0; r0 < n_rep; r0 += batch) {
      const long nb = n_rep - r0 < batch ? n_rep - r0 : batch;
      RellArgs a{};
      a.tab = d_tab.p; a.site = d_site.p; a.soff = d_soff.p; a.part = d_part.p; a.seed = seed;
      a.ls = (int)ls; a.n_genes = n_genes; a.n_chunks = n_chunks; a.t_pad = t_pad; a.rep0 = (int)r0; a.n_items = nb * n_chunks;
      RELLCHK(hipEventRecord(ev0, 0));
      const dim3 grid((unsigned)((a.n_items + RELL_THREADS / 64 - 1) / (RELL_THREADS / 64)), (unsigned)n_tb);
      if (tb == 2) hipLaunchKernelGGL(rell_chunk_sums<2>, grid, dim3(RELL_THREADS), 0, 0, a);
      else if (tb == 4) hipLaunchKernelGGL(rell_chunk_sums<4>, grid, dim3(RELL_THREADS), 0, 0, a);
      else hipLaunchKernelGGL(rell_chunk_sums<8>, grid, dim3(RELL_THREADS), 0, 0, a);
      hipLaunchKernelGGL(rell_sum_chunks, dim3((unsigned)((nb * n_trees + RELL_THREADS - 1) / RELL_THREADS)), dim3(RELL_THREADS), 0, 0, d_part.p, (int)nb, n_chunks,
                         t_pad, n_trees, d_rep.p);
      RELLCHK(hipGetLastError());
      RELLCHK(hipEventRecord(ev1, 0));
      RELLCHK(hipMemcpy(rep + (size_t)r0 * n_trees, d_rep.p, (size_t)nb * n_trees * sizeof(double), hipMemcpyDeviceToHost));
      { float ms = 0; RELLCHK(hipEventElapsedTime(&ms, ev0, ev1)); rell_last_kernel_ms += ms; }
      rell_last_batches++;
   }
#undef RELLCHK
#undef RELLMEM
   return 0;
}

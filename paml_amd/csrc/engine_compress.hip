// engine_compress.hip — site-pattern compression (PatternWeight treesub.c:1386) on the device; kernels in compress.h.
// Stand-alone: no engine.  Built for gfx950 only.
#include <hip/hip_runtime.h>

#include "../../include/paml_amd.h"
#include "dev_buf.h"
#include "compress.h"

using namespace paml_amd;

extern "C" int paml_amd_compress_patterns(int n_seq, int n_sites, int width, const unsigned char *chars, const int *gene, int *n_patt,
                                          int *first_site, double *weights, int *pose)
{
   if (n_seq < 1 || n_sites < 1 || width < 1 || !chars || !n_patt || !first_site || !weights || !pose) return PAML_AMD_EINVAL;
   int ndev = 0;
   if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return PAML_AMD_EHIP;
   const int n = n_sites, n_tiles = (n + CMP_TILE - 1) / CMP_TILE, nb = (n + CMP_THREADS - 1) / CMP_THREADS;
   const size_t row = (size_t)n * width;
   DevBuf<unsigned char> d_chars, d_dig;
   DevBuf<int> d_gene, d_idx[2], d_hist, d_head, d_sums, d_pose, d_first, d_start, d_total, d_rowsum;
   DevBuf<double> d_w;
   int total = 0, cur = 0;
#define CMPCHK(call) do { if ((call) != hipSuccess) return PAML_AMD_EHIP; } while (0)
   CMPCHK(d_chars.ensure(row * n_seq)); CMPCHK(d_dig.ensure((size_t)n));
   CMPCHK(d_idx[0].ensure((size_t)n)); CMPCHK(d_idx[1].ensure((size_t)n));
   CMPCHK(d_hist.ensure((size_t)256 * n_tiles));
   CMPCHK(d_head.ensure((size_t)n)); CMPCHK(d_sums.ensure((size_t)n_tiles));
   CMPCHK(d_pose.ensure((size_t)n)); CMPCHK(d_first.ensure((size_t)n)); CMPCHK(d_start.ensure((size_t)n));
   CMPCHK(d_total.ensure(1)); CMPCHK(d_w.ensure((size_t)n)); CMPCHK(d_rowsum.ensure(256));
   CMPCHK(hipMemcpy(d_chars.p, chars, row * n_seq, hipMemcpyHostToDevice));
   if (gene) { CMPCHK(d_gene.ensure((size_t)n)); CMPCHK(hipMemcpy(d_gene.p, gene, (size_t)n * 4, hipMemcpyHostToDevice)); }
   {
      CompressArgs a{};
      a.n_sites = n; a.n_seq = n_seq; a.width = width; a.n_tiles = n_tiles; a.row_stride = (long)row; a.chars = d_chars.p; a.gene = d_gene.p; a.hist = d_hist.p; a.dig = d_dig.p;
      hipLaunchKernelGGL(cmp_iota, dim3(nb), dim3(CMP_THREADS), 0, 0, d_idx[0].p, n);
      // least significant key byte first: the last character of the last sequence ... the first of the first, then the gene
      for (int kb = n_seq * width - 1; kb >= (gene ? -1 : 0); kb--) {
         a.seq = kb < 0 ? -1 : kb / width; a.pos = kb < 0 ? 0 : kb % width;
         a.idx_in = d_idx[cur].p; a.idx_out = d_idx[cur ^ 1].p;
         hipLaunchKernelGGL(cmp_hist, dim3(n_tiles), dim3(CMP_THREADS), 0, 0, a);
         hipLaunchKernelGGL(cmp_row_sums, dim3(256), dim3(CMP_THREADS), 0, 0, d_hist.p, n_tiles, d_rowsum.p);
         hipLaunchKernelGGL(cmp_row_scan, dim3(256), dim3(CMP_THREADS), 0, 0, d_hist.p, n_tiles, d_rowsum.p);
         hipLaunchKernelGGL(cmp_scatter, dim3(n_tiles), dim3(CMP_THREADS), 0, 0, a);
         cur ^= 1;
      }
      a.idx_in = d_idx[cur].p;
      hipLaunchKernelGGL(cmp_heads, dim3(nb), dim3(CMP_THREADS), 0, 0, a, d_head.p);
      hipLaunchKernelGGL(cmp_tile_sums, dim3(n_tiles), dim3(CMP_THREADS), 0, 0, d_head.p, n, d_sums.p);
      hipLaunchKernelGGL(cmp_scan1, dim3(1), dim3(1024), 0, 0, d_sums.p, (long)n_tiles, d_total.p);
      hipLaunchKernelGGL(cmp_number, dim3(n_tiles), dim3(CMP_THREADS), 0, 0, d_head.p, d_sums.p, d_idx[cur].p, n, d_pose.p, d_first.p, d_start.p);
      CMPCHK(hipGetLastError());
      CMPCHK(hipMemcpy(&total, d_total.p, 4, hipMemcpyDeviceToHost));
      hipLaunchKernelGGL(cmp_weights, dim3((total + CMP_THREADS - 1) / CMP_THREADS), dim3(CMP_THREADS), 0, 0, d_start.p, total, n, d_w.p);
      CMPCHK(hipGetLastError());
   }
   CMPCHK(hipMemcpy(pose, d_pose.p, (size_t)n * 4, hipMemcpyDeviceToHost));
   CMPCHK(hipMemcpy(first_site, d_first.p, (size_t)total * 4, hipMemcpyDeviceToHost));
   CMPCHK(hipMemcpy(weights, d_w.p, (size_t)total * 8, hipMemcpyDeviceToHost));
   *n_patt = total;
#undef CMPCHK
   return 0;
}

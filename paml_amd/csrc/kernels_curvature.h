// The second derivative of lnL along every branch length, with lnL and the gradient, in one call (paml_amd_curvature): what a Newton step
// on every branch at once needs, where a branch-at-a-time sweep (minbranches, treesub.c:8039) walks the tree with 2 (n - 1) dependent calls.
//
// The definition extends the one at the top of kernels_gradient.h: the same down pass, the same outer pass with H_v and L_v at every
// non-root v, and per gene, class k and pattern h one more sum beside f_vk and d_vk,
//   second derivative    e_vk   = sum_y H_v(y) (d2P_v L_v)(y)
//   d2P_v = d^2 P_v / d branch[v]^2 = sum_{k >= 1} U[:, k] mu_k^2 e^{t mu_k} V[k, :]   (the Cijk form likewise; K80 and JC69-like by their two
//                                                                                      and one non-zero rates, as pmat_deriv_kernel writes ddP)
// f, d and e of a node carry the same log factor sigma_vk, so the classes meet exactly as in grad_combine, rho_k = freqK_k e^{sigma_vk - max_k sigma_vk}:
//   curvature            c_v(h) = sum_k rho_k e_vk / sum_k rho_k f_vk - s_v(h)^2        (d^2 log f / dt^2 = f'' / f - (f' / f)^2)
//   results              curv[v] = sum_h w_h c_v(h);   lnL, grad, lnf as paml_amd_gradient — the same statements, the same bytes
// curv[root] = 0; a pattern with w_h = 0 contributes nothing.  curv[v] is the second derivative along branch[v] of exactly the number
// paml_amd_eval returns: nothing is re-rooted, no reversibility is assumed.  It is the diagonal of the Hessian over the branch lengths; the
// cross derivatives are not formed.
//
// Kernels: the bodies are kernels_gradient.h's at CURV = true.  curv_pmat_kernel writes dP, d2P and P^T in one launch (row-major for the
// lanes, A-operand order for the matrix cores); the outer pass does the gradient's work plus one product and one dot product per non-root
// node (matrix cores: through the same stage_p / mfma_matvec / AncMfma::product, the product's result taking the place of the dP product's
// in y / acc once its dot product is taken; a tip feeds its code's indicator through the d2P product); the combination takes 2 n_nodes + 1
// rows — w s, w c, w lnf — in the same 64-pattern chunks and butterfly, and grad_total_kernel adds every row's chunks in its fixed order.
// The workspace holds one more [K][n_nodes][stride] array (e_vk) and no scores.  Ordinary vector stores only; no atomics.
//
// The per-lane bodies compile with no HIP at all (CURV_HOST_ONLY, as GRAD_HOST_ONLY): tools/curvature_host_check.cpp runs them in a loop
// under the host sanitizers.
#pragma once
#ifdef CURV_HOST_ONLY
#ifndef GRAD_HOST_ONLY
#define GRAD_HOST_ONLY
#endif
#endif
#include "kernels_gradient.h"

namespace paml_amd {

// bytes of the batch workspace per pattern: the down partials and the outer messages with their log factors (n_s = 64 on the matrix
// cores), four sums per (class, node) — f, d, e and their log factor — and lnf
inline double curv_bytes_per_pattern(int K, int n_int, int n_nodes, int n_s) { return 2.0 * K * n_int * (n_s + 1) * 8 + 4.0 * K * n_nodes * 8 + 8.0; }

#ifndef GRAD_HOST_ONLY
// ---- kernels: defined in engine_curvature.hip ----------------------------------------------------------------------------------------
__global__ void curv_pmat_kernel(GradPmatArgs a);
__global__ void curv_mfma_kernel(GradArgs a);
__global__ void curv_combine_kernel(GradArgs a);

// one pattern per lane: grid (patterns / 256, K); pass 0: the down pass, 1: the outer pass with both derivatives (the Hessian call launches it too)
template <int N> __global__ __launch_bounds__(256) void curv_lane_kernel(GradArgs a, int pass)
{
   const long p = (long)blockIdx.x * 256 + threadIdx.x;
   if (p >= a.m.nb) return;
   if (pass) grad_lane_outer<N, true>(a, blockIdx.y, p);
   else anc_lane_down<N>(a.m, blockIdx.y, p);
}
#endif

}  // namespace paml_amd

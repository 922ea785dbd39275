// engine_modelgrad.hip — the derivative of lnL with respect to every input of the engine in one call (paml_amd_model_gradient): the
// definition in kernels_modelgrad.h, the kernels here.  P(t) comes from the evaluation's own builders (anc_pmat, engine_ancestral.hip),
// the down pass is the ancestral module's, the outer pass is the gradient's with H_v stored instead of the derivative taken.
// Built for gfx950 only (one of the translation units of libpaml_amd.so, see engine_state.h).
#include "engine_state.h"
#include "kernels_modelgrad.h"
#include "ancestral_host.h"

static thread_local AncCallInfo mg_info;

extern "C" void paml_amd_model_gradient_info(int *last_batches, double *last_kernel_ms) { mg_info.read(last_batches, last_kernel_ms); }
extern "C" int paml_amd_model_gradient_segment(void) { return MODELGRAD_SEG; }
extern "C" int paml_amd_model_gradient_sizes(paml_amd_engine *e, int *n_pi, int *n_eigen)
{
   if (!e) return PAML_AMD_EINVAL;
   if (n_pi) *n_pi = e->n_pi;
   if (n_eigen) *n_eigen = (int)e->eigen.size();
   return 0;
}

namespace paml_amd {

// one pattern per lane: grid (patterns / 256, K); pass 0: the down pass, 1: the outer pass
template <int N> __global__ __launch_bounds__(256) void mg_lane_kernel(ModelGradArgs a, int pass)
{
   const long p = (long)blockIdx.x * 256 + threadIdx.x;
   if (p >= a.m.nb) return;
   if (pass) mg_lane_outer<N>(a, blockIdx.y, p);
   else anc_lane_down<N>(a.m, blockIdx.y, p);
}

// Matrix cores, the outer pass: grad_mfma_kernel's walk (a workgroup of four waves owns ANC_TILE patterns of one class; lane =
// q * 16 + pattern, register m = state 4 m + q) with H_v stored in the resident-partial layout.  Grid (stride / ANC_TILE, K).
__global__ __launch_bounds__(256) void mg_mfma_outer_kernel(ModelGradArgs a)
{
   __shared__ __attribute__((aligned(16))) double sP[4096];
   const AncMargArgs &m = a.m;
   const AncTree &t = m.t;
   const int tid = threadIdx.x, lane = tid & 63, n = m.n;
   const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
   const int q = lane >> 4, k = blockIdx.y;
   const AncMfma w{sP, lane, wave, q};
   const long g16 = (long)blockIdx.x * 4 + wave, p = g16 * 16 + (lane & 15);
   const long pc = p < m.nb ? p : m.nb - 1;      // (lanes past the batch's end read the last pattern and write into the padding: p < stride)
   const long pset = (long)m.gene * m.K + k;
   const long groups = m.stride >> 4;
   const double *pi = m.pi + (long)(m.n_pi > 1 ? m.gene : 0) * n;
   if (t.root >= t.n_tips) {
      const int ri = t.root - t.n_tips;
      double x[16];
#pragma unroll
      for (int i = 0; i < 16; i++) x[i] = 4 * i + q < n ? pi[4 * i + q] : 0.0;
      part_store(m.G + (((long)k * t.n_int + ri) * groups + g16) * 1024, lane, x);
      if (q == 0) m.SG[((long)k * t.n_int + ri) * m.stride + p] = 0;
   }
   else {      // the root is a tip: its partial, for g_pi
      const unsigned long long mask = m.code_mask[m.z[(long)t.root * m.z_stride + m.h0 + pc]];
      double x[16], ls = 0;
#pragma unroll
      for (int j = 0; j < 16; j++) x[j] = (mask >> (4 * j + q)) & 1ull ? 1.0 : 0.0;
      for (int j = t.sons_ptr[t.root]; j < t.sons_ptr[t.root + 1]; j++) anc_mfma_mul_son(m, w, k, g16, pc, t.sons[j], x, &ls);
      part_store(a.R + ((long)k * groups + g16) * 1024, lane, x);
      if (q == 0) a.SR[(long)k * m.stride + p] = ls;
   }
   const int n_walk = t.n_pre + t.n_tips;
   for (int i = 0; i < n_walk; i++) {
      const int v = i < t.n_pre ? t.pre[i] : i - t.n_pre;      // the internal nodes father first, then the tips
      if (v == t.root) continue;
      const int f = t.father[v];
      double h[16], ls = 0;
      __syncthreads();      // (SG of the father was stored by the pattern's q = 0 lane: a workgroup-scope fence before the other lanes read it)
      if (f >= t.n_tips) {
         const int fi = f - t.n_tips;
         part_load(m.G + (((long)k * t.n_int + fi) * groups + g16) * 1024, lane, h);      // (this lane's own stores)
         ls = m.SG[((long)k * t.n_int + fi) * m.stride + pc];
      }
      else {
         const unsigned long long mask = m.code_mask[m.z[(long)f * m.z_stride + m.h0 + pc]];
#pragma unroll
         for (int j = 0; j < 16; j++) h[j] = (4 * j + q < n && ((mask >> (4 * j + q)) & 1ull)) ? pi[4 * j + q] : 0.0;
      }
      for (int j = t.sons_ptr[f]; j < t.sons_ptr[f + 1]; j++)
         if (t.sons[j] != v) anc_mfma_mul_son(m, w, k, g16, pc, t.sons[j], h, &ls);
      part_store(a.H + (((long)k * t.n_nodes + v) * groups + g16) * 1024, lane, h);
      const long slot = pset * t.n_nodes + v;
      const long oi = mg_out_idx(a, k, v, p);
      double x[16], y[16];
      if (v < t.n_tips) {
         const int code = (int)m.z[(long)v * m.z_stride + m.h0 + pc];
         double2 tv[8];
         tip_gather(m.ptip + pset * t.n_nodes * m.tip_words, m.tip_words, v, code, q, tv);
#pragma unroll
         for (int j = 0; j < 8; j++) { y[2 * j] = tv[j].x; y[2 * j + 1] = tv[j].y; }
         const double den = grad_mfma_dot(h, y);
         if (q == 0) { a.den[oi] = den; a.sig[oi] = ls; }
         continue;
      }
      const int vi = v - t.n_tips;
      part_load(m.L + (((long)k * t.n_int + vi) * groups + g16) * 1024, lane, x);
      v4d acc[4];
      w.product(a.PT + slot * 4096, h, acc);      // A_v = P_v^T H_v
#pragma unroll
      for (int j = 0; j < 16; j++) y[j] = acc[j >> 2][j & 3];
      const double den = grad_mfma_dot(y, x);
      if (q == 0) { a.den[oi] = den; a.sig[oi] = ls + m.SL[((long)k * t.n_int + vi) * m.stride + pc]; }
      if (m.scaled) {
         const double mx = anc_mfma_max(y);
         if (mx > 0) {
#pragma unroll
            for (int j = 0; j < 16; j++) y[j] /= mx;
            ls += log(mx);
         }
      }
      part_store(m.G + (((long)k * t.n_int + vi) * groups + g16) * 1024, lane, y);
      if (q == 0) m.SG[((long)k * t.n_int + vi) * m.stride + p] = ls;
   }
}

// the coefficients of every (node, pattern) and the pattern's scalar rows: grid (stride / 256, n_nodes + 1)
__global__ __launch_bounds__(256) void mg_coef_kernel(ModelGradArgs a)
{
   const long p = (long)blockIdx.x * 256 + threadIdx.x;
   if (p < a.m.nb) mg_coef(a, blockIdx.y, p);
}

// the chunks' sums of the scalar rows: grid (stride / 256, 1 + K + n); a wave = one chunk of GRAD_CHUNK patterns
__global__ __launch_bounds__(256) void mg_rows_kernel(ModelGradArgs a)
{
   const long p = (long)blockIdx.x * 256 + threadIdx.x;
   const int r = blockIdx.y;
   double acc = p < a.m.nb ? mg_row_term(a, r, p) : 0.0;
#pragma unroll
   for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off);
   const long chunk = a.chunk0 + (p >> 6);
   if ((threadIdx.x & 63) == 0 && (p & ~63L) < a.m.nb) a.partial[(long)r * a.n_chunks + chunk] = acc;
}

// chunks [lo, lo + cnt) of row first_row + blockIdx.x added in a fixed order: grid (rows)
__global__ __launch_bounds__(256) void mg_total_kernel(const double *partial, long n_chunks, int first_row, long lo, long cnt, double *out)
{
   __shared__ double sw4[4];
   const double s = red_total256(partial + (long)(first_row + blockIdx.x) * n_chunks + lo, (int)cnt, false, sw4);
   if (threadIdx.x == 0) out[blockIdx.x] = s;
}

// W of one (segment of the batch, class, node), one pattern per lane: a wave walks the segment's patterns sixty-four at a time, every
// entry's terms added over the wave in the fixed butterfly; lane l keeps the entries l, l + 64, ...  Grid (segments, K * n_nodes), one wave.
template <int N> __global__ __launch_bounds__(64) void mg_w_lane_kernel(ModelGradArgs a)
{
   const AncMargArgs &m = a.m;
   const int nn = m.t.n_nodes, k = blockIdx.y / nn, v = blockIdx.y % nn, si = blockIdx.x, lane = threadIdx.x;
   constexpr int NA = (N * N + 63) / 64;
   ModelGradSeg sg = mg_segment(a, si);
   if (v == m.t.root) { sg.hi = sg.lo; sg.continued = false; }      // (the root's slot: zeros, so that the running sum adds defined numbers)
   const long slot = (long)k * nn + v;
   double acc[NA];
#pragma unroll
   for (int j = 0; j < NA; j++) acc[j] = sg.continued && j * 64 + lane < N * N ? a.carry_in[slot * a.wn + j * 64 + lane] : 0.0;
   for (long p0 = sg.lo; p0 < sg.hi; p0 += 64) {
      const long p = p0 + lane;
      const double c = p < sg.hi ? a.coef[mg_out_idx(a, k, v, p)] : 0.0;
      double h[N], l[N];
#pragma unroll
      for (int x = 0; x < N; x++) {
         h[x] = c != 0 ? c * a.H[mg_h_idx(a, k, v, x, p)] : 0.0;
         l[x] = c != 0 ? mg_node_L(a, k, v, x, p) : 0.0;
      }
#pragma unroll
      for (int idx = 0; idx < N * N; idx++) {
         double s = h[idx / N] * l[idx % N];
#pragma unroll
         for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off);
         if (lane == (idx & 63)) acc[idx >> 6] += s;
      }
   }
   double *dst = sg.finished ? a.Wpart + ((long)si * m.K * nn + slot) * a.wn : a.carry_out + slot * a.wn;
#pragma unroll
   for (int j = 0; j < NA; j++)
      if (j * 64 + lane < N * N) dst[j * 64 + lane] = acc[j];
}

// element (state s, pattern pp) of a sixteen-pattern group in the resident-partial layout
__device__ __forceinline__ int mg_part_at(int s, int pp) { return ((((s >> 3) * 64) + (s & 3) * 16 + pp) << 1) | ((s >> 2) & 1); }

// W of one (segment of the batch, class, node) on the matrix cores: W += (coef x H_v) L_v^T with the patterns as the k dimension of
// v_mfma_f64_16x16x4, sixteen patterns (four steps) per stage.  Wave w owns rows 16 w .. 16 w + 15 of the 64 x 64 accumulator as four
// 16 x 16 tiles: element r of acc[xb] = W[16 w + 4 r + (lane >> 4)][16 xb + (lane & 15)].  Grid (segments, K * n_nodes), four waves.
__global__ __launch_bounds__(256) void mg_w_mfma_kernel(ModelGradArgs a)
{
   __shared__ double sH[1024], sL[1024];
   const AncMargArgs &m = a.m;
   const AncTree &t = m.t;
   const int nn = t.n_nodes, k = blockIdx.y / nn, v = blockIdx.y % nn, si = blockIdx.x;
   const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, q = lane >> 4, c = lane & 15;
   ModelGradSeg sg = mg_segment(a, si);
   if (v == t.root) { sg.hi = sg.lo; sg.continued = false; }      // (the root's slot: zeros, so that the running sum adds defined numbers)
   const long slot = (long)k * nn + v, groups = m.stride >> 4;
   const bool tip = v < t.n_tips;
   v4d acc[4];
#pragma unroll
   for (int xb = 0; xb < 4; xb++)
#pragma unroll
      for (int r = 0; r < 4; r++) acc[xb][r] = sg.continued ? a.carry_in[slot * 4096 + (16 * wave + 4 * r + q) * 64 + 16 * xb + c] : 0.0;
   const double *Hv = a.H + slot * groups * 1024;
   const double *Lv = tip ? nullptr : m.L + ((long)k * t.n_int + (v - t.n_tips)) * groups * 1024;
   for (long p0 = sg.lo; p0 < sg.hi; p0 += 16) {
      __syncthreads();      // (every wave is done reading the last group)
#pragma unroll
      for (int j = 0; j < 4; j++) {
         const int e = tid + 256 * j, ln = (e >> 1) & 63;
         const long p = p0 + (ln & 15);
         const double cf = p < sg.hi ? a.coef[mg_out_idx(a, k, v, p)] : 0.0;
         sH[e] = cf != 0 ? cf * Hv[(p0 >> 4) * 1024 + e] : 0.0;
         if (tip) {
            const int s = 4 * (((e >> 7) << 1) | (e & 1)) + (ln >> 4);
            const long pz = p < m.nb ? p : m.nb - 1;
            sL[e] = (m.code_mask[m.z[(long)v * m.z_stride + m.h0 + pz]] >> s) & 1ull ? 1.0 : 0.0;
         }
         else sL[e] = Lv[(p0 >> 4) * 1024 + e];
      }
      __syncthreads();
#pragma unroll
      for (int kk = 0; kk < 4; kk++) {
         const int pp = 4 * kk + q;
         const double av = sH[mg_part_at(16 * wave + c, pp)];
#pragma unroll
         for (int xb = 0; xb < 4; xb++) acc[xb] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, sL[mg_part_at(16 * xb + c, pp)], acc[xb], 0, 0, 0);
      }
   }
   double *dst = sg.finished ? a.Wpart + ((long)si * m.K * nn + slot) * 4096 : a.carry_out + slot * 4096;
#pragma unroll
   for (int xb = 0; xb < 4; xb++)
#pragma unroll
      for (int r = 0; r < 4; r++) dst[(16 * wave + 4 * r + q) * 64 + 16 * xb + c] = acc[xb][r];
}

// the batch's finished segments added to the gene's running sum in segment order: one thread per entry of [K][n_nodes][wn]
__global__ __launch_bounds__(256) void mg_add_kernel(double *W, const double *Wpart, long per_seg, int n_finished)
{
   const long i = (long)blockIdx.x * 256 + threadIdx.x;
   if (i >= per_seg) return;
   double s = W[i];
   for (int si = 0; si < n_finished; si++) s += Wpart[(long)si * per_seg + i];
   W[i] = s;
}

__device__ __forceinline__ double mg_block_sum(double s, double *sw4)
{
#pragma unroll
   for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off);
   __syncthreads();
   if ((threadIdx.x & 63) == 0) sw4[threadIdx.x >> 6] = s;
   __syncthreads();
   return (sw4[0] + sw4[1]) + (sw4[2] + sw4[3]);
}

// The pull-back of one (gene, class, node): W -> the slot's term of its set's g_A, and g_eff.  Grid (n_nodes, gene x class); a thread
// owns the entries tid, tid + 256, ... of every n x n intermediate (sixteen at most), which pass through one LDS buffer.
__global__ __launch_bounds__(256) void mg_pull_kernel(ModelGradPullArgs a)
{
   __shared__ double sA[4096], sLam[64], sExp[64], sw4[4];
   const int node = blockIdx.x, pset = blockIdx.y, n = a.n, tid = threadIdx.x, n2 = n * n;
   if (node == a.root) return;
   const int gene = pset / a.K, iclass = pset % a.K, lab = a.label[node];
   const EigenDev es = a.eigen[a.eigen_of[(gene * a.K + iclass) * a.n_labels + lab]];
   const bool uv = es.kind == PAML_AMD_EIGEN_UVROOT;
   const double qf = uv ? a.qfactor[iclass * a.n_labels + lab] : 1.0;
   const double tau = a.branch[node] * (a.gene_rate[gene] * a.rate[gene * a.rate_gs + iclass] * qf);
   const int R = uv ? n : (es.kind == PAML_AMD_EIGEN_CIJK ? es.nR : (es.kind == PAML_AMD_EIGEN_K80 ? 3 : 2));
   const long slot = (long)pset * a.n_nodes + node;
   const double *W = a.W + slot * a.wn;
   const int ld = a.ld;
   double *GA = a.GA + slot * n2;
   if (tid < R) {
      const double lam = mg_lambda(es, n, tid);
      sLam[tid] = lam;
      sExp[tid] = exp(lam * tau);
   }
   double reg[16];
   if (uv) {
      // T1[i][x] = sum_y U[y][i] W[y][x]
#pragma unroll
      for (int j = 0; j < 16; j++) {
         const int idx = tid + 256 * j, i = idx / n, x = idx % n;
         double s = 0;
         if (idx < n2)
            for (int y = 0; y < n; y++) s += es.U[y * n + i] * W[y * ld + x];
         reg[j] = s;
      }
#pragma unroll
      for (int j = 0; j < 16; j++)
         if (tid + 256 * j < n2) sA[tid + 256 * j] = reg[j];
      __syncthreads();
      // M[i][j] = sum_x T1[i][x] V[j][x];  Z = Psi o M;  g_eff = sum_i lambda_i e^{lambda_i tau} M_ii
      double ge = 0;
#pragma unroll
      for (int j = 0; j < 16; j++) {
         const int idx = tid + 256 * j, i = idx / n, c = idx % n;
         double s = 0;
         if (idx < n2) {
            for (int x = 0; x < n; x++) s += sA[i * n + x] * es.V[c * n + x];
            if (i == c) ge += sLam[i] * sExp[i] * s;
            s *= mg_psi(sLam[i], sLam[c], tau);
         }
         reg[j] = s;
      }
      ge = mg_block_sum(ge, sw4);      // (its barriers: every thread is done reading T1)
      if (tid == 0) a.g_eff[slot] = ge;
#pragma unroll
      for (int j = 0; j < 16; j++)
         if (tid + 256 * j < n2) sA[tid + 256 * j] = reg[j];
      __syncthreads();
      // T2[a][j] = sum_i V[i][a] Z[i][j]
#pragma unroll
      for (int j = 0; j < 16; j++) {
         const int idx = tid + 256 * j, r = idx / n, c = idx % n;
         double s = 0;
         if (idx < n2)
            for (int i = 0; i < n; i++) s += es.V[i * n + r] * sA[i * n + c];
         reg[j] = s;
      }
      __syncthreads();
#pragma unroll
      for (int j = 0; j < 16; j++)
         if (tid + 256 * j < n2) sA[tid + 256 * j] = reg[j];
      __syncthreads();
      // g_A term [a][b] = sum_j T2[a][j] U[b][j]
#pragma unroll
      for (int j = 0; j < 16; j++) {
         const int idx = tid + 256 * j, r = idx / n, c = idx % n;
         if (idx < n2) {
            double s = 0;
            for (int i = 0; i < n; i++) s += sA[r * n + i] * es.U[c * n + i];
            GA[idx] = s;
         }
      }
      return;
   }
   // projector form: g_A term = sum_{r,s} Psi_rs Pi_r^T W Pi_s^T;  g_eff = sum_r lambda_r e^{lambda_r tau} <W, Pi_r>
   __syncthreads();
   double ge = 0;
   for (int r = 0; r < R; r++) {
      double s = 0;
      for (int idx = tid; idx < n2; idx += 256) s += W[(idx / n) * ld + idx % n] * mg_proj(es, n, r, idx / n, idx % n);
      ge += sLam[r] * sExp[r] * mg_block_sum(s, sw4);
   }
   if (tid == 0) a.g_eff[slot] = ge;
   double out[16];
#pragma unroll
   for (int j = 0; j < 16; j++) out[j] = 0;
   for (int s = 0; s < R; s++) {
      // T_s[y][b] = sum_x W[y][x] Pi_s[b][x]
#pragma unroll
      for (int j = 0; j < 16; j++) {
         const int idx = tid + 256 * j, y = idx / n, b = idx % n;
         double t = 0;
         if (idx < n2)
            for (int x = 0; x < n; x++) t += W[y * ld + x] * mg_proj(es, n, s, b, x);
         reg[j] = t;
      }
      __syncthreads();      // (every thread is done reading the last T)
#pragma unroll
      for (int j = 0; j < 16; j++)
         if (tid + 256 * j < n2) sA[tid + 256 * j] = reg[j];
      __syncthreads();
      for (int r = 0; r < R; r++) {
         const double psi = mg_psi(sLam[r], sLam[s], tau);
#pragma unroll
         for (int j = 0; j < 16; j++) {
            const int idx = tid + 256 * j, ra = idx / n, b = idx % n;
            double t = 0;
            if (idx < n2)
               for (int y = 0; y < n; y++) t += mg_proj(es, n, r, y, ra) * sA[y * n + b];
            out[j] += psi * t;
         }
      }
   }
#pragma unroll
   for (int j = 0; j < 16; j++)
      if (tid + 256 * j < n2) GA[tid + 256 * j] = out[j];
}

// g_A of every set: the terms of the (gene, class, node) that use it, added in that order.  Grid (n * n / 256, n_eigen)
__global__ __launch_bounds__(256) void mg_ga_sum_kernel(ModelGradPullArgs a, int n_genes)
{
   const int idx = blockIdx.x * 256 + threadIdx.x, set = blockIdx.y, n2 = a.n * a.n;
   if (idx >= n2) return;
   double s = 0;
   for (int pset = 0; pset < n_genes * a.K; pset++)
      for (int v = 0; v < a.n_nodes; v++)
         if (v != a.root && a.eigen_of[pset * a.n_labels + a.label[v]] == set) s += a.GA[((long)pset * a.n_nodes + v) * n2 + idx];
   a.g_A[(long)set * n2 + idx] = s;
}
}  // namespace paml_amd

namespace {

struct ModelGradScratch : AncScratch {
   using AncScratch::AncScratch;
   DevBuf<double> PT, H, den, sig, coef, R, SR, croot, rows, lnf, partial, out, carry, Wpart, W, GA, geff, gA;
};

}  // namespace

extern "C" int paml_amd_model_gradient(paml_amd_engine *e, const double *branch, const double *gene_rate, double *lnL, double *g_eff, double *g_freqK, double *g_pi,
                                       double *g_A, double *Wout)
{
   enter(e);
   mg_info = AncCallInfo{};
   const char *who = "model_gradient";
   if (!e || !branch || !lnL) return fail(e, PAML_AMD_EINVAL, "model_gradient: null argument");
   if (int rc = anc_begin(e, who, "a rate-matrix (UNREST) set has no spectral form to pull the derivative back through")) return rc;
   const TreeDesc &T = e->tree;
   const int nn = T.n_nodes, n = e->n, K = e->K, G = e->n_genes, n_int = nn - e->n_tips, n_eigen = (int)e->eigen.size();
   const bool mfma = e->kk == KK_MFMA64;
   hipStream_t st = e->stream;
   ModelGradScratch w(mg_info);
   ModelGradArgs a{};
   AncMargArgs &m = a.m;
   if (int rc = anc_tree_pack(e, who, w, &m.t)) return rc;
   if (int rc = anc_pmat(e, who, branch, gene_rate, w)) return rc;
   const size_t pn = (size_t)G * K * nn;
   if (mfma) {
      HIPCHK(w.PT.ensure(pn * 4096));
      hipLaunchKernelGGL(nni_pt_all_kernel, dim3(nn, (unsigned)(G * K)), dim3(256), 0, st, (const double *)e->d_rowmajor.p, w.PT.p, n, nn, T.root);
      HIPCHK(hipGetLastError());
   }
   if (int rc = anc_pmat_wait(e, w)) return rc;
   e->pmat_valid = true;      // (d_rowmajor holds every branch's P(t) in the tree's own orientation, as after paml_amd_gradient)

   const std::vector<long> chunk_base = anc_chunk_base(e);      // (also read below: the genes' ranges of chunks, for g_pi)
   const long n_chunks = chunk_base[G];
   const int n_rows = 1 + K + n, ns = mfma ? 64 : n, wn = mfma ? 4096 : n * n;
   const long per_seg = (long)K * nn * wn;
   HIPCHK(w.partial.ensure((size_t)n_rows * std::max<long>(n_chunks, 1)));
   HIPCHK(w.out.ensure((size_t)1 + K + (size_t)e->n_pi * n));
   HIPCHK(w.carry.ensure((size_t)2 * per_seg));
   HIPCHK(w.W.ensure(pn * wn));
   HIPCHK(w.GA.ensure(pn * n * n));
   HIPCHK(w.geff.ensure(pn));
   HIPCHK(w.gA.ensure((size_t)n_eigen * n * n));
   HIPCHK(hipMemsetAsync(w.W.p, 0, pn * wn * 8, st));
   HIPCHK(hipMemsetAsync(w.geff.p, 0, pn * 8, st));

   // per pattern: L, G (internal nodes) and H (every node) with their log factors, den / sig / coef, the root's rows, and the batch's
   // share of the segments' partial sums
   const double per_patt = 2.0 * K * n_int * (ns + 1) * 8 + (double)K * nn * ns * 8 + 3.0 * K * nn * 8 + (double)K * (ns + 2) * 8 + (2.0 + K) * 8
                           + (double)per_seg * 8 / MODELGRAD_SEG;
   long batch = anc_batch(per_patt, e->n_patt, "PAML_AMD_MODELGRAD_ARENA_MB");
   {
      const size_t part = (size_t)K * n_int * ns, sc = (size_t)K * n_int, cl = (size_t)K * nn;
      if (int rc = anc_alloc(e, who, {{&w.L, part}, {&w.G, part}, {&w.SL, sc}, {&w.SG, sc}, {&w.H, cl * ns}, {&w.den, cl}, {&w.sig, cl}, {&w.coef, cl},
                                      {&w.R, (size_t)K * ns}, {&w.SR, (size_t)K}, {&w.croot, (size_t)K}, {&w.rows, (size_t)1 + K}, {&w.lnf, 1}}, &batch))
         return rc;
   }
   const long max_segs = (batch + MODELGRAD_SEG - 1) / MODELGRAD_SEG + 1;      // (a batch that begins inside a segment touches one more)
   HIPCHK(w.Wpart.ensure((size_t)max_segs * per_seg));
   anc_fill(e, w, batch, m);
   a.PT = w.PT.p; a.H = w.H.p; a.den = w.den.p; a.sig = w.sig.p; a.coef = w.coef.p; a.R = w.R.p; a.SR = w.SR.p; a.croot = w.croot.p; a.rows = w.rows.p;
   a.lnf = w.lnf.p; a.weights = e->d_weights.p; a.partial = w.partial.p; a.n_chunks = n_chunks; a.ref_node = T.sons[T.sons_ptr[T.root]];
   a.ld = mfma ? 64 : n; a.wn = wn; a.Wpart = w.Wpart.p;
   // the batch's place in its gene, the carry's two halves and the segments it touches: set by whichever launch comes first of those whose
   // arguments hold them
   int flip = 0, n_segs = 0, n_finished = 0;
   auto place = [&](const AncBatch &b) {
      a.off0 = b.h0 - e->gene_off[b.gene]; a.gene_len = e->gene_off[b.gene + 1] - e->gene_off[b.gene];
      a.carry_in = w.carry.p + (size_t)flip * per_seg; a.carry_out = w.carry.p + (size_t)(flip ^ 1) * per_seg;
      flip ^= 1;
      n_segs = (int)((a.off0 + b.nb - 1) / MODELGRAD_SEG - a.off0 / MODELGRAD_SEG + 1);
      n_finished = mg_segment(a, n_segs - 1).finished ? n_segs : n_segs - 1;
   };
   if (int rc = anc_batches(
          e, w, m, &a.chunk0, batch,
          [&](const AncBatch &b) {
             place(b);
             hipLaunchKernelGGL(mg_mfma_outer_kernel, b.tiles, dim3(256), 0, st, a);
          },
          [&](const AncBatch &b, int pass) {
             if (pass == 0) place(b);
             anc_lanes(e->kk, [&](auto N) { hipLaunchKernelGGL(mg_lane_kernel<N()>, b.lanes, dim3(256), 0, st, a, pass); });
          },
          [&](const AncBatch &b) {
             hipLaunchKernelGGL(mg_coef_kernel, dim3(b.lanes.x, nn + 1), dim3(256), 0, st, a);
             HIPCHK(hipGetLastError());
             hipLaunchKernelGGL(mg_rows_kernel, dim3(b.lanes.x, n_rows), dim3(256), 0, st, a);
             HIPCHK(hipGetLastError());
             if (mfma) hipLaunchKernelGGL(mg_w_mfma_kernel, dim3(n_segs, K * nn), dim3(256), 0, st, a);
             else anc_lanes(e->kk, [&](auto N) { hipLaunchKernelGGL(mg_w_lane_kernel<N()>, dim3(n_segs, K * nn), dim3(64), 0, st, a); });
             HIPCHK(hipGetLastError());
             if (n_finished > 0) {
                hipLaunchKernelGGL(mg_add_kernel, dim3((unsigned)((per_seg + 255) / 256)), dim3(256), 0, st, w.W.p + (size_t)b.gene * per_seg, (const double *)w.Wpart.p, per_seg, n_finished);
                HIPCHK(hipGetLastError());
             }
             return 0;
          },
          [](const AncBatch &) { return 0; }))      // (nothing is copied out per batch)
      return rc;

   // the pull-back through every branch's spectral form, the sets' sums, the scalar rows' totals
   ModelGradPullArgs pa{};
   pa.n = n; pa.K = K; pa.n_nodes = nn; pa.root = T.root; pa.n_labels = e->n_labels; pa.rate_gs = e->rate_per_gene ? K : 0; pa.ld = a.ld; pa.wn = wn; pa.n_eigen = n_eigen;
   pa.label = e->d_label.p; pa.eigen_of = e->d_eigen_of.p; pa.eigen = e->d_eigen.p;
   pa.branch = e->d_branch.p; pa.rate = e->d_rate.p; pa.gene_rate = e->d_gene_rate.p; pa.qfactor = e->d_qfactor.p;
   pa.W = w.W.p; pa.GA = w.GA.p; pa.g_eff = w.geff.p; pa.g_A = w.gA.p;
   HIPCHK(hipEventRecord(w.ev0, st));
   hipLaunchKernelGGL(mg_pull_kernel, dim3(nn, G * K), dim3(256), 0, st, pa);
   HIPCHK(hipGetLastError());
   hipLaunchKernelGGL(mg_ga_sum_kernel, dim3((unsigned)((n * n + 255) / 256), n_eigen), dim3(256), 0, st, pa, G);
   HIPCHK(hipGetLastError());
   hipLaunchKernelGGL(mg_total_kernel, dim3(1 + K), dim3(256), 0, st, (const double *)w.partial.p, n_chunks, 0, 0L, n_chunks, w.out.p);
   HIPCHK(hipGetLastError());
   for (int ip = 0; ip < e->n_pi; ip++) {
      const long lo = e->n_pi > 1 ? chunk_base[ip] : 0, cnt = e->n_pi > 1 ? chunk_base[ip + 1] - chunk_base[ip] : n_chunks;
      hipLaunchKernelGGL(mg_total_kernel, dim3(n), dim3(256), 0, st, (const double *)w.partial.p, n_chunks, 1 + K, lo, cnt, w.out.p + 1 + K + (size_t)ip * n);
      HIPCHK(hipGetLastError());
   }
   HIPCHK(hipEventRecord(w.ev1, st));
   std::vector<double> out((size_t)1 + K + (size_t)e->n_pi * n);
   HIPCHK(hipMemcpyAsync(out.data(), w.out.p, out.size() * 8, hipMemcpyDeviceToHost, st));
   if (g_eff) HIPCHK(hipMemcpyAsync(g_eff, w.geff.p, pn * 8, hipMemcpyDeviceToHost, st));
   if (g_A) HIPCHK(hipMemcpyAsync(g_A, w.gA.p, (size_t)n_eigen * n * n * 8, hipMemcpyDeviceToHost, st));
   std::vector<double> wide;      // matrix cores: the 64 x 64 accumulators, closed up to n x n below
   if (Wout && mfma) wide.resize(pn * 4096);
   if (Wout) HIPCHK(hipMemcpyAsync(mfma ? wide.data() : Wout, w.W.p, pn * wn * 8, hipMemcpyDeviceToHost, st));
   HIPCHK(w.lap(st));
   if (Wout && mfma)
      for (size_t s = 0; s < pn; s++)
         for (int r = 0; r < n; r++) std::copy(wide.begin() + s * 4096 + (size_t)r * 64, wide.begin() + s * 4096 + (size_t)r * 64 + n, Wout + (s * n + r) * n);
   *lnL = out[0];
   if (g_freqK) std::copy(out.begin() + 1, out.begin() + 1 + K, g_freqK);
   if (g_pi) std::copy(out.begin() + 1 + K, out.end(), g_pi);
   return 0;
}

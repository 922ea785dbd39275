/* pamlh_mixture_max (paml_amd/host/pamlh_scan.c) in a program of its own, so that it runs under the host sanitizers:
 *     gcc -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -DPAMLH_MIXTURE_ONLY tools/mixture_host_check.c -lm -o mixture_host_check
 *     ./mixture_host_check        (exit status 0 and "ok" lines when every check holds)
 * Random class likelihoods with -inf entries and patterns of weight 0; a case whose maximum lies on the edge s = 1 - 1e-6; the result is
 * compared with the best point of a 40 x 40 grid of midpoints over (s, r), which it may not be below. */
#include "../paml_amd/host/pamlh_scan.c"

static unsigned long long rng_state = 88172645463325252ull;
static double rnd(void)
{
   rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
   return (double)(rng_state >> 11) / 9007199254740992.0;
}

static double mixture(int n, const double *w, const double *f, double s, double r)
{
   double l = 0;
   int h;
   for (h = 0; h < n; h++)
      if (w[h] > 0) l += w[h] * log(s * r * exp(f[h]) + s * (1 - r) * exp(f[n + h]) + (1 - s) * r * exp(f[2 * n + h]) + (1 - s) * (1 - r) * exp(f[3 * n + h]));
   return l;
}

static int run_case(int n, int edge)
{
   double *w = (double *)malloc(n * sizeof(double)), *f = (double *)malloc((size_t)4 * n * sizeof(double)), p0, p1, l, grid = -INFINITY, starts[3][2] = {{0.5, 0.5}, {0.9, 0.3}, {0.05, 0.95}}, lo = INFINITY, hi = -INFINITY;
   int h, c, i, j, k, ok;
   for (h = 0; h < n; h++) {
      w[h] = h % 7 == 3 ? 0 : 1 + (int)(rnd() * 4);
      for (c = 0; c < 4; c++) f[c * n + h] = log(rnd());
      if (edge) for (c = 2; c < 4; c++) f[c * n + h] = f[(c - 2) * n + h] - 1.0;      /* the foreground classes are worse at every pattern */
      if (!edge && h % 11 == 5) f[2 * n + h] = -INFINITY;
      if (w[h] == 0) for (c = 0; c < 4; c++) f[c * n + h] = -INFINITY;
   }
   for (i = 0; i < 40; i++)
      for (j = 0; j < 40; j++) { const double v = mixture(n, w, f, (i + 0.5) / 40, (j + 0.5) / 40); if (v > grid) grid = v; }
   for (k = 0; k < 3; k++) {
      if (pamlh_mixture_max(n, w, f, starts[k][0], starts[k][1], &p0, &p1, &l)) { printf("FAILED: refused\n"); return 1; }
      if (l < lo) lo = l;
      if (l > hi) hi = l;
      if (edge && fabs(p0 + p1 - (1 - 1e-6)) > 1e-12) { printf("FAILED: the maximum is on the edge, s = %.12f\n", p0 + p1); return 1; }
   }
   ok = lo >= grid && hi - lo <= 1e-9;
   printf("%s: %d patterns%s: three starts within %.3e, above the grid by %.3e\n", ok ? "ok" : "FAILED", n, edge ? " (maximum on the edge)" : "", hi - lo, lo - grid);
   free(w); free(f);
   return !ok;
}

int main(void)
{
   int bad = run_case(86, 0) + run_case(200, 0) + run_case(50, 1);
   return bad ? 1 : 0;
}

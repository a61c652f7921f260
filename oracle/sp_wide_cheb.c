/*
 * oracle/sp_wide_cheb.c -- TEST INFRASTRUCTURE ONLY (ours).
 *
 * The wide problem of ref_shim.c (wide_cheb / wide_cheb_jac) for float callbacks: the same text with float, sinf, cosf.  It drives
 * the host-callback path's slevmar_* entries at the sizes where its kernel changes the way it forms the sums
 * (tests/callback_problems.py).  ref_shim.c includes this file, so oracle/_ref exports the twins next to the double ones; it is
 * also compiled into liboracle.so, which every machine builds from the tree, while a machine without the reference keeps whatever
 * oracle/_ref it was given: the tests take the twins' addresses from liboracle.so.
 */
#include <math.h>

void sp_wide_cheb(float *p, float *x, int m, int n, void *d)
{
  int i, j;
  (void)d;
  for (i = 0; i < n; ++i) {
    const float t = (n > 1) ? -1.0f + 2.0f * i / (n - 1) : 0.0f;
    float tjm1 = 1.0f, tj = t, s = p[0];
    for (j = 1; j < m; ++j) {
      const float next = 2.0f * t * tj - tjm1;
      s += p[j] * tj;
      tjm1 = tj;
      tj = next;
    }
    x[i] = s + 0.05f * sinf(p[0] * t);
  }
}
void sp_wide_cheb_jac(float *p, float *jac, int m, int n, void *d)
{
  int i, j;
  (void)d;
  for (i = 0; i < n; ++i) {
    const float t = (n > 1) ? -1.0f + 2.0f * i / (n - 1) : 0.0f;
    float tjm1 = 1.0f, tj = t;
    jac[i * m] = 1.0f + 0.05f * t * cosf(p[0] * t);
    for (j = 1; j < m; ++j) {
      const float next = 2.0f * t * tj - tjm1;
      jac[i * m + j] = tj;
      tjm1 = tj;
      tj = next;
    }
  }
}

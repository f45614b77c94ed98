/*
 * rt_zero_risk.h -- can a triangle's interpolated normal be exactly zero?
 * Shared verbatim by the host flatten (host/accel.c rt_flatten) and the
 * device geometry update (csrc/rt_geom.hip), so both flag the same objects
 * (RT_REC_ZERO_RISK_BIT) from the same normal rows: plain double arithmetic,
 * both built with -ffp-contract=off.
 */
#ifndef RT_ZERO_RISK_H
#define RT_ZERO_RISK_H

#ifdef __HIPCC__
#define RT_ZR_FN __host__ __device__ __forceinline__
#else
#define RT_ZR_FN static inline
#endif

/* Squared distance from the origin to the triangle (a, b, c), in double
 * (closest point by Voronoi regions, Ericson, Real-Time Collision Detection
 * 5.1.5). */
RT_ZR_FN double origin_tri_dist2(const double a[3], const double b[3], const double c[3])
{
  double ab[3], ac[3], ap[3], bp[3], cp[3], q[3];
  for (int k = 0; k < 3; k++)
  {
    ab[k] = b[k] - a[k];
    ac[k] = c[k] - a[k];
    ap[k] = -a[k];
    bp[k] = -b[k];
    cp[k] = -c[k];
  }
#define RT_ZR_DOT3(x, y) ((x)[0] * (y)[0] + (x)[1] * (y)[1] + (x)[2] * (y)[2])
  double d1 = RT_ZR_DOT3(ab, ap), d2 = RT_ZR_DOT3(ac, ap);
  if (d1 <= 0 && d2 <= 0)
    return RT_ZR_DOT3(a, a);
  double d3 = RT_ZR_DOT3(ab, bp), d4 = RT_ZR_DOT3(ac, bp);
  if (d3 >= 0 && d4 <= d3)
    return RT_ZR_DOT3(b, b);
  double vc = d1 * d4 - d3 * d2;
  if (vc <= 0 && d1 >= 0 && d3 <= 0)
  {
    double v = d1 / (d1 - d3);
    for (int k = 0; k < 3; k++) q[k] = a[k] + v * ab[k];
    return RT_ZR_DOT3(q, q);
  }
  double d5 = RT_ZR_DOT3(ab, cp), d6 = RT_ZR_DOT3(ac, cp);
  if (d6 >= 0 && d5 <= d6)
    return RT_ZR_DOT3(c, c);
  double vb = d5 * d2 - d1 * d6;
  if (vb <= 0 && d2 >= 0 && d6 <= 0)
  {
    double w = d2 / (d2 - d6);
    for (int k = 0; k < 3; k++) q[k] = a[k] + w * ac[k];
    return RT_ZR_DOT3(q, q);
  }
  double va = d3 * d6 - d5 * d4;
  if (va <= 0 && (d4 - d3) >= 0 && (d5 - d6) >= 0)
  {
    double w = (d4 - d3) / ((d4 - d3) + (d5 - d6));
    for (int k = 0; k < 3; k++) q[k] = b[k] + w * (c[k] - b[k]);
    return RT_ZR_DOT3(q, q);
  }
  double den = 1.0 / (va + vb + vc);
  double v = vb * den, w = vc * den;
  for (int k = 0; k < 3; k++) q[k] = a[k] + ab[k] * v + ac[k] * w;
  return RT_ZR_DOT3(q, q);
#undef RT_ZR_DOT3
}

/* Can the reference's interpolated normal (n0'(1-u-v) + n1' u) + n2' v of
 * this triangle (cpu/hit.c:38-40, nk' = the normalised vertex normals) be
 * exactly zero for some accepted (u, v)?  Only if 0 lies in (or within float
 * rounding of) the triangle the three unit normals span: each component is
 * a sum of three products of magnitude <= 1, rounded to a few 2^-24, and u,
 * v, 1-u-v may stray a few ulps outside [0, 1].  Distance < 1e-5 = "can". A
 * NaN normal (normalize of a zero vn) stays NaN, never zero. */
RT_ZR_FN int rt_zero_risk_rows(const float *nrm9)
{
  double n[3][3];
  for (int k = 0; k < 9; k++)
  {
    if (nrm9[k] != nrm9[k]) /* NaN */
      return 0;
    n[k / 3][k % 3] = nrm9[k];
  }
  return origin_tri_dist2(n[0], n[1], n[2]) < 1e-10;
}

#endif

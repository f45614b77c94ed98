/*
 * rt_mt.h -- the reference's float Moller-Trumbore test (cpu/hit.c:15-33) in
 * plain float arithmetic: the same operations in the same order, each rounded
 * to float (build without FMA contraction).  Shared by the host model of the
 * traversal (accel_probe.c) and the light buffers' soundness test
 * (tests/native/lightbuf_geom.cpp); C and C++.
 */
#ifndef RT_MT_H
#define RT_MT_H

#include "rt_scene.h"

static inline rt_vec3 rt_mt_sub(rt_vec3 a, rt_vec3 b) { rt_vec3 r = { a.x - b.x, a.y - b.y, a.z - b.z }; return r; }
static inline rt_vec3 rt_mt_cross(rt_vec3 a, rt_vec3 b)
{
  rt_vec3 r = { a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x };
  return r;
}

/* r: a record's v0, e1, e2; 1 = accepted, with t, u, v */
static inline int mt_exact(rt_vec3 o, rt_vec3 d, const float *r, float *t, float *u, float *v)
{
  const float eps = 0.0000001f;
  rt_vec3 v0 = { r[0], r[1], r[2] }, e1 = { r[3], r[4], r[5] }, e2 = { r[6], r[7], r[8] };
  rt_vec3 h = rt_mt_cross(d, e2);
  float a = e1.x * h.x + e1.y * h.y + e1.z * h.z;
  if (a > -eps && a < eps)
    return 0;
  float f = 1 / a;
  rt_vec3 s = rt_mt_sub(o, v0);
  *u = f * (s.x * h.x + s.y * h.y + s.z * h.z);
  if (*u < 0.0 || *u > 1.0)
    return 0;
  rt_vec3 q = rt_mt_cross(s, e1);
  *v = f * (d.x * q.x + d.y * q.y + d.z * q.z);
  if (*v < 0.0 || *u + *v > 1.0)
    return 0;
  *t = f * (e2.x * q.x + e2.y * q.y + e2.z * q.z);
  return *t > eps;
}

#endif

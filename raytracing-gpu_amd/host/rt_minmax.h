/*
 * rt_minmax.h -- the float min / max of the vertex boxes and the scene box.
 * Shared verbatim by the host flatten (host/accel.c rt_flatten) and the
 * device geometry update (csrc/rt_geom.hip), so both give the same bits
 * whatever the order they meet the values in: by value, and of two zeros
 * the minimum is -0 and the maximum +0.  (fminf / fmaxf leave the zero's
 * sign to the implementation: glibc returns an operand chosen by position,
 * v_min_f32 / v_max_f32 order -0 below +0.)  Finite input only.
 */
#ifndef RT_MINMAX_H
#define RT_MINMAX_H

#ifdef __HIPCC__
#define RT_MM_FN __host__ __device__ __forceinline__
#else
#define RT_MM_FN static inline
#endif

RT_MM_FN float rt_min_f(float a, float b)
{
  return (b < a || (b == a && __builtin_signbit(b))) ? b : a;
}

RT_MM_FN float rt_max_f(float a, float b)
{
  return (b > a || (b == a && !__builtin_signbit(b))) ? b : a;
}

#endif

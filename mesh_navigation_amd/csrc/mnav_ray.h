// mnav_ray.h -- the ray/triangle test of the obstacle layer (mnav_layer_obstacle), host- and device-compilable.
//
// ObstacleLayer::processPointCloud (obstacle_layer.cpp:216-290) casts one ray per point through MeshMap::raycaster()
// (Embree or lvr2's BVH, mesh_map.cpp:312-324).  Neither backend pins its edge / tie behaviour, so the library pins
// its own: the watertight test of Woop, Benthin & Wald, "Watertight Ray/Triangle Intersection", JCGT 2(1) 2013,
// two-sided, t >= 0.  A ray through a shared edge or vertex hits at least one of the faces around it (the edge
// functions of two faces over a shared edge are exact negatives of each other; zeros are recomputed in double).
// Every operation is written out in a fixed order; the library and the CPU test shim are built with
// -ffp-contract=off, and tests/obstacle_model.py restates the same sequence in numpy float32.
#ifndef MNAV_RAY_H
#define MNAV_RAY_H

#include <math.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define MNAV_RAY_HD __host__ __device__ __forceinline__
#else
#define MNAV_RAY_HD inline
#endif

namespace mnav {

// The per-direction constants (all rays of one call share the direction): the dimension where |d| is largest
// becomes z (first index on ties), x / y follow cyclically and swap when d_z < 0 (keeps the winding), then the
// shear that maps d onto the z axis.
struct RaySetup {
  int kx, ky, kz;
  float sx, sy, sz;
};

MNAV_RAY_HD float ray_abs(float a) { return a < 0.f ? -a : a; }
MNAV_RAY_HD float ray_comp(float x, float y, float z, int k) { return k == 0 ? x : (k == 1 ? y : z); }

MNAV_RAY_HD RaySetup ray_setup(float dx, float dy, float dz)
{
  RaySetup s;
  int kz = 0;
  if (ray_abs(dy) > ray_abs(dx)) kz = 1;
  if (ray_abs(dz) > ray_abs(ray_comp(dx, dy, dz, kz))) kz = 2;
  int kx = kz + 1 == 3 ? 0 : kz + 1;
  int ky = kx + 1 == 3 ? 0 : kx + 1;
  const float dkz = ray_comp(dx, dy, dz, kz);
  if (dkz < 0.f) { const int t = kx; kx = ky; ky = t; }
  s.kx = kx; s.ky = ky; s.kz = kz;
  s.sx = ray_comp(dx, dy, dz, kx) / dkz;
  s.sy = ray_comp(dx, dy, dz, ky) / dkz;
  s.sz = 1.0f / dkz;
  return s;
}

// The slope of the BVH's slab test along one axis of the direction: 1 / d, kept finite so that a zero component never
// makes 0 * inf.
MNAV_RAY_HD float ray_slab_inverse(float d) { return fabsf(d) < 1e-30f ? copysignf(1e30f, d) : 1.0f / d; }

// Ray (origin o, direction of `s`) against triangle (a, b, c), each a float[3].  Returns 1 and *t_out = T / det on a
// hit with t >= 0 (either side of the face), 0 otherwise.  A face with det == 0 (degenerate in the ray's shear
// space: repeated or collinear vertices) never hits; neither does anything that produces a NaN t.
MNAV_RAY_HD int ray_triangle(const RaySetup& s, const float* o, const float* a, const float* b, const float* c, float* t_out)
{
  const float ax = a[0] - o[0], ay = a[1] - o[1], az = a[2] - o[2];
  const float bx = b[0] - o[0], by = b[1] - o[1], bz = b[2] - o[2];
  const float cx = c[0] - o[0], cy = c[1] - o[1], cz = c[2] - o[2];
  const float akx = ray_comp(ax, ay, az, s.kx), aky = ray_comp(ax, ay, az, s.ky), akz = ray_comp(ax, ay, az, s.kz);
  const float bkx = ray_comp(bx, by, bz, s.kx), bky = ray_comp(bx, by, bz, s.ky), bkz = ray_comp(bx, by, bz, s.kz);
  const float ckx = ray_comp(cx, cy, cz, s.kx), cky = ray_comp(cx, cy, cz, s.ky), ckz = ray_comp(cx, cy, cz, s.kz);
  const float Ax = akx - s.sx * akz, Ay = aky - s.sy * akz;
  const float Bx = bkx - s.sx * bkz, By = bky - s.sy * bkz;
  const float Cx = ckx - s.sx * ckz, Cy = cky - s.sy * ckz;
  float U = Cx * By - Cy * Bx;
  float V = Ax * Cy - Ay * Cx;
  float W = Bx * Ay - By * Ax;
  if (U == 0.f || V == 0.f || W == 0.f) {             // on an edge in float: decide with exact products (paper, sec. 3)
    U = (float)((double)Cx * (double)By - (double)Cy * (double)Bx);
    V = (float)((double)Ax * (double)Cy - (double)Ay * (double)Cx);
    W = (float)((double)Bx * (double)Ay - (double)By * (double)Ax);
  }
  if ((U < 0.f || V < 0.f || W < 0.f) && (U > 0.f || V > 0.f || W > 0.f)) return 0;
  const float det = (U + V) + W;
  if (det == 0.f) return 0;
  const float Az = s.sz * akz, Bz = s.sz * bkz, Cz = s.sz * ckz;
  const float T = (U * Az + V * Bz) + W * Cz;
  const float t = T / det;
  if (!(t >= 0.f)) return 0;                          // behind the origin, or NaN
  *t_out = t;
  return 1;
}

// The point filter and transform of obstacle_layer.cpp:216-227: kept iff sqrtf(x*x + y*y + z*z) <= max_dist (compared
// in double; NaN fails); o = R p + t with a row-major 3x4 matrix m, each row as ((m0*x + m1*y) + m2*z) + m3.
MNAV_RAY_HD int ray_point_kept(float x, float y, float z, double max_dist)
{
  const float n2 = (x * x + y * y) + z * z;
  const float n = sqrtf(n2);
  return (double)n <= max_dist ? 1 : 0;
}

MNAV_RAY_HD void ray_transform(const float* m, float x, float y, float z, float* o)
{
  for (int r = 0; r < 3; ++r) o[r] = ((m[4 * r] * x + m[4 * r + 1] * y) + m[4 * r + 2] * z) + m[4 * r + 3];
}

// A ray whose origin overflowed to inf / NaN in the transform is cast nowhere (a departure: the reference hands it to
// the backend, whose answer for such a ray is undefined).
MNAV_RAY_HD int ray_origin_finite(const float* o)
{
  return isfinite(o[0]) && isfinite(o[1]) && isfinite(o[2]) ? 1 : 0;
}

}  // namespace mnav

#endif  // MNAV_RAY_H

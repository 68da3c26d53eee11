// ed_kabsch.h — the 3x3 rotation of a least-squares superposition, float64, shared by superpose.hip and flex.hip.  Device only.
//   kabsch_rotation   h (the covariance of two centred point sets) -> the orthogonal r with r a ~ b, by a one-sided Jacobi SVD that
//                     every lane runs redundantly: no lane-dependent branch decides a result, so all lanes end with the same bits.
#pragma once
#include <math.h>

#include <hip/hip_runtime.h>

namespace ed {

// One rotation of the one-sided (Hestenes) Jacobi SVD: columns p and q of G = H V are rotated until orthogonal, V follows.
template <int P, int Q>
__device__ __forceinline__ bool jacobi_rotate(double* g, double* v) {
  const double alpha = g[P] * g[P] + g[3 + P] * g[3 + P] + g[6 + P] * g[6 + P];
  const double beta = g[Q] * g[Q] + g[3 + Q] * g[3 + Q] + g[6 + Q] * g[6 + Q];
  const double gamma = g[P] * g[Q] + g[3 + P] * g[3 + Q] + g[6 + P] * g[6 + Q];
  if (!(fabs(gamma) > 1e-16 * sqrt(alpha * beta))) return false;
  const double zeta = (beta - alpha) / (2.0 * gamma);
  const double tn = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
  const double c = 1.0 / sqrt(1.0 + tn * tn), s = c * tn;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double gp = g[3 * i + P], gq = g[3 * i + Q];
    g[3 * i + P] = c * gp - s * gq;
    g[3 * i + Q] = s * gp + c * gq;
    const double vp = v[3 * i + P], vq = v[3 * i + Q];
    v[3 * i + P] = c * vp - s * vq;
    v[3 * i + Q] = s * vp + c * vq;
  }
  return true;
}

template <int P, int Q>
__device__ __forceinline__ void sort_columns(double* g, double* v, double* n2) {
  if (n2[P] < n2[Q]) {
    double x = n2[P];
    n2[P] = n2[Q];
    n2[Q] = x;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      x = g[3 * i + P], g[3 * i + P] = g[3 * i + Q], g[3 * i + Q] = x;
      x = v[3 * i + P], v[3 * i + P] = v[3 * i + Q], v[3 * i + Q] = x;
    }
  }
}

// h = sum_i a_i b_i^T (centred; row-major) = U S V^T  ->  r = V U^T (row-major), the orthogonal matrix with r a ~ b.
// G = H V has the columns s_k u_k.  u_1 = g_1 / s_1; u_2 = g_2 made orthogonal to u_1 (any perpendicular when s_2 vanishes:
// collinear points, every choice moves them alike); u_3 = +-(u_1 x u_2).  Proper rule: the sign that makes det r = +1.
// Reflection-allowed rule: the sign of g_3 . (u_1 x u_2), i.e. of det h, which is what the bare V U^T carries — unless s_3 vanishes
// (planar points: both signs move them alike), where the proper one is taken.
__device__ __forceinline__ void kabsch_rotation(const double* h, int allow_reflection, double* r) {
  double g[9], v[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
#pragma unroll
  for (int i = 0; i < 9; ++i) g[i] = h[i];
  for (int sweep = 0; sweep < 30; ++sweep) {
    bool any = jacobi_rotate<0, 1>(g, v);
    any |= jacobi_rotate<0, 2>(g, v);
    any |= jacobi_rotate<1, 2>(g, v);
    if (!any) break;
  }
  double n2[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) n2[k] = g[k] * g[k] + g[3 + k] * g[3 + k] + g[6 + k] * g[6 + k];
  sort_columns<0, 1>(g, v, n2);
  sort_columns<0, 2>(g, v, n2);
  sort_columns<1, 2>(g, v, n2);
  const double s1 = sqrt(n2[0]);
  if (!(s1 > 0) || !(s1 < INFINITY)) {   // all points coincide (or non-finite input): nothing to rotate
#pragma unroll
    for (int i = 0; i < 9; ++i) r[i] = (i % 4 == 0) ? 1.0 : 0.0;
    return;
  }
  double u1[3], u2[3], u3[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) u1[i] = g[3 * i] / s1;
  const double p12 = g[1] * u1[0] + g[4] * u1[1] + g[7] * u1[2];
#pragma unroll
  for (int i = 0; i < 3; ++i) u2[i] = g[3 * i + 1] - p12 * u1[i];
  double nw = sqrt(u2[0] * u2[0] + u2[1] * u2[1] + u2[2] * u2[2]);
  if (!(nw > 1e-10 * s1)) {
    const double a0 = fabs(u1[0]), a1 = fabs(u1[1]), a2 = fabs(u1[2]);
    const int e = (a0 <= a1 && a0 <= a2) ? 0 : (a1 <= a2 ? 1 : 2);
    const double ue = e == 0 ? u1[0] : (e == 1 ? u1[1] : u1[2]);
#pragma unroll
    for (int i = 0; i < 3; ++i) u2[i] = (i == e ? 1.0 : 0.0) - ue * u1[i];
    nw = sqrt(u2[0] * u2[0] + u2[1] * u2[1] + u2[2] * u2[2]);
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) u2[i] /= nw;
  u3[0] = u1[1] * u2[2] - u1[2] * u2[1];
  u3[1] = u1[2] * u2[0] - u1[0] * u2[2];
  u3[2] = u1[0] * u2[1] - u1[1] * u2[0];
  const double detv = v[0] * (v[4] * v[8] - v[5] * v[7]) - v[1] * (v[3] * v[8] - v[5] * v[6]) + v[2] * (v[3] * v[7] - v[4] * v[6]);
  double sgn = detv >= 0 ? 1.0 : -1.0;
  if (allow_reflection) {
    const double p3 = g[2] * u3[0] + g[5] * u3[1] + g[8] * u3[2];
    if (fabs(p3) > 1e-10 * s1) sgn = p3 > 0 ? 1.0 : -1.0;
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) u3[i] *= sgn;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) r[3 * i + j] = v[3 * i] * u1[j] + v[3 * i + 1] * u2[j] + v[3 * i + 2] * u3[j];
}

}  // namespace ed

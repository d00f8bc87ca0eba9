// From the moments of a point's neighbours to its oriented normal: the part of open3d's estimate_normals + correct_pcd_normal_direction
// (Utils.py:205-213) that follows the neighbour search.  Shared by the organized search (scene.hip) and the grid search
// (grid_index.hip): one text, so the two give the same bits from the same moments.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#pragma clang fp contract(off)

// One Jacobi rotation of a symmetric 3 x 3 matrix in the (p, q) plane: app, aqq, apq the rotated block, arp, arq the third index's
// row, (v?p, v?q) the two columns of the accumulated eigenvector matrix.
__device__ __forceinline__ void jacobi_rotate(double& app, double& aqq, double& apq, double& arp, double& arq, double& v0p, double& v0q,
                                              double& v1p, double& v1q, double& v2p, double& v2q) {
  if (apq == 0.0) return;
  const double theta = (aqq - app) / (2.0 * apq);
  const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));   // the smaller root: |angle| <= pi/4
  const double c = 1.0 / sqrt(t * t + 1.0), sn = t * c;
  app -= t * apq; aqq += t * apq; apq = 0.0;
  double a = arp, b = arq;
  arp = c * a - sn * b; arq = sn * a + c * b;
  a = v0p; b = v0q; v0p = c * a - sn * b; v0q = sn * a + c * b;
  a = v1p; b = v1q; v1p = c * a - sn * b; v1q = sn * a + c * b;
  a = v2p; b = v2q; v2p = c * a - sn * b; v2q = sn * a + c * b;
}

// unit eigenvector of the smallest eigenvalue of the symmetric matrix (a00 a01 a02; . a11 a12; . . a22): cyclic Jacobi
__device__ __forceinline__ void smallest_eigenvector(double a00, double a01, double a02, double a11, double a12, double a22, double& nx,
                                                     double& ny, double& nz) {
  double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
  for (int sweep = 0; sweep < 12; ++sweep) {
    if (fabs(a01) + fabs(a02) + fabs(a12) <= 1e-19 * (fabs(a00) + fabs(a11) + fabs(a22))) break;
    jacobi_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);
    jacobi_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);
    jacobi_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);
  }
  const bool c0 = a00 <= a11 && a00 <= a22, c1 = !c0 && a11 <= a22;
  nx = c0 ? v00 : c1 ? v01 : v02; ny = c0 ? v10 : c1 ? v11 : v12; nz = c0 ? v20 : c1 ? v21 : v22;
  const double len = sqrt(nx * nx + ny * ny + nz * nz);
  nx /= len; ny /= len; nz /= len;
}

// Moments m (n neighbours; sums sx .. szz of d and d d^T, d = p_j - q) of the point (qx, qy, qz) -> its normal, turned towards the view
// point (vx, vy, vz).
template <typename M>
__device__ __forceinline__ void oriented_normal(const M& m, double qx, double qy, double qz, double vx, double vy, double vz, double& nx,
                                                double& ny, double& nz) {
  nx = 0.0; ny = 0.0; nz = 1.0;                             // open3d's normal of a point with fewer than 3 neighbours
  if (m.n >= 3) {
    const double n = (double)m.n, mx = m.sx / n, my = m.sy / n, mz = m.sz / n;
    smallest_eigenvector(m.sxx / n - mx * mx, m.sxy / n - mx * my, m.sxz / n - mx * mz, m.syy / n - my * my, m.syz / n - my * mz,
                         m.szz / n - mz * mz, nx, ny, nz);
  }
  // correct_pcd_normal_direction
  const double len = sqrt(nx * nx + ny * ny + nz * nz) + 1e-10;
  nx /= len; ny /= len; nz /= len;
  double wx = vx - qx, wy = vy - qy, wz = vz - qz;
  const double wl = sqrt(wx * wx + wy * wy + wz * wz);
  wx /= wl; wy /= wl; wz /= wl;
  if (wx * nx + wy * ny + wz * nz < 0.0) { nx = -nx; ny = -ny; nz = -nz; }
}

// rmsf_device.h -- device math shared by the HIP translation units
// (rmsf_kernels.hip: the superpose/accumulate kernels; covariance.hip,
// pca_project.hip: the dense sweeps over aligned frames; pairwise.hip: the
// all-pairs RMSD): the f32-faithful transform of RMSF.py:99-101 / 133-135 and
// the QCP solve of qcprot (RMSF.py:43-51).  Every kernel calls exactly this
// code, so a frame's rotation, its transformed coordinates and a pair's
// lambda come out of the same instruction sequence on every path.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "rmsf_hip.h"

constexpr int kXform = RMSF_XFORM_DOUBLES;  // doubles of a frame's transform record
constexpr int kRec = 12;                    // ... of which apply_xform reads the first: R (9), the mobile COM (3)

// ---------------------------------------------------------------------------
// f32-faithful superposition transform of RMSF.py:99-101 / 133-135.
//   p = f32(f64(p) - com); p = f32(f64(p) @ R); p = f32(f64(p) + ref_com)
__device__ __forceinline__ void apply_xform(float &x, float &y, float &z, const double *__restrict__ t,
                                            double rc0, double rc1, double rc2) {
  const float p0 = (float)((double)x - t[9]);
  const float p1 = (float)((double)y - t[10]);
  const float p2 = (float)((double)z - t[11]);
  const double d0 = p0, d1 = p1, d2 = p2;
  // out_b = sum_a p_a R[a][b]   (np.dot(positions, R), R row-major), as the
  // host BLAS dgemm accumulates it: an FMA chain over a = 0, 1, 2 from
  // p_0 R[0][b] (tests/test_rotation_rounding.py: numpy's dot equals this
  // chain bit for bit, the unfused sum in only 60-75 % of values).  Explicit fma,
  // so the rounding order does not depend on -ffp-contract.
  const float r0 = (float)__builtin_fma(d2, t[6], __builtin_fma(d1, t[3], d0 * t[0]));
  const float r1 = (float)__builtin_fma(d2, t[7], __builtin_fma(d1, t[4], d0 * t[1]));
  const float r2 = (float)__builtin_fma(d2, t[8], __builtin_fma(d1, t[5], d0 * t[2]));
  x = (float)((double)r0 + rc0);
  y = (float)((double)r1 + rc1);
  z = (float)((double)r2 + rc2);
}

// A stage's transform records on their way to LDS, in the dense sweeps that
// stage KT frames at a time with a workgroup of BLOCK threads: the kRec
// doubles apply_xform reads of frames [fb, fb + KT) -- a frame past the
// range's end reads frame f1 - 1 -- are loaded into registers, 1.5 doubles a
// lane at KT = 32 and BLOCK = 256, ahead of the MFMAs that hide the latency,
// and parked in sxf[KT][kRec] once those are issued, where the 16 lanes of a
// frame read them as a broadcast.
constexpr int rec_loads(int kt, int block) { return (kt * kRec + block - 1) / block; }  // doubles a lane

template <int KT, int BLOCK>
__device__ __forceinline__ void load_records(double (&recv)[rec_loads(KT, BLOCK)], const double *__restrict__ xform,
                                             int64_t fb, int64_t f1, int tid) {
#pragma unroll
  for (int r = 0; r < rec_loads(KT, BLOCK); ++r) {
    const int e = (r * BLOCK + tid) % (KT * kRec);  // (the last round wraps: its extra lanes reload)
    const int64_t f = fb + e / kRec;
    recv[r] = xform[(f < f1 ? f : f1 - 1) * kXform + e % kRec];
  }
}

template <int KT, int BLOCK>
__device__ __forceinline__ void park_records(double *sxf, const double (&recv)[rec_loads(KT, BLOCK)],
                                             int tid) {
#pragma unroll
  for (int r = 0; r < rec_loads(KT, BLOCK); ++r) {
    const int e = r * BLOCK + tid;
    if (e < KT * kRec) sxf[e] = recv[r];
  }
}

// ---------------------------------------------------------------------------
// QCP: the published quaternion-characteristic-polynomial algorithm
// (D. Theobald, Acta Cryst A 61:478, 2005; P. Liu et al., J Comput Chem
// 31:1561, 2010), as used by MDAnalysis.lib.qcprot (RMSF.py:48).  A is the
// row-major inner product sum_i mob_i[a] ref_i[b]; rot is applied as x @ rot.
// SURVEY.md Appendix A.2-A.3 gives the exact sequence followed here.
//
// The largest root of the QCP quartic: the coefficients, Newton's iteration
// from lambda = E0 (an upper bound) and its stopping rule.  *met: the rule
// fired within the 50 steps; *slope: the quartic's derivative at the last
// point it was evaluated at (the last step's denominator).
__host__ __device__ inline double qcp_newton(const double *A, double E0, bool *met, double *slope) {
  const double Sxx = A[0], Sxy = A[1], Sxz = A[2];
  const double Syx = A[3], Syy = A[4], Syz = A[5];
  const double Szx = A[6], Szy = A[7], Szz = A[8];

  const double Sxx2 = Sxx * Sxx, Syy2 = Syy * Syy, Szz2 = Szz * Szz;
  const double Sxy2 = Sxy * Sxy, Syz2 = Syz * Syz, Sxz2 = Sxz * Sxz;
  const double Syx2 = Syx * Syx, Szy2 = Szy * Szy, Szx2 = Szx * Szx;

  const double SyzSzymSyySzz2 = 2.0 * (Syz * Szy - Syy * Szz);
  const double Sxx2Syy2Szz2Syz2Szy2 = Syy2 + Szz2 - Sxx2 + Syz2 + Szy2;

  const double C2 = -2.0 * (Sxx2 + Syy2 + Szz2 + Sxy2 + Syx2 + Sxz2 + Szx2 + Syz2 + Szy2);
  const double C1 = 8.0 * (Sxx * Syz * Szy + Syy * Szx * Sxz + Szz * Sxy * Syx - Sxx * Syy * Szz -
                           Syz * Szx * Sxy - Szy * Syx * Sxz);

  const double SxzpSzx = Sxz + Szx, SyzpSzy = Syz + Szy, SxypSyx = Sxy + Syx;
  const double SyzmSzy = Syz - Szy, SxzmSzx = Sxz - Szx, SxymSyx = Sxy - Syx;
  const double SxxpSyy = Sxx + Syy, SxxmSyy = Sxx - Syy;
  const double Sxy2Sxz2Syx2Szx2 = Sxy2 + Sxz2 - Syx2 - Szx2;

  const double C0 =
      Sxy2Sxz2Syx2Szx2 * Sxy2Sxz2Syx2Szx2 +
      (Sxx2Syy2Szz2Syz2Szy2 + SyzSzymSyySzz2) * (Sxx2Syy2Szz2Syz2Szy2 - SyzSzymSyySzz2) +
      (-(SxzpSzx) * (SyzmSzy) + (SxymSyx) * (SxxmSyy - Szz)) *
          (-(SxzmSzx) * (SyzpSzy) + (SxymSyx) * (SxxmSyy + Szz)) +
      (-(SxzpSzx) * (SyzpSzy) - (SxypSyx) * (SxxpSyy - Szz)) *
          (-(SxzmSzx) * (SyzmSzy) - (SxypSyx) * (SxxpSyy + Szz)) +
      (+(SxypSyx) * (SyzpSzy) + (SxzpSzx) * (SxxmSyy + Szz)) *
          (-(SxymSyx) * (SyzmSzy) + (SxzpSzx) * (SxxpSyy + Szz)) +
      (+(SxypSyx) * (SyzmSzy) + (SxzmSzx) * (SxxmSyy - Szz)) *
          (-(SxymSyx) * (SyzpSzy) + (SxzmSzx) * (SxxpSyy - Szz));

  double l = E0, den = 0.0;
  bool ok = false;
  for (int i = 0; i < 50; ++i) {
    const double old = l;
    const double x2 = l * l;
    const double b = (x2 + C2) * l;
    const double a = b + C1;
    den = 2.0 * x2 * l + b + a;
    const double delta = (a * l + C0) / den;
    l -= delta;
    if (fabs(l - old) < fabs(1e-11 * l)) {
      ok = true;
      break;
    }
  }
  *met = ok;
  *slope = den;
  return l;
}

// qcprot's lambda: whatever Newton's iteration ends at.
__host__ __device__ inline double qcp_lambda(const double *A, double E0) {
  bool met;
  double slope;
  return qcp_newton(A, E0, &met, &slope);
}

// ---------------------------------------------------------------------------
// lambda for the RMSD matrices (pairwise.hip), where only the distance is
// wanted and the pairs are whatever the trajectory holds: mirror images,
// collinear, planar or collapsed frames, symmetric structures.
//
// With s0 >= s1 >= s2 the singular values of A and sigma the sign of det A,
// the quartic's roots are s0 + s1 + sigma s2 (the largest, lambda), s0 - s1 -
// sigma s2, -s0 + s1 - sigma s2 and -s0 - s1 + sigma s2.  Its value P is
// computed to some tens of eps lambda^4 at the best, so the root Newton can
// reach is off by that over the slope P'(lambda) = (lambda - l2)(lambda - l3)
// (lambda - l4).  For a simple root the slope is of the order of lambda^3 and
// the last step, below 1e-11 lambda, leaves that step's square.  Where the two
// largest roots nearly meet (s1 + sigma s2 ~ 0: atoms on a line, a collapsed
// frame, a planar frame against its mirror image, a reflection of a structure
// with s0 = s1 = s2) the slope vanishes: the iteration converges linearly,
// the residual is rounding noise, and the rule fires on that noise -- on the
// first step for two nearly equal frames -- or never.
//
// So Newton's lambda is kept where the rule fired and the slope is at least
// lambda^3 / 16: P is a sum of some twenty products bounded by |A|_F^4 <= 9
// lambda^4, its error below 270 eps lambda^4 = 3e-14 lambda^4, the root's below
// 16 x 3e-14 lambda = 5e-13 lambda, that is 1e-12 E0 in 2 (E0 - lambda).
// Pairs of conformations of one molecule have slopes of 0.7 to 2.4 lambda^3
// and keep qcprot's bits.  Every other pair takes lambda as what it is, the
// largest eigenvalue of the symmetric traceless 4 x 4 key matrix, by cyclic
// Jacobi, whose error is a few eps |K| whatever the gaps are.
constexpr double kPairSlope = 0.0625;

// One Jacobi rotation in the (P, Q) plane of the symmetric k (both triangles
// kept); the indices are template arguments so that k stays in registers.
template <int P, int Q>
__host__ __device__ inline void jacobi_rotate(double (&k)[4][4]) {
  const double apq = k[P][Q];
  if (apq == 0.0) return;
  const double theta = (k[Q][Q] - k[P][P]) / (2.0 * apq);
  // (theta^2 may overflow to inf: t = 0, as it should be)
  const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
  k[P][P] -= t * apq;
  k[Q][Q] += t * apq;
  k[P][Q] = k[Q][P] = 0.0;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    if (r == P || r == Q) continue;
    const double rp = k[r][P], rq = k[r][Q];
    k[r][P] = k[P][r] = c * rp - s * rq;
    k[r][Q] = k[Q][r] = s * rp + c * rq;
  }
}

// The largest eigenvalue of the key matrix of A (the a11..a44 of qcp_solve at
// lambda = 0).  Sweeps stop when the off-diagonal part is below 2^-60 of the
// matrix' norm (which rotations keep), 16 at the most.
// Out of line (`inline` is for the linker): the few lanes that come here must
// not cost the contraction kernels, which inline their epilogue, registers.
// A's entries come by value: a pointer to the caller's registers would put
// them in scratch.
__host__ __device__ inline __attribute__((noinline)) double qcp_key_lambda_max(double Sxx, double Sxy, double Sxz,
                                                                               double Syx, double Syy, double Syz,
                                                                               double Szx, double Szy, double Szz) {
  double k[4][4];
  k[0][0] = Sxx + Syy + Szz, k[1][1] = Sxx - Syy - Szz, k[2][2] = Syy - Sxx - Szz, k[3][3] = Szz - Sxx - Syy;
  k[0][1] = k[1][0] = Syz - Szy, k[0][2] = k[2][0] = Szx - Sxz, k[0][3] = k[3][0] = Sxy - Syx;
  k[1][2] = k[2][1] = Sxy + Syx, k[1][3] = k[3][1] = Sxz + Szx, k[2][3] = k[3][2] = Syz + Szy;
  double norm = 0.0;
#pragma unroll
  for (int p = 0; p < 4; ++p)
#pragma unroll
    for (int q = 0; q < 4; ++q) norm += fabs(k[p][q]);
  if (norm != norm) return norm;  // a non-finite frame stays one
  for (int sweep = 0; sweep < 16; ++sweep) {
    const double off = fabs(k[0][1]) + fabs(k[0][2]) + fabs(k[0][3]) + fabs(k[1][2]) + fabs(k[1][3]) + fabs(k[2][3]);
    if (!(off > 8.673617379884035e-19 * norm)) break;  // 2^-60
    jacobi_rotate<0, 1>(k), jacobi_rotate<0, 2>(k), jacobi_rotate<0, 3>(k);
    jacobi_rotate<1, 2>(k), jacobi_rotate<1, 3>(k), jacobi_rotate<2, 3>(k);
  }
  const double m01 = k[0][0] > k[1][1] ? k[0][0] : k[1][1];
  const double m23 = k[2][2] > k[3][3] ? k[2][2] : k[3][3];
  return m01 > m23 ? m01 : m23;
}

// A pair's lambda; *path receives the way it was found (RMSF_PAIR_* of
// rmsf_hip.h).
__host__ __device__ inline double pair_lambda(const double *A, double E0, int *path) {
  // two all-zero frames: the quartic is 0 / 0; their distance is 0 (and a
  // non-finite frame's NaN stays one)
  if (!(E0 > 0.0)) {
    *path = RMSF_PAIR_ZERO;
    return E0;
  }
  bool met;
  double slope;
  const double l = qcp_newton(A, E0, &met, &slope);
  // (never true of a NaN: 0 / 0 at an exactly double root met on the first
  // step -- a frame of collinear atoms against itself)
  if (met && fabs(slope) >= kPairSlope * fabs(l * l * l)) {
    *path = RMSF_PAIR_NEWTON;
    return l;
  }
  *path = RMSF_PAIR_JACOBI;
  return qcp_key_lambda_max(A[0], A[1], A[2], A[3], A[4], A[5], A[6], A[7], A[8]);
}

// The rotation and the RMSD from that root; the sums and differences of A's
// entries are the adjoint's, the same adds as in qcp_lambda.
__host__ __device__ inline void qcp_solve(const double *A, double E0, double len, double *rot,
                                          double *rmsd) {
  const double Sxx = A[0], Sxy = A[1], Sxz = A[2];
  const double Syx = A[3], Syy = A[4], Syz = A[5];
  const double Szx = A[6], Szy = A[7], Szz = A[8];

  const double SxzpSzx = Sxz + Szx, SyzpSzy = Syz + Szy, SxypSyx = Sxy + Syx;
  const double SyzmSzy = Syz - Szy, SxzmSzx = Sxz - Szx, SxymSyx = Sxy - Syx;
  const double SxxpSyy = Sxx + Syy, SxxmSyy = Sxx - Syy;
  const double l = qcp_lambda(A, E0);
  *rmsd = sqrt(fabs(2.0 * (E0 - l) / len));

  const double a11 = SxxpSyy + Szz - l, a12 = SyzmSzy, a13 = -SxzmSzx, a14 = SxymSyx;
  const double a21 = SyzmSzy, a22 = SxxmSyy - Szz - l, a23 = SxypSyx, a24 = SxzpSzx;
  const double a31 = a13, a32 = a23, a33 = Syy - Sxx - Szz - l, a34 = SyzpSzy;
  const double a41 = a14, a42 = a24, a43 = a34, a44 = Szz - SxxpSyy - l;
  const double a3344_4334 = a33 * a44 - a43 * a34, a3244_4234 = a32 * a44 - a42 * a34;
  const double a3243_4233 = a32 * a43 - a42 * a33, a3143_4133 = a31 * a43 - a41 * a33;
  const double a3144_4134 = a31 * a44 - a41 * a34, a3142_4132 = a31 * a42 - a41 * a32;
  double q1 = a22 * a3344_4334 - a23 * a3244_4234 + a24 * a3243_4233;
  double q2 = -a21 * a3344_4334 + a23 * a3144_4134 - a24 * a3143_4133;
  double q3 = a21 * a3244_4234 - a22 * a3144_4134 + a24 * a3142_4132;
  double q4 = -a21 * a3243_4233 + a22 * a3143_4133 - a23 * a3142_4132;
  double qsqr = q1 * q1 + q2 * q2 + q3 * q3 + q4 * q4;

  const double evecprec = 1e-6;
  if (qsqr < evecprec) {
    q1 = a12 * a3344_4334 - a13 * a3244_4234 + a14 * a3243_4233;
    q2 = -a11 * a3344_4334 + a13 * a3144_4134 - a14 * a3143_4133;
    q3 = a11 * a3244_4234 - a12 * a3144_4134 + a14 * a3142_4132;
    q4 = -a11 * a3243_4233 + a12 * a3143_4133 - a13 * a3142_4132;
    qsqr = q1 * q1 + q2 * q2 + q3 * q3 + q4 * q4;
    if (qsqr < evecprec) {
      const double a1324_1423 = a13 * a24 - a14 * a23, a1224_1422 = a12 * a24 - a14 * a22;
      const double a1223_1322 = a12 * a23 - a13 * a22, a1124_1421 = a11 * a24 - a14 * a21;
      const double a1123_1321 = a11 * a23 - a13 * a21, a1122_1221 = a11 * a22 - a12 * a21;
      q1 = a42 * a1324_1423 - a43 * a1224_1422 + a44 * a1223_1322;
      q2 = -a41 * a1324_1423 + a43 * a1124_1421 - a44 * a1123_1321;
      q3 = a41 * a1224_1422 - a42 * a1124_1421 + a44 * a1122_1221;
      q4 = -a41 * a1223_1322 + a42 * a1123_1321 - a43 * a1122_1221;
      qsqr = q1 * q1 + q2 * q2 + q3 * q3 + q4 * q4;
      if (qsqr < evecprec) {
        q1 = a32 * a1324_1423 - a33 * a1224_1422 + a34 * a1223_1322;
        q2 = -a31 * a1324_1423 + a33 * a1124_1421 - a34 * a1123_1321;
        q3 = a31 * a1224_1422 - a32 * a1124_1421 + a34 * a1122_1221;
        q4 = -a31 * a1223_1322 + a32 * a1123_1321 - a33 * a1122_1221;
        qsqr = q1 * q1 + q2 * q2 + q3 * q3 + q4 * q4;
        if (qsqr < evecprec) {
          rot[0] = rot[4] = rot[8] = 1.0;
          rot[1] = rot[2] = rot[3] = rot[5] = rot[6] = rot[7] = 0.0;
          return;
        }
      }
    }
  }
  const double normq = sqrt(qsqr);
  q1 /= normq;
  q2 /= normq;
  q3 /= normq;
  q4 /= normq;
  const double a2 = q1 * q1, x2 = q2 * q2, y2 = q3 * q3, z2 = q4 * q4;
  const double xy = q2 * q3, az = q1 * q4, zx = q4 * q2, ay = q1 * q3, yz = q3 * q4, ax = q1 * q2;
  rot[0] = a2 + x2 - y2 - z2;
  rot[1] = 2 * (xy + az);
  rot[2] = 2 * (zx - ay);
  rot[3] = 2 * (xy - az);
  rot[4] = a2 - x2 + y2 - z2;
  rot[5] = 2 * (yz + ax);
  rot[6] = 2 * (zx + ay);
  rot[7] = 2 * (yz - ax);
  rot[8] = a2 - x2 - y2 + z2;
}


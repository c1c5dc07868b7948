// pair_image.h -- the squared distance of a pair of atoms, in free space and
// under the minimum image of an orthorhombic box ("Radial
// distribution function").  One rule, host and device, no FMA
// (-ffp-contract=off):
//
//   dx = xa - xb                      (doubles widened from the f32 coordinates)
//   dx = dx - Lx * rint(dx * ix)      ix = 1.0 / Lx formed once a frame on the
//                                     host; rint rounds half to even
//   d2 = (dx*dx + dy*dy) + dz*dz
//
// rint(-x) = -rint(x) bit for bit, so d2(a, b) = d2(b, a).  A non-finite
// coordinate makes d2 NaN (periodic: inf - inf) or inf (free): in no bin, never
// a contact.  csrc/rdf.hip is the one user today; the contact kernels can take
// a box through the same functions.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

namespace pair_image {

// box6 = Lx, Ly, Lz, 1/Lx, 1/Ly, 1/Lz
__host__ __device__ inline double image(double d, double L, double iL) { return d - L * rint(d * iL); }

__host__ __device__ inline double dist2_free(double ax, double ay, double az, double bx, double by, double bz) {
  const double dx = ax - bx, dy = ay - by, dz = az - bz;
  return (dx * dx + dy * dy) + dz * dz;
}

__host__ __device__ inline double dist2_box(double ax, double ay, double az, double bx, double by, double bz,
                                            const double *box6) {
  const double dx = image(ax - bx, box6[0], box6[3]);
  const double dy = image(ay - by, box6[1], box6[4]);
  const double dz = image(az - bz, box6[2], box6[5]);
  return (dx * dx + dy * dy) + dz * dz;
}

}  // namespace pair_image

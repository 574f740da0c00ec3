// Surface-cell rule of GPIS.topcd (gpis.py:127-150), shared by the compaction kernels (cdx_field.hip) and the
// host build (host_ref.cpp: cdxh_surface_extract, the CPU yardstick of those kernels).
//
// mean is a [steps, steps, steps] C-ordered lattice.  internal(c) = mean[c] < 0 (gpis.py:134), so NaN and −0.0
// are not internal.  Cell (i, j, k) is a surface cell iff it is an interior cell of the lattice
// (1 ≤ i, j, k ≤ steps − 2, the reference's loop bounds :137-139), is internal, and at least one of its six face
// neighbours is not (:140-141).  With flip_k every read of the mean (and of the normal the caller gathers) at
// index k goes to steps − 1 − k: the reference views tensor inputs as [:, :, ::−1] (:130-133) while it builds the
// point lattice unflipped (:144-146) — a quirk a drop-in keeps.  The lattice is meshgrid(..., indexing="xy"):
// cell (i, j, k) sits at (ax[j], ay[i], az[k]).
#pragma once
#include "cdx_hd.h"

namespace cdx {

// Index into the mean / normal lattices that cell (i, j, k) reads.
CDX_HD int64_t field_src(int steps, int i, int j, int k, int flip_k) {
  return ((int64_t)i * steps + j) * steps + (flip_k ? steps - 1 - k : k);
}

template <typename T>
CDX_HD bool field_internal(const T* mean, int steps, int i, int j, int k, int flip_k) {
  return mean[field_src(steps, i, j, k, flip_k)] < (T)0;
}

template <typename T>
CDX_HD bool field_surface_cell(const T* mean, int steps, int i, int j, int k, int flip_k) {
  const int hi = steps - 2;
  if (i < 1 || j < 1 || k < 1 || i > hi || j > hi || k > hi) return false;
  if (!field_internal(mean, steps, i, j, k, flip_k)) return false;
  return !field_internal(mean, steps, i - 1, j, k, flip_k) || !field_internal(mean, steps, i + 1, j, k, flip_k) ||
         !field_internal(mean, steps, i, j - 1, k, flip_k) || !field_internal(mean, steps, i, j + 1, k, flip_k) ||
         !field_internal(mean, steps, i, j, k - 1, flip_k) || !field_internal(mean, steps, i, j, k + 1, flip_k);
}

// (i, j, k) of the C-ordered cell index c.
CDX_HD void field_cell(int64_t c, int steps, int& i, int& j, int& k) {
  k = (int)(c % steps);
  const int64_t r = c / steps;
  j = (int)(r % steps);
  i = (int)(r / steps);
}

}  // namespace cdx

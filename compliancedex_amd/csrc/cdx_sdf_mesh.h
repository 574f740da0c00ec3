// Layout of a prepared mesh (cdx_sdf_mesh_prepare's buffer), shared by its builder and distance walk
// (cdx_sdf.hip) and by the ray records built from it (cdx_ray.hip: cdx_ray_mesh_prepare).  Internal: the
// buffer is opaque in include/cdx.h.
#pragma once
#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdint.h>

#include "cdx_sdf.h"

namespace cdx {
namespace mesh {

constexpr int CHUNK = 32;           // faces per chunk (leaf node)
constexpr int TOPB = 16;            // chunks per top node
constexpr int RUN = 8;              // faces per run (a chunk's sub-group with its own node)
constexpr int RPC = 32 / RUN;       // runs per chunk

// Bounding volume of a node: a = (centre xyz, ball radius R), b = (cylinder axis xyz, half-thickness t),
// m = (cylinder radius rc, 1/(1 − α), w = γ·(|centre| + 3R)/(1 − α), γ) with γ = 1e-4 + 1e-8·κ.
struct Node { float4 a, b, m; };
// Disk slab of a face: a = (centroid xyz, in-plane radius r), b = (unit normal xyz, half-thickness t).
struct Slab { float4 a, b; };

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// Mesh: [header words: frame keys ×6, may-NaN flag, 0][face records: C·CHUNK FaceRec][slabs: C·CHUNK Slab]
// [chunk nodes: C Node][top nodes: T Node], C = ⌈F/32⌉, T = ⌈C/16⌉, faces in the build's order.
inline int64_t n_chunks(int64_t F) { return (F + CHUNK - 1) / CHUNK; }
// (runs: RUN-face groups of a chunk, RPC per chunk, each with its own node — tested before the run's faces)
inline int64_t n_tops(int64_t F) { return (n_chunks(F) + TOPB - 1) / TOPB; }
inline size_t mesh_rec_off() { return align256(8 * sizeof(unsigned)); }
inline size_t mesh_slab_off(int64_t C) { return mesh_rec_off() + align256((size_t)C * CHUNK * sizeof(cdx::FaceRec)); }
inline size_t mesh_chunk_off(int64_t C) { return mesh_slab_off(C) + align256((size_t)C * CHUNK * sizeof(Slab)); }
inline size_t mesh_top_off(int64_t C) { return mesh_chunk_off(C) + align256((size_t)C * sizeof(Node)); }
inline size_t mesh_run_off(int64_t C) { return mesh_top_off(C) + align256((size_t)((C + TOPB - 1) / TOPB) * sizeof(Node)); }
inline size_t mesh_bytes(int64_t F) {
  const int64_t C = n_chunks(F);
  return mesh_run_off(C) + align256((size_t)C * RPC * sizeof(Node));
}

}  // namespace mesh
}  // namespace cdx

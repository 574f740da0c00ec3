// Iso-surface mesh of a lattice field by marching tetrahedra: the rule of GPIS.tomesh / surface_mesh, shared by the
// compaction kernels (cdx_mesh.hip) and the host build (host_ref.cpp: cdxh_mesh_extract, their CPU yardstick).
//
// mean is a [s, s, s] C-ordered lattice read as it stands (no flip_k); node c = (i·s + j)·s + k sits at
// P(c) = (px[j], py[i], pz[k]); inside(c) = mean[c] < 0 (field_internal: NaN, +0 and −0 are outside).
//
// Edges.  Node c owns seven edge types d = 0 … 6 to the nodes at (i, j, k) + (1,0,0), (0,1,0), (0,0,1), (1,1,0),
// (1,0,1), (0,1,1), (1,1,1); the edge exists iff that node is in the lattice, its key is 7c + d, and it carries a
// vertex iff inside differs at its ends a = c (lower) and b.  The vertex is Pa + t·(Pb − Pa) per component with
// t = fa/(fa − fb) in f64 (no FMA contraction), t = 0.5 unless 0 ≤ t ≤ 1 — a non-finite value never makes a
// non-finite vertex.  Vertices are numbered in ascending key order.
//
// Faces.  Every lattice cube splits into the six Kuhn tetrahedra, one per permutation π of the axes (i, j, k) in
// lexicographic order, with corners q0 = the cube's origin, q1 = q0 + e_π0, q2 = q1 + e_π1, q3 = q2 + e_π2: the face
// diagonals are the same in every cube, so neighbours agree and the surface is an oriented 2-manifold.  Every edge of
// such a tetrahedron joins a corner to a later one by one of the seven offsets above.  A tetrahedron with one or
// three corners inside gives one triangle, with two inside two, wound so that cross(v1 − v0, v2 − v0) points from
// inside to outside (TorchSDF's sign +1 side).  The winding never comes from vertex positions (coincident vertices
// at a ±0 node must not flip it): the determinant of the corners is sign(π) · the parity of the case's corner order ·
// one global sign of the three axes' directions, negated because (i, j, k) ↔ (y, x, z) is a reflection.
#pragma once
#include "cdx_field.h"

namespace cdx {

// Offset masks: bit 0 = +1 in i, bit 1 = +1 in j, bit 2 = +1 in k.  Edge type d ↔ mask, one nibble each.
CDX_HD int mesh_edge_mask(int d) { return (int)((0x7653421u >> (4 * d)) & 7u); }
CDX_HD int mesh_edge_type(int mask) { return (int)((0x65423100u >> (4 * mask)) & 7u); }

// Corner q of tetrahedron `tet` as an offset mask from the cube's origin.
CDX_HD int mesh_tet_corner(int tet, int q) {
  if (q == 0) return 0;
  if (q == 3) return 7;
  return (int)(((q == 1 ? 0x442211u : 0x656353u) >> (4 * tet)) & 7u);
}
// sign(π) of tetrahedron `tet`: −1 for (0,2,1), (1,0,2) and (2,1,0).
CDX_HD int mesh_tet_sign(int tet) { return ((0x26 >> tet) & 1) ? -1 : 1; }

template <typename T>
CDX_HD bool mesh_inside(const T* mean, int steps, int i, int j, int k) {
  return field_internal(mean, steps, i, j, k, 0);
}

// Bit m of the result: node (i, j, k) + mask m is in the lattice (bit 0: the node itself).
CDX_HD int mesh_exists(int steps, int i, int j, int k) {
  const int bi = i + 1 < steps, bj = j + 1 < steps, bk = k + 1 < steps;
  int e = 1;
  if (bi) e |= 1 << 1;
  if (bj) e |= 1 << 2;
  if (bk) e |= 1 << 4;
  if (bi && bj) e |= 1 << 3;
  if (bi && bk) e |= 1 << 5;
  if (bj && bk) e |= 1 << 6;
  if (bi && bj && bk) e |= 1 << 7;
  return e;
}

// Bit m: node (i, j, k) + mask m exists and is inside.
template <typename T>
CDX_HD int mesh_corner_bits(const T* mean, int steps, int i, int j, int k, int exists) {
  int b = 0;
  for (int m = 0; m < 8; ++m)
    if (((exists >> m) & 1) && mesh_inside(mean, steps, i + (m & 1), j + ((m >> 1) & 1), k + ((m >> 2) & 1))) b |= 1 << m;
  return b;
}

// Bit d: edge type d of the node exists and carries a vertex.
CDX_HD int mesh_cross_mask(int corner_bits, int exists) {
  int x = 0;
  const int in0 = corner_bits & 1;
  for (int d = 0; d < 7; ++d) {
    const int m = mesh_edge_mask(d);
    if (((exists >> m) & 1) && ((corner_bits >> m) & 1) != in0) x |= 1 << d;
  }
  return x;
}

CDX_HD int mesh_popc(int x) {
  int n = 0;
  for (; x; x &= x - 1) ++n;
  return n;
}

// Number of the node's crossing edges of a type below d (its vertex on edge d is base + this).
template <typename T>
CDX_HD int mesh_cross_below(const T* mean, int steps, int i, int j, int k, int d) {
  if (d == 0) return 0;
  const int ex = mesh_exists(steps, i, j, k);
  const bool in0 = mesh_inside(mean, steps, i, j, k);
  int n = 0;
  for (int e = 0; e < d; ++e) {
    const int m = mesh_edge_mask(e);
    if (((ex >> m) & 1) && mesh_inside(mean, steps, i + (m & 1), j + ((m >> 1) & 1), k + ((m >> 2) & 1)) != in0) ++n;
  }
  return n;
}

// The vertex of edge d of node (i, j, k).
template <typename T>
CDX_HD void mesh_vertex(const T* mean, int steps, const double* px, const double* py, const double* pz, int i, int j,
                        int k, int d, double* v) {
  const int m = mesh_edge_mask(d);
  const int ib = i + (m & 1), jb = j + ((m >> 1) & 1), kb = k + ((m >> 2) & 1);
  const double fa = (double)mean[field_src(steps, i, j, k, 0)], fb = (double)mean[field_src(steps, ib, jb, kb, 0)];
  double t = fa / (fa - fb);
  if (!(t >= 0.0 && t <= 1.0)) t = 0.5;
  v[0] = px[j] + t * (px[jb] - px[j]);
  v[1] = py[i] + t * (py[ib] - py[i]);
  v[2] = pz[k] + t * (pz[kb] - pz[k]);
}

// The global sign of the corner determinants: −sgn(Δx)·sgn(Δy)·sgn(Δz) of the axes' first-to-last directions
// (0 for a degenerate axis: no winding is swapped then).
CDX_HD int mesh_axes_sign(double dx, double dy, double dz) {
  const int sx = (dx > 0) - (dx < 0), sy = (dy > 0) - (dy < 0), sz = (dz > 0) - (dz < 0);
  return -sx * sy * sz;
}

// Bits of the four corners of tetrahedron `tet` out of the cube's corner bits (bit q = corner q).
CDX_HD int mesh_tet_bits(int tet, int corner_bits) {
  return (corner_bits & 1) | (((corner_bits >> mesh_tet_corner(tet, 1)) & 1) << 1) |
         (((corner_bits >> mesh_tet_corner(tet, 2)) & 1) << 2) | (((corner_bits >> 7) & 1) << 3);
}

CDX_HD int mesh_tet_count(int bits) {
  const int n = mesh_popc(bits);
  return n == 0 || n == 4 ? 0 : (n == 2 ? 2 : 1);
}

// Faces of a whole cube: all eight corners must exist.
CDX_HD int mesh_cube_count(int corner_bits) {
  int n = 0;
  for (int tet = 0; tet < 6; ++tet) n += mesh_tet_count(mesh_tet_bits(tet, corner_bits));
  return n;
}

// Edge between corners x and y of a tetrahedron as one nibble: lower corner << 2 | higher corner.
CDX_HD uint32_t mesh_tet_edge(int x, int y) { return (uint32_t)(x < y ? (x << 2) | y : (y << 2) | x); }

// The triangles of a tetrahedron with corner bits `bits`: nibble 3·t + v of `tris` is the edge of vertex v of triangle
// t.  `sgn` = mesh_tet_sign · mesh_axes_sign.  Returns the number of triangles.
CDX_HD int mesh_tet_faces(int bits, int sgn, uint32_t& tris) {
  const int n = mesh_popc(bits);
  tris = 0;
  if (n == 0 || n == 4) return 0;
  if (n == 2) {
    int a = -1, b = -1, c = -1, d = -1;
    for (int q = 0; q < 4; ++q) {
      if ((bits >> q) & 1) { if (a < 0) a = q; else b = q; }
      else { if (c < 0) c = q; else d = q; }
    }
    const int inv = (a > c) + (a > d) + (b > c) + (b > d);
    const int det = (inv & 1) ? -sgn : sgn;
    const uint32_t ac = mesh_tet_edge(a, c), ad = mesh_tet_edge(a, d), bd = mesh_tet_edge(b, d), bc = mesh_tet_edge(b, c);
    if (det < 0) tris = ac | (bd << 4) | (ad << 8) | (ac << 12) | (bc << 16) | (bd << 20);
    else tris = ac | (ad << 4) | (bd << 8) | (ac << 12) | (bd << 16) | (bc << 20);
    return 2;
  }
  // one corner alone on its side: x; the others ascending
  const int lone = n == 1 ? bits : (~bits & 15);
  const int x = lone == 1 ? 0 : (lone == 2 ? 1 : (lone == 4 ? 2 : 3));
  const int y1 = x > 0 ? 0 : 1, y2 = x > 1 ? 1 : 2, y3 = x > 2 ? 2 : 3;
  const int det = (x & 1) ? -sgn : sgn;
  const bool swap = n == 1 ? det < 0 : det > 0;
  const uint32_t e1 = mesh_tet_edge(x, y1), e2 = mesh_tet_edge(x, y2), e3 = mesh_tet_edge(x, y3);
  tris = swap ? (e1 | (e3 << 4) | (e2 << 8)) : (e1 | (e2 << 4) | (e3 << 8));
  return 1;
}

// Edge nibble of tetrahedron `tet` → the owning node's offset mask from the cube's origin, and the edge type.
CDX_HD void mesh_tet_edge_node(int tet, uint32_t edge, int& node_mask, int& d) {
  node_mask = mesh_tet_corner(tet, (int)((edge >> 2) & 3u));
  d = mesh_edge_type(mesh_tet_corner(tet, (int)(edge & 3u)) ^ node_mask);
}

// Refinement of a vertex along its own edge by bracketed regula falsi.  The state is (ta, fa, tb, fb), the bracket's
// ends as parameters of the edge and the field there — at first the edge's ends with the lattice's values — and t, the
// vertex.  A step takes the field fv at the vertex, replaces the end whose `inside` is the vertex's, and sets
// t = ta + (tb − ta)·fa/(fa − fb), the midpoint unless that lies in [ta, tb]; a non-finite fv leaves the vertex alone.
CDX_HD double mesh_refine_secant(double ta, double fa, double tb, double fb) {
  const double t = ta + (tb - ta) * (fa / (fa - fb));
  return (t >= ta && t <= tb) ? t : 0.5 * (ta + tb);
}

CDX_HD void mesh_refine_update(double fv, double& ta, double& fa, double& tb, double& fb, double& t) {
  if (!(fabs(fv) <= 1.7976931348623157e308)) return;
  if ((fv < 0.0) == (fa < 0.0)) { ta = t; fa = fv; }
  else { tb = t; fb = fv; }
  t = mesh_refine_secant(ta, fa, tb, fb);
}

// Both ends of the edge with key `key`; false if it is not an edge of the lattice.
CDX_HD bool mesh_key_ends(int64_t key, int steps, int& i, int& j, int& k, int& ib, int& jb, int& kb) {
  const int64_t total = (int64_t)steps * steps * steps;
  if (key < 0 || key >= 7 * total) return false;
  field_cell(key / 7, steps, i, j, k);
  const int m = mesh_edge_mask((int)(key % 7));
  ib = i + (m & 1); jb = j + ((m >> 1) & 1); kb = k + ((m >> 2) & 1);
  return ib < steps && jb < steps && kb < steps;
}

// The point at parameter t of the edge from node (i, j, k) to (ib, jb, kb).
CDX_HD void mesh_edge_point(const double* px, const double* py, const double* pz, int i, int j, int k, int ib, int jb,
                            int kb, double t, double* v) {
  v[0] = px[j] + t * (px[jb] - px[j]);
  v[1] = py[i] + t * (py[ib] - py[i]);
  v[2] = pz[k] + t * (pz[kb] - pz[k]);
}

// One vertex of the refinement: fv null starts the state from the lattice, else one step with the field fv[r].
// state is [5, V]: ta, fa, tb, fb, t.  A key that is no edge of the lattice gives a NaN vertex.
template <typename T>
CDX_HD void mesh_refine_vertex(const T* mean, const double* fv, int steps, const double* px, const double* py,
                               const double* pz, const int64_t* edges, int64_t V, int64_t r, double* state,
                               double* vertices) {
  int i, j, k, ib, jb, kb;
  double* v = vertices + 3 * r;
  if (!mesh_key_ends(edges[r], steps, i, j, k, ib, jb, kb)) {
    const double nan = __builtin_nan("");
    v[0] = v[1] = v[2] = nan;
    return;
  }
  double ta, fa, tb, fb, t;
  if (!fv) {
    ta = 0.0; tb = 1.0;
    fa = (double)mean[field_src(steps, i, j, k, 0)];
    fb = (double)mean[field_src(steps, ib, jb, kb, 0)];
    t = mesh_refine_secant(ta, fa, tb, fb);
  } else {
    ta = state[r]; fa = state[V + r]; tb = state[2 * V + r]; fb = state[3 * V + r]; t = state[4 * V + r];
    mesh_refine_update(fv[r], ta, fa, tb, fb, t);
  }
  state[r] = ta; state[V + r] = fa; state[2 * V + r] = tb; state[3 * V + r] = fb; state[4 * V + r] = t;
  mesh_edge_point(px, py, pz, i, j, k, ib, jb, kb, t, v);
}

}  // namespace cdx

// The 26 moves of the cost-to-go field, shared by geodesic.hip (the costs) and rooms.hip (the labels carried along the
// shortest routes): a move's components, its weight in milli-voxels and the cells its two ends span.  A move is allowed
// when every cell of that box is inside the lattice and passable (include/goslam_hip.h, gs_geodesic_*).
#pragma once

namespace {

// move m of 26: its index 0..26 in the 3 x 3 x 3 neighbourhood (Brick::nb: the centre, 13, is skipped), its components
// and weight
__host__ __device__ constexpr int geo_nb(int m) { return m < 13 ? m : m + 1; }
__host__ __device__ constexpr int geo_d0(int m) { return geo_nb(m) / 9 - 1; }
__host__ __device__ constexpr int geo_d1(int m) { return geo_nb(m) / 3 % 3 - 1; }
__host__ __device__ constexpr int geo_d2(int m) { return geo_nb(m) % 3 - 1; }
__host__ __device__ constexpr int geo_weight(int m) {
  const int nz = (geo_d0(m) != 0) + (geo_d1(m) != 0) + (geo_d2(m) != 0);
  return nz == 1 ? 1000 : (nz == 2 ? 1414 : 1732);
}
// the cells of the box spanned by the centre and move m, as bits of the 3 x 3 x 3 neighbourhood
__host__ __device__ constexpr unsigned geo_box(int m) {
  unsigned bits = 0;
  for (int a = 0; a < 2; ++a)
    for (int b = 0; b < 2; ++b)
      for (int c = 0; c < 2; ++c)
        bits |= 1u << ((a * geo_d0(m) + 1) * 9 + (b * geo_d1(m) + 1) * 3 + (c * geo_d2(m) + 1));
  return bits;
}

}  // namespace

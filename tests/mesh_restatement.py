"""Serial NumPy restatement of the marching-cubes contract of `gs_mcubes_*` (include/goslam_neus.h), written from the
contract and not from the kernel: the GPU tests require the HIP kernels to agree with it bit for bit, the CPU tests check
its topology (watertight, Euler characteristic, no cracks between cubes) on analytic and random fields.

Contract (mcubes.marching_cubes(u, level): vertices in index space, x along axis 0):
  * corner below  <=>  u < level (a NaN corner is not below);
  * a lattice edge crosses iff exactly one endpoint is below; every crossing edge gets exactly one vertex, shared by
    every cube that touches it (on a volume thinner than 2 along some axis no cube exists and such vertices are
    referenced by no face);
  * along the edge from its lower endpoint a0 (value u0) to a1 = a0 + 1 (value u1): t = (level - u0) / (u1 - u0),
    pos = a0 + t * (a1 - a0), fp32 op by op; the other two coordinates are the integer lattice coordinates;
  * vertices ordered by the linear index of the edge's lower endpoint, then axis x < y < z;
  * faces ordered by the linear index of the cube's lowest corner, then the order of the cube's table entry;
  * table: corner c of a cube at offset CORNERS[c], case bit c set iff corner c is below; TRI_TABLE[case] lists the
    case's triangles as cube-edge triples (EDGES[e] = its two corners, lower corner first), wound so that the normal
    (v1 - v0) x (v2 - v0) points toward decreasing u.  Each face of the cube is resolved from its own four corner
    classes: below corners that meet only diagonally on a face stay separated, so two cubes sharing a face agree.
"""
import numpy as np

CORNERS = ((0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1))
# cube edge -> (lower corner, upper corner); the edge runs along the one axis in which the two corners differ
EDGES = ((0, 1), (1, 2), (3, 2), (0, 3), (4, 5), (5, 6), (7, 6), (4, 7), (0, 4), (1, 5), (2, 6), (3, 7))

TRI_TABLE = (
    (),
    (0, 8, 3),
    (0, 1, 9),
    (1, 9, 8, 1, 8, 3),
    (1, 2, 10),
    (0, 8, 3, 1, 2, 10),
    (0, 2, 10, 0, 10, 9),
    (2, 10, 9, 2, 9, 8, 2, 8, 3),
    (2, 3, 11),
    (0, 8, 11, 0, 11, 2),
    (0, 1, 9, 2, 3, 11),
    (1, 9, 8, 1, 8, 11, 1, 11, 2),
    (1, 3, 11, 1, 11, 10),
    (0, 8, 11, 0, 11, 10, 0, 10, 1),
    (0, 3, 11, 0, 11, 10, 0, 10, 9),
    (8, 11, 10, 8, 10, 9),
    (4, 7, 8),
    (0, 4, 7, 0, 7, 3),
    (0, 1, 9, 4, 7, 8),
    (1, 9, 4, 1, 4, 7, 1, 7, 3),
    (1, 2, 10, 4, 7, 8),
    (0, 4, 7, 0, 7, 3, 1, 2, 10),
    (0, 2, 10, 0, 10, 9, 4, 7, 8),
    (2, 10, 9, 2, 9, 4, 2, 4, 7, 2, 7, 3),
    (2, 3, 11, 4, 7, 8),
    (0, 4, 7, 0, 7, 11, 0, 11, 2),
    (0, 1, 9, 2, 3, 11, 4, 7, 8),
    (1, 9, 4, 1, 4, 7, 1, 7, 11, 1, 11, 2),
    (1, 3, 11, 1, 11, 10, 4, 7, 8),
    (0, 4, 7, 0, 7, 11, 0, 11, 10, 0, 10, 1),
    (0, 3, 11, 0, 11, 10, 0, 10, 9, 4, 7, 8),
    (4, 7, 11, 4, 11, 10, 4, 10, 9),
    (4, 9, 5),
    (0, 8, 3, 4, 9, 5),
    (0, 1, 5, 0, 5, 4),
    (1, 5, 4, 1, 4, 8, 1, 8, 3),
    (1, 2, 10, 4, 9, 5),
    (0, 8, 3, 1, 2, 10, 4, 9, 5),
    (0, 2, 10, 0, 10, 5, 0, 5, 4),
    (2, 10, 5, 2, 5, 4, 2, 4, 8, 2, 8, 3),
    (2, 3, 11, 4, 9, 5),
    (0, 8, 11, 0, 11, 2, 4, 9, 5),
    (0, 1, 5, 0, 5, 4, 2, 3, 11),
    (1, 5, 4, 1, 4, 8, 1, 8, 11, 1, 11, 2),
    (1, 3, 11, 1, 11, 10, 4, 9, 5),
    (0, 8, 11, 0, 11, 10, 0, 10, 1, 4, 9, 5),
    (0, 3, 11, 0, 11, 10, 0, 10, 5, 0, 5, 4),
    (4, 8, 11, 4, 11, 10, 4, 10, 5),
    (5, 7, 8, 5, 8, 9),
    (0, 9, 5, 0, 5, 7, 0, 7, 3),
    (0, 1, 5, 0, 5, 7, 0, 7, 8),
    (1, 5, 7, 1, 7, 3),
    (1, 2, 10, 5, 7, 8, 5, 8, 9),
    (0, 9, 5, 0, 5, 7, 0, 7, 3, 1, 2, 10),
    (0, 2, 10, 0, 10, 5, 0, 5, 7, 0, 7, 8),
    (2, 10, 5, 2, 5, 7, 2, 7, 3),
    (2, 3, 11, 5, 7, 8, 5, 8, 9),
    (0, 9, 5, 0, 5, 7, 0, 7, 11, 0, 11, 2),
    (0, 1, 5, 0, 5, 7, 0, 7, 8, 2, 3, 11),
    (1, 5, 7, 1, 7, 11, 1, 11, 2),
    (1, 3, 11, 1, 11, 10, 5, 7, 8, 5, 8, 9),
    (0, 9, 5, 0, 5, 7, 0, 7, 11, 0, 11, 10, 0, 10, 1),
    (0, 3, 11, 0, 11, 10, 0, 10, 5, 0, 5, 7, 0, 7, 8),
    (5, 7, 11, 5, 11, 10),
    (5, 10, 6),
    (0, 8, 3, 5, 10, 6),
    (0, 1, 9, 5, 10, 6),
    (1, 9, 8, 1, 8, 3, 5, 10, 6),
    (1, 2, 6, 1, 6, 5),
    (0, 8, 3, 1, 2, 6, 1, 6, 5),
    (0, 2, 6, 0, 6, 5, 0, 5, 9),
    (2, 6, 5, 2, 5, 9, 2, 9, 8, 2, 8, 3),
    (2, 3, 11, 5, 10, 6),
    (0, 8, 11, 0, 11, 2, 5, 10, 6),
    (0, 1, 9, 2, 3, 11, 5, 10, 6),
    (1, 9, 8, 1, 8, 11, 1, 11, 2, 5, 10, 6),
    (1, 3, 11, 1, 11, 6, 1, 6, 5),
    (0, 8, 11, 0, 11, 6, 0, 6, 5, 0, 5, 1),
    (0, 3, 11, 0, 11, 6, 0, 6, 5, 0, 5, 9),
    (5, 9, 8, 5, 8, 11, 5, 11, 6),
    (4, 7, 8, 5, 10, 6),
    (0, 4, 7, 0, 7, 3, 5, 10, 6),
    (0, 1, 9, 4, 7, 8, 5, 10, 6),
    (1, 9, 4, 1, 4, 7, 1, 7, 3, 5, 10, 6),
    (1, 2, 6, 1, 6, 5, 4, 7, 8),
    (0, 4, 7, 0, 7, 3, 1, 2, 6, 1, 6, 5),
    (0, 2, 6, 0, 6, 5, 0, 5, 9, 4, 7, 8),
    (2, 6, 5, 2, 5, 9, 2, 9, 4, 2, 4, 7, 2, 7, 3),
    (2, 3, 11, 4, 7, 8, 5, 10, 6),
    (0, 4, 7, 0, 7, 11, 0, 11, 2, 5, 10, 6),
    (0, 1, 9, 2, 3, 11, 4, 7, 8, 5, 10, 6),
    (1, 9, 4, 1, 4, 7, 1, 7, 11, 1, 11, 2, 5, 10, 6),
    (1, 3, 11, 1, 11, 6, 1, 6, 5, 4, 7, 8),
    (0, 4, 7, 0, 7, 11, 0, 11, 6, 0, 6, 5, 0, 5, 1),
    (0, 3, 11, 0, 11, 6, 0, 6, 5, 0, 5, 9, 4, 7, 8),
    (11, 6, 5, 11, 5, 9, 11, 9, 4, 11, 4, 7),
    (4, 9, 10, 4, 10, 6),
    (0, 8, 3, 4, 9, 10, 4, 10, 6),
    (0, 1, 10, 0, 10, 6, 0, 6, 4),
    (1, 10, 6, 1, 6, 4, 1, 4, 8, 1, 8, 3),
    (1, 2, 6, 1, 6, 4, 1, 4, 9),
    (0, 8, 3, 1, 2, 6, 1, 6, 4, 1, 4, 9),
    (0, 2, 6, 0, 6, 4),
    (2, 6, 4, 2, 4, 8, 2, 8, 3),
    (2, 3, 11, 4, 9, 10, 4, 10, 6),
    (0, 8, 11, 0, 11, 2, 4, 9, 10, 4, 10, 6),
    (0, 1, 10, 0, 10, 6, 0, 6, 4, 2, 3, 11),
    (1, 10, 6, 1, 6, 4, 1, 4, 8, 1, 8, 11, 1, 11, 2),
    (1, 3, 11, 1, 11, 6, 1, 6, 4, 1, 4, 9),
    (11, 6, 4, 11, 4, 9, 11, 9, 1, 11, 1, 0, 11, 0, 8),
    (0, 3, 11, 0, 11, 6, 0, 6, 4),
    (4, 8, 11, 4, 11, 6),
    (6, 7, 8, 6, 8, 9, 6, 9, 10),
    (0, 9, 10, 0, 10, 6, 0, 6, 7, 0, 7, 3),
    (0, 1, 10, 0, 10, 6, 0, 6, 7, 0, 7, 8),
    (1, 10, 6, 1, 6, 7, 1, 7, 3),
    (1, 2, 6, 1, 6, 7, 1, 7, 8, 1, 8, 9),
    (9, 1, 2, 9, 2, 6, 9, 6, 7, 9, 7, 3, 9, 3, 0),
    (0, 2, 6, 0, 6, 7, 0, 7, 8),
    (2, 6, 7, 2, 7, 3),
    (2, 3, 11, 6, 7, 8, 6, 8, 9, 6, 9, 10),
    (0, 9, 10, 0, 10, 6, 0, 6, 7, 0, 7, 11, 0, 11, 2),
    (0, 1, 10, 0, 10, 6, 0, 6, 7, 0, 7, 8, 2, 3, 11),
    (1, 10, 6, 1, 6, 7, 1, 7, 11, 1, 11, 2),
    (1, 3, 11, 1, 11, 6, 1, 6, 7, 1, 7, 8, 1, 8, 9),
    (0, 9, 1, 6, 7, 11),
    (0, 3, 11, 0, 11, 6, 0, 6, 7, 0, 7, 8),
    (6, 7, 11),
    (6, 11, 7),
    (0, 8, 3, 6, 11, 7),
    (0, 1, 9, 6, 11, 7),
    (1, 9, 8, 1, 8, 3, 6, 11, 7),
    (1, 2, 10, 6, 11, 7),
    (0, 8, 3, 1, 2, 10, 6, 11, 7),
    (0, 2, 10, 0, 10, 9, 6, 11, 7),
    (2, 10, 9, 2, 9, 8, 2, 8, 3, 6, 11, 7),
    (2, 3, 7, 2, 7, 6),
    (0, 8, 7, 0, 7, 6, 0, 6, 2),
    (0, 1, 9, 2, 3, 7, 2, 7, 6),
    (1, 9, 8, 1, 8, 7, 1, 7, 6, 1, 6, 2),
    (1, 3, 7, 1, 7, 6, 1, 6, 10),
    (0, 8, 7, 0, 7, 6, 0, 6, 10, 0, 10, 1),
    (0, 3, 7, 0, 7, 6, 0, 6, 10, 0, 10, 9),
    (6, 10, 9, 6, 9, 8, 6, 8, 7),
    (4, 6, 11, 4, 11, 8),
    (0, 4, 6, 0, 6, 11, 0, 11, 3),
    (0, 1, 9, 4, 6, 11, 4, 11, 8),
    (1, 9, 4, 1, 4, 6, 1, 6, 11, 1, 11, 3),
    (1, 2, 10, 4, 6, 11, 4, 11, 8),
    (0, 4, 6, 0, 6, 11, 0, 11, 3, 1, 2, 10),
    (0, 2, 10, 0, 10, 9, 4, 6, 11, 4, 11, 8),
    (9, 4, 6, 9, 6, 11, 9, 11, 3, 9, 3, 2, 9, 2, 10),
    (2, 3, 8, 2, 8, 4, 2, 4, 6),
    (0, 4, 6, 0, 6, 2),
    (0, 1, 9, 2, 3, 8, 2, 8, 4, 2, 4, 6),
    (1, 9, 4, 1, 4, 6, 1, 6, 2),
    (1, 3, 8, 1, 8, 4, 1, 4, 6, 1, 6, 10),
    (0, 4, 6, 0, 6, 10, 0, 10, 1),
    (3, 8, 4, 3, 4, 6, 3, 6, 10, 3, 10, 9, 3, 9, 0),
    (4, 6, 10, 4, 10, 9),
    (4, 9, 5, 6, 11, 7),
    (0, 8, 3, 4, 9, 5, 6, 11, 7),
    (0, 1, 5, 0, 5, 4, 6, 11, 7),
    (1, 5, 4, 1, 4, 8, 1, 8, 3, 6, 11, 7),
    (1, 2, 10, 4, 9, 5, 6, 11, 7),
    (0, 8, 3, 1, 2, 10, 4, 9, 5, 6, 11, 7),
    (0, 2, 10, 0, 10, 5, 0, 5, 4, 6, 11, 7),
    (2, 10, 5, 2, 5, 4, 2, 4, 8, 2, 8, 3, 6, 11, 7),
    (2, 3, 7, 2, 7, 6, 4, 9, 5),
    (0, 8, 7, 0, 7, 6, 0, 6, 2, 4, 9, 5),
    (0, 1, 5, 0, 5, 4, 2, 3, 7, 2, 7, 6),
    (1, 5, 4, 1, 4, 8, 1, 8, 7, 1, 7, 6, 1, 6, 2),
    (1, 3, 7, 1, 7, 6, 1, 6, 10, 4, 9, 5),
    (0, 8, 7, 0, 7, 6, 0, 6, 10, 0, 10, 1, 4, 9, 5),
    (0, 3, 7, 0, 7, 6, 0, 6, 10, 0, 10, 5, 0, 5, 4),
    (8, 7, 6, 8, 6, 10, 8, 10, 5, 8, 5, 4),
    (5, 6, 11, 5, 11, 8, 5, 8, 9),
    (0, 9, 5, 0, 5, 6, 0, 6, 11, 0, 11, 3),
    (0, 1, 5, 0, 5, 6, 0, 6, 11, 0, 11, 8),
    (1, 5, 6, 1, 6, 11, 1, 11, 3),
    (1, 2, 10, 5, 6, 11, 5, 11, 8, 5, 8, 9),
    (0, 9, 5, 0, 5, 6, 0, 6, 11, 0, 11, 3, 1, 2, 10),
    (0, 2, 10, 0, 10, 5, 0, 5, 6, 0, 6, 11, 0, 11, 8),
    (5, 6, 11, 5, 11, 3, 5, 3, 2, 5, 2, 10),
    (2, 3, 8, 2, 8, 9, 2, 9, 5, 2, 5, 6),
    (0, 9, 5, 0, 5, 6, 0, 6, 2),
    (5, 6, 2, 5, 2, 3, 5, 3, 8, 5, 8, 0, 5, 0, 1),
    (1, 5, 6, 1, 6, 2),
    (3, 8, 9, 3, 9, 5, 3, 5, 6, 3, 6, 10, 3, 10, 1),
    (0, 9, 5, 0, 5, 6, 0, 6, 10, 0, 10, 1),
    (0, 3, 8, 5, 6, 10),
    (5, 6, 10),
    (5, 10, 11, 5, 11, 7),
    (0, 8, 3, 5, 10, 11, 5, 11, 7),
    (0, 1, 9, 5, 10, 11, 5, 11, 7),
    (1, 9, 8, 1, 8, 3, 5, 10, 11, 5, 11, 7),
    (1, 2, 11, 1, 11, 7, 1, 7, 5),
    (0, 8, 3, 1, 2, 11, 1, 11, 7, 1, 7, 5),
    (0, 2, 11, 0, 11, 7, 0, 7, 5, 0, 5, 9),
    (2, 11, 7, 2, 7, 5, 2, 5, 9, 2, 9, 8, 2, 8, 3),
    (2, 3, 7, 2, 7, 5, 2, 5, 10),
    (0, 8, 7, 0, 7, 5, 0, 5, 10, 0, 10, 2),
    (0, 1, 9, 2, 3, 7, 2, 7, 5, 2, 5, 10),
    (8, 7, 5, 8, 5, 10, 8, 10, 2, 8, 2, 1, 8, 1, 9),
    (1, 3, 7, 1, 7, 5),
    (0, 8, 7, 0, 7, 5, 0, 5, 1),
    (0, 3, 7, 0, 7, 5, 0, 5, 9),
    (5, 9, 8, 5, 8, 7),
    (4, 5, 10, 4, 10, 11, 4, 11, 8),
    (0, 4, 5, 0, 5, 10, 0, 10, 11, 0, 11, 3),
    (0, 1, 9, 4, 5, 10, 4, 10, 11, 4, 11, 8),
    (4, 5, 10, 4, 10, 11, 4, 11, 3, 4, 3, 1, 4, 1, 9),
    (1, 2, 11, 1, 11, 8, 1, 8, 4, 1, 4, 5),
    (4, 5, 1, 4, 1, 2, 4, 2, 11, 4, 11, 3, 4, 3, 0),
    (2, 11, 8, 2, 8, 4, 2, 4, 5, 2, 5, 9, 2, 9, 0),
    (2, 11, 3, 4, 5, 9),
    (2, 3, 8, 2, 8, 4, 2, 4, 5, 2, 5, 10),
    (0, 4, 5, 0, 5, 10, 0, 10, 2),
    (0, 1, 9, 2, 3, 8, 2, 8, 4, 2, 4, 5, 2, 5, 10),
    (4, 5, 10, 4, 10, 2, 4, 2, 1, 4, 1, 9),
    (1, 3, 8, 1, 8, 4, 1, 4, 5),
    (0, 4, 5, 0, 5, 1),
    (3, 8, 4, 3, 4, 5, 3, 5, 9, 3, 9, 0),
    (4, 5, 9),
    (4, 9, 10, 4, 10, 11, 4, 11, 7),
    (0, 8, 3, 4, 9, 10, 4, 10, 11, 4, 11, 7),
    (0, 1, 10, 0, 10, 11, 0, 11, 7, 0, 7, 4),
    (1, 10, 11, 1, 11, 7, 1, 7, 4, 1, 4, 8, 1, 8, 3),
    (1, 2, 11, 1, 11, 7, 1, 7, 4, 1, 4, 9),
    (0, 8, 3, 1, 2, 11, 1, 11, 7, 1, 7, 4, 1, 4, 9),
    (0, 2, 11, 0, 11, 7, 0, 7, 4),
    (2, 11, 7, 2, 7, 4, 2, 4, 8, 2, 8, 3),
    (2, 3, 7, 2, 7, 4, 2, 4, 9, 2, 9, 10),
    (7, 4, 9, 7, 9, 10, 7, 10, 2, 7, 2, 0, 7, 0, 8),
    (10, 2, 3, 10, 3, 7, 10, 7, 4, 10, 4, 0, 10, 0, 1),
    (1, 10, 2, 4, 8, 7),
    (1, 3, 7, 1, 7, 4, 1, 4, 9),
    (7, 4, 9, 7, 9, 1, 7, 1, 0, 7, 0, 8),
    (0, 3, 7, 0, 7, 4),
    (4, 8, 7),
    (8, 9, 10, 8, 10, 11),
    (0, 9, 10, 0, 10, 11, 0, 11, 3),
    (0, 1, 10, 0, 10, 11, 0, 11, 8),
    (1, 10, 11, 1, 11, 3),
    (1, 2, 11, 1, 11, 8, 1, 8, 9),
    (9, 1, 2, 9, 2, 11, 9, 11, 3, 9, 3, 0),
    (0, 2, 11, 0, 11, 8),
    (2, 11, 3),
    (2, 3, 8, 2, 8, 9, 2, 9, 10),
    (0, 9, 10, 0, 10, 2),
    (10, 2, 3, 10, 3, 8, 10, 8, 0, 10, 0, 1),
    (1, 10, 2),
    (1, 3, 8, 1, 8, 9),
    (0, 9, 1),
    (0, 3, 8),
    (),
)


def _edge_geometry():
    """per cube edge: (lower-corner offset, axis)"""
    out = []
    for a, b in EDGES:
        ca, cb = CORNERS[a], CORNERS[b]
        axis = [d for d in range(3) if ca[d] != cb[d]][0]
        assert cb[axis] == ca[axis] + 1
        out.append((ca, axis))
    return tuple(out)


EDGE_GEOMETRY = _edge_geometry()


def marching_cubes(u, level=0.0):
    """-> (vertices float32 [V,3], faces int32 [F,3]) by the contract above."""
    u = np.ascontiguousarray(u, dtype=np.float32)
    assert u.ndim == 3 and min(u.shape) >= 1
    nx, ny, nz = u.shape
    lv = np.float32(level)
    below = u < lv
    # crossing edges, owned by their lower endpoint: cross[i, j, k, axis]
    cross = np.zeros(u.shape + (3,), dtype=bool)
    cross[:-1, :, :, 0] = below[:-1] != below[1:]
    cross[:, :-1, :, 1] = below[:, :-1] != below[:, 1:]
    cross[:, :, :-1, 2] = below[:, :, :-1] != below[:, :, 1:]
    flat = cross.reshape(-1)
    vid = np.full(flat.shape, -1, dtype=np.int64)
    vid[flat] = np.arange(int(flat.sum()), dtype=np.int64)     # (point, axis) order = the contract's vertex order
    vid = vid.reshape(cross.shape)
    pi, pj, pk, pa = np.nonzero(cross)                          # C order: ascending point, then axis
    lo = np.stack([pi, pj, pk], 1)
    hi = lo.copy()
    hi[np.arange(len(pa)), pa] += 1
    u0 = u[lo[:, 0], lo[:, 1], lo[:, 2]]
    u1 = u[hi[:, 0], hi[:, 1], hi[:, 2]]
    with np.errstate(invalid="ignore", divide="ignore"):
        t = (lv - u0) / (u1 - u0)
    verts = lo.astype(np.float32)
    a0 = lo[np.arange(len(pa)), pa].astype(np.float32)
    a1 = hi[np.arange(len(pa)), pa].astype(np.float32)
    with np.errstate(invalid="ignore"):
        verts[np.arange(len(pa)), pa] = a0 + t * (a1 - a0)
    if nx < 2 or ny < 2 or nz < 2:
        return verts, np.zeros((0, 3), dtype=np.int32)
    case = np.zeros((nx - 1, ny - 1, nz - 1), dtype=np.int64)
    for c, (dx, dy, dz) in enumerate(CORNERS):
        case |= below[dx:nx - 1 + dx, dy:ny - 1 + dy, dz:nz - 1 + dz].astype(np.int64) << c
    ci, cj, ck = np.nonzero(np.ones(case.shape, dtype=bool))    # cubes in ascending linear index of the lowest corner
    cs = case[ci, cj, ck]
    faces = []
    for n in range(len(cs)):
        entry = TRI_TABLE[cs[n]]
        for e in entry:
            (ox, oy, oz), axis = EDGE_GEOMETRY[e]
            faces.append(vid[ci[n] + ox, cj[n] + oy, ck[n] + oz, axis])
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    assert (f >= 0).all()
    return verts, f.astype(np.int32)


_PLY_TYPES = {"char": "i1", "uchar": "u1", "short": "<i2", "ushort": "<u2", "int": "<i4", "uint": "<u4",
              "float": "<f4", "double": "<f8"}


def read_ply(path):
    """Binary little-endian PLY with a vertex element (x, y, z, optional red, green, blue) and triangles as a counted
    list -> (vertices float64 [V,3], faces int64 [F,3], colours uint8 [V,3] or None).  Independent of Mesh.export."""
    data = open(path, "rb").read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    elements, cur = [], None
    for ln in lines[2:]:
        tok = ln.split()
        if not tok:
            continue
        if tok[0] == "element":
            cur = [tok[1], int(tok[2]), []]
            elements.append(cur)
        elif tok[0] == "property":
            cur[2].append(tok[1:])
    off = end
    out = {}
    for name, count, props in elements:
        if props[0][0] == "list":
            cnt_t, idx_t = _PLY_TYPES[props[0][1]], _PLY_TYPES[props[0][2]]
            dt = np.dtype([("n", cnt_t), ("v", idx_t, (3,))])
        else:
            dt = np.dtype([(p[1], _PLY_TYPES[p[0]]) for p in props])
        arr = np.frombuffer(data, dtype=dt, count=count, offset=off)
        off += dt.itemsize * count
        out[name] = arr
    assert off == len(data)
    v = out["vertex"]
    verts = np.stack([v["x"], v["y"], v["z"]], 1).astype(np.float64).reshape(-1, 3)
    cols = np.stack([v["red"], v["green"], v["blue"]], 1).reshape(-1, 3) if "red" in v.dtype.names else None
    assert (out["face"]["n"] == 3).all()
    return verts, out["face"]["v"].astype(np.int64).reshape(-1, 3), cols

"""Small conforming meshes of irregular valence (test helper).

`box_mesh` gives every edge 4 elements and every vertex 8, and `rotmesh` keeps that.  `star_mesh` builds what an O-grid
around a body looks like to the gather-scatter and to everything assembled through it: a fan of k quads around a centre
vertex (valence k), closed by a ring of 2k quads whose inner vertices alternate between valence 3 and 4, extruded in z.
In 3-D its edges are then shared by 3, 4 and k elements, its vertices by 6, 8 and 2k, and neighbouring elements do not
share an orientation (every element lists its corners counter-clockwise starting from its own first corner).

Element order inside a layer: fan element j is followed by its two ring elements 2j and 2j + 1, so a contiguous block
partition cuts through the fan; the layers follow one another.
"""
from __future__ import annotations

import numpy as np

from neklab_amd import nekio
from neklab_amd.mesh import BoxMesh, gll_points


def base_quads(k):
    """-> (xy (nv, 2) vertex coordinates, quads (3k, 4) vertex ids, counter-clockwise).  Vertex 0 is the centre C, 1 + i is
    P_i, 1 + 2k + i is Q_i = 2 P_i; P_i sits at angle 2 pi i / (2k) + 0.1, radius 1 (even i) or 1.15 (odd i)."""
    if k < 3:
        raise ValueError("star_mesh: the fan needs k >= 3 elements")
    m = 2 * k
    ang = 2.0 * np.pi * np.arange(m) / m + 0.1
    rad = np.where(np.arange(m) % 2 == 1, 1.15, 1.0)
    P = np.stack([rad * np.cos(ang), rad * np.sin(ang)], axis=1)
    xy = np.concatenate([np.zeros((1, 2)), P, 2.0 * P])
    p = lambda i: 1 + i % m
    q = lambda i: 1 + m + i % m
    quads = []
    for j in range(k):
        quads.append((0, p(2 * j), p(2 * j + 1), p(2 * j + 2)))
        for i in (2 * j, 2 * j + 1):
            quads.append((p(i), q(i), q(i + 1), p(i + 1)))
    return xy, np.array(quads, dtype=np.int64)


def star_mesh(k, n, nz, periodic_z=False, deform=0.03):
    """The star mesh of k fan elements with n GLL points per direction: 2-D (nz = 0) or nz layers of height 1 in z."""
    nz = int(nz)
    if nz < 0:
        raise ValueError("star_mesh: nz >= 0")
    if periodic_z and nz < 3:
        # with two layers the four elements around a vertical face of the periodic mesh carry the same four vertex ids on it:
        # labels built from vertex ids (nekio.glo_num_from_vertices, Nek5000's set_vert) cannot tell the two faces apart
        raise ValueError("star_mesh: periodic_z needs nz >= 3 (vertex-based labels are ambiguous with fewer layers)")
    xy, quads = base_quads(k)
    nv, nq = len(xy), len(quads)
    dim = 2 if nz == 0 else 3
    xi = 0.5 * (gll_points(n) + 1.0)                                     # [0, 1]
    sym = quads[:, [0, 1, 3, 2]]                                         # symmetric corner order, r fastest
    c = xy[sym]                                                          # (nq, 4, 2)
    r, s = xi[None, None, :], xi[None, :, None]                          # point (is, ir)
    w = [(1 - r) * (1 - s), r * (1 - s), (1 - r) * s, r * s]
    X2 = sum(w[q] * c[:, q, 0][:, None, None] for q in range(4))         # (nq, n, n): bilinear map, straight sides
    Y2 = sum(w[q] * c[:, q, 1][:, None, None] for q in range(4))
    if dim == 2:
        vert, X, Y, Z = sym, X2, Y2, None
        fx = 1.0
    else:
        nlev = nz if periodic_z else nz + 1
        vert = np.concatenate([np.concatenate([sym + nv * l, sym + nv * ((l + 1) % nlev)], axis=1) for l in range(nz)])
        X = np.tile(X2[:, None, :, :], (nz, n, 1, 1))
        Y = np.tile(Y2[:, None, :, :], (nz, n, 1, 1))
        Z = np.concatenate([np.broadcast_to((l + xi)[None, :, None, None], (nq, n, n, n)) for l in range(nz)]).copy()
        fx = 1.0 + 0.3 * np.cos(2.0 * np.pi * Z / nz)
    E = len(vert)
    # smooth deformation as a function of the undeformed coordinates: coincident points stay coincident
    Xd = X + deform * np.sin(1.3 * Y + 0.2) * fx
    Yd = Y + deform * np.sin(1.1 * X - 0.4)
    glo = nekio.glo_num_from_vertices(vert, n, dim)
    # walls: every face without a partner; all points that carry a label of such a face
    faces = {}
    for e in range(E):
        for d in range(dim):
            for side in (0, 1):
                ids = tuple(sorted(int(vert[e, q]) for q in range(1 << dim) if ((q >> d) & 1) == side))
                faces.setdefault(ids, []).append((e, d, side))
    g = glo.reshape((E,) + (n,) * dim)
    wall_labels = []
    for owners in faces.values():
        if len(owners) > 2:
            raise ValueError("star_mesh: a face is shared by %d elements" % len(owners))
        if len(owners) == 1:
            e, d, side = owners[0]
            wall_labels.append(np.take(g[e], (n - 1) if side else 0, axis=dim - 1 - d).ravel())
    wall = np.isin(glo, np.unique(np.concatenate(wall_labels)))
    m = np.where(wall, 0.0, 1.0)
    flat = lambda a: None if a is None else np.ascontiguousarray(a.reshape(E, -1), dtype=np.float64)
    return BoxMesh(dim=dim, n=n, nel=(nq,) + ((nz,) if dim == 3 else ()), x=flat(Xd), y=flat(Yd), z=flat(Z),
                   glo_num=np.ascontiguousarray(glo), mask=[m.copy() for _ in range(dim)], tmask=m.copy(),
                   periodic=(False,) * (dim - 1) + (bool(periodic_z),), lengths=(), has_outflow=False,
                   elem_gid=np.arange(E, dtype=np.int64), extra={"vert": vert, "k": k, "nz": nz})


def multiplicities(glo):
    """{copies per global dof: number of such dofs} of a labelling."""
    cnt = np.bincount(np.asarray(glo).ravel())
    c, n = np.unique(cnt[cnt > 0], return_counts=True)
    return {int(a): int(b) for a, b in zip(c, n)}


def labels_from_coordinates(hm, fold_z=None, decimals=9):
    """Labels built independently of the vertex ids: points with equal rounded coordinates share one.  fold_z: the period in z
    (the top plane is folded onto the bottom plane first)."""
    cs = [hm.x, hm.y] + ([hm.z] if hm.dim == 3 else [])
    cs = [np.asarray(c, dtype=np.float64).ravel().copy() for c in cs]
    if fold_z is not None:
        cs[2] = np.where(np.abs(cs[2] - fold_z) < 1e-12, 0.0, cs[2])
        # x depends on z through cos(2 pi z / nz): identical on the two planes up to rounding, which the rounding below absorbs
    key = np.round(np.stack(cs, axis=1), decimals) + 0.0
    _, inv = np.unique(key, axis=0, return_inverse=True)
    return inv.reshape(hm.glo_num.shape)

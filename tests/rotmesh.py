"""Meshes with rotated elements (test helper).

`box_mesh` gives every element the same orientation: local r, s, t along +x, +y, +z.  Meshes read from Nek5000 files
(`nekio.read_re2`, `glo_num_from_vertices`) can hold elements in any of the 24 proper orientations of the index cube
(4 in 2-D).  `rotate_elements` gives chosen elements of a box mesh a seeded proper rotation of their local index cube and
permutes every per-point array with it, so that the rotated mesh describes the same discrete problem in another
numbering; `Rotated.fwd1` / `fwd2` carry a field of the aligned mesh over to it.
"""
from __future__ import annotations

import itertools
from dataclasses import replace

import numpy as np

from neklab_amd import nekio


def proper_rotations(dim):
    """(perm, flip) pairs of the orientation-preserving symmetries of the index cube: local index i'[perm[d]] of the new
    element runs along old direction d, reversed when flip[d].  24 in 3-D, 4 in 2-D."""
    out = []
    for perm in itertools.permutations(range(dim)):
        sgn = np.linalg.det(np.eye(dim)[list(perm)])
        for flip in itertools.product((False, True), repeat=dim):
            if sgn * (-1) ** sum(flip) > 0:
                out.append((perm, flip))
    return out


def source_index(m, dim, perm, flip):
    """src[p_new] = p_old for an element with m points per direction (x fastest)."""
    src = np.empty(m ** dim, dtype=np.int64)
    for pn in range(m ** dim):
        inew = [(pn // m ** d) % m for d in range(dim)]
        iold = [inew[perm[d]] if not flip[d] else m - 1 - inew[perm[d]] for d in range(dim)]
        src[pn] = sum(iold[d] * m ** d for d in range(dim))
    return src


class Rotated:
    """A box mesh with rotated elements and the maps between the two numberings."""

    def __init__(self, hm, elems=None, seed=0, rots=None):
        dim, n = hm.dim, hm.n
        self.aligned = hm
        E = hm.E
        rng = np.random.default_rng(seed)
        allr = proper_rotations(dim)
        if elems is None:
            elems = np.arange(E)
        self.rot = [None] * E
        for e in elems:
            self.rot[int(e)] = allr[int(rng.integers(len(allr)))] if rots is None else allr[rots[int(e)] % len(allr)]
        self.src1 = np.tile(np.arange(n ** dim), (E, 1))
        self.src2 = np.tile(np.arange((n - 2) ** dim), (E, 1))
        for e in range(E):
            if self.rot[e] is not None:
                self.src1[e] = source_index(n, dim, *self.rot[e])
                self.src2[e] = source_index(n - 2, dim, *self.rot[e])
        f = self.fwd1
        self.mesh = replace(hm, x=f(hm.x), y=f(hm.y), z=None if hm.z is None else f(hm.z),
                            glo_num=f(hm.glo_num), mask=[f(m) for m in hm.mask], tmask=f(hm.tmask), extra=dict(hm.extra))

    def _take(self, a, src):
        a = np.asarray(a)
        E = self.aligned.E
        flat = a.reshape(E, -1)
        return np.take_along_axis(flat, src, axis=1).reshape(a.shape)

    def fwd1(self, u):
        """velocity-mesh field of the aligned mesh -> the same field in the rotated numbering"""
        return self._take(u, self.src1)

    def fwd2(self, p):
        """pressure-mesh field, likewise"""
        return self._take(p, self.src2)

    def vertex_ids(self):
        """(E, 2**dim) global vertex ids of the rotated mesh's elements, symmetric corner order (x fastest)."""
        hm = self.mesh
        n, dim = hm.n, hm.dim
        corners = []
        for c in range(1 << dim):
            ijk = [(n - 1) if (c >> d) & 1 else 0 for d in range(3)]
            corners.append(ijk[0] + n * (ijk[1] + n * ijk[2]))
        return hm.glo_num[:, corners]

    def labels_from_vertices(self):
        """The rotated mesh's labels built as a Nek5000 reader builds them: nekio.glo_num_from_vertices."""
        return nekio.glo_num_from_vertices(self.vertex_ids(), self.mesh.n, self.mesh.dim)


def same_grouping(a, b):
    """True when two labellings put the local points into the same groups."""
    a, b = np.asarray(a).ravel(), np.asarray(b).ravel()
    pairs = np.unique(np.stack([a, b]), axis=1).shape[1]
    return pairs == len(np.unique(a)) == len(np.unique(b))

// Host arithmetic of the wall forces (forces.hip: nlg_forces_create): the geometry of the listed faces at their GLL points.  Standard
// C++ only: it compiles and runs without a GPU (nlg_forces_geometry through ctypes, tests/cpp/forces_host_main.cpp).
//
// A face is (element, face), face in the preprocessor's numbering 1 = s-, 2 = r+, 3 = s+, 4 = r-, 5 = t-, 6 = t+.  It is normal to
// reference direction a on side sigma; its n^(dim-1) points are numbered with the lower tangential direction fastest.  Per face point q:
//   N_q    = sigma (J grad r_a)_q w_q      the area-weighted outward normal, w_q = the GLL weights of the tangential directions
//   G_q    = (d r_j / d x_i)_q             [j][i], what turns reference derivatives into the pointwise gradient
//   x_q - c                                c = the centre of the face's object
#pragma once
#include <cstdint>

namespace nlg {
namespace forces {

constexpr int kMaxN = 16;   // lx1 the tables are sized for (probe::kMaxN)

// constexpr: the kernels of forces.hip call them too
constexpr int face_dir(int face) { return face == 1 || face == 3 ? 1 : (face == 2 || face == 4 ? 0 : 2); }
constexpr int face_side(int face) { return face == 2 || face == 3 || face == 6 ? +1 : -1; }
constexpr int face_points(int dim, int n) { return dim == 3 ? n * n : n; }
constexpr int nquant(int dim) { return 2 * dim + 2 * (dim == 3 ? 3 : 1) + 1; }   // Fp, Fv, Tp, Tv, Q

void gll_weights(int n, const double *z, double *w);
void deriv_matrix(int n, const double *z, double *D);   // D[i * n + m] = l_m'(z_i)
// M[i * n2 + k] = l_k(z1_i) of the Lagrange basis on the n2 Gauss points: the pressure mesh carried to the GLL points
void gl_to_gll(int n, const double *z1, int n2, const double *z2, double *M);

// X[c]: coordinate fields [E][n^dim] on the GLL nodes z[n].  elem[f]: local element, face[f] in 1..2 dim, obj[f] in 0..nobj-1 (null: all 0);
// centre: [nobj][dim] or null (0).  Out, any may be null: nds [nfaces][nfp][dim], met [nfaces][nfp][dim * dim] (index j * dim + i),
// xc [nfaces][nfp][dim], area [nobj] = sum |N_q| (accumulated face by face in the order given).  1: bad argument.
int geometry(int dim, int n, const double *z, int64_t E, const double *const X[3], int64_t nfaces, const int64_t *elem, const int *face,
             const int *obj, int nobj, const double *centre, double *nds, double *met, double *xc, double *area);

}  // namespace forces
}  // namespace nlg

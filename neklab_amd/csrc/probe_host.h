// Host arithmetic of the history points (probe.hip: nlg_probes_create): the 1-D nodes, the Lagrange weights in barycentric
// form and the point location on the isoparametric elements.  Standard C++ only: it compiles and runs without a GPU
// (nlg_probe_locate through ctypes, tests/cpp/probe_host_main.cpp).
#pragma once
#include <cstdint>

namespace nlg {
namespace probe {

constexpr int kMaxN = 16;          // lx1 the tables are sized for
constexpr int kNewtonMax = 50;     // iterations of the location's Newton loop
constexpr double kNewtonStop = 1e-13;
constexpr double kClamp = 1.5;     // every iterate stays in [-kClamp, kClamp]
constexpr double kBoxGrow = 0.1;   // candidates: the GLL-node bounding box grown by this share of its extent

void gll_nodes(int n, double *z);   // Gauss-Lobatto-Legendre nodes on [-1, 1]
void gl_nodes(int n, double *z);    // Gauss-Legendre nodes
void bary_weights(int n, const double *z, double *bw);
// w[j] = l_j(r), dw[j] = l_j'(r) (dw may be null) of the Lagrange basis on z.  At a node the rule is exact: 1 there, 0 elsewhere.
void lagrange(int n, const double *z, const double *bw, double r, double *w, double *dw);

// nlg_probe_locate (include/neklab_gpu.h) on given GLL nodes z[n]: X[c] = the coordinate fields [E][n^dim], lglel null = 0 .. E-1.
// key (may be null): the point's rank among the holders, smaller wins = global element id, + 2^40 for a status-1 holder; -1: none.
int locate(int dim, int n, const double *z, int64_t E, const double *const X[3], const int64_t *lglel, int64_t npts, const double *xyz,
           double tol_r, int64_t *elem, double *rst, int *status, double *dist, double *key);

}  // namespace probe
}  // namespace nlg

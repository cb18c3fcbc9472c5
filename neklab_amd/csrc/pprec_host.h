// Host arithmetic of the pressure preconditioner's set-up (pprec.hip: pprec_setup), one free function per stage, in the
// order the driver runs them.  Standard C++ only: the stages compile and run without a GPU (tests/cpp/pprec_host_main.cpp)
// and mirror the stages of oracle/pprec.py (_lengths, _setup_local, ext_line / _setup_overlap, _neighbours,
// _setup_coarse, _aggregate).  A stage returns non-zero on failure and leaves the message in `err`.
#pragma once
#include <cstdint>
#include <string>
#include <unordered_map>
#include <vector>

namespace nlg {
namespace pph {

struct Shape {   // one rank's part of the mesh
    int dim = 3, n = 0, n2 = 0;   // lx1, lx2
    int64_t E = 0;
    int np1() const { return dim == 3 ? n * n * n : n * n; }
    int np2() const { return dim == 3 ? n2 * n2 * n2 : n2 * n2; }
    int ncorner() const { return 1 << dim; }
};

struct Ops {   // the 1-D operators the stages read
    const double *w1 = nullptr, *w2 = nullptr;     // GLL / GL weights
    const double *D12 = nullptr, *I12 = nullptr;   // n2 x n derivative / interpolation GLL -> GL
};

// ---- edge lengths and end-point factors
struct Lengths {
    std::vector<double> Lall;     // [E][3] distance between the centres of opposite faces
    std::vector<double> endfac;   // [E][3][side] end-point factor of the 1-D mass: 0 at a wall, vmult elsewhere
};
void edge_lengths(const Shape &s, const double *const X[3], const double *const mask[3], const double *vmult, Lengths &L);

// ---- element-local fast diagonalisation
struct LocalFdm {
    std::vector<double> S;        // [E][3][n2*n2] eigenvector matrices
    std::vector<double> invden;   // [E][n2^dim] 1 / (sum of eigenvalues), zero below 1e-12 of the largest sum
};
int local_fdm(const Shape &s, const Ops &o, const Lengths &L, LocalFdm &F, std::string &err);

// ---- extended lines left neighbour | element | right neighbour
// every element's normal edge length on the interior points of its faces: summed by the gather-scatter, the sum minus
// the own value is the neighbour's
void face_lengths(const Shape &s, const Lengths &L, std::vector<double> &hw);
struct ExtLines {
    std::vector<double> Sx, lamx;   // [E][3][n*n], [E][3][n]
    std::vector<double> wq;         // [E][n2^dim] count^-1/2
    std::vector<char> hasnb;        // [E][2 dd + side]: the face has a neighbour (on this rank or another)
    double thrx = 0.0;              // zero-denominator threshold
};
int extended_lines(const Shape &s, const Ops &o, const Lengths &L, const std::vector<double> &hw_summed, ExtLines &X, std::string &err);

// ---- overlap destinations
// pidx: the two-copy groups of the gather-scatter in the layout of Wret (3-D: face-grouped, 2-D: natural)
struct OverlapDest {
    std::vector<int> pin, pret;   // [E][2 dim n2^(dim-1)], -1 = none
};
int overlap_destinations(const Shape &s, const std::vector<int> &pidx, const std::vector<char> &hasnb, bool halo_active, OverlapDest &D,
                         std::string &err);

// ---- coarse topology
struct CoarseTopo {
    int nvert = 0, ncol = 0;
    std::vector<int> vg;                 // [E][ncorner] vertex of every element corner
    std::vector<int> vp, vi;             // vertex -> incident (element * ncorner + corner) entries, CSR
    std::vector<std::vector<int>> adj;   // element -> elements that share a vertex with it (itself included), ascending
    std::vector<int> colour;             // two elements of one colour have no common neighbour
};
void coarse_topology(const Shape &s, const int64_t *glo, CoarseTopo &T);
// the vertices that hold one of the points `cidx` (local velocity dofs that another rank shares)
void boundary_vertices(const Shape &s, const CoarseTopo &T, const std::vector<int> &cidx, std::vector<char> &viface);

// ---- coarse-operator rows
typedef std::vector<std::unordered_map<int, double>> ProbedRows;   // [nvert] column -> sum of the probed values
struct CoarseCsr {
    std::vector<int> rp, ci;
    std::vector<double> av;
    std::vector<double> dinv;   // 1 / diagonal
};
void coarse_rows(ProbedRows &rows, CoarseCsr &A);

// ---- aggregation
// agg[v] = aggregate of vertex v; returns the number of aggregates.  At most exact_max vertices: every vertex is its own.
// iface: several ranks, the vertices flagged in viface lie on a rank boundary (their A.dinv is then zeroed)
int aggregate(const Shape &s, const CoarseTopo &T, CoarseCsr &A, int exact_max, bool iface, const std::vector<char> &viface, std::vector<int> &agg);

// ---- aggregate-level operator
struct AggLevel {
    int na = 0;
    std::vector<double> Acc;   // [na][na]
    std::vector<int> ap, am;   // aggregate -> its vertices, CSR
};
void assemble_acc(const CoarseCsr &A, const std::vector<int> &agg, int na, bool shift_null_space, AggLevel &G);

}  // namespace pph
}  // namespace nlg

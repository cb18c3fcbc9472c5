// Runs the host stages of the pressure preconditioner's set-up (neklab_amd/csrc/pprec_host.cpp) on a mesh read from a flat
// binary file and writes every stage's output to another: tests/test_cpu_pprec_setup.py compares them with oracle/pprec.py.
// Links pprec_host.cpp and nothing else; needs no GPU.
//
//   pprec_host_main IN OUT
//
// IN : int64 dim, n, E, has_outflow, have_hw, npairs, ncoo, exact_max
//      double X[dim][E np1], mask[dim][E np1], vmult[E np1], w1[n], w2[n2], z2[n2], D12[n2 n], I12[n2 n]; int64 glo[E np1]
//      have_hw: double hw[E np1] (the gather-scatter sum of the field "face_len" of a first run);
//               int32 pairs[npairs][2] (the two-copy groups of glo, natural indices)
//      ncoo > 0: int32 row[ncoo], col[ncoo]; double val[ncoo]  (the coarse operator, as the probing would leave it)
// OUT: records { char name[16]; int64 kind (0 double, 1 int32, 2 char); int64 count; data }
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "fg_slot.h"
#include "pprec_host.h"

using namespace nlg::pph;

static FILE *fin, *fout;

template <typename T>
static std::vector<T> rd(size_t count) {
    std::vector<T> v(count);
    if (count && fread(v.data(), sizeof(T), count, fin) != count) {
        fprintf(stderr, "pprec_host_main: input file too short\n");
        exit(2);
    }
    return v;
}
template <typename T>
static void wr(const char *name, const std::vector<T> &v) {
    char nm[16] = {};
    strncpy(nm, name, 15);
    const int64_t kind = sizeof(T) == 8 ? 0 : (sizeof(T) == 4 ? 1 : 2), count = (int64_t)v.size();
    fwrite(nm, 1, 16, fout);
    fwrite(&kind, 8, 1, fout);
    fwrite(&count, 8, 1, fout);
    if (count) fwrite(v.data(), sizeof(T), v.size(), fout);
}
static void die(const std::string &err) {
    fprintf(stderr, "%s\n", err.c_str());
    exit(1);
}

int main(int argc, char **argv) {
    if (argc != 3 || !(fin = fopen(argv[1], "rb")) || !(fout = fopen(argv[2], "wb"))) {
        fprintf(stderr, "usage: pprec_host_main IN OUT\n");
        return 2;
    }
    const std::vector<int64_t> h = rd<int64_t>(8);
    Shape s;
    s.dim = (int)h[0], s.n = (int)h[1], s.n2 = s.n - 2, s.E = h[2];
    const bool has_outflow = h[3] != 0, have_hw = h[4] != 0;
    const int64_t npairs = h[5], ncoo = h[6];
    const int exact_max = (int)h[7];
    const int dim = s.dim, n = s.n, n2 = s.n2;
    const size_t lvn = (size_t)s.E * s.np1();
    std::vector<double> Xv[3], Mv[3];
    for (int c = 0; c < dim; ++c) Xv[c] = rd<double>(lvn);
    for (int c = 0; c < dim; ++c) Mv[c] = rd<double>(lvn);
    const double *X[3] = {Xv[0].data(), Xv[1].data(), Xv[2].data()}, *msk[3] = {Mv[0].data(), Mv[1].data(), Mv[2].data()};
    const std::vector<double> vmult = rd<double>(lvn), w1 = rd<double>(n), w2 = rd<double>(n2), z2 = rd<double>(n2);
    const std::vector<double> D12 = rd<double>((size_t)n2 * n), I12 = rd<double>((size_t)n2 * n);
    const std::vector<int64_t> glo = rd<int64_t>(lvn);
    const Ops o = {w1.data(), w2.data(), D12.data(), I12.data()};   // (z2 only makes the hats of the driver)
    std::string err;

    Lengths L;
    LocalFdm F;
    edge_lengths(s, X, msk, vmult.data(), L);
    if (local_fdm(s, o, L, F, err)) die(err);
    std::vector<double> hw0;
    face_lengths(s, L, hw0);
    wr("Lall", L.Lall), wr("endfac", L.endfac), wr("S", F.S), wr("invden", F.invden), wr("face_len", hw0);

    if (have_hw) {
        const std::vector<double> hw = rd<double>(lvn);
        std::vector<int> pidx = rd<int>((size_t)2 * npairs);
        if (dim == 3)   // the layout of the return array: face-grouped
            for (int &i : pidx) {
                const int p = i % s.np1();
                i = i / s.np1() * s.np1() + fg_slot(n, p % n, (p / n) % n, p / (n * n));
            }
        ExtLines Xl;
        OverlapDest D;
        if (extended_lines(s, o, L, hw, Xl, err)) die(err);
        if (overlap_destinations(s, pidx, Xl.hasnb, false, D, err)) die(err);
        wr("Sx", Xl.Sx), wr("lamx", Xl.lamx), wr("wq", Xl.wq), wr("hasnb", Xl.hasnb), wr("thrx", std::vector<double>(1, Xl.thrx));
        wr("pin", D.pin), wr("pret", D.pret);
    }

    CoarseTopo T;
    coarse_topology(s, glo.data(), T);
    std::vector<int> adjp(1, 0), adji;
    for (const auto &a : T.adj) {
        adji.insert(adji.end(), a.begin(), a.end());
        adjp.push_back((int)adji.size());
    }
    wr("vg", T.vg), wr("nvert", std::vector<int>(1, T.nvert)), wr("vp", T.vp), wr("vi", T.vi), wr("colour", T.colour);
    wr("ncol", std::vector<int>(1, T.ncol)), wr("adjp", adjp), wr("adji", adji);

    if (ncoo > 0) {
        const std::vector<int> row = rd<int>((size_t)ncoo), col = rd<int>((size_t)ncoo);
        const std::vector<double> val = rd<double>((size_t)ncoo);
        ProbedRows rows((size_t)T.nvert);
        for (int64_t q = 0; q < ncoo; ++q) {
            if (row[q] < 0 || row[q] >= T.nvert || col[q] < 0 || col[q] >= T.nvert) die("pprec_host_main: coarse entry out of range");
            rows[row[q]][col[q]] += val[q];
        }
        CoarseCsr A;
        coarse_rows(rows, A);
        std::vector<int> agg;
        const int na = aggregate(s, T, A, exact_max, false, std::vector<char>((size_t)T.nvert, 0), agg);
        AggLevel G;
        assemble_acc(A, agg, na, !has_outflow, G);
        wr("rp", A.rp), wr("ci", A.ci), wr("av", A.av), wr("dinv", A.dinv), wr("agg", agg), wr("Acc", G.Acc), wr("ap", G.ap), wr("am", G.am);
    }
    fclose(fin);
    return fclose(fout) == 0 ? 0 : 2;
}

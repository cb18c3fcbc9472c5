// Stand-alone driver of the host side of the history points (neklab_amd/csrc/probe_host.cpp), for tests/test_cpu_probe_locate.py: built
// with the host C++ compiler under -fsanitize=address,undefined and run on a tiny mesh read from a flat file.  No GPU, no HIP.
//   in : int64 dim, n, E, npts; double tol_r; double X[dim][E * n^dim]; int64 lglel[E]; double xyz[npts][dim]
//   out: int64 elem[npts]; double rst[npts][dim]; int32 status[npts]; double dist[npts]; then the weights of every located point on the
//        GLL nodes, double w[npts][dim][n] (zeros for a point that was not found)
#include <cstdint>
#include <cstdio>
#include <vector>

#include "neklab_gpu.h"
#include "probe_host.h"

template <typename T>
static bool rd(FILE *f, T *p, size_t n) {
    return fread(p, sizeof(T), n, f) == n;
}

int main(int argc, char **argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: probe_host_main in.bin out.bin\n");
        return 2;
    }
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int64_t hd[4];
    double tol_r;
    if (!rd(f, hd, 4) || !rd(f, &tol_r, 1)) return 2;
    const int dim = (int)hd[0], n = (int)hd[1];
    const int64_t E = hd[2], npts = hd[3];
    if ((dim != 2 && dim != 3) || n < 2 || n > nlg::probe::kMaxN || E < 1 || npts < 1) return 2;
    size_t np = 1;
    for (int d = 0; d < dim; ++d) np *= (size_t)n;
    std::vector<double> X[3];
    for (int c = 0; c < dim; ++c) {
        X[c].resize((size_t)E * np);
        if (!rd(f, X[c].data(), X[c].size())) return 2;
    }
    std::vector<int64_t> lglel((size_t)E);
    std::vector<double> xyz((size_t)npts * dim);
    if (!rd(f, lglel.data(), lglel.size()) || !rd(f, xyz.data(), xyz.size())) return 2;
    fclose(f);

    std::vector<int64_t> elem((size_t)npts);
    std::vector<double> rst((size_t)npts * dim), dist((size_t)npts);
    std::vector<int> status((size_t)npts);
    const int rc = nlg_probe_locate(dim, n, E, X[0].data(), X[1].data(), dim == 3 ? X[2].data() : nullptr, lglel.data(), npts, xyz.data(), tol_r,
                                    elem.data(), rst.data(), status.data(), dist.data());
    if (rc) {
        fprintf(stderr, "nlg_probe_locate returned %d\n", rc);
        return 1;
    }
    // the bad-argument paths
    if (!nlg_probe_locate(4, n, E, X[0].data(), X[1].data(), nullptr, nullptr, npts, xyz.data(), tol_r, elem.data(), rst.data(), status.data(), nullptr) ||
        !nlg_probe_locate(dim, 99, E, X[0].data(), X[1].data(), X[2].data(), nullptr, npts, xyz.data(), tol_r, elem.data(), rst.data(), status.data(), nullptr)) {
        fprintf(stderr, "a bad argument was accepted\n");
        return 1;
    }
    double z[nlg::probe::kMaxN], bw[nlg::probe::kMaxN];
    nlg::probe::gll_nodes(n, z);
    nlg::probe::bary_weights(n, z, bw);
    std::vector<double> w((size_t)npts * dim * n, 0.0);
    for (int64_t p = 0; p < npts; ++p)
        if (status[p] != 2)
            for (int d = 0; d < dim; ++d) nlg::probe::lagrange(n, z, bw, rst[p * dim + d], &w[(p * dim + d) * n], nullptr);

    FILE *g = fopen(argv[2], "wb");
    if (!g) return 2;
    fwrite(elem.data(), sizeof(int64_t), elem.size(), g);
    fwrite(rst.data(), sizeof(double), rst.size(), g);
    fwrite(status.data(), sizeof(int), status.size(), g);
    fwrite(dist.data(), sizeof(double), dist.size(), g);
    fwrite(w.data(), sizeof(double), w.size(), g);
    fclose(g);
    return 0;
}

// Stand-alone driver of the host side of the wall forces (neklab_amd/csrc/forces_host.cpp): built with the host C++ compiler, with
// -fsanitize=address,undefined when memory errors are looked for, and run on small meshes it makes itself.  No GPU, no HIP.
// A cube of 2 x 1 x 1 (3-D) or 2 x 1 (2-D) straight elements, every face of every element listed, at lx1 = 2, 6, 8, 12 and 16: the areas
// must be those of the faces, the normals sum to zero per element, the metrics are the inverse of the constant Jacobian.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "forces_host.h"
#include "neklab_gpu.h"
#include "probe_host.h"

static int run(int dim, int n) {
    const int64_t E = 2;
    const double h[3] = {0.5, 2.0, 3.0};   // element sizes
    double z[nlg::probe::kMaxN];
    nlg::probe::gll_nodes(n, z);
    size_t np = 1;
    for (int d = 0; d < dim; ++d) np *= (size_t)n;
    std::vector<double> X[3];
    for (int c = 0; c < dim; ++c) X[c].resize((size_t)E * np);
    for (int64_t e = 0; e < E; ++e)
        for (size_t p = 0; p < np; ++p) {
            const int i[3] = {(int)(p % n), (int)((p / n) % n), (int)(p / ((size_t)n * n))};
            for (int c = 0; c < dim; ++c) X[c][(size_t)e * np + p] = h[c] * (0.5 * (z[i[c]] + 1.0) + (c == 0 ? (double)e : 0.0));
        }
    const int nfe = 2 * dim;
    const int64_t nf = E * nfe;
    std::vector<int64_t> elem((size_t)nf);
    std::vector<int> face((size_t)nf), obj((size_t)nf);
    for (int64_t f = 0; f < nf; ++f) elem[f] = f / nfe, face[f] = (int)(f % nfe) + 1, obj[f] = (int)(f / nfe);
    const int nfp = nlg::forces::face_points(dim, n);
    std::vector<double> nds((size_t)nf * nfp * dim), met((size_t)nf * nfp * dim * dim), xc((size_t)nf * nfp * dim), area((size_t)E);
    const double centre[6] = {1.0, 2.0, 3.0, -1.0, -2.0, -3.0};
    int rc = nlg_forces_geometry(dim, n, E, X[0].data(), X[1].data(), dim == 3 ? X[2].data() : nullptr, nf, elem.data(), face.data(), obj.data(),
                                 (int)E, centre, nds.data(), met.data(), xc.data(), area.data());
    if (rc) return fprintf(stderr, "dim %d n %d: refused\n", dim, n), 1;
    const double want = dim == 3 ? 2.0 * (h[0] * h[1] + h[0] * h[2] + h[1] * h[2]) : 2.0 * (h[0] + h[1]);
    for (int64_t e = 0; e < E; ++e) {
        if (std::fabs(area[e] - want) > 1e-12 * want) return fprintf(stderr, "dim %d n %d: area %.17g, expected %.17g\n", dim, n, area[e], want), 1;
        double s[3] = {0.0, 0.0, 0.0};
        for (int64_t f = e * nfe; f < (e + 1) * nfe; ++f)
            for (int q = 0; q < nfp; ++q)
                for (int c = 0; c < dim; ++c) s[c] += nds[((size_t)f * nfp + q) * dim + c];
        for (int c = 0; c < dim; ++c)
            if (std::fabs(s[c]) > 1e-12 * want) return fprintf(stderr, "dim %d n %d: the normals of element %lld do not sum to 0\n", dim, n, (long long)e), 1;
    }
    for (size_t q = 0; q < (size_t)nf * nfp; ++q)
        for (int j = 0; j < dim; ++j)
            for (int i = 0; i < dim; ++i) {
                const double g = met[q * dim * dim + j * dim + i], w = i == j ? 2.0 / h[i] : 0.0;
                if (std::fabs(g - w) > 1e-11) return fprintf(stderr, "dim %d n %d: metric %d %d = %.17g, expected %.17g\n", dim, n, j, i, g, w), 1;
            }
    // null outputs, no object list, no centre; then the refusals
    rc = nlg_forces_geometry(dim, n, E, X[0].data(), X[1].data(), dim == 3 ? X[2].data() : nullptr, nf, elem.data(), face.data(), nullptr, 1, nullptr,
                             nullptr, nullptr, nullptr, area.data());
    if (rc || std::fabs(area[0] - 2.0 * want) > 1e-12 * want) return fprintf(stderr, "dim %d n %d: the call with null outputs failed\n", dim, n), 1;
    face[1] = 2 * dim + 1;
    if (!nlg_forces_geometry(dim, n, E, X[0].data(), X[1].data(), dim == 3 ? X[2].data() : nullptr, nf, elem.data(), face.data(), nullptr, 1, nullptr,
                             nds.data(), nullptr, nullptr, nullptr))
        return fprintf(stderr, "a face outside 1..2 dim was accepted\n"), 1;
    face[1] = 2, elem[3] = E;
    if (!nlg_forces_geometry(dim, n, E, X[0].data(), X[1].data(), dim == 3 ? X[2].data() : nullptr, nf, elem.data(), face.data(), nullptr, 1, nullptr,
                             nds.data(), nullptr, nullptr, nullptr))
        return fprintf(stderr, "an element outside the mesh was accepted\n"), 1;
    elem[3] = 0, obj[2] = (int)E;
    if (!nlg_forces_geometry(dim, n, E, X[0].data(), X[1].data(), dim == 3 ? X[2].data() : nullptr, nf, elem.data(), face.data(), obj.data(), (int)E,
                             nullptr, nds.data(), nullptr, nullptr, nullptr) ||
        !nlg_forces_geometry(dim, 17, E, X[0].data(), X[1].data(), nullptr, 0, nullptr, nullptr, nullptr, 1, nullptr, nullptr, nullptr, nullptr, nullptr))
        return fprintf(stderr, "a bad object or lx1 was accepted\n"), 1;
    return 0;
}

int main() {
    const int ns[5] = {2, 6, 8, 12, 16};
    for (int dim = 2; dim <= 3; ++dim)
        for (int n : ns)
            if (run(dim, n)) return 1;
    printf("forces_host_main: ok\n");
    return 0;
}

// The face-grouped element layout, shared by the device code (internal.h) and the HIP-free host set-up (pprec_host.cpp).
#pragma once

#ifdef __HIPCC__
#define NLG_HOST_DEVICE __host__ __device__
#else
#define NLG_HOST_DEVICE
#endif

// Face-grouped slot of point (a, j, k) inside an element: the 8 corners, the 12 edges (interior points of an edge
// contiguous), the 6 face interiors (contiguous (N-2)^2 blocks), then the element interior.  The copies of a shared
// face or edge are then contiguous runs in every element that shares it, so the gather-scatter moves whole runs
// instead of one 8-byte word per 64-byte line.  FG = false gives the natural ix-fastest index.
NLG_HOST_DEVICE inline int fg_slot(int N, int a, int j, int k) {
    const int M = N - 2;
    const int ba = (a == 0 || a == N - 1), bj = (j == 0 || j == N - 1), bk = (k == 0 || k == N - 1);
    const int sa = a == N - 1, sj = j == N - 1, sk = k == N - 1;
    const int nb = ba + bj + bk;
    if (nb == 3) return sa + 2 * sj + 4 * sk;
    if (nb == 2) {
        if (!ba) return 8 + (0 + sj + 2 * sk) * M + (a - 1);
        if (!bj) return 8 + (4 + sa + 2 * sk) * M + (j - 1);
        return 8 + (8 + sa + 2 * sj) * M + (k - 1);
    }
    const int fbase = 8 + 12 * M;
    if (nb == 1) {
        if (ba) return fbase + (0 + sa) * M * M + (j - 1) + M * (k - 1);
        if (bj) return fbase + (2 + sj) * M * M + (a - 1) + M * (k - 1);
        return fbase + (4 + sk) * M * M + (a - 1) + M * (j - 1);
    }
    return fbase + 6 * M * M + (a - 1) + M * ((j - 1) + M * (k - 1));
}

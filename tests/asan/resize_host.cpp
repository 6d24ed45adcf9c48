// Stand-alone sanitizer program for the host side of the camera-size resize (csrc/resize_coeffs.h: the coefficient table behind
// tcsfm_resize_coeffs, the intrinsics scaling behind tcsfm_scale_intrinsics).  Its own main, no Python, no GPU:
//
//     g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I tightly_coupled_sfm_amd/csrc tests/asan/resize_host.cpp -o resize_host && ./resize_host
//
// Every table is written into buffers of exactly out * 2 and out * ksize ints (heap: the sanitizer sees one int too many), and the
// properties the kernel's indexing rests on are checked: windows inside the input, moving monotonically, ksize bounding every window,
// the coefficients of an output summing to 1 << 22 within the rounding of its taps.
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "resize_coeffs.h"

static int check(int in, int out) {
    const int ks = tc::resize_coeffs(in, out, nullptr, nullptr);
    if (ks != tc::resize_ksize(in, out)) return 1;
    std::vector<int> bounds((size_t)out * 2, -1), kk((size_t)out * ks, -1);
    if (tc::resize_coeffs(in, out, bounds.data(), kk.data()) != ks) return 2;
    int prev_min = 0, prev_max = 0;
    for (int o = 0; o < out; o++) {
        const int xmin = bounds[2 * o], n = bounds[2 * o + 1];
        if (xmin < 0 || n < 1 || n > ks || xmin + n > in) return 3;
        if (xmin < prev_min || xmin + n < prev_max) return 4;
        prev_min = xmin; prev_max = xmin + n;
        long long sum = 0;
        for (int x = 0; x < ks; x++) {
            if (x >= n && kk[(size_t)o * ks + x] != 0) return 5;
            sum += kk[(size_t)o * ks + x];
        }
        if (llabs(sum - (1LL << 22)) > n) return 6;
    }
    return 0;
}

int main() {
    const int ins[] = {1, 2, 5, 7, 24, 40, 157, 370, 375, 376, 968, 1226, 1241, 1242, 1296, 5120};
    const int outs[] = {1, 3, 8, 16, 24, 40, 192, 256, 448, 640};
    int bad = 0;
    for (int in : ins)
        for (int out : outs)
            if (int rc = check(in, out)) { printf("in %d out %d: check %d failed\n", in, out, rc); bad++; }
    float K[9] = {718.856f, 0.f, 607.1928f, 0.f, 718.856f, 185.2157f, 0.f, 0.f, 1.f}, Ko[9];
    tc::scale_intrinsics(376, 1241, 192, 640, K, Ko);
    if (Ko[0] != (float)((double)K[0] * (640.0 / 1241)) || Ko[5] != (float)((double)K[5] * (192.0 / 376)) || Ko[8] != 1.f) { printf("scale_intrinsics\n"); bad++; }
    tc::scale_intrinsics(376, 1241, 192, 640, K, K);       // in place
    for (int i = 0; i < 9; i++)
        if (K[i] != Ko[i]) { printf("scale_intrinsics in place, entry %d\n", i); bad++; }
    printf(bad ? "FAILED\n" : "resize_host ok\n");
    return bad ? 1 : 0;
}

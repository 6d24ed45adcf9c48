// Stand-alone sanitizer program for the host side of the flip post-processing (csrc/flip_ramp.h: the table behind tcsfm_flip_ramp).
// Its own main, no Python, no GPU:
//
//     g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I tightly_coupled_sfm_amd/csrc tests/asan/flip_ramp_host.cpp -o flip_ramp_host && ./flip_ramp_host
//
// Every table is written into a heap buffer of exactly W doubles (the sanitizer sees one double too many), and the properties the blend
// rests on are checked: 1 on the left 5 %, 0 from 10 % on, never increasing, inside [0, 1], and l_mask[x] + l_mask[W-1-x] <= 1 for
// W >= 10 (the weight of the mean, 1 - l_mask - r_mask, is not negative there).
#include <stdio.h>
#include <vector>
#include "flip_ramp.h"

static int check(int W) {
    std::vector<double> m((size_t)W, -1.0);
    tc::flip_ramp(W, m.data());
    if (m[0] != 1.0 || m[(size_t)W - 1] != 0.0) return 1;
    for (int i = 0; i < W; i++) {
        if (!(m[i] >= 0.0 && m[i] <= 1.0)) return 2;
        if (i && m[i] > m[i - 1]) return 3;
        const double x = (double)i / (W - 1);
        if (x < 0.0499 && m[i] != 1.0) return 4;
        if (x > 0.1001 && m[i] != 0.0) return 5;
        if (W >= 10 && m[i] + m[(size_t)W - 1 - i] > 1.0) return 6;
    }
    return 0;
}

int main() {
    const int widths[] = {2, 3, 4, 5, 9, 10, 11, 32, 33, 64, 96, 160, 640, 1241, 1248, 16384};
    int bad = 0;
    for (int W : widths) {
        const int rc = check(W);
        if (rc) { printf("W = %d: check %d failed\n", W, rc); bad++; }
    }
    printf("%d widths, %d failures\n", (int)(sizeof(widths) / sizeof(widths[0])), bad);
    return bad ? 1 : 0;
}

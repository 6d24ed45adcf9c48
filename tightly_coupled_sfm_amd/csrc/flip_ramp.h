// The ramp of the flip post-processing (utils/learning_helpers.py:115-123, batch_post_process_disparity), host only: the table behind
// tcsfm_flip_ramp and the device blend k_disp_post (disp_post_kernel.h).  No HIP here: tests/asan/flip_ramp_host.cpp builds it alone.
#pragma once

namespace tc {

// l_mask for width W >= 2: 1.0 - np.clip(20 * (np.linspace(0, 1, W) - 0.05), 0, 1), in double.  np.linspace(0, 1, W) is
// arange(W) * (1.0 / (W - 1)) with the last element set to 1.0 -- NOT arange(W) / (W - 1), whose last bits differ.
inline void flip_ramp(int W, double *l_mask) {
    const double step = 1.0 / (double)(W - 1);
    for (int i = 0; i < W; i++) {
        const double lin = i == W - 1 ? 1.0 : (double)i * step;
        const double c = 20.0 * (lin - 0.05);
        l_mask[i] = 1.0 - (c < 0.0 ? 0.0 : (c > 1.0 ? 1.0 : c));
    }
}

}  // namespace tc

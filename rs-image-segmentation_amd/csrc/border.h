// Border rules of the window operators (k5_window.hip) and of the fixed-point Gaussian (k13_texture.hip).
#pragma once
#include <hip/hip_runtime.h>
#define BORDER_REFLECT 0      // cv2.BORDER_REFLECT: the edge pixel is duplicated (the public border code 0)
#define BORDER_REFLECT_101 1  // cv2.BORDER_REFLECT_101: mirrored about the edge pixel (the public border code 1)
#define BORDER_REPLICATE 2    // internal: erode / dilate (out-of-image taps never win == replicate the edge)

// index of the in-image element that position i of an axis of n elements reads
__device__ __forceinline__ int border_idx(int i, int n, int mode)
{
    if (n == 1) return 0;
    if (mode == BORDER_REPLICATE) return i < 0 ? 0 : (i >= n ? n - 1 : i);
    while (i < 0 || i >= n) {
        if (i < 0) i = mode == BORDER_REFLECT ? -i - 1 : -i;
        else i = mode == BORDER_REFLECT ? 2 * n - 1 - i : 2 * n - 2 - i;
    }
    return i;
}

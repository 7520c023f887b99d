// yolo355_augment -- one entry of cv2.resize's INTER_LINEAR tables for float images (OpenCV 4.x imgproc/src/resize.cpp, see
// include/yolo355_augment.h): oracle/resize_oracle.py's linear_tables expressions (double scale, float fraction), the
// coefficients kept as the float pair (1 - f, f).  Host and device: augment.hip's kernel computes the entries inline (the launch
// has no table to keep), tests/augment_host_check.cpp sweeps the same function on the CPU.  Every operation is rounded on its
// own (no contraction), so both sides give the same bits.
#pragma once
#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define Y355_AUG_HD __host__ __device__
#else
#define Y355_AUG_HD
#endif

struct AugTap {
    int i0, i1;        // the two source indices, both inside 0..src-1
    float c0, c1;      // their coefficients (1 - f, f)
    int single;        // horizontal only: the result is S[i0] alone (OpenCV's dx >= xmax)
};

Y355_AUG_HD inline AugTap y355_aug_tap(int d, int src, int dst, bool vertical) {
#pragma clang fp contract(off)
    const double scale = (double)src / (double)dst;
    const double pos = ((double)d + 0.5) * scale;
    float f = (float)(pos - 0.5);
    int s = (int)floorf(f);
    f = f - (float)s;
    AugTap t;
    t.single = 0;
    if (vertical) {                      // the fraction stays, the two row indices are clipped
        t.i0 = s < 0 ? 0 : (s > src - 1 ? src - 1 : s);
        t.i1 = s + 1 < 0 ? 0 : (s + 1 > src - 1 ? src - 1 : s + 1);
    } else {                             // the offset is clamped AND the fraction zeroed at both borders
        if (s < 0) { s = 0; f = 0.f; }
        if (s >= src - 1) { s = src - 1; f = 0.f; t.single = 1; }
        t.i0 = s;
        t.i1 = t.single ? s : s + 1;
    }
    t.c0 = 1.f - f;
    t.c1 = f;
    return t;
}

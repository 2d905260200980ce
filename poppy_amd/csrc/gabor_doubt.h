// gabor_doubt.h — the doubt rule of the FFT form of the Gabor banks (kernels_gabor_fft.hip), by itself: one function for the kernel and
// for the host (poppy_gabor_rounding_in_doubt, swept against an exact-rational restatement by tests/test_host_gabor_doubt.py).
#pragma once
#include <cmath>
#include <cstring>

#if defined(__HIP__) || defined(__CUDACC__)
#define POPPY_GABOR_HD __host__ __device__
#else
#define POPPY_GABOR_HD
#endif

namespace poppy_hip {

// The width of the doubt band in units of max(1, the patch's largest magnitude); see kernels_gabor_fft.hip for where the number comes from.
constexpr double kGaborBandUnit = 1e-13;

template <class To, class From>
POPPY_GABOR_HD inline To gabor_bit_cast(From v) {
    static_assert(sizeof(To) == sizeof(From), "same size");
    To r;
    memcpy(&r, &v, sizeof(To));
    return r;
}

// Could the float of a plane value v of the FFT form differ from the direct sum's, `band` being the distance the two forms can be apart?
// 0: no, 1: v is near zero, 2: v is near the midpoint between two floats.
POPPY_GABOR_HD inline int rounding_in_doubt(double v, double band) {
    if (v < -band || v > 1.0 + band) return 0;
    if (v < band) return 1;
    // v = f + d with f the nearest float; the midpoints lie half a spacing away: 2^(e - 24) above f and below it, except below a power of two
    // (2^(e - 25)).  In doubt when d comes within `band` of one of them.
    const float f = (float)v;
    const double d = v - (double)f;
    const int fb = gabor_bit_cast<int>(f);
    const bool pow2 = (fb & 0x007fffff) == 0;
    float h = gabor_bit_cast<float>((fb & 0x7f800000) - (24 << 23));
    if (pow2 && d < 0.0) h *= 0.5f;
    if (fabs(d) > (double)h - band) return 2;
    // At or just above a power of two the midpoint below f is the nearer one, half as far from f as the one above.  (It comes within a band of
    // 1e-13 only below 2^-18; the sweep of tests/test_host_gabor_doubt.py found it missing.)
    return pow2 && d >= 0.0 && d + 0.5 * (double)h < band ? 2 : 0;
}

}  // namespace poppy_hip

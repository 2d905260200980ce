// ransac_fundamental.h — the RANSAC fundamental-matrix filter of the descriptor mode (the sketch's ransacTest, src/experiments.hpp:14-144; the rule:
// include/poppy_hip.h, poppy_ransac_fundamental).  The host statement (ransac_fundamental.cpp) and the kernels (kernels_ransac.hip) are pinned to each
// other with ==, so the arithmetic both sides share — the sampler, the null vector of the 8 x 9 system, the two matrix products and the inlier test —
// is written ONCE, here, as functions that compile for either side.  double, + - * / and comparisons only, every sum in the order written, no fused
// products (the build passes -ffp-contract=off to both sides), no libm.
//
// The orders the rule leaves open, as chosen here:
//   * elimination: at step k the pivot is the largest |A[i][j]| over rows i = k..7 and columns j = k..8 of the matrix AS IT STANDS (rows and columns
//     swapped physically by the earlier steps), scanned row by row with a strict >, so ties go to the lowest row and then the lowest column; row k <-> pivot
//     row (columns k..8), column k <-> pivot column (rows 0..7); then for i = k+1..7: f = A[i][k] / A[k][k], for j = k+1..8: A[i][j] = A[i][j] - f * A[k][j];
//   * back-substitution: z[8] = 1; for i = 7..0: s = 0, for j = i+1..8 ascending: s = s + A[i][j] * z[j]; z[i] = (-s) / A[i][i]; entry perm[j] of the
//     null vector is z[j];
//   * F_h = T2^T * (Fhat * T1): first G = Fhat * T1, then F = T2^T * G, every entry (a0 * b0 + a1 * b1) + a2 * b2 over the three products in full
//     (the zeros of T are multiplied like any other entry);
//   * (a, b, c) = (F[r][0] * x1 + F[r][1] * y1) + F[r][2]; e = (a * x2 + b * y2) + c; a' = (F[0][0] * x2 + F[1][0] * y2) + F[2][0], b' with column 1.
#pragma once
#include <cstddef>
#include <cstdint>

#ifndef POPPY_RANSAC_HD
#define POPPY_RANSAC_HD
#endif

namespace poppy_ransac {

constexpr int kHypotheses = 2048, kMinPoints = 8, kMaxPoints = 65536;
constexpr double kPivotFloor = 1e-10;            // a pivot below this share of the first one: the hypothesis is invalid

POPPY_RANSAC_HD inline uint32_t mix32(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}

// The 8 distinct indices of hypothesis h among n >= 8 points, in draw order.  Draw k is below n - k before the mapping and is raised once per earlier draw
// it does not lie below, so every index is at most (n - k - 1) + k = n - 1.
POPPY_RANSAC_HD inline void sample8(uint32_t h, uint32_t n, uint32_t idx[8]) {
    uint32_t sorted[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        uint32_t r = mix32(0x9E3779B9u * (8u * h + (uint32_t)k + 1u)) % (n - (uint32_t)k);
#pragma unroll
        for (int j = 0; j < k; ++j) r += r >= sorted[j] ? 1u : 0u;
        idx[k] = r;
        sorted[k] = r;
#pragma unroll
        for (int j = k; j > 0; --j)
            if (sorted[j - 1] > sorted[j]) { const uint32_t t = sorted[j - 1]; sorted[j - 1] = sorted[j]; sorted[j] = t; }
    }
}

POPPY_RANSAC_HD inline double absd(double v) { return v < 0.0 ? -v : v; }

// Row r of the system from one normalised pair (x1, y1) <-> (x2, y2).  A: element (i, j) at A[(i * 9 + j) * S].
template <int S> POPPY_RANSAC_HD inline void system_row(double* A, int r, double x1, double y1, double x2, double y2) {
    double* row = A + (size_t)r * 9 * S;
    row[0 * S] = x2 * x1; row[1 * S] = x2 * y1; row[2 * S] = x2;
    row[3 * S] = y2 * x1; row[4 * S] = y2 * y1; row[5 * S] = y2;
    row[6 * S] = x1; row[7 * S] = y1; row[8 * S] = 1.0;
}

// The null vector of the 8 x 9 system in A (destroyed) by Gaussian elimination with complete pivoting; false: the hypothesis is invalid.
template <int S> POPPY_RANSAC_HD inline bool null_vector(double* A, double fhat[9]) {
#define POPPY_RANSAC_A(i, j) A[(size_t)((i) * 9 + (j)) * S]
    uint64_t perm = 0x876543210ull;               // nibble j: the unknown that column j holds
    double first = 0.0;
    for (int k = 0; k < 8; ++k) {
        int pi = k, pj = k;
        double big = -1.0;
        for (int i = k; i < 8; ++i)
            for (int j = k; j < 9; ++j) {
                const double v = absd(POPPY_RANSAC_A(i, j));
                if (v > big) { big = v; pi = i; pj = j; }
            }
        if (k == 0) { first = big; if (!(first > 0.0)) return false; }
        else if (!(big >= kPivotFloor * first)) return false;
        if (pi != k)
            for (int j = k; j < 9; ++j) { const double t = POPPY_RANSAC_A(k, j); POPPY_RANSAC_A(k, j) = POPPY_RANSAC_A(pi, j); POPPY_RANSAC_A(pi, j) = t; }
        if (pj != k) {
            for (int i = 0; i < 8; ++i) { const double t = POPPY_RANSAC_A(i, k); POPPY_RANSAC_A(i, k) = POPPY_RANSAC_A(i, pj); POPPY_RANSAC_A(i, pj) = t; }
            const uint64_t a = (perm >> (4 * k)) & 15u, b = (perm >> (4 * pj)) & 15u;
            perm = (perm & ~((15ull << (4 * k)) | (15ull << (4 * pj)))) | (b << (4 * k)) | (a << (4 * pj));
        }
        const double pivot = POPPY_RANSAC_A(k, k);
        for (int i = k + 1; i < 8; ++i) {
            const double f = POPPY_RANSAC_A(i, k) / pivot;
            for (int j = k + 1; j < 9; ++j) POPPY_RANSAC_A(i, j) = POPPY_RANSAC_A(i, j) - f * POPPY_RANSAC_A(k, j);
        }
    }
    double z[9];
    z[8] = 1.0;
#pragma unroll
    for (int i = 7; i >= 0; --i) {
        double s = 0.0;
#pragma unroll
        for (int j = i + 1; j < 9; ++j) s = s + POPPY_RANSAC_A(i, j) * z[j];
        z[i] = (-s) / POPPY_RANSAC_A(i, i);
    }
    // undo the column permutation through the (now free) first row of the storage: no dynamically indexed array in registers
#pragma unroll
    for (int j = 0; j < 9; ++j) A[(size_t)((perm >> (4 * j)) & 15u) * S] = z[j];
#pragma unroll
    for (int j = 0; j < 9; ++j) fhat[j] = A[(size_t)j * S];
    return true;
#undef POPPY_RANSAC_A
}

// C = A * B for row-major 3 x 3; at: A is read transposed
POPPY_RANSAC_HD inline void mul3(const double* A, bool at, const double* B, double* C) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const double a0 = at ? A[0 * 3 + i] : A[i * 3 + 0], a1 = at ? A[1 * 3 + i] : A[i * 3 + 1], a2 = at ? A[2 * 3 + i] : A[i * 3 + 2];
            C[i * 3 + j] = (a0 * B[0 * 3 + j] + a1 * B[1 * 3 + j]) + a2 * B[2 * 3 + j];
        }
}
// F = T2^T * (Fhat * T1)
POPPY_RANSAC_HD inline void denormalise(const double* fhat, const double* T1, const double* T2, double* F) {
    double G[9];
    mul3(fhat, false, T1, G);
    mul3(T2, true, G, F);
}

// the symmetric epipolar test of one pair against F, d2 = distance * distance
POPPY_RANSAC_HD inline bool is_inlier(const double* F, double x1, double y1, double x2, double y2, double d2) {
    const double a = (F[0] * x1 + F[1] * y1) + F[2];
    const double b = (F[3] * x1 + F[4] * y1) + F[5];
    const double c = (F[6] * x1 + F[7] * y1) + F[8];
    const double e = (a * x2 + b * y2) + c;
    const double a2 = (F[0] * x2 + F[3] * y2) + F[6];
    const double b2 = (F[1] * x2 + F[4] * y2) + F[7];
    const double ee = e * e;
    return ee <= d2 * (a * a + b * b) && ee <= d2 * (a2 * a2 + b2 * b2);
}

// ---- host side (ransac_fundamental.cpp) -------------------------------------------------------------------------------------------------------------
// What the host prepares once per call and both the host statement and the kernels start from.
struct Problem {
    int n = 0;
    double d2 = 0;                   // distance * distance
    bool normalised = false;         // false: the mean distance to the centroid is 0 in either image — no model
    double T1[9], T2[9];
    double* norm = nullptr;          // n x 4 doubles, caller-owned: x1^, y1^, x2^, y2^ per pair
};
// Hartley normalisation of `count` points (x, y float pairs picked by `pick`, or all when pick is null) -> T; false when r is 0
bool normalisation(const float* pts, const uint8_t* pick, int n, double* T);
// fills P (P.norm must have room for n x 4 doubles)
void prepare(const float* p1, const float* p2, int n, double distance, Problem& P);
// the 2048 models and counts on the host
void models_and_counts(const Problem& P, const float* p1, const float* p2, int* counts, double* models);
// choice, mask, refit and the no-model rule from the counts and models of either side
void finish(const Problem& P, const float* p1, const float* p2, const int* counts, const double* models, uint8_t* inliers, int* n_inliers, double* f3x3, int* best);

}  // namespace poppy_ransac

// ransac_fundamental.cpp — the host statement of the RANSAC fundamental-matrix filter (include/poppy_hip.h: poppy_ransac_fundamental) and the host
// halves that the GPU path shares with it: the normalisation in front of the kernels, and the choice, the mask and the refit behind them.  No GPU code
// and nothing of the context in here: tools/ransac_host_check.cpp builds this file alone, under the sanitizers.
#include "ransac_fundamental.h"
#include "../../include/poppy_hip.h"
#include <cmath>
#include <cstring>
#include <vector>

namespace poppy_ransac {

static_assert(kHypotheses == POPPY_RANSAC_HYPOTHESES && kMinPoints == POPPY_RANSAC_MIN_POINTS && kMaxPoints == POPPY_RANSAC_MAX_POINTS, "the header's constants");

bool normalisation(const float* pts, const uint8_t* pick, int n, double* T) {
    double sx = 0, sy = 0;
    long count = 0;
    for (int i = 0; i < n; ++i) {
        if (pick && !pick[i]) continue;
        sx = sx + (double)pts[2 * i]; sy = sy + (double)pts[2 * i + 1];
        ++count;
    }
    for (int k = 0; k < 9; ++k) T[k] = 0.0;
    T[8] = 1.0;
    if (!count) return false;
    const double mx = sx / (double)count, my = sy / (double)count;
    double sr = 0;
    for (int i = 0; i < n; ++i) {
        if (pick && !pick[i]) continue;
        const double dx = (double)pts[2 * i] - mx, dy = (double)pts[2 * i + 1] - my;
        sr = sr + std::sqrt(dx * dx + dy * dy);
    }
    const double r = sr / (double)count;
    if (!(r > 0.0)) return false;
    const double s = std::sqrt(2.0) / r;
    T[0] = s; T[2] = -(s * mx);
    T[4] = s; T[5] = -(s * my);
    return true;
}

static inline void apply(const double* T, float x, float y, double* out) {
    out[0] = T[0] * (double)x + T[2];
    out[1] = T[4] * (double)y + T[5];
}

void prepare(const float* p1, const float* p2, int n, double distance, Problem& P) {
    P.n = n;
    P.d2 = distance * distance;
    const bool ok1 = normalisation(p1, nullptr, n, P.T1), ok2 = normalisation(p2, nullptr, n, P.T2);
    P.normalised = ok1 && ok2;
    for (int i = 0; i < n; ++i) {
        apply(P.T1, p1[2 * i], p1[2 * i + 1], P.norm + 4 * (size_t)i);
        apply(P.T2, p2[2 * i], p2[2 * i + 1], P.norm + 4 * (size_t)i + 2);
    }
}

void models_and_counts(const Problem& P, const float* p1, const float* p2, int* counts, double* models) {
    for (int h = 0; h < kHypotheses; ++h) {
        double* F = models + 9 * (size_t)h;
        for (int k = 0; k < 9; ++k) F[k] = 0.0;
        counts[h] = -1;
        if (!P.normalised) continue;
        uint32_t idx[8];
        sample8((uint32_t)h, (uint32_t)P.n, idx);
        double A[72], fhat[9];
        for (int r = 0; r < 8; ++r) {
            const double* q = P.norm + 4 * (size_t)idx[r];
            system_row<1>(A, r, q[0], q[1], q[2], q[3]);
        }
        if (!null_vector<1>(A, fhat)) continue;
        denormalise(fhat, P.T1, P.T2, F);
        int c = 0;
        for (int i = 0; i < P.n; ++i) c += is_inlier(F, (double)p1[2 * i], (double)p1[2 * i + 1], (double)p2[2 * i], (double)p2[2 * i + 1], P.d2) ? 1 : 0;
        counts[h] = c;
    }
}

namespace {

// Cyclic Jacobi on the symmetric N x N matrix S (row-major, destroyed): V's columns become the eigenvectors, S's diagonal the eigenvalues.
// Sweeps over (p, q), p < q, row by row, until a sweep finds nothing to rotate or kSweeps are through.
template <int N> void jacobi_eigen(double* S, double* V) {
    constexpr int kSweeps = 64;
    for (int i = 0; i < N; ++i) for (int j = 0; j < N; ++j) V[i * N + j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < kSweeps; ++sweep) {
        bool rotated = false;
        for (int p = 0; p < N - 1; ++p)
            for (int q = p + 1; q < N; ++q) {
                const double apq = S[p * N + q];
                if (apq == 0.0) continue;
                const double app = S[p * N + p], aqq = S[q * N + q];
                // a rotation too small to change either diagonal entry ends the element
                if (absd(app) + absd(apq) == absd(app) && absd(aqq) + absd(apq) == absd(aqq)) { S[p * N + q] = S[q * N + p] = 0.0; continue; }
                const double theta = (aqq - app) / (2.0 * apq);
                const double t = (theta < 0.0 ? -1.0 : 1.0) / (absd(theta) + std::sqrt(theta * theta + 1.0));
                const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
                rotated = true;
                for (int k = 0; k < N; ++k) {                      // columns p, q of S
                    const double kp = S[k * N + p], kq = S[k * N + q];
                    S[k * N + p] = c * kp - s * kq; S[k * N + q] = s * kp + c * kq;
                }
                for (int k = 0; k < N; ++k) {                      // rows p, q of S
                    const double pk = S[p * N + k], qk = S[q * N + k];
                    S[p * N + k] = c * pk - s * qk; S[q * N + k] = s * pk + c * qk;
                }
                S[p * N + q] = S[q * N + p] = 0.0;
                for (int k = 0; k < N; ++k) {
                    const double kp = V[k * N + p], kq = V[k * N + q];
                    V[k * N + p] = c * kp - s * kq; V[k * N + q] = s * kp + c * kq;
                }
            }
        if (!rotated) break;
    }
}

// Rank 2 by a one-sided Jacobi SVD of the 3 x 3 matrix F (row-major, in place): right rotations make the columns of B = F * V orthogonal, their
// lengths are the singular values; the shortest column is zeroed and F = B * V^T.
void enforce_rank2(double* F) {
    double B[9], V[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    memcpy(B, F, sizeof(B));
    for (int sweep = 0; sweep < 64; ++sweep) {
        bool rotated = false;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                double alpha = 0, beta = 0, gamma = 0;
                for (int k = 0; k < 3; ++k) { alpha = alpha + B[k * 3 + p] * B[k * 3 + p]; beta = beta + B[k * 3 + q] * B[k * 3 + q]; gamma = gamma + B[k * 3 + p] * B[k * 3 + q]; }
                if (gamma == 0.0 || gamma * gamma <= 1e-32 * (alpha * beta)) continue;
                const double zeta = (beta - alpha) / (2.0 * gamma);
                const double t = (zeta < 0.0 ? -1.0 : 1.0) / (absd(zeta) + std::sqrt(zeta * zeta + 1.0));
                const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
                rotated = true;
                for (int k = 0; k < 3; ++k) {
                    const double bp = B[k * 3 + p], bq = B[k * 3 + q];
                    B[k * 3 + p] = c * bp - s * bq; B[k * 3 + q] = s * bp + c * bq;
                    const double vp = V[k * 3 + p], vq = V[k * 3 + q];
                    V[k * 3 + p] = c * vp - s * vq; V[k * 3 + q] = s * vp + c * vq;
                }
            }
        if (!rotated) break;
    }
    int least = 0;
    double least_len = 0;
    for (int j = 0; j < 3; ++j) {
        const double len = (B[0 * 3 + j] * B[0 * 3 + j] + B[1 * 3 + j] * B[1 * 3 + j]) + B[2 * 3 + j] * B[2 * 3 + j];
        if (j == 0 || len < least_len) { least = j; least_len = len; }
    }
    for (int k = 0; k < 3; ++k) B[k * 3 + least] = 0.0;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) F[i * 3 + j] = (B[i * 3 + 0] * V[j * 3 + 0] + B[i * 3 + 1] * V[j * 3 + 1]) + B[i * 3 + 2] * V[j * 3 + 2];
}

// The normalised 8-point fit over the picked pairs -> F (Frobenius norm 1, largest-magnitude entry positive); false: no such fit
bool refit(const float* p1, const float* p2, const uint8_t* pick, int n, double* F) {
    double T1[9], T2[9];
    if (!normalisation(p1, pick, n, T1) || !normalisation(p2, pick, n, T2)) return false;
    double S[81], V[81];
    for (int k = 0; k < 81; ++k) S[k] = 0.0;
    for (int i = 0; i < n; ++i) {
        if (!pick[i]) continue;
        double a[2], b[2], row[9];
        apply(T1, p1[2 * i], p1[2 * i + 1], a); apply(T2, p2[2 * i], p2[2 * i + 1], b);
        system_row<1>(row, 0, a[0], a[1], b[0], b[1]);
        for (int r = 0; r < 9; ++r) for (int c = r; c < 9; ++c) S[r * 9 + c] = S[r * 9 + c] + row[r] * row[c];
    }
    for (int r = 0; r < 9; ++r) for (int c = 0; c < r; ++c) S[r * 9 + c] = S[c * 9 + r];
    jacobi_eigen<9>(S, V);
    int least = 0;
    for (int j = 1; j < 9; ++j) if (S[j * 9 + j] < S[least * 9 + least]) least = j;
    double fhat[9];
    for (int k = 0; k < 9; ++k) fhat[k] = V[k * 9 + least];
    enforce_rank2(fhat);
    denormalise(fhat, T1, T2, F);
    double sum = 0;
    for (int k = 0; k < 9; ++k) sum = sum + F[k] * F[k];
    const double norm = std::sqrt(sum);
    if (!(norm > 0.0) || !(norm <= 1.7976931348623157e308)) return false;
    int big = 0;
    for (int k = 1; k < 9; ++k) if (absd(F[k]) > absd(F[big])) big = k;
    const double scale = F[big] < 0.0 ? -norm : norm;
    for (int k = 0; k < 9; ++k) F[k] = F[k] / scale;
    return true;
}

}  // namespace

void finish(const Problem& P, const float* p1, const float* p2, const int* counts, const double* models, uint8_t* inliers, int* n_inliers, double* f3x3, int* best) {
    const int n = P.n;
    int b = -1;
    for (int h = 0; h < kHypotheses; ++h) if (counts[h] >= 0 && (b < 0 || counts[h] > counts[b])) b = h;
    bool model = b >= 0 && counts[b] >= kMinPoints;
    int kept = 0;
    if (model) {
        const double* F = models + 9 * (size_t)b;
        for (int i = 0; i < n; ++i) {
            inliers[i] = is_inlier(F, (double)p1[2 * i], (double)p1[2 * i + 1], (double)p2[2 * i], (double)p2[2 * i + 1], P.d2) ? 1 : 0;
            kept += inliers[i];
        }
        // (an inlier set the 8-point fit cannot take — all of its points of one image in one place, or a fit without a finite norm — is no model either)
        model = refit(p1, p2, inliers, n, f3x3);
    }
    if (!model) {                                  // no model never throws pairs away
        memset(inliers, 1, (size_t)n);
        for (int k = 0; k < 9; ++k) f3x3[k] = 0.0;
        kept = n; b = -1;
    }
    *n_inliers = kept;
    *best = b;
}

}  // namespace poppy_ransac

extern "C" int poppy_ransac_fundamental(const float* points1, const float* points2, int n_points, double distance, uint8_t* inliers, int* n_inliers,
                                        double* f3x3, int* best, int* counts, double* models) {
    using namespace poppy_ransac;
    if (!points1 || !points2 || !inliers || !n_inliers || !f3x3 || !best) return POPPY_E_ARG;
    if (n_points < kMinPoints || n_points > kMaxPoints || !(distance >= 0.0) || !(distance <= 1.7976931348623157e308)) return POPPY_E_ARG;
    std::vector<double> norm((size_t)n_points * 4), own_models;
    std::vector<int> own_counts;
    if (!counts) { own_counts.resize(kHypotheses); counts = own_counts.data(); }
    if (!models) { own_models.resize((size_t)kHypotheses * 9); models = own_models.data(); }
    Problem P;
    P.norm = norm.data();
    prepare(points1, points2, n_points, distance, P);
    models_and_counts(P, points1, points2, counts, models);
    finish(P, points1, points2, counts, models, inliers, n_inliers, f3x3, best);
    return POPPY_OK;
}

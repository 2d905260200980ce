// kernels_ransac.hip — the 2048 hypotheses of the RANSAC fundamental-matrix filter on the GPU (the rule: include/poppy_hip.h, poppy_ransac_fundamental;
// the arithmetic both sides share: ransac_fundamental.h).  Two launches on one stream:
//   k_ransac_models  one lane per hypothesis: its 8 samples, the 8 x 9 system, the null vector by complete pivoting, F_h = T2^T * Fhat * T1
//   k_ransac_score   hypotheses x point tiles: every valid hypothesis's inlier count
// The choice over the counts, the mask and the refit are the host's (ransac_fundamental.cpp: finish), from the downloaded counts and models.
#include <hip/hip_runtime.h>
#define POPPY_RANSAC_HD __host__ __device__
#include "ransac_fundamental.h"
#include "kernels.h"
#include "writer_buffers.h"
#include <string>

namespace poppy_hip {

namespace {

using namespace poppy_ransac;

struct RansacFrames { double T1[9], T2[9]; };

constexpr int kModelLanes = 64;              // hypotheses per block of k_ransac_models (one wave)
constexpr int kTilePoints = 1024;            // points per block of k_ransac_score: 4 x 8 KB of LDS
constexpr int kScoreWaves = 4, kHypPerWave = 4, kHypPerBlock = kScoreWaves * kHypPerWave;
static_assert(kHypotheses % kModelLanes == 0 && kHypotheses % kHypPerBlock == 0, "the grids cover the hypotheses exactly");

// The elimination indexes its 72 doubles by row and column at run time, so they live in LDS and not in 72 registers per lane, which those indices would send
// to scratch.  Element-major: element e of lane t at sys[e * 64 + t].  Lanes that are at the same element read 64 consecutive doubles; a lane whose pivot sits
// elsewhere reads the same banks at another element, which costs a conflict and no more.
__global__ void __launch_bounds__(kModelLanes) k_ransac_models(const double* __restrict__ norm, int n, RansacFrames t, double* __restrict__ models,
                                                               int* __restrict__ counts, int* __restrict__ valid) {
    __shared__ double sys[72 * kModelLanes];
    const int h = blockIdx.x * kModelLanes + threadIdx.x;
    double* A = sys + threadIdx.x;
    uint32_t idx[8];
    sample8((uint32_t)h, (uint32_t)n, idx);                        // every index < n (ransac_fundamental.h: sample8)
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const double4 q = ((const double4*)norm)[idx[r]];
        system_row<kModelLanes>(A, r, q.x, q.y, q.z, q.w);
    }
    double fhat[9], F[9];
    const bool ok = null_vector<kModelLanes>(A, fhat);
    if (ok) denormalise(fhat, t.T1, t.T2, F);
#pragma unroll
    for (int k = 0; k < 9; ++k) models[(size_t)h * 9 + k] = ok ? F[k] : 0.0;
    counts[h] = ok ? 0 : -1;
    valid[h] = ok ? 1 : 0;
}

// Block (x, y): hypotheses 16 x .. 16 x + 15 against points 1024 y .. 1024 y + 1023.  The tile's points are widened to double into LDS once; each wave takes
// four hypotheses, one after the other, F_h in registers, 64 points per step; the wave's count comes from ballots and goes to counts[h] in one integer atomic
// per (hypothesis, tile) — integer addition has no order, so the counts do not depend on scheduling.
__global__ void __launch_bounds__(kScoreWaves * 64) k_ransac_score(const float2* __restrict__ p1, const float2* __restrict__ p2, int n, double d2,
                                                                   const double* __restrict__ models, const int* __restrict__ valid, int* __restrict__ counts) {
    __shared__ double px1[kTilePoints], py1[kTilePoints], px2[kTilePoints], py2[kTilePoints];
    const int base = blockIdx.y * kTilePoints;
    const int m = min(kTilePoints, n - base);                      // >= 1: the grid has ceil(n / 1024) rows
    for (int j = threadIdx.x; j < m; j += kScoreWaves * 64) {
        const float2 a = p1[base + j], b = p2[base + j];
        px1[j] = (double)a.x; py1[j] = (double)a.y; px2[j] = (double)b.x; py2[j] = (double)b.y;
    }
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int q = 0; q < kHypPerWave; ++q) {
        const int h = blockIdx.x * kHypPerBlock + wave * kHypPerWave + q;
        if (!valid[h]) continue;                                   // the same for the whole wave
        double F[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) F[k] = models[(size_t)h * 9 + k];
        int count = 0;
        for (int j0 = 0; j0 < m; j0 += 64) {
            const int j = j0 + lane;
            const bool in = j < m;
            const int jj = in ? j : 0;
            const bool inl = in && is_inlier(F, px1[jj], py1[jj], px2[jj], py2[jj], d2);
            count += __popcll(__ballot(inl));
        }
        if (lane == 0) atomicAdd(&counts[h], count);
    }
}

}  // namespace

// The 2048 counts and models of problem P (P.normalised) into the host arrays, on stream s, which is synchronised.  buf: the context's grow-only scratch.
// The points' indices: the sampler keeps below P.n (ransac_fundamental.h: sample8), the score kernel below min(1024, n - base); both take n as it is
// checked here.
int ransac_counts_device(DeviceBuffer& buf, hipStream_t s, const poppy_ransac::Problem& P, const float* p1, const float* p2, int* counts, double* models, std::string& err) {
    const int n = P.n;
    if (n < kMinPoints || n > kMaxPoints || !P.normalised || !P.norm) { err = "ransac: the launch takes 8 .. 65536 normalised pairs"; return POPPY_E_ARG; }
    const size_t norm_bytes = (size_t)n * 32, pts_bytes = (size_t)n * 8, models_bytes = (size_t)kHypotheses * 72, counts_bytes = (size_t)kHypotheses * 4;
    const size_t in_bytes = norm_bytes + 2 * pts_bytes, out_bytes = models_bytes + counts_bytes;
    hipError_t e = buf.reserve(in_bytes + out_bytes + counts_bytes, s);
    if (e != hipSuccess) { err = std::string("ransac: ") + hipGetErrorString(e); return POPPY_E_DEVICE; }
    std::vector<uint8_t> in(in_bytes), out(out_bytes);
    memcpy(in.data(), P.norm, norm_bytes);
    memcpy(in.data() + norm_bytes, p1, pts_bytes);
    memcpy(in.data() + norm_bytes + pts_bytes, p2, pts_bytes);
    const double* d_norm = (const double*)buf.p;
    const float2* d_p1 = (const float2*)(buf.p + norm_bytes);
    const float2* d_p2 = (const float2*)(buf.p + norm_bytes + pts_bytes);
    double* d_models = (double*)(buf.p + in_bytes);
    int* d_counts = (int*)(buf.p + in_bytes + models_bytes);
    int* d_valid = d_counts + kHypotheses;
    RansacFrames t;
    memcpy(t.T1, P.T1, sizeof(t.T1)); memcpy(t.T2, P.T2, sizeof(t.T2));
    e = hipMemcpyAsync(buf.p, in.data(), in_bytes, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_ransac_models, dim3(kHypotheses / kModelLanes), dim3(kModelLanes), 0, s, d_norm, n, t, d_models, d_counts, d_valid);
        hipLaunchKernelGGL(k_ransac_score, dim3(kHypotheses / kHypPerBlock, (n + kTilePoints - 1) / kTilePoints), dim3(kScoreWaves * 64), 0, s,
                           d_p1, d_p2, n, P.d2, (const double*)d_models, (const int*)d_valid, d_counts);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out.data(), d_models, out_bytes, hipMemcpyDeviceToHost, s);
    const hipError_t synced = hipStreamSynchronize(s);             // also behind a failure: the upload reads `in`
    if (e == hipSuccess) e = synced;
    if (e != hipSuccess) { err = std::string("ransac: ") + hipGetErrorString(e); return POPPY_E_DEVICE; }
    memcpy(models, out.data(), models_bytes);
    memcpy(counts, out.data() + models_bytes, counts_bytes);
    return POPPY_OK;
}

}  // namespace poppy_hip

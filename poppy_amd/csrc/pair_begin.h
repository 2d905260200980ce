// pair_begin.h — the pair set-up from raw images (pair_begin.cpp: poppy::morph up to its frame loop, src/poppy.hpp:46-160) and those of its
// stages that other units run too: sharded_setup.cpp (one image's filter chain, gabor2, the matcher's points) and pair_setup.cpp's ORB entry.
#pragma once
#include "context.h"

// What a stage reports.  rc is read by the other chain's thread once both details are known, msg only after the threads have joined.
struct SetupStatus {
    std::atomic<int> rc{POPPY_OK}; std::string msg;
    bool fail(std::string m, int code = POPPY_E_DEVICE) { msg = std::move(m); rc = code; return false; }
};

// One image's filter chain on stream st with chain slot `slot`: Extractor::foreground -> dft_detail2 -> the ORB input of Extractor::keypoints.
// true: *orb_in is the ORB input where it lies on the device (queued on st) and *detail is known; false: s says why.
bool chain_filter(poppy_hip_ctx* c, int slot, const uint8_t* d_bgr, hipStream_t st, double* detail, const uint8_t** orb_in, SetupStatus& s);

// gabor2 = gabor_filter(second image / 255) (src/poppy.hpp:119-122) into the pair state: fg's gabor_field of c->c2 and its copy into c->gabor2, both queued on st.
// concurrent: another thread is inside fg — its buffers were prepared beforehand and the error goes to s alone, not to fg.err.  false: s says why.
bool gabor2_into_state(poppy_hip_ctx* c, ForegroundFilter& fg, hipStream_t st, SetupStatus& s, bool concurrent = false);

// The matcher's points in two steps, so that the set-up from raw images can align the second image in between (Matcher::find):
// Extractor::points (extractor.cpp:96-99) — image 1's keypoints and image 2's positions (n2 x, y pairs), both cut to the shorter list's length —
// then Matcher::match / prepare in place: the lists become the prepared point sets for set_points.  helper: takes half of the matcher's sums, or null.
struct PointLists { std::vector<float> p1, p2; };
PointLists extractor_points(const std::vector<OrbKeyPoint>& k1, const float* xy2, size_t n2);
int prepare_points(poppy_hip_ctx* c, PointLists& pts, int W, int H, Worker* helper);
std::vector<float> keypoint_xy(const std::vector<OrbKeyPoint>& k);
void keypoint_rows7(const std::vector<OrbKeyPoint>& k, float* rows);      // cv::KeyPoint's field order, all as float: x, y, size, angle, response, octave, class_id

// The RANSAC fundamental-matrix filter on the context's GPU (pair_setup.cpp; poppy_hip_ransac_fundamental is this behind hipSetDevice): arguments and result as
// poppy_ransac_fundamental's.  The set-up with the filter calls it between drop_out_of_image and the corners.
int ransac_filter(poppy_hip_ctx* c, const float* p1, const float* p2, int n, double distance, uint8_t* inliers, int* n_inliers, double* f3x3, int* best,
                  int* counts, double* models);

// poppy_match_points with a helper thread for the sums
int match_points_with(Worker* helper, const float* p1, const float* p2, int n, int W, int H, double tol, float* o1, float* o2, int* n_out, double* imd);

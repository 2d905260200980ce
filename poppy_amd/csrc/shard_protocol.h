// shard_protocol.h — the two pure pieces of the sharded pair set-up's protocol (sharded_setup.cpp): which rank plays which role, and the
// format in which image 2's keypoints travel to the matcher's rank.  Host only (tools/comm_guard_check.cpp checks both tables alone).
#pragma once
#include "pair_state_limits.h"
#include <cstddef>
#include <cstring>
#include <vector>

namespace poppy_hip {

// A: image 1's chain, its detection and the matcher, on `root`; B: image 2's chain and detection, on root + 1; C: gabor2 -> m2, on root + 2
// (with B when there are two ranks, all on one rank when there is one).
struct ShardRoles {
    int a, b, c;
    bool is_a, is_b, is_c;                         // ... of the rank asked about
};
inline ShardRoles shard_roles(int rank, int world, int root) {
    ShardRoles r;
    r.a = root;
    r.b = world >= 2 ? (root + 1) % world : root;
    r.c = world >= 3 ? (root + 2) % world : r.b;
    r.is_a = rank == r.a; r.is_b = rank == r.b; r.is_c = rank == r.c;
    return r;
}

// The keypoint hand-off B -> A through the pair state's point area: [count or -1][unused][x, y pairs], all 4-byte words.  The count -1 says
// "image 2's detection failed, or it found more keypoints than travel": one fewer than the area's kPairMaxPoints pairs, the two leading words
// taking the last pair's place.
constexpr int kHandoffMaxPoints = kPairMaxPoints - 1;
constexpr size_t kHandoffWords = 2 + 2 * (size_t)kPairMaxPoints;      // what the matcher's rank reads back (it never reads behind the count's pairs)

// buf becomes the words to send (2 + 2 * count of them); returns the count sent: n, or -1 (detect_rc < 0, or n > kHandoffMaxPoints)
inline int pack_handoff(const float* xy, size_t n, int detect_rc, std::vector<float>& buf) {
    const int count = detect_rc < 0 || n > (size_t)kHandoffMaxPoints ? -1 : (int)n;
    buf.assign(2 + 2 * (size_t)(count < 0 ? 0 : count), 0.f);
    memcpy(&buf[0], &count, 4);
    if (count > 0) memcpy(&buf[2], xy, 2 * (size_t)count * 4);
    return count;
}
// buf: kHandoffWords words as received.  *n2 = the count and xy its pairs, or *n2 = -1 and xy empty for "failed" and for any count no sender writes
// (negative, or above kHandoffMaxPoints: stale or foreign words — nothing behind the count is read then)
inline void unpack_handoff(const float* buf, int* n2, std::vector<float>& xy) {
    int count;
    memcpy(&count, buf, 4);
    if (count < 0 || count > kHandoffMaxPoints) count = -1;
    xy.assign(buf + 2, buf + 2 + 2 * (size_t)(count < 0 ? 0 : count));
    *n2 = count;
}

}  // namespace poppy_hip

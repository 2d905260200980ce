// pair_state_limits.h — the one capacity of the packed pair state (context.h: PairStateHeader and the point area behind it) that host-only code
// needs as well: the sharded set-up's keypoint hand-off travels through the point area (shard_protocol.h).  Nothing of HIP in here.
#pragma once

namespace poppy_hip {
constexpr int kPairMaxPoints = 16384;              // point pairs the packed state has room for
}

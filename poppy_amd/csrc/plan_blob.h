// plan_blob.h — the one description of a frame slot's plan blob: what the host writes into the slot's pinned copy, k_upload moves to the device copy and the
// frame's kernels read there.  Host arithmetic only (no HIP): ensure_ring sizes the blobs with plan_blob_capacity, prepare_slot lays a frame out with
// plan_blob_layout and fills it with fill_plan_blob, and the device pointers of both halves of a frame come from the same PlanBlobLayout (frame_render.cpp).
//
//   header (kBlobHeader bytes) | warp records, (T + 1) x kWarpRecordFloats floats | fill-edge tables, T RasterTri |
//     fused path:   outline segments, 3 T OutlineSeg | per-tile offsets, n_toff int32 | per-tile triangle lists, n_ttri uint16
//     id-map path:  integer corners, 6 T int32 | inverse matrices, 9 T floats of inv1 then 9 T of inv2 | k_raster's work list, n_work pairs of int32
// Every group begins on a 16-byte boundary.  A frame uploads what ITS kernels read: the fused path's two kernels never look at the id-map group
// (round 6: ~255 KB instead of ~400 KB per 1080p frame over PCIe, k_upload 12 -> 8 us), so a blob holds one of the two groups, never both.
#pragma once
#include "frame_plan.h"
#include <algorithm>
#include <cstddef>
#include <cstring>

namespace poppy_hip {

constexpr size_t kBlobHeader = 64;            // [0] float: unsharp amount; [16], [24] double: the frame's mask (alpha, beta)
constexpr size_t kBlobMaskAB = 16;

// byte offsets of the groups in the blob; the offsets of the group the frame does not upload are 0
struct PlanBlobLayout {
    size_t rec_bytes = 0;                      // the warp records, which begin at kBlobHeader
    size_t o_edges = 0;
    size_t o_outl = 0, o_toff = 0, o_ttri = 0; // fused path
    size_t o_tri = 0, o_inv = 0, o_work = 0;   // id-map path
    size_t used = 0;                           // end of the last group: what k_upload moves
};

inline PlanBlobLayout plan_blob_layout(int T, size_t n_work, size_t n_toff, size_t n_ttri, bool fused) {
    auto pad16 = [](size_t b) { return (b + 15) & ~(size_t)15; };
    PlanBlobLayout l;
    l.rec_bytes = (size_t)(T + 1) * kWarpRecordFloats * sizeof(float);
    size_t off = kBlobHeader + l.rec_bytes;
    l.o_edges = off; off += (size_t)T * sizeof(RasterTri);                       // 96-byte entries: stays 16-byte aligned
    if (fused) {
        l.o_outl = off; off += (size_t)T * 3 * sizeof(OutlineSeg);
        l.o_toff = off; off += pad16(n_toff * 4);
        l.o_ttri = off; off += pad16(n_ttri * 2);
    } else {
        l.o_tri = off; off += pad16((size_t)T * 6 * sizeof(int));
        l.o_inv = off; off += pad16((size_t)T * 18 * sizeof(float));
        l.o_work = off; off += pad16(n_work * 8);
    }
    l.used = off;
    return l;
}

// What a slot's blob is allocated with: the larger of the two worst cases of a pair with a budget of max_tris triangles on an image H rows high — the fused
// path with every tile offset and every list entry the planner bins with (bins_cap: tile_bins_capacity), the id-map path with every triangle spanning
// the whole image height in its work list.
inline size_t plan_blob_capacity(int max_tris, int H, size_t n_tiles, size_t bins_cap) {
    const size_t n_work = (size_t)max_tris * ((size_t)H / kPlanRasterRows + 3);
    return std::max(plan_blob_layout(max_tris, 0, n_tiles + 1, bins_cap, true).used, plan_blob_layout(max_tris, n_work, 0, 0, false).used);
}

// the plan's arrays into a host blob laid out as `l` (the header and the warp records are the caller's: pack_warp_records writes the latter in place)
inline void fill_plan_blob(uint8_t* blob, const PlanBlobLayout& l, const FramePlan& plan, bool fused) {
    const size_t T = (size_t)plan.n_tris;
    auto put = [blob](size_t off, const void* src, size_t bytes) { if (bytes) memcpy(blob + off, src, bytes); };
    put(l.o_edges, plan.raster.data(), T * sizeof(RasterTri));
    if (fused) {
        put(l.o_outl, plan.outline.data(), T * 3 * sizeof(OutlineSeg));
        put(l.o_toff, plan.tile_off.data(), plan.tile_off.size() * 4);
        put(l.o_ttri, plan.tile_tris.data(), plan.tile_tris.size() * 2);
    } else if (T) {
        put(l.o_tri, plan.tri_xy.data(), T * 6 * sizeof(int));
        put(l.o_inv, plan.inv1.data(), T * 9 * sizeof(float));
        put(l.o_inv + T * 9 * sizeof(float), plan.inv2.data(), T * 9 * sizeof(float));
        put(l.o_work, plan.work.data(), plan.work.size() / 2 * 8);
    }
}

}  // namespace poppy_hip

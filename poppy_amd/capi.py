"""ctypes binding of libpoppy_hip.so — mirrors include/poppy_hip.h one to one.

Importing this module never touches the GPU; Context() does and raises if there is no usable
gfx950 device or the extension is missing (no fallback path exists).
"""
import ctypes as C
import os
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# POPPY_HIP_LIB: another build of the same sources (tools/experiments load libpoppy_hip_experiments.so, `python -m poppy_amd.build --experiments`,
# the only build in which the result-changing measurement switches exist); tests and bench.py run on the shipped library
SO_PATH = os.environ.get("POPPY_HIP_LIB") or os.path.join(HERE, "libpoppy_hip.so")

_lib = None


class PoppySettings(C.Structure):
    _fields_ = [("number_of_frames", C.c_int), ("match_tolerance", C.c_double), ("max_keypoints", C.c_int),
                ("pyramid_levels", C.c_int), ("enable_radial_mask", C.c_int), ("enable_auto_align", C.c_int)]


WARP_KERNELS = ("k_warp_bin", "k_warp_tile", "k_warp4")        # order of poppy_hip_warp_counts
# kinds 1.. of poppy_hip_last_pyramid_forms (POPPY_PYR_*)
PYRAMID_FORMS = ("down", "down2", "tail", "tail_nl", "mix_top", "cone", "up2", "up", "unsharp")
WRITE_CB = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(C.c_uint8), C.c_int, C.c_int, C.c_size_t)
# formats of the frames handed to writers (poppy_hip_set_frame_format) and the file sinks (poppy_sink_open)
FRAME_BGR, FRAME_I420, FRAME_PAL8, FRAME_PAL8_SEQ, FRAME_GIF, FRAME_GIF_SEQ, FRAME_JPEG, FRAME_JPEG444 = 0, 1, 8, 16, 64, 128, 256, 512
FRAME_PNG, FRAME_PNG_RUNS = 1024, 2048
FRAME_JPEG_OPT, FRAME_JPEG444_OPT = 4096, 8192
FRAME_JPEG_SEQ, FRAME_JPEG444_SEQ = 32768, 65536      # JPEG_OPT's frames on one Huffman table set for all the frames a call hands to its writer
FRAME_PNG_OPT = 16384
FRAME_PNG_SEQ = 131072      # PNG_OPT's frames on one ninth table for all the frames a call hands to its writer
FRAMES_CODED = (FRAME_GIF, FRAME_GIF_SEQ, FRAME_JPEG, FRAME_JPEG444, FRAME_PNG, FRAME_PNG_RUNS, FRAME_JPEG_OPT, FRAME_JPEG444_OPT, FRAME_PNG_OPT, FRAME_JPEG_SEQ, FRAME_JPEG444_SEQ, FRAME_PNG_SEQ)      # a frame whose length its first four bytes hold
JPEG_QUALITY_DEFAULT = 90
SINK_RAW, SINK_PPM, SINK_Y4M, SINK_Y4M420, SINK_GIF, SINK_GIF_GLOBAL, SINK_GIF_CODED, SINK_GIF_GLOBAL_CODED, SINK_MJPEG = 0, 1, 2, 3, 8, 16, 64, 128, 256
SINK_PNG = 1024
PNG_SEGMENT_BYTES, PNG_TABLES, PNG_HEADER_BYTES = 8192, 8, 236
PNG_RUN_MIN, PNG_RUNS_SYMBOLS = 8, 286
PNG_SEQ_MAX_SYMBOLS, PNG_SEQ_HEADER_BYTES = (1 << 32) - 1, 261

# every symbol include/poppy_hip.h declares (tests check the library exports all of them)
SYMBOLS = [
    "poppy_settings_default", "poppy_hip_create", "poppy_hip_destroy", "poppy_hip_last_error", "poppy_hip_create_error",
    "poppy_hip_morph_images", "poppy_hip_pair_load", "poppy_hip_pair_load_device", "poppy_hip_render", "poppy_hip_pair_reset",
    "poppy_hip_frame_device", "poppy_hip_frame_wait", "poppy_hip_frame_stream", "poppy_hip_sync", "poppy_hip_stream", "poppy_frame_ratio", "poppy_hip_morph_frames",
    "poppy_hip_dissolve", "poppy_hip_set_debug", "poppy_hip_last_warp_kind", "poppy_warp_records", "poppy_hip_hamming_knn2", "poppy_ratio_symmetry",
    "poppy_hip_pair_begin_descriptors", "poppy_hip_warp_affine", "poppy_hip_auto_align", "poppy_hip_align_step",
    "poppy_procrustes", "poppy_perspective_from4", "poppy_hip_pair_corrected2", "poppy_hip_debug_fetch", "poppy_hip_debug_triangles", "poppy_plan_frame", "poppy_plan_tile_counts", "poppy_plan_tile_tris", "poppy_plan_blob_layout",
    "poppy_hip_timing_summary", "poppy_hip_set_timing", "poppy_hip_render_many",
    "poppy_hip_orb_describe", "poppy_hip_hamming_match",
    "poppy_sink_open", "poppy_sink_write", "poppy_sink_close", "poppy_hip_render_phases", "poppy_hip_pool_set_timing", "poppy_hip_pool_timing_summary", "poppy_hip_pool_warp_counts", "poppy_hip_pool_create", "poppy_hip_pool_create_tuned", "poppy_hip_pool_destroy", "poppy_hip_pool_morph_pairs", "poppy_hip_pool_submit_pairs", "poppy_hip_pool_wait", "poppy_count_pair_frames_cb", "poppy_hip_warp_counts", "poppy_hip_time_last_warp", "poppy_hip_mask_rider", "poppy_hip_pool_mask_rider", "poppy_hip_comm_id", "poppy_hip_comm_init", "poppy_hip_comm_free", "poppy_hip_comm_info", "poppy_hip_pair_broadcast", "poppy_hip_comm_max",
    "poppy_hip_pair_begin_sharded", "poppy_hip_sharded_setups", "poppy_hip_pair_begin_sharded_local", "poppy_hip_pair_state_bytes", "poppy_hip_pair_export_device", "poppy_hip_pair_import_device", "poppy_hip_morph_sharded", "poppy_hip_morph_pairs",
    "poppy_dft_plan", "poppy_hip_pair_begin_device", "poppy_count_frames_cb", "poppy_hip_morph", "poppy_hip_pair_distance", "poppy_printed_morph_distance", "poppy_hypotf_selfcheck",
    "poppy_hip_orb_detect", "poppy_hip_foreground", "poppy_hip_median_blur", "poppy_median_cols_geom", "poppy_median_cols_hint", "poppy_hip_foreground_median_links", "poppy_match_points", "poppy_hip_pair_begin_prefiltered", "poppy_hip_pair_begin", "poppy_hip_pair_begin_info", "poppy_hip_orb_input", "poppy_hip_gabor_field", "poppy_hip_set_gabor_direct", "poppy_hip_set_setup_chains", "poppy_hip_gabor_doubt", "poppy_radial_gradient", "poppy_radial_mask", "poppy_gabor_tables", "poppy_gabor_rounding_in_doubt", "poppy_gabor_band_unit", "poppy_pyr_tail_plan", "poppy_hip_blur_margin", "poppy_hip_pair_points",
    "poppy_hip_pair_begin_next", "poppy_hip_pair_begin_next_device", "poppy_hip_chain_counts", "poppy_hip_morph_list",
    "poppy_hip_last_pyramid_forms",
    "poppy_hip_set_frame_format", "poppy_hip_pool_set_frame_format", "poppy_frame_bytes", "poppy_bgr_to_i420", "poppy_bgr_to_pal8", "poppy_bgr_frames_to_pal8",
    "poppy_gif_frame_bytes", "poppy_pal8_to_gif_frame", "poppy_bgr_to_gif_frame", "poppy_hip_pal8_to_gif_frame",
    "poppy_bgr_frames_to_gif_frames", "poppy_hip_bgr_frames_to_gif_frames",
    "poppy_jpeg_frame_bytes", "poppy_i420_to_jpeg_frame", "poppy_bgr_to_jpeg_frame", "poppy_hip_i420_to_jpeg_frame", "poppy_hip_set_jpeg_quality", "poppy_hip_pool_set_jpeg_quality",
    "poppy_jpeg_budget_pick", "poppy_jpeg_frame_quality", "poppy_i420_to_jpeg_budget_frame", "poppy_i444_to_jpeg_budget_frame", "poppy_bgr_to_jpeg_budget_frame",
    "poppy_bgr_to_jpeg444_budget_frame", "poppy_hip_i420_to_jpeg_budget_frame", "poppy_hip_i444_to_jpeg_budget_frame", "poppy_hip_set_jpeg_budget",
    "poppy_hip_get_jpeg_budget", "poppy_hip_pool_set_jpeg_budget",
    "poppy_i420_frames_to_jpeg_seq_budget_frames", "poppy_i444_frames_to_jpeg_seq_budget_frames", "poppy_bgr_frames_to_jpeg_seq_budget_frames",
    "poppy_bgr_frames_to_jpeg444_seq_budget_frames", "poppy_hip_bgr_frames_to_jpeg_seq_budget_frames", "poppy_hip_bgr_frames_to_jpeg444_seq_budget_frames",
    "poppy_hip_set_jpeg_sequence_budget", "poppy_hip_get_jpeg_sequence_budget", "poppy_hip_pool_set_jpeg_sequence_budget",
    "poppy_bgr_to_i444", "poppy_hip_bgr_to_i444", "poppy_i444_to_jpeg_frame", "poppy_bgr_to_jpeg444_frame", "poppy_hip_i444_to_jpeg_frame",
    "poppy_jpeg_optimal_table", "poppy_i420_to_jpeg_opt_frame", "poppy_i444_to_jpeg_opt_frame", "poppy_bgr_to_jpeg_opt_frame", "poppy_bgr_to_jpeg444_opt_frame",
    "poppy_hip_i420_to_jpeg_opt_frame", "poppy_hip_i444_to_jpeg_opt_frame", "poppy_hip_jpeg_optimal_table",
    "poppy_i420_frames_to_jpeg_seq_frames", "poppy_i444_frames_to_jpeg_seq_frames", "poppy_bgr_frames_to_jpeg_seq_frames", "poppy_bgr_frames_to_jpeg444_seq_frames",
    "poppy_hip_bgr_frames_to_jpeg_seq_frames", "poppy_hip_bgr_frames_to_jpeg444_seq_frames",
    "poppy_png_frame_bytes", "poppy_png_table", "poppy_bgr_to_png_frame", "poppy_hip_bgr_to_png_frame",
    "poppy_png_runs_table", "poppy_bgr_to_png_runs_frame", "poppy_hip_bgr_to_png_runs_frame",
    "poppy_png_optimal_lengths", "poppy_bgr_to_png_opt_frame", "poppy_hip_bgr_to_png_opt_frame", "poppy_hip_png_optimal_lengths",
    "poppy_png_seq_table", "poppy_bgr_frames_to_png_seq_frames", "poppy_hip_bgr_frames_to_png_seq_frames", "poppy_hip_png_seq_table",
    "poppy_hip_set_frame_scale", "poppy_hip_pool_set_frame_scale", "poppy_frame_scaled_size", "poppy_bgr_downscale", "poppy_hip_bgr_downscale",
    "poppy_hip_set_frame_size", "poppy_hip_pool_set_frame_size", "poppy_frame_fit_size", "poppy_bgr_resize_area", "poppy_hip_bgr_resize_area",
    "poppy_hip_bgr_resize_area_form",
    "poppy_hip_unsharp_frame", "poppy_hip_align_scores",
    "poppy_ransac_fundamental", "poppy_hip_ransac_fundamental", "poppy_hip_pair_begin_descriptors_ransac", "poppy_hip_pair_fundamental",
    "poppy_blur_margin_rects", "poppy_blur_margin_taps", "poppy_hip_blur_margin_max_rows",
    "poppy_denoise_weights", "poppy_bgr_denoise", "poppy_denoise_tile", "poppy_denoise_table_bound",
    "poppy_hip_denoise", "poppy_hip_denoise_device", "poppy_hip_set_denoise", "poppy_hip_get_denoise",
]


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(SO_PATH):
            raise RuntimeError(f"{SO_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                               "(the HIP extension is the product; there is no fallback)")
        L = C.CDLL(SO_PATH)
        L.poppy_hip_create.restype = C.c_void_p
        L.poppy_hip_create.argtypes = [C.c_int, C.POINTER(PoppySettings)]
        L.poppy_hip_destroy.argtypes = [C.c_void_p]
        L.poppy_hip_last_error.restype = C.c_char_p
        L.poppy_hip_last_error.argtypes = [C.c_void_p]
        L.poppy_hip_create_error.restype = C.c_char_p
        L.poppy_frame_ratio.restype = C.c_double
        L.poppy_frame_ratio.argtypes = [C.c_int, C.c_int, C.c_double]
        L.poppy_hip_frame_device.restype = C.c_void_p
        L.poppy_hip_frame_device.argtypes = [C.c_void_p]
        L.poppy_hip_stream.restype = C.c_void_p
        L.poppy_hip_stream.argtypes = [C.c_void_p]
        L.poppy_hip_frame_stream.restype = C.c_void_p
        L.poppy_hip_frame_stream.argtypes = [C.c_void_p]
        L.poppy_hip_frame_wait.argtypes = [C.c_void_p, C.c_void_p]
        vp, sz, i, d = C.c_void_p, C.c_size_t, C.c_int, C.c_double
        L.poppy_hip_morph_images.argtypes = [vp, vp, sz, vp, sz, vp, i, i, vp, vp, i, d, d, vp, sz, vp]
        L.poppy_hip_pair_load.argtypes = [vp, vp, sz, vp, sz, vp, i, i, vp, vp, i]
        L.poppy_hip_pair_load_device.argtypes = [vp, vp, vp, vp, i, i, vp, vp, i]
        L.poppy_hip_render.argtypes = [vp, d, d, i, vp, sz]
        L.poppy_hip_pair_reset.argtypes = [vp]
        L.poppy_hip_sync.argtypes = [vp]
        L.poppy_hip_morph_frames.argtypes = [vp, d, vp, vp]
        L.poppy_hip_dissolve.argtypes = [vp, vp, sz, vp, sz, i, i, d, vp, sz]
        L.poppy_hip_set_debug.argtypes = [vp, i]
        L.poppy_hip_last_warp_kind.argtypes = [vp]
        L.poppy_hip_last_pyramid_forms.argtypes = [vp, vp, i]
        L.poppy_hip_set_timing.argtypes = [vp, i]
        L.poppy_hip_debug_fetch.argtypes = [vp, C.c_char_p, vp, sz]
        L.poppy_hip_debug_triangles.argtypes = [vp, vp, vp, vp, vp, i]
        L.poppy_plan_frame.argtypes = [i, i, vp, vp, i, d, i, vp, vp, vp, vp, vp, vp, vp, vp]
        L.poppy_plan_tile_counts.argtypes = [i, i, vp, vp, i, d, i, vp, i, vp, vp, vp]
        L.poppy_plan_tile_tris.argtypes = [i, i, vp, vp, i, d, i, vp, C.c_longlong, vp]
        L.poppy_plan_blob_layout.argtypes = [i, i, C.c_longlong, C.c_longlong, C.c_longlong, i, vp]
        L.poppy_warp_records.argtypes = [vp, vp, i, i, i, vp]
        L.poppy_hip_hamming_knn2.argtypes = [vp, vp, i, vp, i, vp]
        L.poppy_hip_warp_affine.argtypes = [vp, vp, C.c_size_t, i, i, vp, vp, C.c_size_t]
        L.poppy_hip_auto_align.argtypes = [vp, vp, C.c_size_t, i, i, vp, vp, i, vp]
        L.poppy_hip_align_step.argtypes = [vp, i, vp, C.c_size_t, i, i, vp, vp, i, vp]
        L.poppy_hip_align_scores.argtypes = [vp, vp, vp, i, i, i, i, vp, vp, vp, vp]
        L.poppy_procrustes.argtypes = [vp, vp, i, vp, vp, vp]
        L.poppy_hip_pair_corrected2.argtypes = [vp, vp, C.c_size_t]
        L.poppy_perspective_from4.argtypes = [vp, vp, vp]
        L.poppy_ratio_symmetry.argtypes = [vp, i, vp, i, C.c_float, vp, vp]
        L.poppy_hip_pair_begin_descriptors.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, i, i, C.c_float]
        L.poppy_hip_pair_begin_descriptors_ransac.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, i, i, C.c_float, d]
        L.poppy_ransac_fundamental.argtypes = [vp, vp, i, d, vp, vp, vp, vp, vp, vp]
        L.poppy_hip_ransac_fundamental.argtypes = [vp, vp, vp, i, d, vp, vp, vp, vp, vp, vp]
        L.poppy_hip_pair_fundamental.argtypes = [vp, vp, vp, vp, vp]
        L.poppy_hip_timing_summary.argtypes = [vp, vp, vp, vp, i]
        L.poppy_hip_render_many.argtypes = [vp, vp, vp, i, i, vp, vp]
        L.poppy_hip_orb_detect.argtypes = [vp, vp, sz, i, i, i, vp, i, vp]
        L.poppy_hip_foreground.argtypes = [vp, vp, sz, i, i, vp, vp]
        L.poppy_hip_median_blur.argtypes = [vp, vp, i, i, i, i, vp]
        L.poppy_median_cols_geom.argtypes = [i, i, vp, vp, vp, vp]
        L.poppy_median_cols_hint.argtypes = [vp, sz, i, i]
        L.poppy_hip_foreground_median_links.argtypes = [vp, i, vp, vp]
        L.poppy_hip_unsharp_frame.argtypes = [vp, vp, i, i, i, C.c_float, i, i, vp, vp]
        L.poppy_hip_comm_info.argtypes = [vp, vp, vp, vp, vp]
        L.poppy_hip_pair_begin.argtypes = [vp, vp, sz, vp, sz, i, i]
        L.poppy_hip_pair_begin_info.argtypes = [vp, vp, vp]
        L.poppy_hip_orb_input.argtypes = [vp, vp, i, i, vp, vp, vp, vp]
        L.poppy_hip_gabor_field.argtypes = [vp, vp, sz, i, i, vp]
        L.poppy_hip_set_gabor_direct.argtypes = [vp, i]
        L.poppy_hip_set_setup_chains.argtypes = [vp, i]
        L.poppy_radial_gradient.argtypes = [i, i, vp]
        L.poppy_radial_mask.argtypes = [i, i, vp]
        L.poppy_gabor_tables.argtypes = [i, vp, vp]
        L.poppy_gabor_rounding_in_doubt.argtypes = [C.c_double, C.c_double]
        L.poppy_gabor_band_unit.argtypes = []
        L.poppy_gabor_band_unit.restype = C.c_double
        L.poppy_pyr_tail_plan.argtypes = [i, i, i, i, vp, vp]
        L.poppy_hip_blur_margin.argtypes = [vp, vp, sz, i, i, i, i, vp, sz]
        L.poppy_blur_margin_rects.argtypes = [i, i, i, i, vp, vp]
        L.poppy_blur_margin_taps.argtypes = [vp]
        L.poppy_hip_blur_margin_max_rows.argtypes = [vp, vp]
        L.poppy_denoise_weights.argtypes = [C.c_float, i, i, vp, i, vp, vp, vp, vp]
        L.poppy_bgr_denoise.argtypes = [vp, sz, i, i, C.c_float, i, i, vp, sz]
        L.poppy_denoise_tile.argtypes = [vp, vp]
        L.poppy_denoise_table_bound.argtypes = [vp]
        L.poppy_hip_denoise.argtypes = [vp, vp, sz, i, i, C.c_float, i, i, vp, sz]
        L.poppy_hip_denoise_device.argtypes = [vp, vp, vp, i, i, C.c_float, i, i]
        L.poppy_hip_set_denoise.argtypes = [vp, C.c_float, i, i]
        L.poppy_hip_get_denoise.argtypes = [vp, vp, vp, vp]
        L.poppy_hip_orb_describe.argtypes = [vp, vp, sz, i, i, vp, i, vp]
        L.poppy_hip_hamming_match.argtypes = [vp, vp, i, vp, i, vp, vp]
        L.poppy_match_points.argtypes = [vp, vp, i, i, i, d, vp, vp, vp, vp]
        L.poppy_hip_pair_begin_prefiltered.argtypes = [vp, vp, sz, vp, sz, vp, vp, vp, i, i, i]
        L.poppy_hip_pair_begin.argtypes = [vp, vp, sz, vp, sz, i, i]
        L.poppy_hip_pair_points.argtypes = [vp, vp, vp, i, vp]
        L.poppy_dft_plan.argtypes = [i, vp, vp, vp, vp]
        L.poppy_hip_warp_counts.argtypes = [vp, vp, vp, vp]
        L.poppy_hip_mask_rider.argtypes = [vp]
        L.poppy_hip_time_last_warp.argtypes = [vp, i, vp]
        L.poppy_hip_pool_mask_rider.argtypes = [vp]
        L.poppy_hip_pool_create.restype = C.c_void_p
        L.poppy_hip_pool_create.argtypes = [vp, i, i, vp, vp, sz]
        L.poppy_hip_pool_create_tuned.restype = C.c_void_p
        L.poppy_hip_pool_create_tuned.argtypes = [vp, i, i, vp, i, i, i, vp, vp, vp, vp, sz]
        L.poppy_hip_pool_destroy.argtypes = [vp]
        L.poppy_hip_render_phases.argtypes = [vp, vp, i, vp, vp]
        L.poppy_sink_open.restype = C.c_void_p
        L.poppy_sink_open.argtypes = [C.c_char_p, i, i, i, i, i]
        L.poppy_sink_write.argtypes = [vp, vp, i, i, sz]
        L.poppy_sink_close.argtypes = [vp]
        L.poppy_hip_pool_set_timing.argtypes = [vp, i]
        L.poppy_hip_pool_timing_summary.argtypes = [vp, vp, vp, vp, i]
        L.poppy_hip_pool_warp_counts.argtypes = [vp, vp, vp, vp]
        L.poppy_hip_pool_morph_pairs.argtypes = [vp, i, i, i, d, i, vp, vp, vp, vp, sz]
        L.poppy_hip_pool_submit_pairs.argtypes = [vp, i, i, i, d, i, vp, vp, vp]
        L.poppy_hip_pool_wait.argtypes = [vp, vp, sz]
        L.poppy_hip_comm_id.argtypes = [vp]
        L.poppy_hip_comm_init.argtypes = [vp, i, i, vp]
        L.poppy_hip_comm_free.argtypes = [vp]
        L.poppy_hip_pair_broadcast.argtypes = [vp, i, i, i]
        L.poppy_hip_comm_max.argtypes = [vp, vp]
        L.poppy_hip_pair_state_bytes.argtypes = [i, i, vp]
        L.poppy_hip_pair_export_device.argtypes = [vp, vp, sz]
        L.poppy_hip_pair_import_device.argtypes = [vp, vp, sz, i, i]
        L.poppy_hip_morph_sharded.argtypes = [vp, i, vp, vp, sz, vp, sz, i, i, i, vp, vp, vp, sz]
        L.poppy_hip_morph_pairs.argtypes = [vp, i, i, vp, i, i, i, d, vp, vp, vp, vp, sz]
        L.poppy_hip_pair_begin_device.argtypes = [vp, vp, vp, i, i]
        L.poppy_hip_pair_begin_next.argtypes = [vp, vp, sz, i, i]
        L.poppy_hip_pair_begin_next_device.argtypes = [vp, vp, i, i]
        L.poppy_hip_chain_counts.argtypes = [vp, vp, vp]
        L.poppy_hip_morph_list.argtypes = [vp, i, i, i, d, i, vp, vp, vp, vp, vp]
        L.poppy_hip_pair_begin_sharded.argtypes = [vp, vp, vp, i, i, i]
        L.poppy_hip_pair_begin_sharded_local.argtypes = [C.POINTER(vp), i, vp, vp, i, i, i]
        L.poppy_hip_morph.argtypes = [vp, vp, sz, vp, sz, i, i, d, i, vp, vp, vp]
        L.poppy_hip_pair_distance.argtypes = [vp, vp]
        L.poppy_printed_morph_distance.argtypes = [vp, vp, i, i, i, vp]
        L.poppy_hip_set_frame_format.argtypes = [vp, i]
        L.poppy_hip_pool_set_frame_format.argtypes = [vp, i]
        L.poppy_frame_bytes.restype = sz
        L.poppy_frame_bytes.argtypes = [i, i, i]
        L.poppy_bgr_to_i420.argtypes = [vp, sz, i, i, vp]
        L.poppy_bgr_to_pal8.argtypes = [vp, sz, i, i, vp]
        L.poppy_bgr_frames_to_pal8.argtypes = [vp, sz, sz, i, i, i, vp]
        L.poppy_gif_frame_bytes.restype = sz
        L.poppy_gif_frame_bytes.argtypes = [vp]
        L.poppy_pal8_to_gif_frame.argtypes = [vp, i, i, vp]
        L.poppy_bgr_to_gif_frame.argtypes = [vp, sz, i, i, vp]
        L.poppy_hip_pal8_to_gif_frame.argtypes = [vp, vp, i, i, vp]
        L.poppy_bgr_frames_to_gif_frames.argtypes = [vp, sz, sz, i, i, i, vp]
        L.poppy_hip_bgr_frames_to_gif_frames.argtypes = [vp, vp, sz, sz, i, i, i, vp]
        L.poppy_jpeg_frame_bytes.restype = sz
        L.poppy_jpeg_frame_bytes.argtypes = [vp]
        L.poppy_i420_to_jpeg_frame.argtypes = [vp, i, i, i, vp]
        L.poppy_bgr_to_jpeg_frame.argtypes = [vp, sz, i, i, i, vp]
        L.poppy_hip_i420_to_jpeg_frame.argtypes = [vp, vp, i, i, i, vp]
        L.poppy_hip_set_jpeg_quality.argtypes = [vp, i]
        L.poppy_bgr_to_i444.argtypes = [vp, sz, i, i, vp]
        L.poppy_hip_bgr_to_i444.argtypes = [vp, vp, sz, i, i, vp]
        L.poppy_i444_to_jpeg_frame.argtypes = [vp, i, i, i, vp]
        L.poppy_bgr_to_jpeg444_frame.argtypes = [vp, sz, i, i, i, vp]
        L.poppy_hip_i444_to_jpeg_frame.argtypes = [vp, vp, i, i, i, vp]
        L.poppy_hip_pool_set_jpeg_quality.argtypes = [vp, i]
        L.poppy_jpeg_budget_pick.argtypes = [vp, i, sz]
        L.poppy_jpeg_frame_quality.argtypes = [vp]
        L.poppy_i420_to_jpeg_budget_frame.argtypes = [vp, i, i, i, sz, vp, vp]
        L.poppy_i444_to_jpeg_budget_frame.argtypes = [vp, i, i, i, sz, vp, vp]
        L.poppy_bgr_to_jpeg_budget_frame.argtypes = [vp, sz, i, i, i, sz, vp, vp]
        L.poppy_bgr_to_jpeg444_budget_frame.argtypes = [vp, sz, i, i, i, sz, vp, vp]
        L.poppy_hip_i420_to_jpeg_budget_frame.argtypes = [vp, vp, i, i, i, sz, vp, vp]
        L.poppy_hip_i444_to_jpeg_budget_frame.argtypes = [vp, vp, i, i, i, sz, vp, vp]
        L.poppy_hip_set_jpeg_budget.argtypes = [vp, sz]
        L.poppy_hip_get_jpeg_budget.argtypes = [vp, vp]
        L.poppy_hip_pool_set_jpeg_budget.argtypes = [vp, sz]
        u64 = C.c_uint64
        L.poppy_i420_frames_to_jpeg_seq_budget_frames.argtypes = [vp, sz, i, i, i, i, u64, vp, vp]
        L.poppy_i444_frames_to_jpeg_seq_budget_frames.argtypes = [vp, sz, i, i, i, i, u64, vp, vp]
        L.poppy_bgr_frames_to_jpeg_seq_budget_frames.argtypes = [vp, sz, sz, i, i, i, i, u64, vp, vp]
        L.poppy_bgr_frames_to_jpeg444_seq_budget_frames.argtypes = [vp, sz, sz, i, i, i, i, u64, vp, vp]
        L.poppy_hip_bgr_frames_to_jpeg_seq_budget_frames.argtypes = [vp, vp, sz, sz, i, i, i, i, u64, vp, vp]
        L.poppy_hip_bgr_frames_to_jpeg444_seq_budget_frames.argtypes = [vp, vp, sz, sz, i, i, i, i, u64, vp, vp]
        L.poppy_hip_set_jpeg_sequence_budget.argtypes = [vp, u64]
        L.poppy_hip_get_jpeg_sequence_budget.argtypes = [vp, vp]
        L.poppy_hip_pool_set_jpeg_sequence_budget.argtypes = [vp, u64]
        L.poppy_jpeg_optimal_table.argtypes = [vp, vp, vp, vp]
        L.poppy_hip_jpeg_optimal_table.argtypes = [vp, vp, vp, vp, vp]
        L.poppy_i420_to_jpeg_opt_frame.argtypes = [vp, i, i, i, vp]
        L.poppy_i444_to_jpeg_opt_frame.argtypes = [vp, i, i, i, vp]
        L.poppy_bgr_to_jpeg_opt_frame.argtypes = [vp, sz, i, i, i, vp]
        L.poppy_bgr_to_jpeg444_opt_frame.argtypes = [vp, sz, i, i, i, vp]
        L.poppy_hip_i420_to_jpeg_opt_frame.argtypes = [vp, vp, i, i, i, vp]
        L.poppy_hip_i444_to_jpeg_opt_frame.argtypes = [vp, vp, i, i, i, vp]
        L.poppy_i420_frames_to_jpeg_seq_frames.argtypes = [vp, sz, i, i, i, i, vp]
        L.poppy_i444_frames_to_jpeg_seq_frames.argtypes = [vp, sz, i, i, i, i, vp]
        L.poppy_bgr_frames_to_jpeg_seq_frames.argtypes = [vp, sz, sz, i, i, i, i, vp]
        L.poppy_bgr_frames_to_jpeg444_seq_frames.argtypes = [vp, sz, sz, i, i, i, i, vp]
        L.poppy_hip_bgr_frames_to_jpeg_seq_frames.argtypes = [vp, vp, sz, sz, i, i, i, i, vp]
        L.poppy_hip_bgr_frames_to_jpeg444_seq_frames.argtypes = [vp, vp, sz, sz, i, i, i, i, vp]
        L.poppy_png_frame_bytes.restype = sz
        L.poppy_png_frame_bytes.argtypes = [vp]
        L.poppy_png_table.argtypes = [i, vp, vp, vp]
        L.poppy_bgr_to_png_frame.argtypes = [vp, sz, i, i, vp]
        L.poppy_hip_bgr_to_png_frame.argtypes = [vp, vp, sz, i, i, vp]
        L.poppy_png_runs_table.argtypes = [i, vp, vp, vp]
        L.poppy_bgr_to_png_runs_frame.argtypes = [vp, sz, i, i, vp]
        L.poppy_hip_bgr_to_png_runs_frame.argtypes = [vp, vp, sz, i, i, vp]
        L.poppy_png_optimal_lengths.argtypes = [vp, i, i, vp]
        L.poppy_bgr_to_png_opt_frame.argtypes = [vp, sz, i, i, vp]
        L.poppy_hip_bgr_to_png_opt_frame.argtypes = [vp, vp, sz, i, i, vp]
        L.poppy_hip_png_optimal_lengths.argtypes = [vp, vp, i, i, vp]
        L.poppy_png_seq_table.argtypes = [vp, vp, vp, vp]
        L.poppy_bgr_frames_to_png_seq_frames.argtypes = [vp, sz, sz, i, i, i, vp]
        L.poppy_hip_bgr_frames_to_png_seq_frames.argtypes = [vp, vp, sz, sz, i, i, i, vp]
        L.poppy_hip_png_seq_table.argtypes = [vp, vp, vp, vp, vp]
        L.poppy_hip_set_frame_scale.argtypes = [vp, i]
        L.poppy_hip_pool_set_frame_scale.argtypes = [vp, i]
        L.poppy_frame_scaled_size.argtypes = [i, i, i, vp, vp]
        L.poppy_bgr_downscale.argtypes = [vp, sz, i, i, i, vp, sz]
        L.poppy_hip_bgr_downscale.argtypes = [vp, vp, sz, i, i, i, vp, sz]
        L.poppy_hip_set_frame_size.argtypes = [vp, i, i]
        L.poppy_hip_pool_set_frame_size.argtypes = [vp, i, i]
        L.poppy_frame_fit_size.argtypes = [i, i, i, i, vp, vp]
        L.poppy_bgr_resize_area.argtypes = [vp, sz, i, i, i, i, vp, sz]
        L.poppy_hip_bgr_resize_area.argtypes = [vp, vp, sz, i, i, i, i, vp, sz]
        L.poppy_hip_bgr_resize_area_form.argtypes = [i, i, i, i]
        L.poppy_hypotf_selfcheck.restype = C.c_long
        L.poppy_hypotf_selfcheck.argtypes = [C.c_long, C.c_uint64]
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


MEDIAN_BY_HINT, MEDIAN_BY_DEVICE, MEDIAN_BY_ENV = 1, 2, 3      # decided_by of Context.foreground_median_links (include/poppy_hip.h)


def median_cols_geom(w, h):
    """(tiles_x, tiles_y, rows, tile_cols): how k_median_cols cuts a w x h image (host only)."""
    v = [C.c_int(0) for _ in range(4)]
    if lib().poppy_median_cols_geom(int(w), int(h), *[C.byref(x) for x in v]) != 0:
        raise ValueError("median_cols_geom: bad size")
    return tuple(x.value for x in v)


def median_cols_hint(bgr):
    """1: the set-up's sparse sample of this host BGR image says "few values per tile" (its chain of medians takes k_median_cols), 0: not (host only)."""
    a = np.ascontiguousarray(bgr, np.uint8)
    h, w = a.shape[:2]
    r = lib().poppy_median_cols_hint(_p(a), w * 3, w, h)
    if r < 0:
        raise ValueError("median_cols_hint: bad image")
    return r


def frame_bytes(fmt, w, h):
    """Host-only: bytes of a w x h frame in format fmt (FRAME_BGR / FRAME_I420 / FRAME_PAL8 / FRAME_PAL8_SEQ; FRAME_GIF and FRAME_GIF_SEQ: the capacity, an upper bound for any
    content — a frame's own length is gif_frame_bytes; FRAME_JPEG and FRAME_JPEG444: the capacity too, a frame's own length is jpeg_frame_bytes; 0 for anything else)."""
    return int(lib().poppy_frame_bytes(int(fmt), int(w), int(h)))


def _padded_rows(bgr, row_pad):
    """An HxWx3 BGR frame as it is handed over, (array, stride, w, h): row_pad extra bytes per row, filled with a pattern no pixel may come from."""
    a = np.ascontiguousarray(bgr, np.uint8)
    h, w = a.shape[:2]
    stride = w * 3 + int(row_pad)
    if row_pad:
        buf = np.full((h, stride), 0xA5, np.uint8)
        buf[:, :w * 3] = a.reshape(h, w * 3)
        a = buf
    return a, stride, w, h


def _padded_frames(frames, row_pad, frame_pad):
    """n HxWx3 BGR frames as they are handed over, (array, stride, frame_stride, n, w, h): row_pad extra bytes per row and frame_pad between frames, filled alike."""
    a = np.ascontiguousarray(frames, np.uint8)
    n, h, w = a.shape[:3]
    stride = w * 3 + int(row_pad)
    frame_stride = stride * h + int(frame_pad)
    if row_pad or frame_pad:
        buf = np.full((n, frame_stride), 0xA5, np.uint8)
        buf[:, :stride * h].reshape(n, h, stride)[:, :, :w * 3] = a.reshape(n, h, w * 3)
        a = buf
    return a, stride, frame_stride, n, w, h


def bgr_to_i420(bgr):
    """Host-only: the library's I420 of an HxWx3 BGR frame (poppy_bgr_to_i420), as a flat uint8 array of frame_bytes(FRAME_I420, W, H)."""
    a = np.ascontiguousarray(bgr, np.uint8)
    h, w = a.shape[:2]
    out = np.empty(frame_bytes(FRAME_I420, w, h), np.uint8)
    rc = lib().poppy_bgr_to_i420(_p(a), w * 3, w, h, _p(out))
    if rc:
        raise PoppyError(f"poppy_bgr_to_i420: {rc}")
    return out


def bgr_to_pal8(bgr, row_pad=0):
    """Host-only: the library's PAL8 of an HxWx3 BGR frame (poppy_bgr_to_pal8), as a flat uint8 array of frame_bytes(FRAME_PAL8, W, H): W * H
    index bytes, then 256 R, G, B palette entries.  row_pad: the frame is handed over with that many extra bytes per row."""
    a, stride, w, h = _padded_rows(bgr, row_pad)
    out = np.empty(frame_bytes(FRAME_PAL8, w, h), np.uint8)
    rc = lib().poppy_bgr_to_pal8(_p(a), stride, w, h, _p(out))
    if rc:
        raise PoppyError(f"poppy_bgr_to_pal8: {rc}")
    return out


def bgr_frames_to_pal8(frames, row_pad=0, frame_pad=0):
    """Host-only: the library's PAL8_SEQ frames of a sequence of n HxWx3 BGR frames (poppy_bgr_frames_to_pal8): an n x frame_bytes(FRAME_PAL8_SEQ, W, H)
    uint8 array, every row W * H index bytes and the sequence's one palette.  row_pad / frame_pad: the frames are handed over with that many extra
    bytes per row / between frames."""
    a, stride, frame_stride, n, w, h = _padded_frames(frames, row_pad, frame_pad)
    out = np.empty((n, frame_bytes(FRAME_PAL8_SEQ, w, h)), np.uint8)
    rc = lib().poppy_bgr_frames_to_pal8(_p(a), stride, frame_stride, n, w, h, _p(out))
    if rc:
        raise PoppyError(f"poppy_bgr_frames_to_pal8: {rc}")
    return out


def coded_frame_bytes(frame, coder):
    """Host-only: `total` of a coded frame, its length in bytes (poppy_<coder>_frame_bytes, coder "gif", "jpeg" or "png": the first four bytes, little-endian)."""
    f = np.ascontiguousarray(frame, np.uint8)
    if f.size < 4:
        raise PoppyError(f"{coder}_frame_bytes: a coded frame has at least four bytes")
    return int(getattr(lib(), f"poppy_{coder}_frame_bytes")(_p(f)))


def gif_frame_bytes(frame):
    """Host-only: `total` of a FRAME_GIF frame, its length in bytes (poppy_gif_frame_bytes: the first four bytes, little-endian)."""
    return coded_frame_bytes(frame, "gif")


def jpeg_frame_bytes(frame):
    """Host-only: `total` of a FRAME_JPEG frame, its length in bytes (poppy_jpeg_frame_bytes: the first four bytes, little-endian)."""
    return coded_frame_bytes(frame, "jpeg")


def png_frame_bytes(frame):
    """Host-only: `total` of a FRAME_PNG, FRAME_PNG_RUNS, FRAME_PNG_OPT or FRAME_PNG_SEQ frame, its length in bytes (poppy_png_frame_bytes: the first four bytes, little-endian)."""
    return coded_frame_bytes(frame, "png")


def _coded_frame(call, what, w, h, fmt, chk=None):
    """A coded frame of format fmt out of call(dst), `what` by name, cut to its `total`.  chk(rc, what): the context's check; without one a status raises as poppy_<what>'s."""
    out = np.empty(max(frame_bytes(fmt, w, h), 4), np.uint8)
    rc = call(_p(out))
    if chk:
        chk(rc, what)
    elif rc:
        raise PoppyError(f"poppy_{what}: {rc}")
    return out[:coded_frame_bytes(out, "gif" if fmt == FRAME_GIF else "jpeg")].copy()


def _pal8_to_gif(call, pal8, w, h, chk=None):
    a = np.ascontiguousarray(pal8, np.uint8)
    if a.size != w * h + 768:
        raise PoppyError("pal8_to_gif_frame: a PAL8 frame has w * h + 768 bytes")
    return _coded_frame(lambda dst: call(_p(a), int(w), int(h), dst), "pal8_to_gif_frame", w, h, FRAME_GIF, chk)


def pal8_to_gif_frame(pal8, w, h):
    """Host-only: the FRAME_GIF frame of a flat PAL8 frame (poppy_pal8_to_gif_frame): `total`, the palette, the LZW-coded indices as GIF image data; a flat
    uint8 array of exactly `total` bytes."""
    return _pal8_to_gif(lib().poppy_pal8_to_gif_frame, pal8, w, h)


def bgr_to_gif_frame(bgr):
    """Host-only: the FRAME_GIF frame of an HxWx3 BGR frame (poppy_bgr_to_gif_frame = bgr_to_pal8, then pal8_to_gif_frame)."""
    a = np.ascontiguousarray(bgr, np.uint8)
    h, w = a.shape[:2]
    return _coded_frame(lambda dst: lib().poppy_bgr_to_gif_frame(_p(a), w * 3, w, h, dst), "bgr_to_gif_frame", w, h, FRAME_GIF)


def _planes_to_jpeg(call, fmt, planes, w, h, quality, chk=None):
    """The body of i420_to_jpeg_frame (fmt FRAME_JPEG), i444_to_jpeg_frame (FRAME_JPEG444) and their OPT forms, on the host or a context."""
    name, size, says = ("i444", 3 * w * h, "3 * w * h") if fmt in (FRAME_JPEG444, FRAME_JPEG444_OPT) else ("i420", frame_bytes(FRAME_I420, w, h), "w * h + 2 * cw * ch")
    a = np.ascontiguousarray(planes, np.uint8).ravel()
    if w > 0 and h > 0 and a.size != size:
        raise PoppyError(f"{name}_to_jpeg_frame: an {name.upper()} frame has {says} bytes")
    return _coded_frame(lambda dst: call(_p(a), int(w), int(h), int(quality), dst), f"{name}_to_jpeg_frame", w, h, fmt, chk)


def i420_to_jpeg_frame(i420, w, h, quality=JPEG_QUALITY_DEFAULT):
    """Host-only: the FRAME_JPEG frame of a flat I420 frame (poppy_i420_to_jpeg_frame): `total`, then one baseline JFIF file; a flat uint8 array of its own length."""
    return _planes_to_jpeg(lib().poppy_i420_to_jpeg_frame, FRAME_JPEG, i420, w, h, quality)


def jpeg_budget_pick(sizes, quality_max, budget):
    """Host-only: the quality the byte budget's search picks on a table of file sizes, sizes[q] for q = 1..quality_max (entry 0 is not read)
    (poppy_jpeg_budget_pick); PoppyError with the status on a refusal."""
    a = None if sizes is None else np.ascontiguousarray(sizes, np.uint32)
    if a is not None and a.size <= int(quality_max) and 1 <= int(quality_max) <= 100:
        raise PoppyError("jpeg_budget_pick: the table has quality_max + 1 entries")
    rc = lib().poppy_jpeg_budget_pick(None if a is None else _p(a), int(quality_max), int(budget))
    if rc < 0:
        raise PoppyError(f"poppy_jpeg_budget_pick: {rc}")
    return rc


def jpeg_frame_quality(frame):
    """Host-only: the quality whose tables a JPEG frame of any of the six formats carries in its DQT, the largest of equals (poppy_jpeg_frame_quality); 0 if none
    does or the frame is no such frame."""
    a = np.ascontiguousarray(frame, np.uint8).ravel()
    if a.size < 4 or a.size < coded_frame_bytes(a, "jpeg"):
        return 0
    return lib().poppy_jpeg_frame_quality(_p(a))


def _planes_to_jpeg_budget(call, fmt, planes, w, h, quality_max, budget, chk=None):
    """The body of i420_to_jpeg_budget_frame (fmt FRAME_JPEG) and i444_to_jpeg_budget_frame (FRAME_JPEG444), on the host or a context: (frame, quality used)."""
    name, size, says = ("i444", 3 * w * h, "3 * w * h") if fmt == FRAME_JPEG444 else ("i420", frame_bytes(FRAME_I420, w, h), "w * h + 2 * cw * ch")
    a = np.ascontiguousarray(planes, np.uint8).ravel()
    if w > 0 and h > 0 and a.size != size:
        raise PoppyError(f"{name}_to_jpeg_budget_frame: an {name.upper()} frame has {says} bytes")
    used = C.c_int(0)
    frame = _coded_frame(lambda dst: call(_p(a), int(w), int(h), int(quality_max), int(budget), dst, C.byref(used)), f"{name}_to_jpeg_budget_frame", w, h, fmt, chk)
    return frame, used.value


def i420_to_jpeg_budget_frame(i420, w, h, quality_max, budget):
    """Host-only: (the FRAME_JPEG frame of a flat I420 frame at the quality the byte budget's search picks at or below quality_max, that quality)
    (poppy_i420_to_jpeg_budget_frame)."""
    return _planes_to_jpeg_budget(lib().poppy_i420_to_jpeg_budget_frame, FRAME_JPEG, i420, w, h, quality_max, budget)


def i444_to_jpeg_budget_frame(i444, w, h, quality_max, budget):
    """Host-only: the same for FRAME_JPEG444 on flat I444 planes (poppy_i444_to_jpeg_budget_frame)."""
    return _planes_to_jpeg_budget(lib().poppy_i444_to_jpeg_budget_frame, FRAME_JPEG444, i444, w, h, quality_max, budget)


def bgr_to_jpeg_budget_frame(bgr, quality_max, budget, fmt=FRAME_JPEG):
    """Host-only: (frame, quality used) of an HxWx3 BGR frame under a byte budget, fmt FRAME_JPEG (poppy_bgr_to_jpeg_budget_frame) or FRAME_JPEG444
    (poppy_bgr_to_jpeg444_budget_frame)."""
    a = np.ascontiguousarray(bgr, np.uint8)
    h, w = a.shape[:2]
    call = lib().poppy_bgr_to_jpeg444_budget_frame if fmt == FRAME_JPEG444 else lib().poppy_bgr_to_jpeg_budget_frame
    used = C.c_int(0)
    frame = _coded_frame(lambda dst: call(_p(a), w * 3, w, h, int(quality_max), int(budget), dst, C.byref(used)), "bgr_to_jpeg_budget_frame", w, h, fmt)
    return frame, used.value


def bgr_to_jpeg_frame(bgr, quality=JPEG_QUALITY_DEFAULT):
    """Host-only: the FRAME_JPEG frame of an HxWx3 BGR frame (poppy_bgr_to_jpeg_frame = bgr_to_i420, then i420_to_jpeg_frame)."""
    a = np.ascontiguousarray(bgr, np.uint8)
    h, w = a.shape[:2]
    return _coded_frame(lambda dst: lib().poppy_bgr_to_jpeg_frame(_p(a), w * 3, w, h, int(quality), dst), "bgr_to_jpeg_frame", w, h, FRAME_JPEG)


def _i444(call, what, bgr, row_pad, chk=None):
    a, stride, w, h = _padded_rows(bgr, row_pad)
    out = np.empty(3 * w * h, np.uint8)
    rc = call(_p(a), stride, w, h, _p(out))
    if chk:
        chk(rc, what)
    elif rc:
        raise PoppyError(f"poppy_{what}: {rc}")
    return out


def bgr_to_i444(bgr, row_pad=0):
    """Host-only: the I444 planes of an HxWx3 BGR frame (poppy_bgr_to_i444), as a flat uint8 array of 3 * W * H: the Y, the U and the V plane, every sample from
    its own pixel — what FRAME_JPEG444 codes.  row_pad: the frame is handed over with that many extra bytes per row."""
    return _i444(lib().poppy_bgr_to_i444, "bgr_to_i444", bgr, row_pad)


def i444_to_jpeg_frame(i444, w, h, quality=JPEG_QUALITY_DEFAULT):
    """Host-only: the FRAME_JPEG444 frame of flat I444 planes (poppy_i444_to_jpeg_frame): `total`, then one baseline JFIF file with 4:4:4 sampling; a flat uint8
    array of its own length."""
    return _planes_to_jpeg(lib().poppy_i444_to_jpeg_frame, FRAME_JPEG444, i444, w, h, quality)


def bgr_to_jpeg444_frame(bgr, quality=JPEG_QUALITY_DEFAULT):
    """Host-only: the FRAME_JPEG444 frame of an HxWx3 BGR frame (poppy_bgr_to_jpeg444_frame = bgr_to_i444, then i444_to_jpeg_frame)."""
    a = np.ascontiguousarray(bgr, np.uint8)
    h, w = a.shape[:2]
    return _coded_frame(lambda dst: lib().poppy_bgr_to_jpeg444_frame(_p(a), w * 3, w, h, int(quality), dst), "bgr_to_jpeg444_frame", w, h, FRAME_JPEG444)


def _optimal_table(call, counts, what, chk=None):
    a = np.ascontiguousarray(counts, np.uint32).ravel()
    if a.size != 256:
        raise PoppyError(f"{what}: a table has 256 counts")
    bits, vals, n = np.zeros(16, np.uint8), np.zeros(256, np.uint8), C.c_int(0)
    rc = call(_p(a), _p(bits), _p(vals), C.byref(n))
    if chk:
        chk(rc, what)
    elif rc:
        raise PoppyError(f"poppy_{what}: {rc}")
    return bits, vals[:n.value].copy()


def jpeg_optimal_table(counts):
    """Host-only: the Huffman table of 256 symbol counts by FRAME_JPEG_OPT's rule (poppy_jpeg_optimal_table): (bits[16], vals[n]) as a DHT segment holds them."""
    return _optimal_table(lib().poppy_jpeg_optimal_table, counts, "jpeg_optimal_table")


def i420_to_jpeg_opt_frame(i420, w, h, quality=JPEG_QUALITY_DEFAULT):
    """Host-only: the FRAME_JPEG_OPT frame of a flat I420 frame (poppy_i420_to_jpeg_opt_frame): FRAME_JPEG's file on Huffman tables built from the frame's own symbols."""
    return _planes_to_jpeg(lib().poppy_i420_to_jpeg_opt_frame, FRAME_JPEG_OPT, i420, w, h, quality)


def i444_to_jpeg_opt_frame(i444, w, h, quality=JPEG_QUALITY_DEFAULT):
    """Host-only: the FRAME_JPEG444_OPT frame of flat I444 planes (poppy_i444_to_jpeg_opt_frame)."""
    return _planes_to_jpeg(lib().poppy_i444_to_jpeg_opt_frame, FRAME_JPEG444_OPT, i444, w, h, quality)


def bgr_to_jpeg_opt_frame(bgr, quality=JPEG_QUALITY_DEFAULT):
    """Host-only: the FRAME_JPEG_OPT frame of an HxWx3 BGR frame (poppy_bgr_to_jpeg_opt_frame = bgr_to_i420, then i420_to_jpeg_opt_frame)."""
    a = np.ascontiguousarray(bgr, np.uint8)
    h, w = a.shape[:2]
    return _coded_frame(lambda dst: lib().poppy_bgr_to_jpeg_opt_frame(_p(a), w * 3, w, h, int(quality), dst), "bgr_to_jpeg_opt_frame", w, h, FRAME_JPEG_OPT)


def bgr_to_jpeg444_opt_frame(bgr, quality=JPEG_QUALITY_DEFAULT):
    """Host-only: the FRAME_JPEG444_OPT frame of an HxWx3 BGR frame (poppy_bgr_to_jpeg444_opt_frame = bgr_to_i444, then i444_to_jpeg_opt_frame)."""
    a = np.ascontiguousarray(bgr, np.uint8)
    h, w = a.shape[:2]
    return _coded_frame(lambda dst: lib().poppy_bgr_to_jpeg444_opt_frame(_p(a), w * 3, w, h, int(quality), dst), "bgr_to_jpeg444_opt_frame", w, h, FRAME_JPEG444_OPT)


def png_table(k):
    """Host-only: table k of the FRAME_PNG format (poppy_png_table): its 257 code lengths (literal 0..255, end-of-block) as a uint8 array, and its block header as
    an array of bits in stream order (bit 0 is BFINAL, left 0)."""
    lengths = np.zeros(257, np.uint8)
    header = np.zeros(PNG_HEADER_BYTES, np.uint8)
    n = C.c_int(0)
    rc = lib().poppy_png_table(int(k), _p(lengths), _p(header), C.byref(n))
    if rc:
        raise PoppyError(f"poppy_png_table: {rc}")
    return lengths, np.unpackbits(header, bitorder="little")[:n.value].copy()


def png_runs_table(k):
    """Host-only: table k of the FRAME_PNG_RUNS format (poppy_png_runs_table): its 286 code lengths (literal 0..255, end-of-block, the length symbols 257..285) as
    a uint8 array, and its block header as an array of bits in stream order (bit 0 is BFINAL, left 0)."""
    lengths = np.zeros(PNG_RUNS_SYMBOLS, np.uint8)
    header = np.zeros(PNG_HEADER_BYTES, np.uint8)
    n = C.c_int(0)
    rc = lib().poppy_png_runs_table(int(k), _p(lengths), _p(header), C.byref(n))
    if rc:
        raise PoppyError(f"poppy_png_runs_table: {rc}")
    return lengths, np.unpackbits(header, bitorder="little")[:n.value].copy()


PNG_CANARY = 0xA5


def _png_frame(call, what, bgr, row_pad, chk=None, whole=False, fmt=FRAME_PNG):
    a, stride, w, h = _padded_rows(bgr, row_pad)
    out = np.full(max(frame_bytes(fmt, w, h), 4) + 64, PNG_CANARY, np.uint8)
    rc = call(_p(a), stride, w, h, _p(out))
    if chk:
        chk(rc, what)
    elif rc:
        raise PoppyError(f"poppy_{what}: {rc}")
    return out if whole else out[:png_frame_bytes(out)].copy()


def bgr_to_png_frame(bgr, row_pad=0, whole=False):
    """Host-only: the FRAME_PNG frame of an HxWx3 BGR frame (poppy_bgr_to_png_frame): `total`, then one complete PNG file that decodes to exactly the frame; a flat
    uint8 array of its own length.  row_pad: the frame is handed over with that many extra bytes per row.  whole: the whole destination buffer instead — the
    capacity and 64 bytes more, filled with PNG_CANARY before the call."""
    return _png_frame(lib().poppy_bgr_to_png_frame, "bgr_to_png_frame", bgr, row_pad, None, whole)


def bgr_to_png_runs_frame(bgr, row_pad=0, whole=False):
    """Host-only: the FRAME_PNG_RUNS frame of an HxWx3 BGR frame (poppy_bgr_to_png_runs_frame): bgr_to_png_frame's file with runs of equal bytes coded as matches;
    row_pad and whole as there (the capacity is FRAME_PNG_RUNS's)."""
    return _png_frame(lib().poppy_bgr_to_png_runs_frame, "bgr_to_png_runs_frame", bgr, row_pad, None, whole, FRAME_PNG_RUNS)


def bgr_to_png_opt_frame(bgr, row_pad=0, whole=False):
    """Host-only: the FRAME_PNG_OPT frame of an HxWx3 BGR frame (poppy_bgr_to_png_opt_frame): bgr_to_png_runs_frame's file with every segment coded on the table
    that is shortest for it, the eight fixed ones or one built from its own symbol counts; row_pad and whole as there (the capacity is FRAME_PNG_RUNS's)."""
    return _png_frame(lib().poppy_bgr_to_png_opt_frame, "bgr_to_png_opt_frame", bgr, row_pad, None, whole, FRAME_PNG_OPT)


def _optimal_lengths(call, counts, limit, what, chk=None):
    a = np.ascontiguousarray(counts, np.uint32).ravel()
    lengths = np.zeros(max(a.size, 1), np.uint8)
    rc = call(_p(a), int(a.size), int(limit), _p(lengths))
    if chk:
        chk(rc, what)
    elif rc:
        raise PoppyError(f"poppy_{what}: {rc}")
    return lengths[:a.size]


def png_optimal_lengths(counts, limit=15):
    """Host-only: the code lengths of 1..286 symbol counts by FRAME_PNG_OPT's rule (poppy_png_optimal_lengths), none above `limit` (7 or 15); 0 for a symbol
    without a count."""
    return _optimal_lengths(lib().poppy_png_optimal_lengths, counts, limit, "png_optimal_lengths")


def _png_seq_frames(call, what, frames, row_pad, frame_pad, chk=None):
    a, stride, frame_stride, n, w, h = _padded_frames(frames, row_pad, frame_pad)
    out = np.empty((max(n, 1), max(frame_bytes(FRAME_PNG_SEQ, w, h), 4)), np.uint8)
    rc = call(_p(a), stride, frame_stride, n, w, h, _p(out))
    if chk:
        chk(rc, what)
    elif rc:
        raise PoppyError(f"poppy_{what}: {rc}")
    return [f[:png_frame_bytes(f)].copy() for f in out]


def bgr_frames_to_png_seq_frames(frames, row_pad=0, frame_pad=0):
    """Host-only: the FRAME_PNG_SEQ frames of a sequence of n HxWx3 BGR frames (poppy_bgr_frames_to_png_seq_frames): every frame's token counts summed, one table
    built from the sums, every frame a complete PNG file whose segments choose among FRAME_PNG_RUNS' eight tables and that one.  A list of n flat uint8 arrays,
    each cut to its `total`.  row_pad / frame_pad: as in bgr_frames_to_pal8."""
    return _png_seq_frames(lib().poppy_bgr_frames_to_png_seq_frames, "bgr_frames_to_png_seq_frames", frames, row_pad, frame_pad)


def _png_seq_table(call, counts, what, chk=None):
    a = np.ascontiguousarray(counts, np.uint32).ravel()
    if a.size != PNG_RUNS_SYMBOLS:
        raise PoppyError(f"{what}: counts has {PNG_RUNS_SYMBOLS} entries")
    lengths = np.zeros(PNG_RUNS_SYMBOLS, np.uint8)
    header = np.zeros(PNG_SEQ_HEADER_BYTES, np.uint8)
    n = C.c_int(0)
    rc = call(_p(a), _p(lengths), _p(header), C.byref(n))
    if chk:
        chk(rc, what)
    elif rc:
        raise PoppyError(f"poppy_{what}: {rc}")
    return lengths, np.unpackbits(header, bitorder="little")[:n.value].copy()


def png_seq_table(counts):
    """Host-only: the one table of a FRAME_PNG_SEQ sequence from its 286 summed counts (poppy_png_seq_table): the code lengths as a uint8 array, and the table's
    block header as an array of bits in stream order (bit 0 is BFINAL, left 0)."""
    return _png_seq_table(lib().poppy_png_seq_table, counts, "png_seq_table")


def _gif_frames(call, frames, row_pad, frame_pad, chk=None):
    a, stride, frame_stride, n, w, h = _padded_frames(frames, row_pad, frame_pad)
    out = np.empty((n, max(frame_bytes(FRAME_GIF_SEQ, w, h), 4)), np.uint8)
    rc = call(_p(a), stride, frame_stride, n, w, h, _p(out))
    if chk:
        chk(rc, "bgr_frames_to_gif_frames")
    elif rc:
        raise PoppyError(f"poppy_bgr_frames_to_gif_frames: {rc}")
    return [f[:gif_frame_bytes(f)].copy() for f in out]


def bgr_frames_to_gif_frames(frames, row_pad=0, frame_pad=0):
    """Host-only: the library's GIF_SEQ frames of a sequence of n HxWx3 BGR frames (poppy_bgr_frames_to_gif_frames = bgr_frames_to_pal8, then pal8_to_gif_frame
    of every frame): a list of n flat uint8 arrays, each cut to its `total`.  row_pad / frame_pad: as in bgr_frames_to_pal8."""
    return _gif_frames(lib().poppy_bgr_frames_to_gif_frames, frames, row_pad, frame_pad)


def _jpeg_seq_frames(call, what, fmt, n, w, h, chk=None):
    """The frames of a JPEG sequence of format fmt out of call(dst), a list of n flat uint8 arrays, each cut to its `total`; chk: as in _coded_frame."""
    if fmt not in (FRAME_JPEG_SEQ, FRAME_JPEG444_SEQ):
        raise PoppyError(f"{what}: fmt is FRAME_JPEG_SEQ or FRAME_JPEG444_SEQ")
    out = np.empty((max(n, 1), max(frame_bytes(fmt, w, h), 4)), np.uint8)
    rc = call(_p(out))
    if chk:
        chk(rc, what)
    elif rc:
        raise PoppyError(f"poppy_{what}: {rc}")
    return [f[:jpeg_frame_bytes(f)].copy() for f in out]


def bgr_frames_to_jpeg_seq_frames(frames, quality=JPEG_QUALITY_DEFAULT, fmt=FRAME_JPEG_SEQ, row_pad=0, frame_pad=0):
    """Host-only: the FRAME_JPEG_SEQ (fmt FRAME_JPEG444_SEQ: 4:4:4) frames of a sequence of n HxWx3 BGR frames (poppy_bgr_frames_to_jpeg_seq_frames,
    poppy_bgr_frames_to_jpeg444_seq_frames): every frame's symbol counts summed, one Huffman table set, every frame a complete JFIF file on it.  A list of n flat
    uint8 arrays, each cut to its `total`.  row_pad / frame_pad: as in bgr_frames_to_pal8."""
    a, stride, frame_stride, n, w, h = _padded_frames(frames, row_pad, frame_pad)
    call = lib().poppy_bgr_frames_to_jpeg444_seq_frames if fmt == FRAME_JPEG444_SEQ else lib().poppy_bgr_frames_to_jpeg_seq_frames
    return _jpeg_seq_frames(lambda dst: call(_p(a), stride, frame_stride, n, w, h, int(quality), dst), "bgr_frames_to_jpeg_seq_frames", fmt, n, w, h)


def _jpeg_seq_budget_frames(call, what, fmt, n, w, h, chk=None):
    """The frames of a JPEG sequence under a sequence budget out of call(dst, quality_used): (a list of n flat uint8 arrays, each cut to its `total`, the one
    quality); fmt FRAME_JPEG or FRAME_JPEG444; chk: as in _coded_frame."""
    if fmt not in (FRAME_JPEG, FRAME_JPEG444):
        raise PoppyError(f"{what}: fmt is FRAME_JPEG or FRAME_JPEG444")
    out = np.empty((max(n, 1), max(frame_bytes(fmt, w, h), 4)), np.uint8)
    used = C.c_int(0)
    rc = call(_p(out), C.byref(used))
    if chk:
        chk(rc, what)
    elif rc:
        raise PoppyError(f"poppy_{what}: {rc}")
    return [f[:jpeg_frame_bytes(f)].copy() for f in out], used.value


def bgr_frames_to_jpeg_seq_budget_frames(frames, quality_max, budget, fmt=FRAME_JPEG, row_pad=0, frame_pad=0):
    """Host-only: (frames, quality used) of a sequence of n HxWx3 BGR frames whose FRAME_JPEG (fmt FRAME_JPEG444: 4:4:4) files together have at most `budget`
    bytes, all at the one quality the budget's search picks at or below quality_max (poppy_bgr_frames_to_jpeg_seq_budget_frames,
    poppy_bgr_frames_to_jpeg444_seq_budget_frames).  row_pad / frame_pad: as in bgr_frames_to_pal8."""
    a, stride, frame_stride, n, w, h = _padded_frames(frames, row_pad, frame_pad)
    call = lib().poppy_bgr_frames_to_jpeg444_seq_budget_frames if fmt == FRAME_JPEG444 else lib().poppy_bgr_frames_to_jpeg_seq_budget_frames
    return _jpeg_seq_budget_frames(lambda dst, used: call(_p(a), stride, frame_stride, n, w, h, int(quality_max), int(budget), dst, used),
                                   "bgr_frames_to_jpeg_seq_budget_frames", fmt, n, w, h)


def planes_to_jpeg_seq_budget_frames(planes, w, h, quality_max, budget, fmt=FRAME_JPEG, frame_pad=0):
    """Host-only: the same from the planes (poppy_i420_frames_to_jpeg_seq_budget_frames; fmt FRAME_JPEG444: poppy_i444_frames_to_jpeg_seq_budget_frames):
    `planes` is n flat I420 (I444) frames, an n x bytes array; frame_pad: that many extra bytes between frames."""
    a = np.ascontiguousarray(planes, np.uint8)
    n, size = a.shape
    want = 3 * w * h if fmt == FRAME_JPEG444 else frame_bytes(FRAME_I420, w, h)
    if w > 0 and h > 0 and size != want:
        raise PoppyError(f"planes_to_jpeg_seq_budget_frames: a frame of planes has {want} bytes")
    if frame_pad:
        buf = np.full((n, size + int(frame_pad)), 0xA5, np.uint8)
        buf[:, :size] = a
        a = buf
    call = lib().poppy_i444_frames_to_jpeg_seq_budget_frames if fmt == FRAME_JPEG444 else lib().poppy_i420_frames_to_jpeg_seq_budget_frames
    return _jpeg_seq_budget_frames(lambda dst, used: call(_p(a), a.shape[1], n, int(w), int(h), int(quality_max), int(budget), dst, used),
                                   "planes_to_jpeg_seq_budget_frames", fmt, n, w, h)


def planes_to_jpeg_seq_frames(planes, w, h, quality=JPEG_QUALITY_DEFAULT, fmt=FRAME_JPEG_SEQ, frame_pad=0):
    """Host-only: the same from the planes (poppy_i420_frames_to_jpeg_seq_frames; fmt FRAME_JPEG444_SEQ: poppy_i444_frames_to_jpeg_seq_frames): `planes` is n flat
    I420 (I444) frames, an n x bytes array; frame_pad: that many extra bytes between frames."""
    a = np.ascontiguousarray(planes, np.uint8)
    n, size = a.shape
    want = 3 * w * h if fmt == FRAME_JPEG444_SEQ else frame_bytes(FRAME_I420, w, h)
    if w > 0 and h > 0 and size != want:
        raise PoppyError(f"planes_to_jpeg_seq_frames: a frame of planes has {want} bytes")
    if frame_pad:
        buf = np.full((n, size + int(frame_pad)), 0xA5, np.uint8)
        buf[:, :size] = a
        a = buf
    call = lib().poppy_i444_frames_to_jpeg_seq_frames if fmt == FRAME_JPEG444_SEQ else lib().poppy_i420_frames_to_jpeg_seq_frames
    return _jpeg_seq_frames(lambda dst: call(_p(a), a.shape[1], n, int(w), int(h), int(quality), dst), "planes_to_jpeg_seq_frames", fmt, n, w, h)


def frame_scaled_size(w, h, factor):
    """Host-only: (ow, oh) of a w x h frame scaled down by the whole factor 1..8 (poppy_frame_scaled_size): what a writer under Context.set_frame_scale is
    told, and what its sink is opened with."""
    ow, oh = C.c_int(0), C.c_int(0)
    rc = lib().poppy_frame_scaled_size(int(w), int(h), int(factor), C.byref(ow), C.byref(oh))
    if rc:
        raise PoppyError(f"poppy_frame_scaled_size: {rc}")
    return ow.value, oh.value


def _scaled_frame(call, what, bgr, size, args, row_pad, dst_pad, chk=None):
    """An HxWx3 BGR frame through one of the four scaling calls, `what` by name: size(w, h) is the result's (ow, oh), args what the call takes between the source's
    size and dst.  chk(rc): the context's check; without one a status raises as poppy_<what>'s."""
    a, stride, w, h = _padded_rows(bgr, row_pad)
    ow, oh = size(w, h)
    out = np.full((max(oh, 1), max(ow, 1) * 3 + int(dst_pad)), 0xA5, np.uint8)
    rc = call(_p(a), stride, w, h, *args, _p(out), ow * 3 + int(dst_pad))
    if chk:
        chk(rc, what)
    elif rc:
        raise PoppyError(f"poppy_{what}: {rc}")
    if dst_pad and not (out[:, ow * 3:] == 0xA5).all():
        raise PoppyError(f"{what} wrote into the padding of dst")
    return out[:, :ow * 3].reshape(oh, ow, 3).copy()


def _downscale(call, bgr, factor, row_pad, dst_pad, chk=None):
    return _scaled_frame(call, "bgr_downscale", bgr, lambda w, h: frame_scaled_size(w, h, factor), (int(factor),), row_pad, dst_pad, chk)


def _resize_area(call, bgr, ow, oh, row_pad, dst_pad, chk=None):
    return _scaled_frame(call, "bgr_resize_area", bgr, lambda w, h: (int(ow), int(oh)), (int(ow), int(oh)), row_pad, dst_pad, chk)


def bgr_downscale(bgr, factor, row_pad=0, dst_pad=0):
    """Host-only: an HxWx3 BGR frame scaled down by the whole factor 1..8 (poppy_bgr_downscale, the host statement of Context.set_frame_scale's rule), as an
    oh x ow x 3 array.  row_pad / dst_pad: the frame is handed over / taken back with that many extra bytes per row."""
    return _downscale(lib().poppy_bgr_downscale, bgr, factor, row_pad, dst_pad)


def frame_fit_size(w, h, max_w, max_h):
    """Host-only: the largest (ow, oh) inside a max_w x max_h box that keeps the aspect ratio of a w x h frame (poppy_frame_fit_size); (w, h) when the frame
    fits.  PoppyError with the status when the result would need more than a factor of 8 on an axis."""
    ow, oh = C.c_int(0), C.c_int(0)
    rc = lib().poppy_frame_fit_size(int(w), int(h), int(max_w), int(max_h), C.byref(ow), C.byref(oh))
    if rc:
        raise PoppyError(f"poppy_frame_fit_size: {rc}")
    return ow.value, oh.value


def bgr_resize_area(bgr, ow, oh, row_pad=0, dst_pad=0):
    """Host-only: an HxWx3 BGR frame resampled to ow x oh by exact area weights (poppy_bgr_resize_area, the host statement of Context.set_frame_size's rule),
    as an oh x ow x 3 array.  row_pad / dst_pad: the frame is handed over / taken back with that many extra bytes per row."""
    return _resize_area(lib().poppy_bgr_resize_area, bgr, ow, oh, row_pad, dst_pad)


def bgr_resize_area_form(w, h, ow, oh):
    """Host-only: the width of arithmetic the device takes for a w x h -> ow x oh resize (poppy_hip_bgr_resize_area_form): 2 for 32-bit sums and indices, 1 for
    32-bit sums and 64-bit indices (a side above 32768), 0 for 64-bit sums (above 2^24 pixels)."""
    rc = lib().poppy_hip_bgr_resize_area_form(int(w), int(h), int(ow), int(oh))
    if rc < 0:
        raise PoppyError(f"poppy_hip_bgr_resize_area_form: {rc}")
    return rc


def pal8_to_bgr(frame, w, h):
    """palette[index] of a flat PAL8 frame, as an HxWx3 BGR array (what a viewer of the frame sees)."""
    f = np.asarray(frame, np.uint8)
    return f[w * h:].reshape(256, 3)[f[:w * h]][:, ::-1].reshape(h, w, 3)


def _frame_view(ptr, w, h, stride, fmt):
    """A writer's frame as numpy: HxWx3 for BGR, the flat bytes (frame_bytes long) for I420, PAL8 and PAL8_SEQ, the flat `total` bytes for GIF, GIF_SEQ, JPEG, JPEG444, PNG, PNG_RUNS, PNG_OPT and PNG_SEQ.  A view: valid during the callback."""
    if fmt in FRAMES_CODED:                                                      # a coded frame: its own length, not the capacity (every coded format keeps it in its first four bytes)
        return np.ctypeslib.as_array(ptr, shape=(int(lib().poppy_gif_frame_bytes(ptr)),))
    if fmt in (FRAME_I420, FRAME_PAL8, FRAME_PAL8_SEQ):
        return np.ctypeslib.as_array(ptr, shape=(frame_bytes(fmt, w, h),))
    return np.ctypeslib.as_array(ptr, shape=(h, stride))[:, :w * 3].reshape(h, w, 3)


class PoppyError(RuntimeError):
    pass


def plan_frame(w, h, p1, p2, shape):
    """Host-only mesh planning (no GPU)."""
    p1 = np.ascontiguousarray(p1, np.float32)
    p2 = np.ascontiguousarray(p2, np.float32)
    n = len(p1)
    mt = 2 * n + 16
    nt = C.c_int(0)
    idx3 = np.zeros((mt, 3), np.int32); tri = np.zeros((mt, 3, 2), np.int32)
    M1, M2, i1, i2 = (np.zeros((mt, 3, 3), np.float32) for _ in range(4))
    mp = np.zeros((n, 2), np.float32)
    rc = lib().poppy_plan_frame(w, h, _p(p1), _p(p2), n, shape, mt, C.byref(nt), _p(idx3), _p(tri), _p(M1), _p(M2), _p(i1), _p(i2), _p(mp))
    if rc:
        raise PoppyError(f"poppy_plan_frame: {rc}")
    t = nt.value
    return dict(idx3=idx3[:t], tri_xy=tri[:t], M1=M1[:t], M2=M2[:t], inv1=i1[:t], inv2=i2[:t], morphed=mp)


def plan_tile_counts(w, h, p1, p2, shape, tile_w):
    """Host-only: what the planner hands the fused warp kernels for this frame in tiles tile_w wide — (list length of every tile, row-major
    (tiles_y, tiles_x) int32, their sum, whether the lists fit the room a context keeps for len(p1) point pairs)."""
    p1 = np.ascontiguousarray(p1, np.float32)
    p2 = np.ascontiguousarray(p2, np.float32)
    th = 1024 // tile_w
    ty, tx = (h + th - 1) // th, (w + tile_w - 1) // tile_w
    counts = np.zeros((ty, tx), np.int32)
    nt, total, ok = C.c_int(0), C.c_longlong(0), C.c_int(0)
    rc = lib().poppy_plan_tile_counts(w, h, _p(p1), _p(p2), len(p1), shape, tile_w, _p(counts), counts.size, C.byref(nt), C.byref(total), C.byref(ok))
    if rc or nt.value != counts.size:
        raise PoppyError(f"poppy_plan_tile_counts: {rc} ({nt.value} tiles)")
    return counts, int(total.value), bool(ok.value)


def plan_tile_tris(w, h, p1, p2, shape, tile_w):
    """Host-only: the tile lists themselves, as a list (tile after tile, row-major) of int32 arrays of triangle numbers in painter's order."""
    counts, total, _ = plan_tile_counts(w, h, p1, p2, shape, tile_w)
    p1 = np.ascontiguousarray(p1, np.float32)
    p2 = np.ascontiguousarray(p2, np.float32)
    tris = np.zeros(max(total, 1), np.int32)
    tot = C.c_longlong(0)
    rc = lib().poppy_plan_tile_tris(w, h, _p(p1), _p(p2), len(p1), shape, tile_w, _p(tris), total, C.byref(tot))
    if rc or tot.value != total:
        raise PoppyError(f"poppy_plan_tile_tris: {rc}")
    return np.split(tris[:total], np.cumsum(counts.ravel())[:-1])


BLOB_FIELDS = ("rec_bytes", "o_edges", "o_outl", "o_toff", "o_ttri", "o_tri", "o_inv", "o_work", "used")


def plan_blob_layout(n_tris, n_work, n_toff, n_ttri, fused):
    """Host-only: the byte offsets of a frame's plan groups in a slot's plan blob (csrc/plan_blob.h), as a dict over BLOB_FIELDS."""
    out = (C.c_ulonglong * 9)()
    rc = lib().poppy_plan_blob_layout(0, n_tris, n_work, n_toff, n_ttri, int(bool(fused)), out)
    if rc:
        raise PoppyError(f"poppy_plan_blob_layout: {rc}")
    return dict(zip(BLOB_FIELDS, (int(v) for v in out)))


def plan_blob_capacity(n_points, w, h, tile_w=0):
    """Host-only: what a context allocates for a slot's plan blob — dict(capacity, max_tris, n_tiles, bins_cap, tile_w); tile_w 0: the context's choice."""
    out = (C.c_ulonglong * 9)()
    rc = lib().poppy_plan_blob_layout(1, n_points, w, h, tile_w, 0, out)
    if rc:
        raise PoppyError(f"poppy_plan_blob_layout: {rc}")
    return dict(zip(("capacity", "max_tris", "n_tiles", "bins_cap", "tile_w"), (int(v) for v in out)))


def warp_records(inv1, inv2, w, h):
    """Host-only: (records (T+1, 20) float32, admitted to the tiled warp kernel?)."""
    inv1 = np.ascontiguousarray(inv1, np.float32).reshape(-1, 9)
    inv2 = np.ascontiguousarray(inv2, np.float32).reshape(-1, 9)
    t = len(inv1)
    rec = np.zeros((t + 1, 20), np.float32)
    rc = lib().poppy_warp_records(_p(inv1), _p(inv2), t, w, h, _p(rec))
    if rc < 0:
        raise PoppyError(f"poppy_warp_records: {rc}")
    return rec, bool(rc)


def ratio_symmetry(knn12, knn21, ratio=0.7):
    """Host-only ratioTest + symmetryTest (src/experiments.hpp:14-144): rows queryIdx, trainIdx, distance."""
    knn12 = np.ascontiguousarray(knn12, np.int32).reshape(-1, 4)
    knn21 = np.ascontiguousarray(knn21, np.int32).reshape(-1, 4)
    out = np.zeros((max(len(knn12), 1), 3), np.int32)
    n = C.c_int(0)
    rc = lib().poppy_ratio_symmetry(_p(knn12), len(knn12), _p(knn21), len(knn21), ratio, _p(out), C.byref(n))
    if rc:
        raise PoppyError(f"poppy_ratio_symmetry: {rc}")
    return out[:n.value]


RANSAC_HYPOTHESES, RANSAC_MIN_POINTS, RANSAC_MAX_POINTS = 2048, 8, 65536


def _ransac(call, what, points1, points2, distance, chk=None):
    a = np.ascontiguousarray(points1, np.float32).reshape(-1, 2); b = np.ascontiguousarray(points2, np.float32).reshape(-1, 2)
    n = len(a)
    assert len(b) == n
    res = {"inliers": np.zeros(max(n, 1), np.uint8), "f": np.zeros((3, 3), np.float64), "counts": np.zeros(RANSAC_HYPOTHESES, np.int32),
           "models": np.zeros((RANSAC_HYPOTHESES, 3, 3), np.float64)}
    n_in, best = C.c_int(0), C.c_int(0)
    rc = call(_p(a), _p(b), n, float(distance), _p(res["inliers"]), C.byref(n_in), _p(res["f"]), C.byref(best), _p(res["counts"]), _p(res["models"]))
    if chk:
        chk(rc, what)
    elif rc:
        raise PoppyError(f"{what}: {rc}")
    res["inliers"] = res["inliers"][:n]
    res["n_inliers"], res["best"] = n_in.value, best.value
    return res


def ransac_fundamental(points1, points2, distance=3.0):
    """Host statement of the RANSAC fundamental-matrix filter (include/poppy_hip.h: poppy_ransac_fundamental): dict(inliers u8 [n], n_inliers, f 3x3,
    best, counts i32 [2048], models f64 [2048, 3, 3])."""
    return _ransac(lib().poppy_ransac_fundamental, "poppy_ransac_fundamental", points1, points2, distance)


def procrustes(x, y):
    """Host-only Procrustes(true, false)::procrustes: dict(rotation 2x2, scale, error, yprime n x 2)."""
    x = np.ascontiguousarray(x, np.float32).reshape(-1, 2); y = np.ascontiguousarray(y, np.float32).reshape(-1, 2)
    rot = np.zeros((2, 2), np.float32); se = np.zeros(2, np.float32); yp = np.zeros_like(x)
    rc = lib().poppy_procrustes(_p(x), _p(y), len(x), _p(rot), _p(se), _p(yp))
    if rc:
        raise PoppyError(f"poppy_procrustes: {rc}")
    return dict(rotation=rot, scale=se[0], error=se[1], yprime=yp)


def perspective_from4(src4, dst4):
    s = np.ascontiguousarray(src4, np.float32).reshape(4, 2); d = np.ascontiguousarray(dst4, np.float32).reshape(4, 2)
    m = np.zeros((3, 3), np.float64)
    rc = lib().poppy_perspective_from4(_p(s), _p(d), _p(m))
    if rc:
        raise PoppyError(f"poppy_perspective_from4: {rc}")
    return m


def gabor_doubt():
    """(plane values near zero, near a float midpoint, pixels formed again as direct sums because of them) in the FFT form of the Gabor banks on the current device
    since the last call."""
    out = (C.c_ulonglong * 3)()
    rc = lib().poppy_hip_gabor_doubt(out)
    if rc:
        raise PoppyError(f"poppy_hip_gabor_doubt: {rc}")
    return int(out[0]), int(out[1]), int(out[2])


def gabor_tables(which):
    """(bank [16, ks, ks] float32, spectra [8, 64, 64] complex128 in the FFT kernel's position order) of the 31 / 13 tap Gabor bank (host only)."""
    bank = np.zeros((16, which, which), np.float32); spec = np.zeros((8, 64, 64, 2), np.float64)
    rc = lib().poppy_gabor_tables(int(which), _p(bank), _p(spec))
    if rc:
        raise PoppyError(f"poppy_gabor_tables: {rc}")
    return bank, spec[..., 0] + 1j * spec[..., 1]


def gabor_rounding_in_doubt(v, band):
    """The doubt rule of the FFT form of the Gabor banks on one plane value (host only): 0 no, 1 near zero, 2 near a float midpoint."""
    return int(lib().poppy_gabor_rounding_in_doubt(float(v), float(band)))


def gabor_band_unit():
    """The doubt band of the FFT form per unit of max(1, the largest magnitude in the tile's 64 x 64 patch) (host only)."""
    return float(lib().poppy_gabor_band_unit())


def pyr_tail_plan(w, h, levels=64, tail_px=600):
    """(info dict, descriptors [n, 4] uint32) of the pyramid tail's tap table for a w x h frame (host only)."""
    info = (C.c_int * 6)()
    rc = lib().poppy_pyr_tail_plan(w, h, levels, tail_px, info, None)
    if rc:
        raise PoppyError(f"poppy_pyr_tail_plan: {rc}")
    desc = np.zeros((max(info[3], 1), 4), np.uint32)
    lib().poppy_pyr_tail_plan(w, h, levels, tail_px, info, _p(desc))
    keys = ("first", "wide_steps", "single_pixel_reductions", "descriptors", "lds_bytes", "ok")
    return dict(zip(keys, list(info))), desc[:info[3]]


def radial_gradient(w, h):
    """draw_radial_gradiant2 (host only)."""
    out = np.zeros((h, w), np.float32)
    rc = lib().poppy_radial_gradient(w, h, _p(out))
    if rc:
        raise PoppyError(f"poppy_radial_gradient: {rc}")
    return out


def radial_mask(w, h):
    """draw_radial_gradiant as Extractor::foreground uses it under enable_radial_mask (host only)."""
    out = np.zeros((h, w), np.float32)
    rc = lib().poppy_radial_mask(w, h, _p(out))
    if rc:
        raise PoppyError(f"poppy_radial_mask: {rc}")
    return out


WRITE_INDEXED_CB = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.POINTER(C.c_uint8), C.c_int, C.c_int, C.c_size_t)
PAIR_SOURCE_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t))
WRITE_PAIR_CB = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_uint8), C.c_int, C.c_int, C.c_size_t)
IMAGE_SOURCE_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(C.c_int), C.POINTER(C.c_int))


def comm_id():
    """128 bytes to hand to every rank's Context.comm_init (ncclGetUniqueId)."""
    b = (C.c_uint8 * 128)()
    rc = lib().poppy_hip_comm_id(b)
    if rc:
        raise PoppyError(f"poppy_hip_comm_id: {rc} (librccl missing?)")
    return bytes(b)


def sharded_setups():
    """Runs of the sharded set-up protocol in this process (poppy_hip_sharded_setups)."""
    f = lib().poppy_hip_sharded_setups
    f.restype = C.c_ulonglong
    return int(f())


def pair_state_bytes(w, h):
    n = C.c_size_t(0)
    lib().poppy_hip_pair_state_bytes(w, h, C.byref(n))
    return n.value


def morph_sharded(devices, bgr1, bgr2, total_frames, collect=True, reduce=None, **settings):
    """One total_frames-frame phase-mode morph across `devices` (one process, one thread per GPU): list of frames by index.
    reduce(index, frame_view) -> what is kept instead of a copy of the frame (a digest, None ...): a 480-frame 1080p job is 3 GB of frames."""
    a = np.ascontiguousarray(bgr1, np.uint8); b = np.ascontiguousarray(bgr2, np.uint8)
    h, w = a.shape[:2]
    s = PoppySettings(); lib().poppy_settings_default(C.byref(s))
    for k, v in settings.items():
        setattr(s, k, v)
    frames = {}
    import threading
    lock = threading.Lock()

    def cb(user, idx, ptr, ww, hh, stride):
        f = np.ctypeslib.as_array(ptr, shape=(hh, stride))[:, :ww * 3].reshape(hh, ww, 3)
        f = reduce(idx, f) if reduce else f.copy()
        with lock:
            frames[idx] = f
    fn = WRITE_INDEXED_CB(cb) if collect else None
    dv = (C.c_int * len(devices))(*devices)
    err = C.create_string_buffer(512)
    rc = lib().poppy_hip_morph_sharded(dv, len(devices), C.byref(s), _p(a), w * 3, _p(b), w * 3, w, h, total_frames,
                                       C.cast(fn, C.c_void_p) if fn else None, None, err, 512)
    if rc:
        raise PoppyError(f"poppy_hip_morph_sharded: {rc}: {err.value.decode()}")
    return [frames[j] for j in sorted(frames)]


def morph_pairs(devices, pairs, contexts_per_device=2, phase=-1.0, collect=True, reduce=None, **settings):
    """`pairs` = list of (bgr1, bgr2): every pair one whole poppy::morph, spread over the devices.  Returns {pair: [frames]}
    (or the number of frames written when collect is False)."""
    pairs = [(np.ascontiguousarray(a, np.uint8), np.ascontiguousarray(b, np.uint8)) for a, b in pairs]
    h, w = pairs[0][0].shape[:2]
    s = PoppySettings(); lib().poppy_settings_default(C.byref(s))
    for k, v in settings.items():
        setattr(s, k, v)
    out = {}
    count = [0]
    import threading
    lock = threading.Lock()

    def src(user, p, device, pa, sa, pb, sb):
        pa[0] = pairs[p][0].ctypes.data; sa[0] = w * 3
        pb[0] = pairs[p][1].ctypes.data; sb[0] = w * 3
        return 0

    def wr(user, p, j, ptr, ww, hh, stride):
        if collect:
            f = np.ctypeslib.as_array(ptr, shape=(hh, stride))[:, :ww * 3].reshape(hh, ww, 3)
            f = reduce(p, j, f) if reduce else f.copy()      # reduce(pair, index, frame_view) -> what is kept instead of a copy
            with lock:
                out.setdefault(p, {})[j] = f
        else:
            with lock:
                count[0] += 1
    fs, fw = PAIR_SOURCE_CB(src), WRITE_PAIR_CB(wr)
    dv = (C.c_int * len(devices))(*devices)
    err = C.create_string_buffer(512)
    rc = lib().poppy_hip_morph_pairs(dv, len(devices), contexts_per_device, C.byref(s), len(pairs), w, h, phase,
                                     C.cast(fs, C.c_void_p), C.cast(fw, C.c_void_p), None, err, 512)
    if rc:
        raise PoppyError(f"poppy_hip_morph_pairs: {rc}: {err.value.decode()}")
    return {p: [v[j] for j in sorted(v)] for p, v in out.items()} if collect else count[0]


def pair_begin_sharded_local(ctxs, d1, d2, w, h, root=0):
    """The sharded pair set-up between contexts of this process (context k plays rank k; d1 / d2 valid for ctxs[root]'s device)."""
    arr = (C.c_void_p * len(ctxs))(*[c.h for c in ctxs])
    rc = lib().poppy_hip_pair_begin_sharded_local(arr, len(ctxs), d1, d2, w, h, root)
    if rc:
        raise PoppyError(f"pair_begin_sharded_local: {rc}: " + "; ".join(lib().poppy_hip_last_error(c.h).decode() for c in ctxs))
    for c in ctxs:
        c.w, c.h_ = w, h


class Pool:
    """Persistent contexts for batches of independent pairs (poppy_hip_pool_*)."""

    def __init__(self, devices, contexts_per_device=2, tuned_for=None, max_candidates=3, **settings):
        """tuned_for=(width, height): poppy_hip_pool_create_tuned — the library makes up to max_candidates pools, times a calibration batch on each and keeps
        the fastest (self.candidates_ms: every pool's batch time in the order made, self.kept: the index kept)."""
        s = PoppySettings(); lib().poppy_settings_default(C.byref(s))
        for k, v in settings.items():
            setattr(s, k, v)
        dv = (C.c_int * len(devices))(*devices)
        err = C.create_string_buffer(512)
        self.candidates_ms, self.kept = None, None
        if tuned_for is None:
            self.h = lib().poppy_hip_pool_create(dv, len(devices), contexts_per_device, C.byref(s), err, 512)
        else:
            ms = (C.c_float * max_candidates)(); n = C.c_int(0); kept = C.c_int(-1)
            self.h = lib().poppy_hip_pool_create_tuned(dv, len(devices), contexts_per_device, C.byref(s), int(tuned_for[0]), int(tuned_for[1]), max_candidates,
                                                       ms, C.byref(n), C.byref(kept), err, 512)
            self.candidates_ms, self.kept = [float(ms[k]) for k in range(n.value)], kept.value
        if not self.h:
            raise PoppyError("poppy_hip_pool_create: " + err.value.decode())
        self.frame_format = FRAME_BGR
        self.frame_scale = 1
        self.frame_size = (0, 0)

    def set_frame_size(self, ow, oh):
        """The size every frame handed to a writer is resized to, for every context of the pool (poppy_hip_pool_set_frame_size); (0, 0): none.  PoppyError with
        the status while submitted batches have not been waited for."""
        rc = lib().poppy_hip_pool_set_frame_size(self.h, int(ow), int(oh))
        if rc:
            raise PoppyError(f"poppy_hip_pool_set_frame_size: {rc}")
        self.frame_size = (int(ow), int(oh))

    def set_frame_scale(self, factor):
        """The whole factor 1..8 every frame handed to a writer is scaled down by, for every context of the pool (poppy_hip_pool_set_frame_scale); PoppyError with the
        status while submitted batches have not been waited for."""
        rc = lib().poppy_hip_pool_set_frame_scale(self.h, int(factor))
        if rc:
            raise PoppyError(f"poppy_hip_pool_set_frame_scale: {rc}")
        self.frame_scale = int(factor)

    def set_frame_format(self, fmt):
        """FRAME_BGR, FRAME_I420, FRAME_PAL8, FRAME_PAL8_SEQ (one palette per pair) FRAME_GIF or FRAME_GIF_SEQ (FRAME_PAL8_SEQ coded) for every context of the pool (poppy_hip_pool_set_frame_format); PoppyError with the status while submitted
        batches have not been waited for."""
        rc = lib().poppy_hip_pool_set_frame_format(self.h, int(fmt))
        if rc:
            raise PoppyError(f"poppy_hip_pool_set_frame_format: {rc}")
        self.frame_format = int(fmt)

    def set_jpeg_quality(self, quality):
        """The quality, 1..100, of the FRAME_JPEG frames of every context of the pool (poppy_hip_pool_set_jpeg_quality); PoppyError with the status outside
        that range or while submitted batches have not been waited for."""
        rc = lib().poppy_hip_pool_set_jpeg_quality(self.h, int(quality))
        if rc:
            raise PoppyError(f"poppy_hip_pool_set_jpeg_quality: {rc}")

    def set_jpeg_budget(self, max_frame_bytes):
        """The byte budget of the FRAME_JPEG and FRAME_JPEG444 frames of every context of the pool, 0 for none (poppy_hip_pool_set_jpeg_budget); PoppyError with
        the status on a refusal or while submitted batches have not been waited for."""
        rc = lib().poppy_hip_pool_set_jpeg_budget(self.h, int(max_frame_bytes))
        if rc:
            raise PoppyError(f"poppy_hip_pool_set_jpeg_budget: {rc}")

    def set_jpeg_sequence_budget(self, max_sequence_bytes):
        """The sequence budget of the FRAME_JPEG and FRAME_JPEG444 frames of every context of the pool, 0 for none (poppy_hip_pool_set_jpeg_sequence_budget);
        PoppyError with the status on a refusal or while submitted batches have not been waited for."""
        rc = lib().poppy_hip_pool_set_jpeg_sequence_budget(self.h, int(max_sequence_bytes))
        if rc:
            raise PoppyError(f"poppy_hip_pool_set_jpeg_sequence_budget: {rc}")

    def close(self):
        if self.h:
            lib().poppy_hip_pool_destroy(self.h)
            self.h = None

    def set_timing(self, on):
        lib().poppy_hip_pool_set_timing(self.h, int(on))

    def timing_summary(self):
        names = (C.c_char_p * 32)(); ms = (C.c_float * 32)(); cnt = (C.c_int * 32)()
        n = lib().poppy_hip_pool_timing_summary(self.h, names, ms, cnt, 32)
        return [(names[k].decode(), ms[k], cnt[k]) for k in range(n)]

    def warp_counts(self):
        f, a, b = C.c_ulonglong(0), C.c_ulonglong(0), C.c_ulonglong(0)
        lib().poppy_hip_pool_warp_counts(self.h, C.byref(f), C.byref(a), C.byref(b))
        return f.value, a.value, b.value

    def mask_rider(self):
        """True when the warp kernel also writes lbmask (else the level-0 blend kernels compute it from m2)."""
        return lib().poppy_hip_pool_mask_rider(self.h) == 1

    def warp_kernel_name(self):
        n = self.warp_counts()
        return WARP_KERNELS[n.index(max(n))]

    def morph_pairs_device_counted(self, ptr_pairs, w, h, phase=-1.0):
        """ptr_pairs: list of (device pointer of image 1, of image 2) on the pool's (single) device; frames go to the counting
        writer.  Returns the number of frames written."""
        def src(user, p, device, pa, sa, pb, sb):
            pa[0] = ptr_pairs[p][0]; sa[0] = w * 3
            pb[0] = ptr_pairs[p][1]; sb[0] = w * 3
            return 0
        fs = PAIR_SOURCE_CB(src)
        n = C.c_longlong(0)
        err = C.create_string_buffer(512)
        rc = lib().poppy_hip_pool_morph_pairs(self.h, len(ptr_pairs), w, h, phase, 1, C.cast(fs, C.c_void_p),
                                              C.cast(lib().poppy_count_pair_frames_cb, C.c_void_p), C.cast(C.byref(n), C.c_void_p), err, 512)
        if rc:
            raise PoppyError(f"poppy_hip_pool_morph_pairs: {rc}: {err.value.decode()}")
        return n.value

    # ---- batches without waiting for them (poppy_hip_pool_submit_pairs / poppy_hip_pool_wait) ----
    def submit_pairs_device_counted(self, ptr_pairs, w, h, phase=-1.0, on_device=True):
        """Queues the batch and returns; wait() returns the frames written by every batch submitted since the last wait().  on_device=False: the pointers are
        HOST pointers (tight rows; pinned memory if the uploads are to overlap anything) and every pair goes through poppy_hip_morph."""
        ptr_pairs = list(ptr_pairs)
        def src(user, p, device, pa, sa, pb, sb):
            pa[0] = ptr_pairs[p][0]; sa[0] = w * 3
            pb[0] = ptr_pairs[p][1]; sb[0] = w * 3
            return 0
        fs = PAIR_SOURCE_CB(src)
        if not hasattr(self, "_pending"):
            self._pending, self._count = [], C.c_longlong(0)
        self._pending.append((fs, ptr_pairs))                     # the callbacks stay alive until the wait
        rc = lib().poppy_hip_pool_submit_pairs(self.h, len(ptr_pairs), w, h, phase, 1 if on_device else 0, C.cast(fs, C.c_void_p),
                                               C.cast(lib().poppy_count_pair_frames_cb, C.c_void_p), C.cast(C.byref(self._count), C.c_void_p))
        if rc:
            raise PoppyError(f"poppy_hip_pool_submit_pairs: {rc}")

    def submit_pairs(self, pairs, write, phase=-1.0, inputs_on_device=False, w=None, h=None):
        """pairs: list of (bgr1, bgr2) host arrays — or (pointer 1, pointer 2) device pointers with inputs_on_device, w, h; write(pair, frame, view) is called
        from the pool's threads.  Returns at once; wait() returns when everything submitted has been written."""
        if not inputs_on_device:
            pairs = [(np.ascontiguousarray(a, np.uint8), np.ascontiguousarray(b, np.uint8)) for a, b in pairs]
            h, w = pairs[0][0].shape[:2]
        def src(user, p, device, pa, sa, pb, sb):
            pa[0] = pairs[p][0] if inputs_on_device else pairs[p][0].ctypes.data; sa[0] = w * 3
            pb[0] = pairs[p][1] if inputs_on_device else pairs[p][1].ctypes.data; sb[0] = w * 3
            return 0
        fmt = self.frame_format

        def wr(user, p, j, ptr, ww, hh, stride):
            write(p, j, _frame_view(ptr, ww, hh, stride, fmt))
        fs, fw = PAIR_SOURCE_CB(src), WRITE_PAIR_CB(wr)
        if not hasattr(self, "_pending"):
            self._pending, self._count = [], C.c_longlong(0)
        self._pending.append((fs, fw, pairs))
        rc = lib().poppy_hip_pool_submit_pairs(self.h, len(pairs), w, h, phase, 1 if inputs_on_device else 0, C.cast(fs, C.c_void_p), C.cast(fw, C.c_void_p), None)
        if rc:
            raise PoppyError(f"poppy_hip_pool_submit_pairs: {rc}")

    def wait(self):
        """Every batch submitted so far has been rendered and written; returns the frames the counting writer saw since the last wait()."""
        err = C.create_string_buffer(512)
        rc = lib().poppy_hip_pool_wait(self.h, err, 512)
        n = 0
        if hasattr(self, "_pending"):
            n, self._count.value = self._count.value, 0
            self._pending.clear()
        if rc:
            raise PoppyError(f"poppy_hip_pool_wait: {rc}: {err.value.decode()}")
        return n


def blur_margin_rects(w, h, union_w, union_h):
    """Host-only: (status, rects [4, 4] int32 = left, right, top, bottom as (x, y, width, height), origin (x, y)) of blur_margin's geometry.
    status is POPPY_OK, or POPPY_E_UNSUPPORTED (-6) where a strip leaves the canvas (the reference throws; the entry points refuse);
    bad sizes raise."""
    rects = np.zeros((4, 4), np.int32); origin = np.zeros(2, np.int32)
    rc = lib().poppy_blur_margin_rects(int(w), int(h), int(union_w), int(union_h), _p(rects), _p(origin))
    if rc not in (0, -6):
        raise PoppyError(f"poppy_blur_margin_rects: {rc}")
    return rc, rects, (int(origin[0]), int(origin[1]))


def blur_margin_taps():
    """Host-only: blur_margin's 127 fixed-point (8.8) taps."""
    taps = np.zeros(127, np.int32)
    rc = lib().poppy_blur_margin_taps(_p(taps))
    if rc:
        raise PoppyError(f"poppy_blur_margin_taps: {rc}")
    return taps


DENOISE_MAX_TABLE = 3 * 255 * 255 + 1      # no weight table is longer


def denoise_weights(hs, tw=7, sw=21):
    """Host-only: the weight table of the non-local-means denoise and its constants (poppy_denoise_weights, the one place they are formed):
    dict(table uint32 [n], n, L, fpm, shift).  A refusal raises PoppyError with the status."""
    t = np.zeros(DENOISE_MAX_TABLE, np.uint32)
    n, last, shift, fpm = C.c_int(0), C.c_int(0), C.c_int(0), C.c_uint32(0)
    rc = lib().poppy_denoise_weights(float(hs), int(tw), int(sw), _p(t), len(t), C.byref(n), C.byref(last), C.byref(fpm), C.byref(shift))
    if rc:
        raise PoppyError(f"poppy_denoise_weights: {rc}")
    return dict(table=t[:n.value].copy(), n=n.value, L=last.value, fpm=fpm.value, shift=shift.value)


def _denoise(call, bgr, hs, tw, sw, row_pad, dst_pad, chk=None):
    return _scaled_frame(call, "bgr_denoise", bgr, lambda w, h: (w, h), (float(hs), int(tw), int(sw)), row_pad, dst_pad, chk)


def bgr_denoise(bgr, hs, tw=7, sw=21, row_pad=0, dst_pad=0):
    """Host-only: an HxWx3 BGR image denoised by non-local means (poppy_bgr_denoise, the host statement that defines Context.denoise's rule).  row_pad /
    dst_pad: the image is handed over / taken back with that many extra bytes per row."""
    return _denoise(lib().poppy_bgr_denoise, bgr, hs, tw, sw, row_pad, dst_pad)


def denoise_tile():
    """Host-only: (width, height) of the output tile of the denoise kernel's workgroups."""
    w, h = C.c_int(0), C.c_int(0)
    if lib().poppy_denoise_tile(C.byref(w), C.byref(h)):
        raise PoppyError("poppy_denoise_tile")
    return w.value, h.value


def denoise_table_bound():
    """Host-only: the longest non-zero table prefix L the denoise kernel stages in LDS; a longer one is read from global memory."""
    n = C.c_int(0)
    if lib().poppy_denoise_table_bound(C.byref(n)):
        raise PoppyError("poppy_denoise_table_bound")
    return n.value


def dft_plan(n):
    """Host-only: (factors, itab, wave) of the length-n transform plan."""
    f = np.zeros(34, np.int32); nf = C.c_int(0); itab = np.zeros(n, np.int32); wave = np.zeros((n, 2), np.float32)
    rc = lib().poppy_dft_plan(n, _p(f), C.byref(nf), _p(itab), _p(wave))
    if rc:
        raise PoppyError(f"poppy_dft_plan: {rc}")
    return f[:nf.value].copy(), itab, wave


def printed_morph_distance(p1, p2, w, h):
    """Host-only: the "morph distance" poppy::morph prints for prepared point lists (src/poppy.hpp:142-159)."""
    p1 = np.ascontiguousarray(p1, np.float32); p2 = np.ascontiguousarray(p2, np.float32)
    d = C.c_double(0)
    rc = lib().poppy_printed_morph_distance(_p(p1), _p(p2), len(p1), w, h, C.byref(d))
    if rc:
        raise PoppyError(f"poppy_printed_morph_distance: {rc}")
    return d.value


def match_points(p1, p2, w, h, tolerance=1.0):
    """Host-only matcher (no GPU): returns (points1, points2, initial_morph_distance)."""
    p1 = np.ascontiguousarray(p1, np.float32); p2 = np.ascontiguousarray(p2, np.float32)
    n = len(p1)
    o1 = np.zeros((n + 4, 2), np.float32); o2 = np.zeros((n + 4, 2), np.float32)
    m = C.c_int(0); imd = C.c_double(0)
    rc = lib().poppy_match_points(_p(p1), _p(p2), n, w, h, tolerance, _p(o1), _p(o2), C.byref(m), C.byref(imd))
    if rc:
        raise PoppyError(f"poppy_match_points: {rc}")
    return o1[:m.value].copy(), o2[:m.value].copy(), imd.value


class Context:
    def __init__(self, device=0, **settings):
        L = lib()
        s = PoppySettings()
        L.poppy_settings_default(C.byref(s))
        for k, v in settings.items():
            setattr(s, k, v)
        self.settings = s
        self.h = L.poppy_hip_create(device, C.byref(s))
        if not self.h:
            raise PoppyError("poppy_hip_create failed: " + L.poppy_hip_create_error().decode())
        self.w = self.h_ = 0
        self.frame_format = FRAME_BGR
        self.frame_scale = 1
        self.frame_size = (0, 0)

    def set_frame_size(self, ow, oh):
        """The size (default (0, 0): none) every frame handed to a writer is resized to on the GPU by exact area weights, in front of the format conversion
        (poppy_hip_set_frame_size): writers get ow x oh frames in the context's format.  An alternative to set_frame_scale: downscale only, by at most 8 per
        axis.  Frames fetched with render(), frames kept on the device and the chain itself stay full size."""
        self._chk(lib().poppy_hip_set_frame_size(self.h, int(ow), int(oh)), "set_frame_size")
        self.frame_size = (int(ow), int(oh))

    def bgr_resize_area(self, bgr, ow, oh, row_pad=0, dst_pad=0):
        """An HxWx3 BGR frame resized on this context's GPU (poppy_hip_bgr_resize_area: upload, the kernel, download): the bytes of the host's bgr_resize_area.
        The low four bits of row_pad place the device copy of the source that many bytes behind a 256-byte boundary."""
        return _resize_area(lambda *args: lib().poppy_hip_bgr_resize_area(self.h, *args), bgr, ow, oh, row_pad, dst_pad, self._chk)

    def set_frame_scale(self, factor):
        """The whole factor 1..8 (default 1) every frame handed to a writer is scaled down by on the GPU, in front of the format conversion
        (poppy_hip_set_frame_scale): writers get frames of frame_scaled_size(W, H, factor) in the context's format.  Frames fetched with render(), frames kept
        on the device and the chain itself stay full size."""
        self._chk(lib().poppy_hip_set_frame_scale(self.h, int(factor)), "set_frame_scale")
        self.frame_scale = int(factor)

    def bgr_downscale(self, bgr, factor, row_pad=0, dst_pad=0):
        """An HxWx3 BGR frame scaled down on this context's GPU (poppy_hip_bgr_downscale: upload, the kernel, download): the bytes of the host's bgr_downscale.
        The low four bits of row_pad place the device copy of the source that many bytes behind a 256-byte boundary."""
        return _downscale(lambda *args: lib().poppy_hip_bgr_downscale(self.h, *args), bgr, factor, row_pad, dst_pad, self._chk)

    def set_frame_format(self, fmt):
        """FRAME_BGR (default), FRAME_I420, FRAME_PAL8 or FRAME_PAL8_SEQ (one palette for all frames of a call, which are handed over when the last
        one is rendered): the format of every frame handed to a writer (poppy_hip_set_frame_format).  Under I420 and both PAL8 formats the collecting wrappers return flat uint8 arrays of frame_bytes(format, W, H).
        FRAME_GIF: PAL8 frames with the indices LZW-coded on the GPU; the wrappers return flat arrays of each frame's own length (gif_frame_bytes).
        FRAME_GIF_SEQ: FRAME_PAL8_SEQ's sequences with every frame coded like FRAME_GIF's, one palette in all frames of a call.
        FRAME_JPEG: every frame one baseline JPEG file, coded on the GPU at set_jpeg_quality's quality; flat arrays of each frame's own length (jpeg_frame_bytes).
        FRAME_JPEG444: the same with full-resolution chroma (4:4:4), coded from the frame's I444 planes.
        FRAME_JPEG_OPT, FRAME_JPEG444_OPT: the same files on Huffman tables built on the GPU from each frame's own symbols: the same pixels in fewer bytes.
        FRAME_JPEG_SEQ, FRAME_JPEG444_SEQ: FRAME_JPEG_OPT's files on ONE table set for all the frames a call hands to its writer, built from their summed symbol
        counts; the writer is first called after the last frame is rendered.
        FRAME_PNG: every frame one PNG file, lossless, coded on the GPU; flat arrays of each frame's own length (png_frame_bytes).
        FRAME_PNG_RUNS: the same with runs of equal bytes coded as matches: several times smaller on frames with flat or smooth regions.
        FRAME_PNG_OPT: FRAME_PNG_RUNS with every segment on the shortest of the eight tables and one built on the GPU from its own symbols: never larger.
        FRAME_PNG_SEQ: FRAME_PNG_OPT's files on ONE ninth table for all the frames a call hands to its writer, built once from their summed token counts; the
        frames wait on the GPU as filtered streams and reach the writer after the last is rendered.  Never larger than FRAME_PNG_RUNS."""
        self._chk(lib().poppy_hip_set_frame_format(self.h, int(fmt)), "set_frame_format")
        self.frame_format = int(fmt)

    def set_jpeg_quality(self, quality):
        """The quality, 1..100 (default JPEG_QUALITY_DEFAULT), of the FRAME_JPEG frames this context hands to writers (poppy_hip_set_jpeg_quality)."""
        self._chk(lib().poppy_hip_set_jpeg_quality(self.h, int(quality)), "set_jpeg_quality")

    def set_jpeg_budget(self, max_frame_bytes):
        """The most bytes a FRAME_JPEG or FRAME_JPEG444 frame's file may have, 0 (the default) for none (poppy_hip_set_jpeg_budget): every frame is coded at the
        quality the budget's search picks at or below set_jpeg_quality's."""
        self._chk(lib().poppy_hip_set_jpeg_budget(self.h, int(max_frame_bytes)), "set_jpeg_budget")

    def get_jpeg_budget(self):
        """The context's byte budget (poppy_hip_get_jpeg_budget); 0: none."""
        v = C.c_size_t(0)
        self._chk(lib().poppy_hip_get_jpeg_budget(self.h, C.byref(v)), "get_jpeg_budget")
        return v.value

    def set_jpeg_sequence_budget(self, max_sequence_bytes):
        """The most bytes the files of all FRAME_JPEG or FRAME_JPEG444 frames of one sequence (a call's frames, a pair's) may have together, 0 (the default) for
        none (poppy_hip_set_jpeg_sequence_budget): the frames wait on the GPU and are all coded at the one quality the search picks at or below set_jpeg_quality's."""
        self._chk(lib().poppy_hip_set_jpeg_sequence_budget(self.h, int(max_sequence_bytes)), "set_jpeg_sequence_budget")

    def get_jpeg_sequence_budget(self):
        """The context's sequence budget (poppy_hip_get_jpeg_sequence_budget); 0: none."""
        v = C.c_uint64(0)
        self._chk(lib().poppy_hip_get_jpeg_sequence_budget(self.h, C.byref(v)), "get_jpeg_sequence_budget")
        return v.value

    def bgr_frames_to_jpeg_seq_budget_frames(self, frames, quality_max, budget, fmt=FRAME_JPEG, row_pad=0, frame_pad=0):
        """(frames, quality used) of a sequence of HxWx3 BGR frames under a sequence budget, searched and coded on this context's GPU on a sequence that lives for
        the call (poppy_hip_bgr_frames_to_jpeg_seq_budget_frames, poppy_hip_bgr_frames_to_jpeg444_seq_budget_frames): what the host's
        bgr_frames_to_jpeg_seq_budget_frames gives."""
        a, stride, frame_stride, n, w, h = _padded_frames(frames, row_pad, frame_pad)
        call = lib().poppy_hip_bgr_frames_to_jpeg444_seq_budget_frames if fmt == FRAME_JPEG444 else lib().poppy_hip_bgr_frames_to_jpeg_seq_budget_frames
        return _jpeg_seq_budget_frames(lambda dst, used: call(self.h, _p(a), stride, frame_stride, n, w, h, int(quality_max), int(budget), dst, used),
                                       "bgr_frames_to_jpeg_seq_budget_frames", fmt, n, w, h, self._chk)

    def i420_to_jpeg_budget_frame(self, i420, w, h, quality_max, budget):
        """(frame, quality used) of a flat I420 frame under a byte budget, searched and coded on this context's GPU (poppy_hip_i420_to_jpeg_budget_frame): what the
        host's i420_to_jpeg_budget_frame gives."""
        return _planes_to_jpeg_budget(lambda *args: lib().poppy_hip_i420_to_jpeg_budget_frame(self.h, *args), FRAME_JPEG, i420, w, h, quality_max, budget, self._chk)

    def i444_to_jpeg_budget_frame(self, i444, w, h, quality_max, budget):
        """The same for FRAME_JPEG444 on flat I444 planes (poppy_hip_i444_to_jpeg_budget_frame)."""
        return _planes_to_jpeg_budget(lambda *args: lib().poppy_hip_i444_to_jpeg_budget_frame(self.h, *args), FRAME_JPEG444, i444, w, h, quality_max, budget, self._chk)

    def i420_to_jpeg_frame(self, i420, w, h, quality=JPEG_QUALITY_DEFAULT):
        """The FRAME_JPEG frame of a flat I420 frame, coded on this context's GPU (poppy_hip_i420_to_jpeg_frame: upload, the two kernels, download): the bytes
        of the host's i420_to_jpeg_frame."""
        return _planes_to_jpeg(lambda *args: lib().poppy_hip_i420_to_jpeg_frame(self.h, *args), FRAME_JPEG, i420, w, h, quality, self._chk)

    def bgr_to_i444(self, bgr, row_pad=0):
        """The I444 planes of an HxWx3 BGR frame, converted on this context's GPU (poppy_hip_bgr_to_i444: upload, the kernel, download): the bytes of the host's
        bgr_to_i444.  The low four bits of row_pad place the device copy of the source that many bytes behind a 256-byte boundary."""
        return _i444(lambda *args: lib().poppy_hip_bgr_to_i444(self.h, *args), "bgr_to_i444", bgr, row_pad, self._chk)

    def bgr_to_png_frame(self, bgr, row_pad=0, whole=False):
        """The FRAME_PNG frame of an HxWx3 BGR frame, coded on this context's GPU (poppy_hip_bgr_to_png_frame: upload, the six kernels, download of `total` bytes):
        the bytes of the host's bgr_to_png_frame.  The low four bits of row_pad place the device copy of the source that many bytes behind a 256-byte boundary."""
        return _png_frame(lambda *args: lib().poppy_hip_bgr_to_png_frame(self.h, *args), "bgr_to_png_frame", bgr, row_pad, self._chk, whole)

    def bgr_to_png_runs_frame(self, bgr, row_pad=0, whole=False):
        """The FRAME_PNG_RUNS frame of an HxWx3 BGR frame, coded on this context's GPU (poppy_hip_bgr_to_png_runs_frame): the bytes of the host's
        bgr_to_png_runs_frame.  row_pad and whole as in bgr_to_png_frame."""
        return _png_frame(lambda *args: lib().poppy_hip_bgr_to_png_runs_frame(self.h, *args), "bgr_to_png_runs_frame", bgr, row_pad, self._chk, whole, FRAME_PNG_RUNS)

    def bgr_to_png_opt_frame(self, bgr, row_pad=0, whole=False):
        """The FRAME_PNG_OPT frame of an HxWx3 BGR frame, coded on this context's GPU (poppy_hip_bgr_to_png_opt_frame): the bytes of the host's
        bgr_to_png_opt_frame.  row_pad and whole as in bgr_to_png_frame."""
        return _png_frame(lambda *args: lib().poppy_hip_bgr_to_png_opt_frame(self.h, *args), "bgr_to_png_opt_frame", bgr, row_pad, self._chk, whole, FRAME_PNG_OPT)

    def png_optimal_lengths(self, counts, limit=15):
        """The length-build routine of the FRAME_PNG_OPT coder alone on 1..286 symbol counts (poppy_hip_png_optimal_lengths): what the host's png_optimal_lengths gives."""
        return _optimal_lengths(lambda *args: lib().poppy_hip_png_optimal_lengths(self.h, *args), counts, limit, "png_optimal_lengths", self._chk)

    def i420_to_jpeg_opt_frame(self, i420, w, h, quality=JPEG_QUALITY_DEFAULT):
        """The FRAME_JPEG_OPT frame of a flat I420 frame, coded on this context's GPU (poppy_hip_i420_to_jpeg_opt_frame: upload, the four kernels, download): the
        bytes of the host's i420_to_jpeg_opt_frame."""
        return _planes_to_jpeg(lambda *args: lib().poppy_hip_i420_to_jpeg_opt_frame(self.h, *args), FRAME_JPEG_OPT, i420, w, h, quality, self._chk)

    def i444_to_jpeg_opt_frame(self, i444, w, h, quality=JPEG_QUALITY_DEFAULT):
        """The FRAME_JPEG444_OPT frame of flat I444 planes, coded on this context's GPU (poppy_hip_i444_to_jpeg_opt_frame): the bytes of the host's."""
        return _planes_to_jpeg(lambda *args: lib().poppy_hip_i444_to_jpeg_opt_frame(self.h, *args), FRAME_JPEG444_OPT, i444, w, h, quality, self._chk)

    def jpeg_optimal_table(self, counts):
        """The table-build kernel alone on 256 symbol counts (poppy_hip_jpeg_optimal_table): what the host's jpeg_optimal_table gives."""
        return _optimal_table(lambda *args: lib().poppy_hip_jpeg_optimal_table(self.h, *args), counts, "jpeg_optimal_table", self._chk)

    def i444_to_jpeg_frame(self, i444, w, h, quality=JPEG_QUALITY_DEFAULT):
        """The FRAME_JPEG444 frame of flat I444 planes, coded on this context's GPU (poppy_hip_i444_to_jpeg_frame: upload, the two kernels, download): the bytes
        of the host's i444_to_jpeg_frame."""
        return _planes_to_jpeg(lambda *args: lib().poppy_hip_i444_to_jpeg_frame(self.h, *args), FRAME_JPEG444, i444, w, h, quality, self._chk)

    def pal8_to_gif_frame(self, pal8, w, h):
        """The FRAME_GIF frame of a flat PAL8 frame, coded on this context's GPU (poppy_hip_pal8_to_gif_frame: upload, the two kernels, download): the bytes of
        the host's pal8_to_gif_frame."""
        return _pal8_to_gif(lambda *args: lib().poppy_hip_pal8_to_gif_frame(self.h, *args), pal8, w, h, self._chk)

    def bgr_frames_to_png_seq_frames(self, frames, row_pad=0, frame_pad=0):
        """The FRAME_PNG_SEQ frames of a sequence of n HxWx3 BGR frames, coded on this context's GPU on a sequence that lives for the call
        (poppy_hip_bgr_frames_to_png_seq_frames: per frame upload, filter and counting kernel; one table build; per frame choice, pack and download): the bytes of
        the host's bgr_frames_to_png_seq_frames, as its list."""
        return _png_seq_frames(lambda *args: lib().poppy_hip_bgr_frames_to_png_seq_frames(self.h, *args), "bgr_frames_to_png_seq_frames", frames, row_pad, frame_pad, self._chk)

    def png_seq_table(self, counts):
        """The table-build kernel of the FRAME_PNG_SEQ coder alone on 286 summed counts (poppy_hip_png_seq_table): what the host's png_seq_table gives."""
        return _png_seq_table(lambda *args: lib().poppy_hip_png_seq_table(self.h, *args), counts, "png_seq_table", self._chk)

    def bgr_frames_to_jpeg_seq_frames(self, frames, quality=JPEG_QUALITY_DEFAULT, fmt=FRAME_JPEG_SEQ, row_pad=0, frame_pad=0):
        """The FRAME_JPEG_SEQ (FRAME_JPEG444_SEQ) frames of a sequence of n HxWx3 BGR frames, coded on this context's GPU on a sequence that lives for the call
        (poppy_hip_bgr_frames_to_jpeg_seq_frames: per frame upload, raster and counting kernels; one table build; per frame coder, gather and download): the bytes of
        the host's bgr_frames_to_jpeg_seq_frames, as its list."""
        a, stride, frame_stride, n, w, h = _padded_frames(frames, row_pad, frame_pad)
        call = lib().poppy_hip_bgr_frames_to_jpeg444_seq_frames if fmt == FRAME_JPEG444_SEQ else lib().poppy_hip_bgr_frames_to_jpeg_seq_frames
        return _jpeg_seq_frames(lambda dst: call(self.h, _p(a), stride, frame_stride, n, w, h, int(quality), dst), "bgr_frames_to_jpeg_seq_frames", fmt, n, w, h, self._chk)

    def bgr_frames_to_gif_frames(self, frames, row_pad=0, frame_pad=0):
        """The FRAME_GIF_SEQ frames of a sequence of n HxWx3 BGR frames, palette and coding on this context's GPU (poppy_hip_bgr_frames_to_gif_frames: upload, the
        sequence pass per frame, the palette build, the coder and the gather per frame, download): the bytes of the host's bgr_frames_to_gif_frames, as its list."""
        return _gif_frames(lambda *args: lib().poppy_hip_bgr_frames_to_gif_frames(self.h, *args), frames, row_pad, frame_pad, self._chk)

    def close(self):
        if self.h:
            lib().poppy_hip_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, what):
        if rc:
            raise PoppyError(f"{what}: {rc}: {lib().poppy_hip_last_error(self.h).decode()}")

    def morph_images(self, c1, c2, gabor2, p1, p2, shape, mask):
        c1 = np.ascontiguousarray(c1, np.uint8); c2 = np.ascontiguousarray(c2, np.uint8)
        g = np.ascontiguousarray(gabor2, np.float32)
        p1 = np.ascontiguousarray(p1, np.float32); p2 = np.ascontiguousarray(p2, np.float32)
        h, w = c1.shape[:2]
        out = np.empty((h, w, 3), np.uint8)
        mp = np.empty((len(p1), 2), np.float32)
        self._chk(lib().poppy_hip_morph_images(self.h, _p(c1), w * 3, _p(c2), w * 3, _p(g), w, h, _p(p1), _p(p2), len(p1),
                                               shape, mask, _p(out), w * 3, _p(mp)), "morph_images")
        self.w, self.h_ = w, h
        return out, mp

    def pair_load(self, c1, c2, gabor2, p1, p2):
        c1 = np.ascontiguousarray(c1, np.uint8); c2 = np.ascontiguousarray(c2, np.uint8)
        g = np.ascontiguousarray(gabor2, np.float32)
        p1 = np.ascontiguousarray(p1, np.float32); p2 = np.ascontiguousarray(p2, np.float32)
        h, w = c1.shape[:2]
        self._chk(lib().poppy_hip_pair_load(self.h, _p(c1), w * 3, _p(c2), w * 3, _p(g), w, h, _p(p1), _p(p2), len(p1)), "pair_load")
        self.w, self.h_ = w, h

    def pair_load_device(self, d1, d2, dg, w, h, p1, p2):
        p1 = np.ascontiguousarray(p1, np.float32); p2 = np.ascontiguousarray(p2, np.float32)
        self._chk(lib().poppy_hip_pair_load_device(self.h, d1, d2, dg, w, h, _p(p1), _p(p2), len(p1)), "pair_load_device")
        self.w, self.h_ = w, h

    def render(self, shape, mask, chain=False, fetch=True):
        out = np.empty((self.h_, self.w, 3), np.uint8) if fetch else None
        self._chk(lib().poppy_hip_render(self.h, shape, mask, int(chain), _p(out), self.w * 3), "render")
        return out

    def orb_detect(self, gray, nfeatures):
        g = np.ascontiguousarray(gray, np.uint8)
        h, w = g.shape
        cap = max(2 * nfeatures + 64, 64)
        kp = np.zeros((cap, 7), np.float32)
        n = C.c_int(0)
        rc = lib().poppy_hip_orb_detect(self.h, _p(g), w, w, h, nfeatures, _p(kp), cap, C.byref(n))
        if rc == -1 and n.value > cap:      # POPPY_E_ARG, count reported: retainBest kept more ties with the n-th response than the guess holds
            cap = n.value
            kp = np.zeros((cap, 7), np.float32)
            rc = lib().poppy_hip_orb_detect(self.h, _p(g), w, w, h, nfeatures, _p(kp), cap, C.byref(n))
        self._chk(rc, "orb_detect")
        return kp[:n.value].copy()

    def median_blur(self, img, ksize, form=0):
        """cv::medianBlur on a single-channel u8 image; form: 0 chain default, 1 lane per column, 2 column histograms over the ranks of each tile's values,
        3 the same without presence maps, 4 no one-count tiles, 5 every tile by windows of ranks, 6 / 7 first window at the top / bottom (include/poppy_hip.h)."""
        a = np.ascontiguousarray(img, np.uint8)
        h, w = a.shape
        out = np.zeros((h, w), np.uint8)
        self._chk(lib().poppy_hip_median_blur(self.h, _p(a), w, h, int(ksize), int(form), _p(out)), "median_blur")
        return out

    def foreground_median_links(self, which=0):
        """(cols_mask, decided_by) of the last chain of medians that image slot `which` ran: bit i of cols_mask = the link of ksize 8 i + 1 went
        through k_median_cols (0xffe: all eleven real links); decided_by: MEDIAN_BY_HINT / _DEVICE / _ENV, 0 before any chain."""
        m, d = C.c_uint(0), C.c_int(0)
        self._chk(lib().poppy_hip_foreground_median_links(self.h, int(which), C.byref(m), C.byref(d)), "foreground_median_links")
        return m.value, d.value

    def unsharp_frame(self, src, amount, form=0, pitch=None, amount_on_device=False, want_float=False):
        """The frame path's last stage on a float image (h, w, 3): unsharp_mask(src, 1, amount, 0.3) + convertTo(CV_8U, 255) -> u8 (h, w, 3), with
        want_float=True (u8, the float image before the conversion).  form: 0 what a frame of this geometry takes, 1 tile kernel, 2 streaming kernel,
        3 separable kernels (include/poppy_hip.h).  pitch: pixels per row of the array `src` is cut from — `src` is then the `[:, :w]` view of a
        C-contiguous (h, pitch, 3) array, whose padding pixels go to the device with the rows.  amount_on_device: the kernel reads the amount from
        device memory, as a captured frame body's does."""
        v = np.asarray(src)
        if v.dtype != np.float32 or v.ndim != 3 or v.shape[2] != 3:
            raise ValueError("unsharp_frame takes a float32 (h, w, 3) image")
        h, w = v.shape[:2]
        if pitch is None:
            a = np.ascontiguousarray(v); pitch = w
        else:                                   # `src` is the first w columns of a C-contiguous (h, pitch, 3) array: handed over with its padding
            if pitch < w or v.strides != (pitch * 12, 12, 4):
                raise ValueError("with a pitch, src must be the [:, :w] view of a C-contiguous (h, pitch, 3) array")
            a = v
        out = np.zeros((h, w, 3), np.uint8)
        outf = np.zeros((h, w, 3), np.float32) if want_float else None
        self._chk(lib().poppy_hip_unsharp_frame(self.h, a.ctypes.data, w, h, int(pitch), float(amount), int(form), int(bool(amount_on_device)),
                                                _p(out), _p(outf) if want_float else None), "unsharp_frame")
        return (out, outf) if want_float else out

    def foreground(self, bgr, debug=False):
        """Extractor::foreground for one BGR image -> goodFeatures (u8); with debug=True a dict with every intermediate."""
        a = np.ascontiguousarray(bgr, np.uint8)
        h, w = a.shape[:2]
        out = np.zeros((h, w), np.uint8)
        if not debug:
            self._chk(lib().poppy_hip_foreground(self.h, _p(a), w * 3, w, h, _p(out), None), "foreground")
            return out
        grey = np.zeros((h, w), np.uint8); masked = np.zeros((h, w), np.uint8)
        stages = np.zeros((50, h, w), np.uint8); floats = np.zeros((3, h, w), np.float32)

        class Dbg(C.Structure):
            _fields_ = [("grey", C.c_void_p), ("stages", C.c_void_p), ("floats", C.c_void_p), ("masked", C.c_void_p)]
        d = Dbg(grey.ctypes.data, stages.ctypes.data, floats.ctypes.data, masked.ctypes.data)
        self._chk(lib().poppy_hip_foreground(self.h, _p(a), w * 3, w, h, _p(out), C.byref(d)), "foreground")
        res = dict(foreground=out, grey=grey, masked=masked, lin=floats[0], logged=floats[1], finalMask=floats[2],
                   flow0=stages[0], acc0=stages[1])
        for k in range(12):
            res[f"med{k + 1}"], res[f"flow{k + 1}"], res[f"acc{k + 1}"], res[f"blur{k + 1}"] = stages[2 + 4 * k: 6 + 4 * k]
        return res

    def pair_begin(self, bgr1, bgr2):
        """Raw BGR pair -> resident pair (pre-ORB chain, ORB, matcher, gabor2 on the GPU). Returns (nfeatures, (d1, d2))."""
        a = np.ascontiguousarray(bgr1, np.uint8); b = np.ascontiguousarray(bgr2, np.uint8)
        h, w = a.shape[:2]
        self._chk(lib().poppy_hip_pair_begin(self.h, _p(a), w * 3, _p(b), w * 3, w, h), "pair_begin")
        self.w, self.h_ = w, h
        nf = C.c_int(0); d = (C.c_double * 2)()
        lib().poppy_hip_pair_begin_info(self.h, C.byref(nf), d)
        return nf.value, (d[0], d[1])

    def pair_begin_info(self):
        """(nfeatures, (detail of image 1, of image 2)) of the resident pair's set-up."""
        nf = C.c_int(0); d = (C.c_double * 2)()
        lib().poppy_hip_pair_begin_info(self.h, C.byref(nf), d)
        return nf.value, (d[0], d[1])

    def comm_init(self, rank, world, id128):
        buf = (C.c_uint8 * 128).from_buffer_copy(id128)
        self._chk(lib().poppy_hip_comm_init(self.h, rank, world, buf), "comm_init")

    def comm_info(self):
        """(rank, world) as given to comm_init and (rank, count) as the RCCL communicator reports them (-1 without one)."""
        v = [C.c_int(-1) for _ in range(4)]
        self._chk(lib().poppy_hip_comm_info(self.h, *[C.byref(x) for x in v]), "comm_info")
        return tuple(x.value for x in v)

    def comm_free(self):
        lib().poppy_hip_comm_free(self.h)

    def pair_broadcast(self, root, w, h):
        self._chk(lib().poppy_hip_pair_broadcast(self.h, root, w, h), "pair_broadcast")
        self.w, self.h_ = w, h

    def comm_max(self, value):
        d = C.c_double(value)
        self._chk(lib().poppy_hip_comm_max(self.h, C.byref(d)), "comm_max")
        return d.value

    def pair_export_device(self, d_dst, nbytes):
        self._chk(lib().poppy_hip_pair_export_device(self.h, d_dst, nbytes), "pair_export_device")

    def pair_import_device(self, d_src, nbytes, w, h):
        self._chk(lib().poppy_hip_pair_import_device(self.h, d_src, nbytes, w, h), "pair_import_device")
        self.w, self.h_ = w, h

    def pair_begin_sharded(self, d1, d2, w, h, root=0):
        """Collective over this context's communicator: the pair set-up itself spread over the ranks (d1 / d2: device pointers of the raw
        pair on rank `root`, None elsewhere); every rank ends up with the resident pair."""
        self._chk(lib().poppy_hip_pair_begin_sharded(self.h, d1, d2, w, h, root), "pair_begin_sharded")
        self.w, self.h_ = w, h

    def pair_begin_device(self, d1, d2, w, h):
        """Raw BGR pair already in this GPU's memory (device pointers, tight rows)."""
        self._chk(lib().poppy_hip_pair_begin_device(self.h, d1, d2, w, h), "pair_begin_device")
        self.w, self.h_ = w, h

    def pair_begin_next(self, bgr):
        """The next pair of the CLI's loop: image 1 = the resident pair's corrected2, image 2 = bgr (image 1's filter chain is reused when it can be)."""
        b = np.ascontiguousarray(bgr, np.uint8)
        h, w = b.shape[:2]
        self._chk(lib().poppy_hip_pair_begin_next(self.h, _p(b), w * 3, w, h), "pair_begin_next")
        self.w, self.h_ = w, h

    def pair_begin_next_device(self, d_bgr, w, h):
        """pair_begin_next with image 2 already in this GPU's memory (device pointer, tight rows)."""
        self._chk(lib().poppy_hip_pair_begin_next_device(self.h, d_bgr, w, h), "pair_begin_next_device")
        self.w, self.h_ = w, h

    def chain_counts(self):
        """(image chains run, image chains reused) by this context's pair set-ups since it was created."""
        run, reused = C.c_ulonglong(0), C.c_ulonglong(0)
        self._chk(lib().poppy_hip_chain_counts(self.h, C.byref(run), C.byref(reused)), "chain_counts")
        return run.value, reused.value

    def morph_list(self, images, phase=-1.0, canvas=None, collect=True, counted=False, on_device=False, write=None):
        """The CLI's loop over an image list in one call (poppy_hip_morph_list): returns (status, frames per pair, printed distance per pair,
        pairs done).  status is POPPY_OK (0) or POPPY_E_NOMATCH (-5, the failing pair's fallback frames written); anything else raises.
        images: HxWx3 uint8 arrays, or with on_device=True (device pointer, w, h) tuples.  canvas: (width, height) to pad every image into by
        blur_margin's rule, None = one size for all.  counted: frames go to the library's counting writer; frames per pair is then [total].
        write: optional callable(pair, frame, view) instead of collecting (the view of the pinned host copy is valid during the call)."""
        imgs = list(images) if on_device else [np.ascontiguousarray(a, np.uint8) for a in images]
        n = len(imgs)

        def src(user, k, pp, ps, pw, ph):
            if on_device:
                ptr, w, h = imgs[k]
                pp[0], ps[0], pw[0], ph[0] = ptr, w * 3, w, h
            else:
                a = imgs[k]
                pp[0], ps[0], pw[0], ph[0] = a.ctypes.data, a.shape[1] * 3, a.shape[1], a.shape[0]
            return 0
        frames = [[] for _ in range(max(n - 1, 0))]

        fmt = self.frame_format

        def wr(user, k, j, ptr, ww, hh, stride):
            view = _frame_view(ptr, ww, hh, stride, fmt)
            if write is not None:
                write(k, j, view)
            else:
                frames[k].append(view.copy())
        fs = IMAGE_SOURCE_CB(src)
        count = C.c_longlong(0)
        if counted:
            wcb, user = C.cast(lib().poppy_count_pair_frames_cb, C.c_void_p), C.cast(C.byref(count), C.c_void_p)
        else:
            fw = WRITE_PAIR_CB(wr) if (collect or write is not None) else None
            wcb, user = (C.cast(fw, C.c_void_p) if fw else None), None
        dist = np.full(max(n - 1, 1), np.nan)
        done = C.c_int(0)
        cw, ch = canvas if canvas is not None else (0, 0)
        rc = lib().poppy_hip_morph_list(self.h, n, int(cw), int(ch), float(phase), int(on_device), C.cast(fs, C.c_void_p), wcb, user,
                                        _p(dist), C.byref(done))
        if rc not in (0, -5):
            self._chk(rc, "morph_list")
        if canvas is not None:
            self.w, self.h_ = int(cw), int(ch)
        elif n:
            self.w, self.h_ = (imgs[0][1], imgs[0][2]) if on_device else (imgs[0].shape[1], imgs[0].shape[0])
        return rc, ([count.value] if counted else frames), [float(x) for x in dist[:max(n - 1, 0)]], done.value

    def morph_frames_counted(self, phase=-1.0):
        """The frame loop with every frame handed to the library's counting writer (pinned host hand-off, no Python per frame)."""
        n = C.c_longlong(0)
        cb = C.cast(lib().poppy_count_frames_cb, C.c_void_p)
        self._chk(lib().poppy_hip_morph_frames(self.h, phase, cb, C.cast(C.byref(n), C.c_void_p)), "morph_frames")
        return n.value

    def render_phases(self, ts, write=None, counted=False):
        """Frames of the sharded job: phase t_k each (t == 0 / 1: copies of image 1 / 2).  counted: frames go to the library's
        counting writer and the count is returned."""
        t = np.ascontiguousarray(ts, np.float64)
        if counted:
            n = C.c_longlong(0)
            self._chk(lib().poppy_hip_render_phases(self.h, _p(t), len(t), C.cast(lib().poppy_count_frames_cb, C.c_void_p), C.cast(C.byref(n), C.c_void_p)), "render_phases")
            return n.value
        fn = None
        if write is not None:
            fmt = self.frame_format

            def cb(user, ptr, w, h, stride):
                write(_frame_view(ptr, w, h, stride, fmt))
            fn = WRITE_CB(cb)
        self._chk(lib().poppy_hip_render_phases(self.h, _p(t), len(t), C.cast(fn, C.c_void_p) if fn else None, None), "render_phases")

    def render_many_counted(self, shapes, chain=False):
        sh = np.ascontiguousarray(shapes, np.float64)
        n = C.c_longlong(0)
        cb = C.cast(lib().poppy_count_frames_cb, C.c_void_p)
        self._chk(lib().poppy_hip_render_many(self.h, _p(sh), _p(sh), len(sh), int(chain), cb, C.cast(C.byref(n), C.c_void_p)), "render_many")
        return n.value

    def orb_input(self, good_features):
        gf = np.ascontiguousarray(good_features, np.uint8)
        h, w = gf.shape
        g = np.zeros((h, w), np.uint8); us = np.zeros((h, w), np.float32); gb = np.zeros((h, w), np.float32); d = C.c_double(0)
        self._chk(lib().poppy_hip_orb_input(self.h, _p(gf), w, h, _p(g), _p(us), _p(gb), C.byref(d)), "orb_input")
        return dict(g=g, us=us, gb=gb, detail=d.value)

    def blur_margin(self, bgr, union_w, union_h, src_pad=0, dst_pad=0):
        """blur_margin's padded image.  bgr: HxWx3 uint8 whose rows may be strided (pixels contiguous), read in place; src_pad > 0 copies it
        into rows src_pad bytes longer first.  dst_pad: the destination's rows are that many bytes longer (the pad bytes must come back untouched)."""
        a = np.asarray(bgr, np.uint8)
        h, w = a.shape[:2]
        if a.strides[1:] != (3, 1) or a.strides[0] < w * 3 or src_pad:
            buf = np.full((h, w * 3 + src_pad), 0x5A, np.uint8)
            buf[:, :w * 3] = a.reshape(h, w * 3)
            a = buf[:, :w * 3].reshape(h, w, 3)
        stride = a.strides[0]
        full = np.full((union_h, union_w * 3 + dst_pad), 0xA5, np.uint8)
        self._chk(lib().poppy_hip_blur_margin(self.h, a.ctypes.data, stride, w, h, union_w, union_h, _p(full), union_w * 3 + dst_pad), "blur_margin")
        if dst_pad and not (full[:, union_w * 3:] == 0xA5).all():
            raise PoppyError("blur_margin wrote into the destination's row padding")
        return np.ascontiguousarray(full[:, :union_w * 3]).reshape(union_h, union_w, 3)

    def denoise(self, bgr, hs, tw=7, sw=21, row_pad=0, dst_pad=0):
        """capi.bgr_denoise on this context's GPU (poppy_hip_denoise: upload, the kernel, download): the same bytes."""
        return _denoise(lambda *args: lib().poppy_hip_denoise(self.h, *args), bgr, hs, tw, sw, row_pad, dst_pad, self._chk)

    def denoise_device(self, d_src, d_dst, w, h, hs, tw=7, sw=21):
        """Device image (pointer, tight rows) -> device image, queued on the context's stream (poppy_hip_denoise_device); sync() before reading d_dst."""
        self._chk(lib().poppy_hip_denoise_device(self.h, d_src, d_dst, int(w), int(h), float(hs), int(tw), int(sw)), "denoise_device")

    def set_denoise(self, hs, tw=7, sw=21):
        """The CLI's --denoise for morph_list (poppy_hip_set_denoise): every image of a list is denoised on the GPU as it arrives, at its own size and in
        front of the canvas padding.  hs = 0 (the default): off.  morph, the pair loaders, pools and the multi-GPU entry points are not affected."""
        self._chk(lib().poppy_hip_set_denoise(self.h, float(hs), int(tw), int(sw)), "set_denoise")

    def get_denoise(self):
        """(hs, tw, sw) of set_denoise; hs 0.0: off."""
        hs, tw, sw = C.c_float(0), C.c_int(0), C.c_int(0)
        self._chk(lib().poppy_hip_get_denoise(self.h, C.byref(hs), C.byref(tw), C.byref(sw)), "get_denoise")
        return hs.value, tw.value, sw.value

    def blur_margin_max_rows(self):
        """The most canvas rows blur_margin takes on this context's device."""
        n = C.c_int(0)
        self._chk(lib().poppy_hip_blur_margin_max_rows(self.h, C.byref(n)), "blur_margin_max_rows")
        return n.value

    def time_last_warp(self, reps=50):
        """Average milliseconds per launch of the last frame's fused raster + warp kernel, relaunched back to back, nothing else running."""
        ms = C.c_float(0)
        self._chk(lib().poppy_hip_time_last_warp(self.h, int(reps), C.byref(ms)), "time_last_warp")
        return ms.value

    def set_gabor_direct(self, on=True):
        """Gabor banks as direct double sums (True) or tiled FFTs (False, the default)."""
        self._chk(lib().poppy_hip_set_gabor_direct(self.h, int(on)), "set_gabor_direct")

    def set_setup_chains(self, serial=True):
        """pair set-up: the two images' chains one after the other (True; what a pool of >= 3 contexts uses) or side by side (False, a context's default)."""
        self._chk(lib().poppy_hip_set_setup_chains(self.h, int(serial)), "set_setup_chains")

    def gabor_field(self, bgr):
        a = np.ascontiguousarray(bgr, np.uint8)
        h, w = a.shape[:2]
        out = np.zeros((h, w, 3), np.float32)
        self._chk(lib().poppy_hip_gabor_field(self.h, _p(a), w * 3, w, h, _p(out)), "gabor_field")
        return out

    def orb_describe(self, gray, kps7):
        g = np.ascontiguousarray(gray, np.uint8)
        k = np.ascontiguousarray(kps7, np.float32)
        h, w = g.shape
        out = np.zeros((len(k), 32), np.uint8)
        self._chk(lib().poppy_hip_orb_describe(self.h, _p(g), w, w, h, _p(k), len(k), _p(out)), "orb_describe")
        return out

    def hamming_match(self, query, train):
        q = np.ascontiguousarray(query, np.uint8); t = np.ascontiguousarray(train, np.uint8)
        out = np.zeros((len(q), 3), np.int32)
        n = C.c_int(0)
        self._chk(lib().poppy_hip_hamming_match(self.h, _p(q), len(q), _p(t), len(t), _p(out), C.byref(n)), "hamming_match")
        return out[:n.value].copy()

    def pair_corrected2(self, w, h):
        out = np.zeros((h, w, 3), np.uint8)
        self._chk(lib().poppy_hip_pair_corrected2(self.h, _p(out), w * 3), "pair_corrected2")
        return out

    def warp_affine(self, img, M):
        a = np.ascontiguousarray(img, np.uint8)
        h, w = a.shape[:2]
        m = np.ascontiguousarray(M, np.float64).reshape(6)
        out = np.zeros_like(a)
        self._chk(lib().poppy_hip_warp_affine(self.h, _p(a), w * 3, w, h, _p(m), _p(out), w * 3), "warp_affine")
        return out

    def align(self, which, img, p1, p2):
        """which: 'retranslate' | 'reprocrustes' | 'rerotate' | 'auto' -> (image, points2, distance)."""
        im = np.ascontiguousarray(img, np.uint8).copy()
        a = np.ascontiguousarray(p1, np.float32).reshape(-1, 2); b = np.ascontiguousarray(p2, np.float32).reshape(-1, 2).copy()
        h, w = im.shape[:2]
        d = C.c_double(0)
        if which == "auto":
            self._chk(lib().poppy_hip_auto_align(self.h, _p(im), w * 3, w, h, _p(a), _p(b), len(a), C.byref(d)), "auto_align")
        else:
            code = {"retranslate": 0, "reprocrustes": 1, "rerotate": 2}[which]
            self._chk(lib().poppy_hip_align_step(self.h, code, _p(im), w * 3, w, h, _p(a), _p(b), len(a), C.byref(d)), "align_step")
        return im, b, d.value

    def align_scores(self, p1, sets, w, h):
        """What the align searches rank by, for candidate versions of the second point list (sets: n_cand x n x 2):
        (morph distances f64, totals f32, pair counts i32, raw offset sums f32), one entry per candidate."""
        a = np.ascontiguousarray(p1, np.float32).reshape(-1, 2)
        s = np.ascontiguousarray(sets, np.float32).reshape(-1, len(a), 2)
        k = len(s)
        d = np.zeros(k, np.float64); total = np.zeros(k, np.float32); n_pairs = np.zeros(k, np.int32); inner = np.zeros(k, np.float32)
        self._chk(lib().poppy_hip_align_scores(self.h, _p(a), _p(s), len(a), k, int(w), int(h), _p(d), _p(total), _p(n_pairs), _p(inner)), "align_scores")
        return d, total, n_pairs, inner

    def hamming_knn2(self, query, train):
        q = np.ascontiguousarray(query, np.uint8).reshape(-1, 32); t = np.ascontiguousarray(train, np.uint8).reshape(-1, 32)
        out = np.zeros((len(q), 4), np.int32)
        self._chk(lib().poppy_hip_hamming_knn2(self.h, _p(q), len(q), _p(t), len(t), _p(out)), "hamming_knn2")
        return out

    def pair_begin_descriptors(self, bgr1, bgr2, ratio=0.7):
        """Opt-in descriptor mode of the pair set-up; returns nfeatures."""
        a = np.ascontiguousarray(bgr1, np.uint8); b = np.ascontiguousarray(bgr2, np.uint8)
        h, w = a.shape[:2]
        self._chk(lib().poppy_hip_pair_begin_descriptors(self.h, _p(a), w * 3, _p(b), w * 3, w, h, ratio), "pair_begin_descriptors")
        nf = C.c_int(0)
        lib().poppy_hip_pair_begin_info(self.h, C.byref(nf), None)
        return nf.value

    def pair_begin_descriptors_ransac(self, bgr1, bgr2, ratio=0.7, distance=3.0):
        """The descriptor mode with the RANSAC fundamental-matrix filter behind the symmetry test; returns nfeatures."""
        a = np.ascontiguousarray(bgr1, np.uint8); b = np.ascontiguousarray(bgr2, np.uint8)
        h, w = a.shape[:2]
        self._chk(lib().poppy_hip_pair_begin_descriptors_ransac(self.h, _p(a), w * 3, _p(b), w * 3, w, h, ratio, distance), "pair_begin_descriptors_ransac")
        self.w, self.h_ = w, h
        nf = C.c_int(0)
        lib().poppy_hip_pair_begin_info(self.h, C.byref(nf), None)
        return nf.value

    def pair_fundamental(self):
        """What the filter of the last pair_begin_descriptors_ransac found: dict(f 3x3, n_matches, n_inliers, best)."""
        f = np.zeros((3, 3), np.float64)
        n_m, n_in, best = C.c_int(0), C.c_int(0), C.c_int(0)
        self._chk(lib().poppy_hip_pair_fundamental(self.h, _p(f), C.byref(n_m), C.byref(n_in), C.byref(best)), "pair_fundamental")
        return {"f": f, "n_matches": n_m.value, "n_inliers": n_in.value, "best": best.value}

    def ransac_fundamental(self, points1, points2, distance=3.0):
        """capi.ransac_fundamental with the 2048 hypotheses on this context's GPU: the same bytes."""
        return _ransac(lambda *args: lib().poppy_hip_ransac_fundamental(self.h, *args), "ransac_fundamental", points1, points2, distance, self._chk)

    def pair_begin_prefiltered(self, bgr1, bgr2, g1, g2, gabor2, nfeatures):
        a = np.ascontiguousarray(bgr1, np.uint8); b = np.ascontiguousarray(bgr2, np.uint8)
        g1 = np.ascontiguousarray(g1, np.uint8); g2 = np.ascontiguousarray(g2, np.uint8)
        g = np.ascontiguousarray(gabor2, np.float32)
        h, w = a.shape[:2]
        self._chk(lib().poppy_hip_pair_begin_prefiltered(self.h, _p(a), w * 3, _p(b), w * 3, _p(g1), _p(g2), _p(g), w, h, nfeatures), "pair_begin_prefiltered")
        self.w, self.h_ = w, h

    def pair_points(self, max_points=8192):
        p1 = np.zeros((max_points, 2), np.float32); p2 = np.zeros((max_points, 2), np.float32)
        n = C.c_int(0)
        self._chk(lib().poppy_hip_pair_points(self.h, _p(p1), _p(p2), max_points, C.byref(n)), "pair_points")
        return p1[:n.value].copy(), p2[:n.value].copy()

    def morph(self, bgr1, bgr2, phase=-1.0, distance=False, collect=True, row_pad=(0, 0)):
        """poppy::morph end to end: returns (status, frames, printed morph distance or None).  status is POPPY_OK (0) or
        POPPY_E_NOMATCH (-5, fallback frames written); anything else raises.  row_pad = (bytes, bytes): the two images are handed over with that many
        extra bytes per row (cv::Mat ROIs, src/poppy.cpp:234-239: step > cols * 3), the padding filled with a pattern no pixel may come from."""
        a, stride_a, w, h = _padded_rows(bgr1, row_pad[0])
        b, stride_b = _padded_rows(bgr2, row_pad[1])[:2]
        frames = []
        fmt = self.frame_format

        def cb(user, ptr, ww, hh, stride):
            frames.append(_frame_view(ptr, ww, hh, stride, fmt).copy())
        fn = WRITE_CB(cb) if collect else None
        d = C.c_double(float("nan"))
        rc = lib().poppy_hip_morph(self.h, _p(a), stride_a, _p(b), stride_b, w, h, phase, int(distance),
                                   C.cast(fn, C.c_void_p) if fn else None, None, C.byref(d))
        if rc not in (0, -5):
            self._chk(rc, "morph")
        self.w, self.h_ = w, h
        return rc, frames, (None if d.value != d.value else d.value)

    def pair_distance(self):
        d = C.c_double(0)
        self._chk(lib().poppy_hip_pair_distance(self.h, C.byref(d)), "pair_distance")
        return d.value

    def reset(self):
        self._chk(lib().poppy_hip_pair_reset(self.h), "pair_reset")

    def sync(self):
        self._chk(lib().poppy_hip_sync(self.h), "sync")

    def morph_frames(self, phase=-1.0, collect=True):
        frames = []
        fmt = self.frame_format

        def cb(user, ptr, w, h, stride):
            frames.append(_frame_view(ptr, w, h, stride, fmt).copy())
        fn = WRITE_CB(cb) if collect else None
        self._chk(lib().poppy_hip_morph_frames(self.h, phase, C.cast(fn, C.c_void_p) if fn else None, None), "morph_frames")
        return frames

    def dissolve(self, img1, img2, phase):
        a = np.ascontiguousarray(img1, np.uint8); b = np.ascontiguousarray(img2, np.uint8)
        h, w = a.shape[:2]
        out = np.empty((h, w, 3), np.uint8)
        self._chk(lib().poppy_hip_dissolve(self.h, _p(a), w * 3, _p(b), w * 3, w, h, phase, _p(out), w * 3), "dissolve")
        return out

    def warp_counts(self):
        f, a, b = C.c_ulonglong(0), C.c_ulonglong(0), C.c_ulonglong(0)
        lib().poppy_hip_warp_counts(self.h, C.byref(f), C.byref(a), C.byref(b))
        return f.value, a.value, b.value

    def mask_rider(self):
        """True when the warp kernel also writes lbmask (else the level-0 blend kernels compute it from m2)."""
        return lib().poppy_hip_mask_rider(self.h) == 1

    def warp_kernel_name(self):
        n = self.warp_counts()
        return WARP_KERNELS[n.index(max(n))]

    def last_warp_kind(self):
        return int(lib().poppy_hip_last_warp_kind(self.h))

    def last_pyramid_forms(self):
        """[(kind, level, arg)] of the last debug-mode frame's pyramid launches in launch order (include/poppy_hip.h: poppy_hip_last_pyramid_forms)."""
        n = lib().poppy_hip_last_pyramid_forms(self.h, None, 0)
        self._chk(min(n, 0), "last_pyramid_forms")
        out = np.zeros((max(n, 1), 3), np.int32)
        lib().poppy_hip_last_pyramid_forms(self.h, _p(out), n)
        return [(PYRAMID_FORMS[k - 1], int(lv), int(arg)) for k, lv, arg in out[:n]]

    def set_debug(self, on=True):
        lib().poppy_hip_set_debug(self.h, int(on))

    def set_timing(self, on=1):
        """0 off, 1 every kernel group (frames issued launch by launch), 2 the map+remap kernel only."""
        lib().poppy_hip_set_timing(self.h, int(on))

    def fetch(self, name):
        h, w = self.h_, self.w
        shapes = {"gabor2": ((h, w, 3), np.float32), "triMap": ((h, w), np.int32), "trImg1": ((h, w, 3), np.uint8), "trImg2": ((h, w, 3), np.uint8),
                  "lbmask": ((h, w), np.float32), "m2": ((h, w), np.float32), "lapBlend": ((h, w, 3), np.float32),
                  "unsharp": ((h, w, 3), np.float32)}
        shp, dt = shapes[name]
        out = np.empty(shp, dt)
        self._chk(lib().poppy_hip_debug_fetch(self.h, name.encode(), _p(out), out.nbytes), "debug_fetch " + name)
        return out

    def triangles(self, max_tris=8192):
        nt = C.c_int(0)
        idx3 = np.zeros((max_tris, 3), np.int32)
        M1 = np.zeros((max_tris, 3, 3), np.float32); M2 = np.zeros((max_tris, 3, 3), np.float32)
        self._chk(lib().poppy_hip_debug_triangles(self.h, C.byref(nt), _p(idx3), _p(M1), _p(M2), max_tris), "debug_triangles")
        t = nt.value
        return idx3[:t], M1[:t], M2[:t]

    def timing_summary(self):
        """[(kernel group, total ms, launches)] since timing was switched on / last summary (drains the stream)."""
        names = (C.c_char_p * 32)()
        ms = (C.c_float * 32)()
        cnt = (C.c_int * 32)()
        n = lib().poppy_hip_timing_summary(self.h, names, ms, cnt, 32)
        return [(names[i].decode(), ms[i], cnt[i]) for i in range(n)]

    def render_many(self, shapes, masks=None, chain=False, write=None):
        """write: optional callable(frame_view) invoked for every frame with a view of the pinned host copy (valid during the call)."""
        sh = np.ascontiguousarray(shapes, np.float64)
        mk = sh if masks is None else np.ascontiguousarray(masks, np.float64)
        fn = None
        if write is not None:
            fmt = self.frame_format

            def cb(user, ptr, w, h, stride):
                write(_frame_view(ptr, w, h, stride, fmt))
            fn = WRITE_CB(cb)
        self._chk(lib().poppy_hip_render_many(self.h, _p(sh), _p(mk), len(sh), int(chain), C.cast(fn, C.c_void_p) if fn else None, None), "render_many")

    def frame_device_ptr(self):
        return lib().poppy_hip_frame_device(self.h)

    def stream_ptr(self):
        return lib().poppy_hip_stream(self.h)

    def frame_stream_ptr(self):
        return lib().poppy_hip_frame_stream(self.h)

    def frame_wait(self, stream_ptr=None):
        """Orders `stream_ptr` (a hipStream_t; None: the host) behind the last frame rendered (phase-mode frames run on streams of their own)."""
        self._chk(lib().poppy_hip_frame_wait(self.h, stream_ptr), "frame_wait")

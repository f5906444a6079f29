"""ctypes loader for libdvsraster.so — mirrors include/dvs_raster.h and include/dvs_scene.h 1:1."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DVS_RASTER_LIB") or os.path.join(_HERE, "lib", "libdvsraster.so")     # override: another build of the library (tools/lib_ab.sh A/Bs two builds)


class DvsError(RuntimeError):
    pass


if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"{LIB_PATH} is missing: build it with `make -C divshot_amd/csrc` (or __graft_entry__.build()). "
        "divshot_amd has no CPU fallback.")

lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)


class Splats(C.Structure):
    _fields_ = [("pos", C.c_void_p), ("sh0", C.c_void_p), ("shN", C.c_void_p), ("opacity", C.c_void_p),
                ("scale", C.c_void_p), ("rot", C.c_void_p), ("n", C.c_int32), ("_pad", C.c_int32)]


class Camera(C.Structure):
    _fields_ = [("view", C.c_float * 16), ("proj", C.c_float * 16), ("tan_fovx", C.c_float), ("tan_fovy", C.c_float),
                ("focal_x", C.c_float), ("focal_y", C.c_float), ("campos", C.c_float * 3), ("width", C.c_int32),
                ("height", C.c_int32), ("bg", C.c_float * 3)]


class Opts(C.Structure):
    _fields_ = [("sh_degree", C.c_int32), ("antialias", C.c_int32), ("absgrad", C.c_int32), ("accumulate", C.c_int32),
                ("shn_layout", C.c_int32), ("grad_mode", C.c_int32), ("tile_bounds", C.c_int32), ("_reserved", C.c_int32 * 1)]


class FwdState(C.Structure):
    _fields_ = [("radii", C.c_void_p), ("splat2d", C.c_void_p), ("depth", C.c_void_p), ("flags", C.c_void_p), ("tiles_touched", C.c_void_p), ("sorted_tile", C.c_void_p),
                ("sorted_splat", C.c_void_p), ("ranges", C.c_void_p), ("final_T", C.c_void_p), ("n_contrib", C.c_void_p),
                ("num_rendered", C.c_uint64), ("n", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
                ("tiles_x", C.c_int32), ("tiles_y", C.c_int32), ("_pad", C.c_int32)]


class SplatGrads(C.Structure):
    _fields_ = [("pos", C.c_void_p), ("sh0", C.c_void_p), ("shN", C.c_void_p), ("opacity", C.c_void_p),
                ("scale", C.c_void_p), ("rot", C.c_void_p), ("absgrad2d", C.c_void_p), ("mean2d", C.c_void_p), ("dcolor", C.c_void_p)]


class Sky(C.Structure):
    _fields_ = [("tex", C.c_void_p), ("width", C.c_int32), ("height", C.c_int32)]


class DensifyParams(C.Structure):
    _fields_ = [("grad_threshold", C.c_float), ("scale_threshold", C.c_float), ("min_opacity", C.c_float), ("max_world_scale", C.c_float),
                ("max_screen_radius", C.c_int32), ("cap_max", C.c_int32), ("seed", C.c_uint32), ("shn_layout", C.c_int32), ("revised_opacity", C.c_int32)]


class AdamGroup(C.Structure):
    _fields_ = [("param", C.c_void_p), ("grad", C.c_void_p), ("m", C.c_void_p), ("v", C.c_void_p), ("count", C.c_uint64),
                ("lr", C.c_float), ("width", C.c_int32), ("layout", C.c_int32), ("active_chunks", C.c_int32)]


class MetricsView(C.Structure):
    _fields_ = [("img", C.c_void_p), ("target", C.c_void_p), ("mask", C.c_void_p)]


class DownsampleView(C.Structure):
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p)]


class McmcSets(C.Structure):
    _fields_ = [("param", C.c_void_p * 6), ("m", C.c_void_p * 6), ("v", C.c_void_p * 6)]


class SceneSpec(C.Structure):
    _fields_ = [("n", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("sh_degree", C.c_int32),
                ("n_cams", C.c_int32), ("seed", C.c_uint64), ("fov_x_deg", C.c_float), ("scale_log_offset", C.c_float)]


# every symbol include/*.h declares (tests/test_abi.py checks this list against the headers)
_PROTOS = {
    "dvs_create": (C.c_void_p, [C.c_int, C.c_size_t, C.c_int, C.c_int]),
    "dvs_create_views": (C.c_void_p, [C.c_int, C.c_size_t, C.c_int, C.c_int, C.c_int]),
    "dvs_destroy": (None, [C.c_void_p]),
    "dvs_raster_forward_views": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(Splats), C.POINTER(Camera), C.c_int, C.POINTER(Opts), C.c_void_p]),
    "dvs_raster_depth_views": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(Opts), C.c_void_p, C.c_void_p]),
    "dvs_raster_importance_views": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(Opts), C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p, C.c_void_p]),
    "dvs_raster_foreground_views": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(Opts), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p]),
    "dvs_sky_forward_views": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(Camera), C.c_int, C.POINTER(Sky), C.c_void_p, C.c_void_p]),
    "dvs_sky_backward_views": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(Camera), C.c_int, C.POINTER(Opts), C.POINTER(Sky), C.c_void_p, C.c_void_p,
                                         C.c_void_p]),
    "dvs_raster_forward_cancel_prepared": (C.c_int, [C.c_void_p]),
    "dvs_raster_forward_views_prepare": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(Splats), C.POINTER(Camera), C.c_int, C.POINTER(Opts), C.c_int64, C.c_int64]),
    "dvs_raster_backward_views": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(Splats), C.POINTER(Camera), C.c_int, C.POINTER(Opts),
                                            C.c_void_p, C.POINTER(SplatGrads)]),
    "dvs_get_view_state": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(FwdState)]),
    "dvs_raster_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(Splats), C.POINTER(Camera), C.POINTER(Opts),
                                     C.c_void_p, C.POINTER(FwdState), C.POINTER(C.c_uint64)]),
    "dvs_raster_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(Splats), C.POINTER(Camera), C.POINTER(Opts),
                                      C.c_void_p, C.POINTER(SplatGrads)]),
    "dvs_raster_backward_composite": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Opts), C.c_void_p]),
    "dvs_raster_backward_project": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(Splats), C.c_void_p, C.POINTER(Opts),
                                              C.POINTER(SplatGrads)]),
    "dvs_raster_backward_project_chunk": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(Splats), C.c_void_p, C.POINTER(Opts),
                                                    C.POINTER(SplatGrads), C.c_int64, C.c_int64]),
    "dvs_raster_backward_dcolor": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "dvs_sh_grad_combine": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_int, C.c_int]),
    "dvs_shn_relayout": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]),
    "dvs_sort_pairs_u32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_int]),
    "dvs_export_sorted_keys": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "dvs_get_bwd_intermediates": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int)]),
    "dvs_keep_bwd_intermediates": (C.c_int, [C.c_void_p, C.c_int]),
    "dvs_set_async": (C.c_int, [C.c_void_p, C.c_int]),
    "dvs_get_num_rendered": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]),
    "dvs_get_sort_rank_mode": (C.c_int, [C.c_void_p]),
    "dvs_debug_sort_depth_keys": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "dvs_set_export_sorted_tiles": (C.c_int, [C.c_void_p, C.c_int]),
    "dvs_get_arena_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "dvs_set_backward_variant": (C.c_int, [C.c_void_p, C.c_int]),
    "dvs_debug_record_decisions": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64]),
    "dvs_set_forward_variant": (C.c_int, [C.c_void_p, C.c_int]),
    "dvs_set_live_lists": (C.c_int, [C.c_void_p, C.c_int]),
    "dvs_enable_stage_timing": (C.c_int, [C.c_void_p, C.c_int]),
    "dvs_enable_kernel_probe": (C.c_int, [C.c_void_p, C.c_int]),
    "dvs_read_kernel_probe": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int)]),
    "dvs_get_stage_timing": (C.c_int, [C.c_void_p, C.POINTER(C.POINTER(C.c_char_p)), C.POINTER(C.POINTER(C.c_float))]),
    "dvs_memcpy_d2h": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    "dvs_memcpy_h2d": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    "dvs_device_malloc": (C.c_void_p, [C.c_void_p, C.c_size_t]),
    "dvs_device_free": (None, [C.c_void_p, C.c_void_p]),
    "dvs_comm_create": (C.c_void_p, [C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_int]),
    "dvs_comm_bootstrap": (C.c_int, [C.c_int, C.c_int, C.c_char_p, C.c_int, C.c_void_p]),
    "dvs_comm_destroy": (None, [C.c_void_p]),
    "dvs_comm_rank": (C.c_int, [C.c_void_p]),
    "dvs_comm_world": (C.c_int, [C.c_void_p]),
    "dvs_comm_backend_ranks": (C.c_int, [C.c_void_p]),
    "dvs_comm_backend_name": (C.c_char_p, [C.c_void_p]),
    "dvs_comm_all_reduce_sum_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    "dvs_comm_all_reduce_max_i32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    "dvs_comm_reduce_scatter_sum_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    "dvs_comm_all_gather_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    "dvs_comm_broadcast": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]),
    "dvs_comm_group_start": (C.c_int, [C.c_void_p]),
    "dvs_comm_group_end": (C.c_int, [C.c_void_p]),
    "dvs_last_error": (C.c_char_p, []),
    "dvs_version": (C.c_char_p, []),
    "dvs_synth_splats": (C.c_int, [C.POINTER(SceneSpec)] + [C.c_void_p] * 6),
    "dvs_synth_camera": (C.c_int, [C.POINTER(SceneSpec), C.c_int, C.POINTER(Camera)]),
    "dvs_synth_target": (C.c_int, [C.POINTER(SceneSpec), C.c_int, C.c_void_p]),
    "dvs_make_camera": (C.c_int, [C.c_void_p, C.c_void_p, C.c_float, C.c_int, C.c_int, C.POINTER(Camera)]),
    "dvs_make_camera_intrinsics": (C.c_int, [C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int, C.c_int, C.POINTER(Camera)]),
    "dvs_camera_downscale": (C.c_int, [C.POINTER(Camera), C.c_int, C.POINTER(Camera)]),
    "dvs_l1_loss_grad": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "dvs_l1_loss_grad_w": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_float, C.c_void_p, C.c_void_p]),
    "dvs_l2_loss_grad": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_float, C.c_void_p, C.c_void_p]),
    "dvs_ssim_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "dvs_ssim_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float,
                                    C.c_void_p, C.c_int]),
    "dvs_loss_l1_ssim_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float,
                                            C.c_void_p, C.c_void_p]),
    "dvs_image_metrics_scratch_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "dvs_image_metrics_views": (C.c_int, [C.c_void_p, C.POINTER(MetricsView), C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "dvs_downsample_views": (C.c_int, [C.c_void_p, C.POINTER(DownsampleView), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "dvs_densify_accumulate": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "dvs_densify_accumulate_rows": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "dvs_any_view_radius": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "dvs_densify_plan": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(DensifyParams),
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "dvs_densify_apply": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(DensifyParams), C.c_int, C.c_void_p, C.c_void_p, C.c_int]),
    "dvs_importance_scratch_bytes": (C.c_size_t, [C.c_int]),
    "dvs_importance_plan": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "dvs_foreground_plan": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "dvs_reset_opacity": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p]),
    "dvs_adam_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_float, C.c_float,
                                C.c_float, C.c_float, C.c_int]),
    "dvs_mcmc_scratch_bytes": (C.c_size_t, [C.c_int]),
    "dvs_mcmc_init_scratch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "dvs_mcmc_relocate": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(McmcSets), C.c_float, C.c_uint32, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "dvs_mcmc_grow": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(McmcSets), C.c_float, C.c_uint32, C.c_int, C.c_void_p, C.c_int]),
    "dvs_mcmc_add_noise": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_uint32]),
    "dvs_mcmc_regularize": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float]),
    "dvs_mcmc_add_noise_range": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_uint32]),
    "dvs_mcmc_regularize_range": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float]),
    "dvs_filter3d_pack_cameras": (C.c_int, [C.POINTER(Camera), C.c_int, C.c_void_p]),
    "dvs_filter3d_compute": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "dvs_filter3d_apply_range": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "dvs_filter3d_apply": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "dvs_filter3d_chain_range": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "dvs_filter3d_chain": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "dvs_adam_step_groups": (C.c_int, [C.c_void_p, C.POINTER(AdamGroup), C.c_int, C.c_float, C.c_float, C.c_float, C.c_int, C.c_void_p,
                                       C.c_int32]),
}
# include/dvs_export.h: the model export packers (a table of their own: _PROTOS is the list of the four headers above)
class SpzLayout(C.Structure):          # dvs_spz_layout: positions, alphas, colors, scales, rotations, sh
    _fields_ = [("off", C.c_uint64 * 6), ("bytes", C.c_uint64 * 6), ("total", C.c_uint64)]


class ReducedLayout(C.Structure):      # dvs_reduced_layout: the four per-degree vertex blocks, then the codebook table
    _fields_ = [("count", C.c_uint64 * 4), ("off", C.c_uint64 * 4), ("stride", C.c_uint64 * 4), ("table_off", C.c_uint64), ("total", C.c_uint64),
                ("half", C.c_int32), ("_pad", C.c_int32)]


class Similarity(C.Structure):         # dvs_similarity: p' = s R p + t, R row-major
    _fields_ = [("R", C.c_float * 9), ("t", C.c_float * 3), ("s", C.c_float)]


class LodLattice(C.Structure):         # dvs_lod_lattice: the cells the LOD merge clusters by
    _fields_ = [("origin", C.c_float * 3), ("cell", C.c_float), ("dims", C.c_int32 * 3)]


_EXPORT_PROTOS = {
    "dvs_lod_lattice_for": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(LodLattice)]),
    "dvs_lod_scratch_bytes": (C.c_size_t, [C.c_int]),
    "dvs_lod_merge_count": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(LodLattice), C.c_void_p,
                                      C.POINTER(C.c_uint32)]),
    "dvs_lod_merge_write": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "dvs_similarity_from_trs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_float, C.POINTER(Similarity)]),
    "dvs_similarity_inverse": (C.c_int, [C.POINTER(Similarity), C.POINTER(Similarity)]),
    "dvs_sh_rotation": (C.c_int, [C.c_void_p, C.c_void_p]),
    "dvs_transform_splats": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(Similarity), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "dvs_transform_points": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(Similarity), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "dvs_reduced_scratch_bytes": (C.c_size_t, [C.c_int]),
    "dvs_sh_degree_select": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_float, C.c_void_p]),
    "dvs_codebooks_build": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                      C.c_void_p, C.c_void_p, C.c_void_p]),
    "dvs_reduced_degree_counts": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "dvs_reduced_layout_for": (C.c_int, [C.POINTER(C.c_uint32), C.c_int, C.POINTER(ReducedLayout)]),
    "dvs_pack_reduced": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.POINTER(ReducedLayout), C.c_void_p]),
    "dvs_unpack_reduced": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(ReducedLayout), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "dvs_pack_scratch_bytes": (C.c_size_t, [C.c_int]),
    "dvs_pack_compressed": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p]),
    "dvs_pack_splat32": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "dvs_spz_layout_for": (C.c_int, [C.c_int, C.c_int, C.POINTER(SpzLayout)]),
    "dvs_pack_spz": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                               C.c_void_p]),
    "dvs_unpack_spz": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                 C.c_void_p]),
}
# include/dvs_init.h: splat initialisation from a sparse point cloud
_INIT_PROTOS = {
    "dvs_knn_scratch_bytes": (C.c_size_t, [C.c_int]),
    "dvs_knn_mean_dist2": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "dvs_knn_mean_dist2_stats": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "dvs_init_from_points": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
}
# include/dvs_image.h: JPEG reconstruction from quantised DCT coefficients; undistortion of a distorted COLMAP camera's view
class JpegDesc(C.Structure):           # dvs_jpeg_desc
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("components", C.c_int32), ("hs", C.c_int32), ("vs", C.c_int32),
                ("blocks_w", C.c_int32 * 3), ("blocks_h", C.c_int32 * 3), ("_pad", C.c_int32), ("offset", C.c_uint64 * 3),
                ("quant", (C.c_uint16 * 64) * 3)]


class UndistortDesc(C.Structure):      # dvs_undistort_desc
    _fields_ = [("width", C.c_int32), ("height", C.c_int32)] + [(n, C.c_float) for n in ("fx", "fy", "cx", "cy", "ifx", "ify", "k1", "k2", "p1", "p2")]


class PngDesc(C.Structure):            # dvs_png_desc
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("bit_depth", C.c_int32), ("color_type", C.c_int32), ("has_key", C.c_int32),
                ("key", C.c_uint16 * 3), ("palette", (C.c_uint8 * 4) * 256)]


_IMAGE_PROTOS = {
    "dvs_png_band_rows": (C.c_int, []),
    "dvs_png_filtered_bytes": (C.c_size_t, [C.POINTER(PngDesc)]),
    "dvs_png_reconstruct": (C.c_int, [C.c_void_p, C.POINTER(PngDesc), C.c_void_p, C.c_void_p, C.c_void_p]),
    "dvs_mask_combine": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "dvs_png_encode_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "dvs_png_encode_views": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_void_p, C.c_int]),
    "dvs_jpeg_reconstruct": (C.c_int, [C.c_void_p, C.POINTER(JpegDesc), C.c_void_p, C.c_void_p]),
    "dvs_jpeg_encode_desc": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(JpegDesc)]),
    "dvs_jpeg_encode_coef_count": (C.c_size_t, [C.POINTER(JpegDesc)]),
    "dvs_jpeg_encode_views": (C.c_int, [C.c_void_p, C.POINTER(JpegDesc), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int]),
    "dvs_undistort_desc_from_colmap": (C.c_int, [C.c_int, C.POINTER(C.c_double), C.c_int, C.c_int, C.POINTER(UndistortDesc)]),
    "dvs_undistort_view": (C.c_int, [C.c_void_p, C.POINTER(UndistortDesc), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
}


# include/dvs_mesh.h: TSDF fusion of depth maps and marching tetrahedra
class TsdfGridDesc(C.Structure):       # dvs_tsdf_grid
    _fields_ = [("origin", C.c_float * 3), ("voxel", C.c_float), ("dims", C.c_int32 * 3), ("_pad", C.c_int32), ("tsdf", C.c_void_p),
                ("weight", C.c_void_p), ("rgb", C.c_void_p)]


class MeshCleanInfo(C.Structure):      # dvs_mesh_clean_info
    _fields_ = [(n, C.c_uint32) for n in ("n_components", "largest", "kept_components", "kept_vertices", "kept_triangles", "n_bad")]


class MeshDecimateInfo(C.Structure):   # dvs_mesh_decimate_info
    _fields_ = [(n, C.c_uint32) for n in ("out_vertices", "out_triangles", "n_clusters", "n_degenerate", "n_duplicate", "n_bad")]


_MESH_PROTOS = {
    "dvs_tsdf_bytes": (C.c_size_t, [C.POINTER(C.c_int32)]),
    "dvs_tsdf_create": (C.c_int, [C.POINTER(C.c_float), C.c_float, C.POINTER(C.c_int32), C.POINTER(TsdfGridDesc)]),
    "dvs_tsdf_destroy": (None, [C.POINTER(TsdfGridDesc)]),
    "dvs_tsdf_clear": (C.c_int, [C.c_void_p, C.POINTER(TsdfGridDesc)]),
    "dvs_tsdf_integrate": (C.c_int, [C.c_void_p, C.POINTER(TsdfGridDesc), C.POINTER(Camera), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_float]),
    "dvs_mesh_scratch_bytes": (C.c_size_t, [C.POINTER(C.c_int32)]),
    "dvs_mesh_extract_count": (C.c_int, [C.c_void_p, C.POINTER(TsdfGridDesc), C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "dvs_mesh_extract_write": (C.c_int, [C.c_void_p, C.POINTER(TsdfGridDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "dvs_mesh_extract_normals": (C.c_int, [C.c_void_p, C.POINTER(TsdfGridDesc), C.c_void_p, C.c_void_p]),
    "dvs_mesh_components": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
    "dvs_mesh_clean_scratch_bytes": (C.c_size_t, [C.c_uint32, C.c_uint32]),
    "dvs_mesh_clean_count": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(MeshCleanInfo)]),
    "dvs_mesh_clean_write": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "dvs_mesh_decimate_scratch_bytes": (C.c_size_t, [C.c_uint32, C.c_uint32]),
    "dvs_mesh_decimate_count": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_float), C.c_float,
                                          C.POINTER(C.c_int32), C.c_void_p, C.POINTER(MeshDecimateInfo)]),
    "dvs_mesh_decimate_write": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
}


# include/dvs_region.h: the focus region (an oriented box): which splats it keeps, which pixels' rays cross it
class Region(C.Structure):             # dvs_region
    _fields_ = [("w2b", C.c_float * 12), ("lo", C.c_float * 3), ("hi", C.c_float * 3)]


class RegionMaskView(C.Structure):     # dvs_region_mask_view
    _fields_ = [("cam", Camera), ("in_mask", C.c_void_p), ("out", C.c_void_p)]


_REGION_PROTOS = {
    "dvs_region_from_trs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Region), C.c_void_p]),
    "dvs_region_plan": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(Region), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "dvs_region_mask_views": (C.c_int, [C.c_void_p, C.POINTER(RegionMaskView), C.c_int, C.c_int, C.c_int, C.POINTER(Region)]),
}


def undistort_desc(model, params, width, height):
    """-> UndistortDesc of COLMAP model id 2, 3 or 4 and its parameter list (dvs_undistort_desc_from_colmap); DvsError when refused"""
    prm = (C.c_double * len(params))(*[float(v) for v in params])
    if len(params) != {2: 4, 3: 5, 4: 8}.get(int(model), -1):
        raise DvsError(f"camera model {model} with {len(params)} parameters has no undistortion descriptor")
    d = UndistortDesc()
    if lib.dvs_undistort_desc_from_colmap(int(model), prm, int(width), int(height), C.byref(d)) != 0:
        raise DvsError(f"dvs_undistort_desc_from_colmap refused model {model}, {width}x{height}, {list(params)}")
    return d
for _name, (_res, _args) in list(_PROTOS.items()) + list(_EXPORT_PROTOS.items()) + list(_INIT_PROTOS.items()) + list(_IMAGE_PROTOS.items()) + list(_MESH_PROTOS.items()) + list(_REGION_PROTOS.items()):
    _f = getattr(lib, _name)          # AttributeError here = the .so does not export a declared symbol
    _f.restype = _res
    _f.argtypes = _args


def check(status, what="dvs call"):
    if status != 0:
        raise DvsError(f"{what} failed with status {status}: {lib.dvs_last_error().decode()}")


# libgsplyio.so, the host-only library of the plugin's file readers and writers (no HIP runtime behind it): the JPEG coefficient decoder
_JPEG_HOST_PROTOS = {
    "gstrain_jpeg_open": (C.c_void_p, [C.c_char_p, C.c_char_p, C.c_int]),
    "gstrain_jpeg_info": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gstrain_jpeg_coefficients": (C.c_int, [C.c_void_p, C.c_void_p]),
    "gstrain_jpeg_close": (None, [C.c_void_p]),
    "gstrain_jpeg_open_memory": (C.c_void_p, [C.c_void_p, C.c_uint64, C.c_char_p, C.c_int]),
    "gstrain_jpeg_encode": (C.c_void_p, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_int]),
    "gstrain_jpeg_encoded_size": (C.c_uint64, [C.c_void_p]),
    "gstrain_jpeg_encoded_bytes": (C.c_int, [C.c_void_p, C.c_void_p]),
    "gstrain_jpeg_encoded_free": (None, [C.c_void_p]),
}
# ... the PNG host half (png_io.hpp: chunk parsing and inflate, file -> filtered scanlines)
_PNG_HOST_PROTOS = {
    "gstrain_png_open": (C.c_void_p, [C.c_char_p, C.c_char_p, C.c_int]),
    "gstrain_png_open_memory": (C.c_void_p, [C.c_void_p, C.c_uint64, C.c_char_p, C.c_int]),
    "gstrain_png_info": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gstrain_png_filtered": (C.c_int, [C.c_void_p, C.c_void_p]),
    "gstrain_png_close": (None, [C.c_void_p]),
    "gstrain_png_write": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), C.c_int, C.c_void_p, C.c_uint64,
                                    C.POINTER(C.c_uint64), C.c_char_p, C.c_int]),
}
# ... and the mesh file writer (ply_io.hpp write_mesh_ply)
_MESH_HOST_PROTOS = {
    "gstrain_write_mesh_ply": (C.c_int, [C.c_char_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_char_p, C.c_uint64]),
    "gstrain_write_mesh_ply_normals": (C.c_int, [C.c_char_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_char_p, C.c_uint64]),
}
# ... and the export frame's orientation from the training cameras (export_frame.hpp)
_FRAME_HOST_PROTOS = {
    "gstrain_host_read_ply": (C.c_int64, [C.c_char_p] + [C.c_void_p] * 6 + [C.c_uint64]),
    "gstrain_export_orientation": (C.c_int, [C.c_uint64, C.c_void_p, C.c_void_p, C.c_char_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_uint64]),
}
# ... and the extension options' table (ext_options.hpp): one row's grammar and messages
_OPTION_HOST_PROTOS = {
    "gstrain_ext_option_check": (C.c_int, [C.c_char_p, C.c_char_p, C.POINTER(C.c_double), C.c_char_p, C.c_int]),
}
_host_lib = None


def host_lib():
    """libgsplyio.so with the gstrain_jpeg_* prototypes bound; loaded on first use (divshot_amd/gstrain builds it)"""
    global _host_lib
    if _host_lib is None:
        path = os.path.join(_HERE, "lib", "libgsplyio.so")
        if not os.path.exists(path):
            raise ImportError(f"{path} is missing: build it with `make -C divshot_amd/gstrain`")
        h = C.CDLL(path)
        for name, (res, args) in list(_JPEG_HOST_PROTOS.items()) + list(_PNG_HOST_PROTOS.items()) + list(_MESH_HOST_PROTOS.items()) + list(_FRAME_HOST_PROTOS.items()) + list(_OPTION_HOST_PROTOS.items()):
            f = getattr(h, name)
            f.restype = res
            f.argtypes = args
        _host_lib = h
    return _host_lib


def ext_option_check(name_or_var, text):
    """gstrain_ext_option_check: `text` against the extension option's table row, found by its flag name (no dashes; the text is then the
    flag's spelling) or by its variable name -> (True, [8 floats], "") when it is of the row's grammar, (False, None, message) when it is
    not — the CLI's message for a flag, the plugin's log line for a variable; DvsError when there is no such row"""
    out = (C.c_double * 8)()
    err = C.create_string_buffer(1024)
    status = host_lib().gstrain_ext_option_check(name_or_var.encode(), text.encode(), out, err, 1024)
    if status < 0:
        raise DvsError(f"no extension option is called {name_or_var!r}")
    return (True, list(out), "") if status == 0 else (False, None, err.value.decode())


def write_mesh_ply(path, xyz, rgb, tri, normals=None):
    """gsply::write_mesh_ply through libgsplyio.so: xyz float32 [nv,3], rgb uint8 [nv,3], tri uint32 [nt,3], normals None or float32 [nv,3]
    (then the vertex carries nx ny nz between z and red); DvsError with the writer's message when it refuses (an index >= nv, a file it
    cannot write)"""
    import numpy as np
    h = host_lib()
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    rgb = np.ascontiguousarray(rgb, np.uint8).reshape(-1, 3)
    tri = np.ascontiguousarray(tri, np.uint32).reshape(-1, 3)
    if rgb.shape[0] != xyz.shape[0]:
        raise DvsError("write_mesh_ply: xyz and rgb differ in length")
    err = C.create_string_buffer(1024)
    if normals is None:
        rc = h.gstrain_write_mesh_ply(os.fsencode(path), xyz.shape[0], xyz.ctypes.data, rgb.ctypes.data, tri.shape[0], tri.ctypes.data, err, 1024)
    else:
        normals = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
        if normals.shape[0] != xyz.shape[0]:
            raise DvsError("write_mesh_ply: xyz and normals differ in length")
        rc = h.gstrain_write_mesh_ply_normals(os.fsencode(path), xyz.shape[0], xyz.ctypes.data, normals.ctypes.data, rgb.ctypes.data, tri.shape[0],
                                              tri.ctypes.data, err, 1024)
    if rc != 0:
        raise DvsError(err.value.decode(errors="replace"))


def read_ply(path):
    """gsply::read_ply through libgsplyio.so -> dict of float32 arrays pos [n,3], sh0 [n,3], shN [n,45], opacity [n], scale [n,3], rot [n,4]"""
    import numpy as np
    h = host_lib()
    n = h.gstrain_host_read_ply(os.fsencode(path), None, None, None, None, None, None, 0)
    if n < 0:
        raise DvsError(f"read_ply: {path} is not a splat PLY this build reads")
    out = {k: np.zeros((n, w), np.float32) for k, w in (("pos", 3), ("sh0", 3), ("shN", 45), ("opacity", 1), ("scale", 3), ("rot", 4))}
    h.gstrain_host_read_ply(os.fsencode(path), *[out[k].ctypes.data for k in ("pos", "sh0", "shN", "opacity", "scale", "rot")], n)
    out["opacity"] = out["opacity"].reshape(-1)
    return out


def jpeg_encode_desc(width, height, sampling, quality):
    """-> JpegDesc of dvs_jpeg_encode_desc (host only); sampling 0 = 4:2:0, 1 = 4:4:4; DvsError when refused"""
    d = JpegDesc()
    if lib.dvs_jpeg_encode_desc(int(width), int(height), int(sampling), int(quality), C.byref(d)) != 0:
        raise DvsError(f"dvs_jpeg_encode_desc refused {width}x{height}, sampling {sampling}, quality {quality}")
    return d


def jpeg_encode_coefficients(desc, coef):
    """-> bytes: gsjpeg::encode_coefficients of a frame given as (JpegDesc, int16 numpy array), the pair jpeg_decode_coefficients
    returns; DvsError with the encoder's message for a frame it refuses"""
    import numpy as np
    h = host_lib()
    coef = np.ascontiguousarray(coef, np.int16)
    ints, offs = (C.c_int32 * 15)(), (C.c_uint64 * 4)()
    ints[0], ints[1], ints[2] = desc.width, desc.height, desc.components
    for k in range(3):
        ints[3 + k], ints[6 + k] = (desc.hs, desc.vs) if k == 0 else (1, 1)
        ints[9 + k], ints[12 + k], offs[k] = desc.blocks_w[k], desc.blocks_h[k], desc.offset[k]
    offs[3] = coef.size
    err = C.create_string_buffer(1024)
    e = h.gstrain_jpeg_encode(ints, C.addressof(desc.quant), offs, coef.ctypes.data, err, 1024)
    if not e:
        raise DvsError(err.value.decode(errors="replace"))
    try:
        out = np.zeros(h.gstrain_jpeg_encoded_size(e), np.uint8)
        check(h.gstrain_jpeg_encoded_bytes(e, out.ctypes.data), "gstrain_jpeg_encoded_bytes")
        return out.tobytes()
    finally:
        h.gstrain_jpeg_encoded_free(e)


def png_decode_filtered(path):
    """-> (PngDesc, uint8 numpy array): gspng::decode_filtered of a file (or of `bytes` in memory): the descriptor and the filtered
    scanlines dvs_png_reconstruct takes; DvsError with the decoder's message when the file is refused"""
    import numpy as np
    h = host_lib()
    err = C.create_string_buffer(1024)
    if isinstance(path, (bytes, bytearray)):
        f = h.gstrain_png_open_memory(bytes(path), len(path), err, 1024)
    else:
        f = h.gstrain_png_open(os.fsencode(path), err, 1024)
    if not f:
        raise DvsError(err.value.decode(errors="replace"))
    try:
        desc = PngDesc()
        ints = (C.c_int32 * 5)()
        size = C.c_uint64()
        check(h.gstrain_png_info(f, ints, C.addressof(desc.key), C.addressof(desc.palette), C.byref(size)), "gstrain_png_info")
        desc.width, desc.height, desc.bit_depth, desc.color_type, desc.has_key = list(ints)
        filtered = np.zeros(size.value, np.uint8)
        check(h.gstrain_png_filtered(f, filtered.ctypes.data), "gstrain_png_filtered")
        return desc, filtered
    finally:
        h.gstrain_png_close(f)


def png_write(width, height, bit_depth, color_type, filtered, level=6, text=None):
    """-> bytes: gspng::write_png of a filtered stream (uint8 array or bytes; what dvs_png_encode_views writes) at zlib `level`, with one
    tEXt chunk per (keyword, text) pair of `text` (str as Latin-1, or bytes); DvsError with the writer's message when it refuses"""
    import numpy as np
    h = host_lib()
    stream = np.ascontiguousarray(np.frombuffer(bytes(filtered), np.uint8) if isinstance(filtered, (bytes, bytearray)) else filtered, np.uint8)
    pairs = [tuple(s if isinstance(s, bytes) else s.encode("latin-1") for s in kv) for kv in (text or [])]
    keys, texts = (C.c_char_p * max(1, len(pairs)))(*[k for k, _ in pairs]), (C.c_char_p * max(1, len(pairs)))(*[t for _, t in pairs])
    ints = (C.c_int32 * 5)(int(width), int(height), int(bit_depth), int(color_type), int(level))
    err, size = C.create_string_buffer(1024), C.c_uint64()
    cap = stream.size + stream.size // 1000 + 4096 + sum(len(k) + len(t) + 16 for k, t in pairs)      # above deflate's worst case and the chunk frames
    out = np.zeros(cap, np.uint8)
    if h.gstrain_png_write(ints, stream.ctypes.data, stream.size, keys, texts, len(pairs), out.ctypes.data, cap, C.byref(size), err, 1024) != 0:
        raise DvsError(err.value.decode(errors="replace"))
    return out[:size.value].tobytes()


def jpeg_decode_coefficients(path):
    """-> (JpegDesc, int16 numpy array): gsjpeg::decode_coefficients of a file (or of `bytes` in memory), as dvs_jpeg_reconstruct takes
    them; DvsError with the decoder's message for a file it rejects"""
    import numpy as np
    h = host_lib()
    err = C.create_string_buffer(1024)
    if isinstance(path, (bytes, bytearray)):
        f = h.gstrain_jpeg_open_memory(bytes(path), len(path), err, 1024)
    else:
        f = h.gstrain_jpeg_open(os.fsencode(path), err, 1024)
    if not f:
        raise DvsError(err.value.decode(errors="replace"))
    try:
        ints, offs, desc = (C.c_int32 * 15)(), (C.c_uint64 * 4)(), JpegDesc()
        check(h.gstrain_jpeg_info(f, ints, C.addressof(desc.quant), offs), "gstrain_jpeg_info")
        desc.width, desc.height, desc.components, desc.hs, desc.vs = ints[0], ints[1], ints[2], ints[3], ints[6]
        for k in range(3):
            desc.blocks_w[k], desc.blocks_h[k], desc.offset[k] = ints[9 + k], ints[12 + k], offs[k]
        coef = np.zeros(offs[3], np.int16)
        check(h.gstrain_jpeg_coefficients(f, coef.ctypes.data), "gstrain_jpeg_coefficients")
        return desc, coef
    finally:
        h.gstrain_jpeg_close(f)

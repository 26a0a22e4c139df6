"""The C ABI of libpar_raytracer.so as ctypes signatures: one table a header of include/, the hooks the library exports
beside them, and the one loop that sets them on a loaded library. A table is in its header's order: symbol -> argument
types, or (return type, argument types) where the function does not return an int. Every pointer is a c_void_p.
The package's lib() calls install() once, at load, and so does an add-on module's with its own table;
tests/test_abi_cpu.py holds every table to its header's prototypes and the tables together to what the library exports."""
import ctypes as C

_p, _i, _u = C.c_void_p, C.c_int, C.c_uint

# include/par_raytracer.h
ABI = {
    "par_status_string": (C.c_char_p, [_i]),
    "par_last_error": (C.c_char_p, [_p]),
    "par_default_params": (None, [_p]),
    "par_grid_dims": [_p, _p, _p, _p],
    "par_device_count": [],
    "par_create": [_p, _i, _p],
    "par_destroy": (None, [_p]),
    "par_set_sprites": [_p, _p, _i],
    "par_set_entities": [_p, _p, _p, _i],
    "par_set_entities_ref_layout": [_p, _p, _p, _i],
    "par_update_aabbs": [_p, _p, _i, _i],
    "par_update_aabbs_async": [_p, _p, _i, _i, _p],
    "par_set_light": [_p, _p],
    "par_set_lights": [_p, _p, _i],
    "par_set_light_model": [_p, _i],
    "par_set_light_tints": [_p, _p, _i],
    "par_render": [_p, _p, _u],
    "par_render_rows": [_p, _i, _i, _p, _u],
    "par_render_device": [_p, _p, _i, _i, _p, _u],
    "par_render_device_slots": [_p, _p, _p, _i, _i, _i, _i, _i, _u],
    "par_render_device_timed": [_p, _p, _i, _i, _p, _u, _p],
    "par_relight_device": [_p, _p, _i, _i, _p, _p, _u],
    "par_relight_rows": [_p, _i, _i, _p, _u],
    "par_graph_capture": [_p, _p, _i, _i, _p, _u],
    "par_graph_stage": [_p, _p, _i, _i, _p],
    "par_graph_launch": [_p, _p],
    "par_graph_capture_lights": [_p, _p, _i, _i, _p, _u],
    "par_graph_stage_lights": [_p, _p, _i, _i, _p, _i],
    "par_pick": [_p, _i, _i, _p],
    "par_get_stats": [_p, _p],
    "par_read_grid": [_p, _p, _p, _p],
    "par_debug_units": [_i, _i, _p, _p, _i, _p],
    "par_sprite_tile_floor": (None, [_p]),
    "par_scene_graybox": [_i, _i, _p, _i],
    "par_scene_synthetic": [_i, _i, _i, _i, C.c_uint64, _p, _p],
    "par_row_block": (None, [_i, _i, _i, _i, _p, _p]),
    "par_scene_tiles": [_p, _p, _i, _p, _i],
    "par_tiles_pack": [_p, _p, _p, _i, _p, _i, _i, _p],
    "par_tiles_unpack": [_p, _p, _p, _i, _p, _p],
    "par_background_fill": [_p, _p, _p, _i],
    "par_tiles_assemble": [_p, _p, _p, _p, _p, _i, _i],
    "par_scene_tile_map": [_p, _p, _i, _p, _i],
    "par_tiles_changed_device": [_p, _p, _p, _p, _i, _i, _p, _p, _i, _p],
    "par_tiles_pack_counted": [_p, _p, _p, _p, _i, _p, _i, _i, _p],
    "par_tiles_fetch": [_p, _p, _p, _p, _p, _i, _p, _p, _p, _p],
    "par_tiles_apply_host": [_p, _p, _i, _p, _i, _i, _p],
    "par_plane_tiles_changed_device": [_p, _p, _i, _p, _p, _i, _i, _p, _p, _i, _p],
    "par_plane_tiles_pack": [_p, _p, _i, _p, _i, _p, _i, _i, _p],
    "par_plane_tiles_pack_counted": [_p, _p, _i, _p, _p, _i, _p, _i, _i, _p],
    "par_plane_tiles_unpack": [_p, _p, _i, _p, _i, _p, _p],
    "par_plane_tiles_assemble": [_p, _p, _i, _p, _p, _p, _p, _i, _i],
    "par_plane_tiles_fetch": [_p, _p, _i, _p, _p, _p, _i, _p, _p, _p, _p],
    "par_plane_tiles_apply_host": [_p, _i, _p, _i, _p, _i, _i, _p],
    "par_outline_device": [_p, _p, _p, _p, _i, _i, _p, _i, _i, _p, _p],
    "par_outline_host": [_p, _i, _p, _p, _i, _i, _p, _i, _i, _p, _p],
    "par_quantize_device": [_p, _p, _p, _i, _i, _p, _i, _i, _p, _p],
    "par_quantize_host": [_p, _i, _p, _i, _i, _p, _i, _i, _p, _p],
    "par_palette_ramp": [_p, _i, _p, _i],
    "par_quantize_pattern_device": [_p, _p, _p, _i, _i, _i, _p, _i, _i, _p, _p],
    "par_quantize_pattern_host": [_p, _i, _p, _i, _i, _i, _p, _i, _i, _p, _p],
    "par_palette_reset_device": [_p, _p],
    "par_palette_count_device": [_p, _p, _p, _i, _i, _p],
    "par_palette_cut_device": [_p, _p, _i],
    "par_palette_sum_device": [_p, _p, _p, _i, _i, _p],
    "par_palette_emit_device": [_p, _p, _i, _p],
    "par_palette_fit_host": [_p, _i, _p, _i, _i, _i, _p, _p],
    "par_palette_refine_device": [_p, _p, _p, _i, _i, _p, _i, _i, _p, _p, _p],
    "par_palette_refine_host": [_p, _i, _p, _i, _i, _p, _i, _i, _p],
    "par_present_device": [_p, _p, _p, _p, _p, _p, _i, _i, _i, _p],
    "par_present_host": [_p, _i, _p, _p, _p, _p, _i, _i, _i, _p],
    "par_finish_device": [_p, _p, _p, _p, _i, _i, _p, _i, _i, _p, _p, _i, _i, _p, _p],
    "par_finish_host": [_p, _i, _p, _p, _i, _i, _p, _i, _i, _p, _p, _i, _i, _p, _p],
    "par_upscale_device": [_p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _p, _p],
    "par_upscale_host": [_p, _i, _p, _p, _p, _p, _i, _i, _i, _i, _i, _p, _p],
    "par_debug_line": (None, [_p, _p, _i, _p, _p]),
}
# include/par_cells.h
ABI_CELLS = {
    "par_quantize_cells_device": [_p, _p, _p, _i, _i, _i, _i, _i, _p, _i, _i, _p, _p, _p],
    "par_quantize_cells_host": [_p, _i, _p, _i, _i, _i, _i, _i, _p, _i, _i, _p, _p, _p],
    "par_cells_pairs": [_p, _i, _p, _i],
}
# include/par_tileset.h
ABI_TILESET = {
    "par_tileset_work_bytes": (C.c_size_t, [_i]),
    "par_tileset_build_device": [_p, _p, _p, _i, _i, _i, _i, _i, _i, _p, _p, _i, _p, _p],
    "par_tileset_expand_device": [_p, _p, _p, _i, _i, _i, _p, _i, _i, _p],
    "par_tileset_build_host": [_p, _i, _p, _i, _i, _i, _i, _i, _i, _p, _i, _p, _p],
    "par_tileset_expand_host": [_p, _i, _p, _i, _i, _i, _p, _i, _i, _p],
}
# include/par_tileset_extend.h
ABI_TILESET_EXTEND = {
    "par_tileset_extend_work_bytes": (C.c_size_t, [_i, _i]),
    "par_tileset_extend_device": [_p, _p, _p, _i, _i, _i, _i, _i, _i, _p, _p, _i, _p, _p, _p],
    "par_tileset_extend_host": [_p, _i, _p, _i, _i, _i, _i, _i, _i, _p, _i, _p, _p, _p],
}
# exported for the tests and tools, declared in no public header (csrc/par_context.hip)
ABI_DEBUG_HOOKS = {
    "par_debug_read_stamps": [_p, _p, C.c_size_t],
    "par_debug_set_hooks": [_p, _u, _i],
    "par_debug_read_light_walks": [_p, _p],
    "par_debug_read_items": [_p, _p, C.c_size_t, _p],
}
ABI_HEADERS = {"par_raytracer.h": ABI, "par_cells.h": ABI_CELLS, "par_tileset.h": ABI_TILESET,
               "par_tileset_extend.h": ABI_TILESET_EXTEND}


def install(L, *tables):
    """Set restype and argtypes of every function of `tables` on the loaded library L: an add-on's own table, or, with
    none given, every table above (the core library)."""
    for table in tables or (*ABI_HEADERS.values(), ABI_DEBUG_HOOKS):
        for name, sig in table.items():
            fn = getattr(L, name)
            if type(sig) is tuple:
                fn.restype, sig = sig
            fn.argtypes = sig

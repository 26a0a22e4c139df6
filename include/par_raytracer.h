/*
 * par_raytracer.h — C ABI of the MI355X-native pixel-art raytracer (libpar_raytracer.so).
 *
 * This is the drop-in boundary for the reference's render call: the three statements plus the inline loop in
 * `main` at src/alternative.cpp:690-760 (memset + count_entities_in_bins + trace_hash_for_pixel + the
 * shading/quantise loop around trace_hash_for_light). The reference has no FFI of its own; each entry
 * point below names the reference interface it replaces (alt = src/alternative.cpp, spr = src/sprites.hpp).
 *
 * Conventions
 *   - plain C, plain pointers and sizes, no exceptions cross this boundary; every call returns a par_status.
 *   - ownership follows the reference (alt:503-517): the caller owns every input and output buffer; the context
 *     owns only its device-side copies and work arrays.
 *   - one context = one GPU = one host thread at a time (the reference is single-threaded).
 *   - the library REQUIRES a gfx950 device: there is no CPU fallback. par_create fails with PAR_ERR_NO_DEVICE.
 */
#ifndef PAR_RAYTRACER_H
#define PAR_RAYTRACER_H

#include "par_types.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct par_context par_context;

/* Most lights one frame can be rendered with (par_set_lights): the `lit` plane holds one bit per light. */
#define PAR_MAX_LIGHTS 8

typedef enum par_status {
    PAR_OK = 0,
    PAR_ERR_INVALID_ARG = 1, /* null pointer, negative size, rows out of range, ambient outside [0,1] ... */
    PAR_ERR_NO_DEVICE = 2,   /* no HIP device / not gfx950 */
    PAR_ERR_HIP = 3,         /* a HIP runtime call failed; see par_last_error */
    PAR_ERR_OOM = 4,         /* host or device allocation failed */
    PAR_ERR_UNSUPPORTED = 5, /* grid dimension or bin size outside what the kernels are built for */
    PAR_ERR_EXTENT = 6,      /* an AABB extent the 20x40 sprite cannot express (reference UB: alt:330, SURVEY a-3b) */
    PAR_ERR_SPRITE_ID = 7,   /* sprite id or sprite palette index out of range */
    PAR_ERR_NOT_READY = 8,   /* render before sprites / entities / light were set */
    PAR_ERR_DEVICE = 9       /* a kernel reported a failure since the flag was last read (the hash build's barrier timed
                              * out, or a column overflowed its record in a frame that was sized for none to): a frame
                              * rendered since then is NOT valid. Reported once, by the first call that looks: par_render,
                              * par_render_rows, par_render_device_timed, par_get_stats */
} par_status;

/* Render flags. */
enum {
    /* Cast the shadow ray of uncovered (background) pixels too, as the reference does (alt:703,738). Their colour
     * cannot depend on the result (SURVEY a-6), so by default the ray is skipped; requesting the `lit` plane turns
     * this on implicitly because the result then is observable. */
    PAR_RENDER_TRACE_BACKGROUND = 1u << 0,
    /* Count the shadow rays actually traced into par_frame_stats (one atomic per workgroup). */
    PAR_RENDER_COUNT_RAYS = 1u << 1,
    /* This frame is one of several in flight on the device (a swap chain, par_render_device_slots): favour the
     * device's throughput over the frame's own latency (one wavefront per screen column builds its record and does
     * all its shadow walks, instead of two sharing the walks). Same pixels either way. */
    PAR_RENDER_PIPELINED = 1u << 2,
    /* par_render_device_timed only: time the frame's launches AS A PRODUCTION FRAME MAKES THEM (the background fill
     * riding with the hash-build and column launches) into par_frame_stats.ms_launch, instead of the kernels apart. */
    PAR_RENDER_TIMED_AS_LAUNCHED = 1u << 3,
    /* par_render_device, par_render_device_timed, par_render_device_slots: the caller promises that
     *   - the planes passed in this call are the ones this context's most recent frame was rendered into,
     *   - the rows are the same as in that frame, and
     *   - nothing has written to those rows of those planes since.
     * The frame then sets back to background only the tiles that frame can have drawn into (the device's own record of
     * its hash build; the scene may have changed in between) instead of filling every pixel; the `fb` and `palidx`
     * planes alone are concerned, and the result is the same frame. Of those tiles it sets back only the ones in whose
     * screen column an entity was rewritten since the context's previous frame (par_update_aabbs[_async] and the graph
     * stages by their index range, identical values included; par_set_entities*, par_set_sprites and whatever ends the
     * record below count as every entity): the covered pixels of every other tile are the same set as before, and the
     * frame stores each of them again. A frame with nothing rewritten sets back nothing. The promise is unchanged; what
     * the library relies on besides is that it sees every change of the scene, which it does: they all come through its
     * own entry points. The library keeps a record of the context's last
     * enqueued frame (plane pointers, which of the two planes were given, the rows) and takes this path only when the
     * record matches; otherwise the flag is ignored and the frame fills as without it, so a caller whose promise holds
     * whenever the record matches may always set it. The record is dropped by par_graph_launch and the graph captures,
     * the relight calls, par_render / par_render_rows / par_pick (they render into the context's own buffers), a
     * reported PAR_ERR_DEVICE, any failed enqueue, and a frame timed with its kernels apart; a captured graph never
     * takes this path, and every other entry point accepts the flag and ignores it. What the library cannot see is a
     * write by somebody else:
     * two contexts drawing into one buffer, or a consumer that post-processes the frame in place, must not set it. */
    PAR_RENDER_KEPT_OUTPUTS = 0x10u /* bit 4 */
    /* other bits are rejected; bit 29 is reserved for the library's profiling time stamps */
};

/* Output planes of one render, each nullable. Every pointer addresses the element of (row_begin, column 0);
 * a plane holds (row_end - row_begin) * width elements, row-major like the reference's buffers. */
typedef struct par_outputs {
    par_color* fb;     /* final RGBA8 frame, `p_texture` alt:515,735,757 */
    par_pixel* gbuf;   /* G-buffer, `p_pixel_buffer` alt:511,379 */
    uint8_t* palidx;   /* sprite palette index per pixel (alt:352-354), PAR_PALIDX_BACKGROUND where uncovered */
    float* brightness; /* pre-quantise brightness factor: ambient or min(1, diffuse + ambient), alt:735,757-758 */
    uint8_t* lit;      /* bit l set where trace_hash_for_light returned true for light l (alt:738): 1 or 0 with one
                        * light, a bitmask of the lights that reach the pixel with several (par_set_lights) */
} par_outputs;

typedef struct par_frame_stats {
    int64_t entities;        /* entities uploaded */
    int64_t bin_insertions;  /* (entity, bin) pairs the device inserted in the last frame (alt:243-267 iterations; the
                              * insert kernel's own node count) */
    int64_t shadow_rays;     /* shadow rays traced (only with PAR_RENDER_COUNT_RAYS), else -1 */
    int64_t occupied_columns; /* screen columns (bin footprints) in the rendered rows that show a primitive */
    int64_t overflow_columns; /* ... of which did not fit a column record (rendered straight from the hash) */
    float ms_bin;            /* device time of the hash build + column kernels of the last timed render, else -1 */
    float ms_fill;           /* device time of the background fill kernel of the last timed render, else -1 */
    float ms_render;         /* device time of the render kernels (render_items_kernel, and render_tiles_kernel in a
                              * dense frame) of the last timed render, else -1 */
    float ms_overflow;       /* device time of the overflow-column kernel of the last timed render, else -1 */
    float ms_launch[5];      /* PAR_RENDER_TIMED_AS_LAUNCHED: device time of the frame's launches as a production frame
                              * makes them: [0] hash build (+ its share of the fill), [1] column records (+ the rest of the
                              * fill), [2] render_items_kernel (entry work items), [3] render_tiles_kernel (whole-tile
                              * items of a dense frame), [4] overflow list; 0 where the frame has no such launch;
                              * else -1 */
    int32_t render_merged;   /* PAR_RENDER_TIMED_AS_LAUNCHED: 1 when the frame rendered its entry items, tile items and
                              * overflow columns in ONE launch (render_both_kernel, small frames; its time is
                              * ms_launch[2]), else 0 */
} par_frame_stats;

const char* par_status_string(int status);
/* Detail of the last failure on this context ("" when none). The pointer stays valid until the next call. */
const char* par_last_error(const par_context* ctx);

/* Reference defaults: 480x320x320, bin 40, ambient 0.25, background 127, 4-entry gray palette
 * (alt:116-131, alt:281, alt:702, spr:60-65). */
void par_default_params(par_params* params);
/* hash_width/height/length (alt:120-122) for these parameters. */
int par_grid_dims(const par_params* params, int* gx, int* gy, int* gz);

/* Number of visible HIP devices (0 when there is none); never fails. */
int par_device_count(void);

/* Create a renderer on HIP device `device` (-1: the current device). Allocates the grid and work arrays. */
int par_create(const par_params* params, int device, par_context** out);
void par_destroy(par_context* ctx);

/* --- scene surface: replaces `Entities<N>{aabbs, sprites}` (alt:92-114) and `lights` (alt:619-626) ----------- */

/* Unique sprite table. Palette indices are validated against params.palette_size. */
int par_set_sprites(par_context* ctx, const par_sprite* sprites, int n_sprites);
/* All entities; entity index == array index (alt:93-97). `sprite_ids` nullable (all entities use sprite 0). */
int par_set_entities(par_context* ctx, const par_aabb* aabbs, const int32_t* sprite_ids, int n);
/* The reference's own layout: one Sprite per entity (`std::vector<Sprite>`, alt:95,107). Identical sprites are
 * stored once on the device; entity order is kept. */
int par_set_entities_ref_layout(par_context* ctx, const par_aabb* aabbs, const par_sprite* sprite_per_entity, int n);
/* Per-frame mutation (alt:643-660 moves aabbs[0]): overwrite aabbs[first, first+n). */
int par_update_aabbs(par_context* ctx, const par_aabb* aabbs, int first, int n);
/* The same without blocking: the new AABBs are copied to the device in `stream` order, i.e. after the frames already
 * enqueued on `stream` and before the next one. `stream` must be the stream this context's frames are rendered on
 * (par_render_device); `aabbs` may be reused as soon as the call returns. For a render loop with frames in flight:
 * the call does no cull or bin-range arithmetic on the host (the frames that follow size their launches by what the
 * entities' extents allow wherever they stand, and always carry the launch for overflowed columns), until a blocking
 * call (par_update_aabbs, par_set_entities, the graph calls) brings the exact bookkeeping up to date. */
int par_update_aabbs_async(par_context* ctx, const par_aabb* aabbs, int first, int n, void* stream);
/* lights[0] (alt:712-714, 729-732: the only light the reference reads). The same as par_set_lights(ctx, light, 1): it
 * also returns a context that had several lights to one. */
int par_set_light(par_context* ctx, const par_light* light);
/* All of the reference's `lights` (alt:619-626), 1 <= n <= PAR_MAX_LIGHTS; the array may be reused when the call
 * returns. PAR_ERR_INVALID_ARG, before any device work, for a null context, a null `lights` with n > 0 or n outside
 * [1, PAR_MAX_LIGHTS]. The primary pass and the G-buffer do not change. For each light l a covered pixel gets what the
 * reference's shading loop (alt:703-742) gives it with lights[0] replaced by lights[l]: the L1-normalised direction
 * t_l to the light (spr:28-35), lit_l = trace_hash_for_light from the pixel's bin towards light l's bin, and
 * d_l = std::max(0.f, n . t_l) (the dot product summed left to right, no contraction, alt:745-747). Then
 *     s = 0.f; for l = 0 .. n-1 (ascending): if lit_l, s = s + d_l      (fp32 additions, one after the other)
 *     brightness = std::min(1.f, s + ambient);  fb = Color::operator*(color, brightness)  (spr:8-16, truncating)
 *     lit plane: bit l set <=> lit_l
 * With n = 1 this is the reference's formula exactly. A background pixel keeps its colour (its normal is zero); its lit
 * bits are traced only when rays are asked for (PAR_RENDER_TRACE_BACKGROUND or a lit plane), each the reference's
 * background ray towards light l. `radius` is not read (but see par_set_light_model). With PAR_RENDER_COUNT_RAYS, shadow_rays counts (pixel, light)
 * rays. A frame with n >= 2 runs the hash build, the background fill and one render launch (the light kernel); a
 * timed one reports the light kernel as ms_render and ms_launch[2] and 0 for the launches it does not have.
 * par_graph_capture and par_graph_launch (on a one-light graph) on a context with more than one light return
 * PAR_ERR_UNSUPPORTED; par_graph_capture_lights captures the frame of several lights. */
int par_set_lights(par_context* ctx, const par_light* lights, int n);

/* The light model of a context. A new context is PAR_LIGHTS_UNBOUNDED: everything above, `radius` not read. */
enum { PAR_LIGHTS_UNBOUNDED = 0, PAR_LIGHTS_RANGED = 1 };
/* PAR_ERR_INVALID_ARG, before any device work, for a null context or a model that is neither of the two. Under
 * PAR_LIGHTS_RANGED everything par_set_lights says holds, with these changes for light l at (lx, ly, lz) with radius
 * r_l and a covered pixel at P = (x, gbuf.y, gbuf.z):
 *   r_l <= 0: the light is unbounded, treated exactly as under PAR_LIGHTS_UNBOUNDED (a sun beside torches).
 *   r_l > 0:  with dx, dy, dz the fp32 differences the shading loop forms (alt:712-714) and
 *             len = (|dx| + |dy|) + |dz|, the L1 length Vector::normalize divides by (spr:28-35; the distance of the
 *             reference's own commented-out attenuation, alt:748-755), the pixel is IN RANGE iff len < (float)r_l.
 *       out of range: the light contributes nothing, bit l of `lit` is 0 and no shadow ray is traced towards it;
 *       in range:     lit_l as before, w_l = 1.f - len / (float)r_l (one IEEE division, one subtraction, no
 *                     contraction), and the sum becomes: if lit_l, s = s + d_l * w_l (the product rounded, then the
 *                     addition, no fma). An unbounded light keeps s = s + d_l.
 *   brightness, fb, the order of the sum, the G-buffer and the palette index are unchanged.
 *   A background pixel's position is (x, 0, 0) as in the reference (alt:707-709 on a zeroed Pixel): its bit l, traced
 *   only when rays are asked for, is (in range && the background ray towards light l), by the same len.
 *   With PAR_RENDER_COUNT_RAYS, shadow_rays counts the (covered pixel, light) pairs that are in range or unbounded.
 *   A frame takes the light kernel whatever the light count (one light too). par_graph_capture on a ranged context,
 *   and par_graph_launch of a one-light graph on one, return PAR_ERR_UNSUPPORTED. par_graph_capture_lights captures the
 *   model the context has; par_set_light_model with a DIFFERENT model drops the captured graphs as par_set_sprites
 *   does (PAR_ERR_NOT_READY from the stage and launch calls afterwards); the same model again does nothing. Radii
 *   staged with par_graph_stage_lights, par_graph_stage or set with par_set_light[s] reach the next launch as the
 *   positions do.
 *   With every r_l <= 0 a ranged frame equals the unbounded frame, byte for byte on every plane. */
int par_set_light_model(par_context* ctx, int model);

/* The lights' colours. `tints` != NULL with 1 <= n <= PAR_MAX_LIGHTS makes the context TINTED: light l < n gets tints[l],
 * the lights l >= n are white ({1, 1, 1}); tints go by the light's index, whatever the light count is or becomes, and
 * the array may be reused when the call returns. `tints` == NULL with n == 0 makes the context UNTINTED again, the state
 * of a new context, in which everything above holds as it stands. PAR_ERR_INVALID_ARG, before any device work and with
 * nothing changed, for a null context, `tints` and n disagreeing about being empty, n outside [0, PAR_MAX_LIGHTS], and
 * any component that is not finite or is negative. Components above 1 are allowed (a bright light; the min below clamps).
 * On a tinted context everything par_set_lights and par_set_light_model say holds, with this change for a covered pixel.
 * Let t_l be the term the untinted sum adds for light l: d_l under PAR_LIGHTS_UNBOUNDED or for a light with radius <= 0,
 * d_l * w_l (rounded) for a ranged light in range. Then, in ascending l, for the lit lights that are in range or
 * unbounded only:
 *     s_r = s_r + t_l * tint_l.r;  s_g = s_g + t_l * tint_l.g;  s_b = s_b + t_l * tint_l.b;
 *           (each product rounded to fp32, then the addition, no fma)
 *     b_c = std::min(1.f, s_c + ambient)                  for c = r, g, b   (`ambient` stays white)
 *     fb.c = (unsigned char)((float)color.c * b_c)        per channel, truncating as spr:8-16; alpha passes through
 *     brightness plane = std::max(std::max(b_r, b_g), b_b)
 *   The lit plane, the G-buffer, the palette index, background pixels, shadow_rays and the pairs the ranged kernel walks
 *   and culls do not depend on the tints at all: a black light {0, 0, 0} still traces, sets its bit and counts its rays.
 *   A frame takes the light kernel whatever the light count and model, as a ranged context's does. par_graph_capture
 *   on a tinted context, and par_graph_launch of a one-light graph on one, return PAR_ERR_UNSUPPORTED.
 *   par_graph_capture_lights captures the state the context has; a call that CHANGES the state (tinted <-> untinted)
 *   drops the captured graphs as a change of the light model does (PAR_ERR_NOT_READY from the stage and launch calls
 *   afterwards); a call that only changes the tints' values keeps them, and the new values reach the next
 *   par_graph_launch as positions and radii do (there is no stage call for tints).
 *   With every tint {1, 1, 1} a tinted frame equals the untinted frame, byte for byte on every plane: t * 1.f == t, so
 *   the three sums are the untinted sum and the three factors the untinted brightness. */
int par_set_light_tints(par_context* ctx, const par_light_tint* tints, int n);

/* --- render: replaces alt:690-760 ----------------------------------------------------------------------------- */

/* One frame into caller-owned HOST buffers: bin, trace, shade, copy back, synchronise. */
int par_render(par_context* ctx, const par_outputs* host_out, unsigned flags);
/* Rows [row_begin,row_end) only (multi-GPU row-block sharding); host buffers, synchronous. */
int par_render_rows(par_context* ctx, int row_begin, int row_end, const par_outputs* host_out, unsigned flags);
/* Asynchronous: enqueue on `stream` (a hipStream_t, NULL = default stream) writing DEVICE buffers. No sync.
 * Several frames may be in flight at once, each on its own context and stream (a frame alone is a chain of short
 * kernels that leaves most of the chip idle). A scene update (par_update_aabbs) waits for the context's last
 * asynchronous frame first; par_update_aabbs_async does not. */
int par_render_device(par_context* ctx, void* stream, int row_begin, int row_end, const par_outputs* device_out,
                      unsigned flags);
/* The render loop of a swap chain in one call: frames first_frame .. first_frame + n_frames - 1, frame i on slot
 * i % n_slots (its context, its stream, its device outputs), enqueued back to back without a host wait. Each slot is
 * a context of its own; all of them render the same rows. Like par_render_device it never waits for the device, so it
 * cannot see a kernel's failure flag (PAR_ERR_DEVICE): the caller polls par_get_stats on each slot's context when it
 * next waits for that slot anyway (the flag is sticky until read). */
int par_render_device_slots(par_context* const* ctxs, void* const* streams, const par_outputs* device_outs,
                            int n_slots, int row_begin, int row_end, int first_frame, int n_frames, unsigned flags);
/* As par_render_device, bracketing the kernel groups with HIP events on `stream`; blocks until the frame is done
 * and fills stats->ms_bin (hash build + column kernels) / ms_fill / ms_render / ms_overflow. */
int par_render_device_timed(par_context* ctx, void* stream, int row_begin, int row_end,
                            const par_outputs* device_out, unsigned flags, par_frame_stats* stats);

/* Relit frames: re-shade a frame from its G-buffer when only the lights changed (the reference's own keys move
 * lights[0] while the world stands still, alt:641-681; its shading loop, alt:703-758, is a pass over the G-buffer).
 * No hash build and no primary pass: the covered pixels are shaded again under the lights, the light model and the
 * tints the context holds at the call.
 * Retained frame. A context has one once par_render, par_render_rows, par_render_device, par_render_device_timed,
 * par_pick (its one row) or par_render_device_slots (per slot context) has returned PAR_OK: the rows [r0, r1) of that
 * frame, and what its hash build left on the device. Nothing new is stored. Every later call that enqueues a hash
 * build replaces it. The context has none after par_set_sprites, par_set_entities[_ref_layout],
 * par_update_aabbs[_async], par_graph_capture[_lights], par_graph_stage[_lights], par_graph_launch, or a
 * PAR_ERR_DEVICE report. par_set_light, par_set_lights, par_set_light_model, par_set_light_tints, par_get_stats and
 * par_read_grid keep it, and so does a relit frame: relit frames can follow one another.
 * `gbuf` is the G-buffer plane of the retained frame, device memory addressing (row_begin, 0) as every plane does; it
 * is only read. device_out->fb, ->brightness and ->lit are written, each nullable; they may be the very buffers the
 * retained frame wrote. ->gbuf and ->palidx must be NULL: they do not depend on lights, the caller keeps the ones it
 * has. On every requested plane a relit frame equals, byte for byte, what par_render_device would write now for the
 * same scene, rows and flags (1 to PAR_MAX_LIGHTS lights, both light models, tinted or not; one white unbounded light
 * too, whose full frame takes another path), provided `gbuf` holds what that render would put in its gbuf plane.
 * A pixel is covered iff its 28-byte texel differs from the background texel (normal 0, colour {bg, bg, bg, 0}, y, z
 * and entity 0); a covered pixel whose texel equals it has a zero normal and gets the background's colour either way.
 * Background pixels get the fill's colour, `ambient`, and, when rays are asked for (PAR_RENDER_TRACE_BACKGROUND or a
 * lit plane), the background bits of a frame with these lights.
 * Checked in this order, before any device work (a refused call changes nothing): PAR_ERR_INVALID_ARG for a null
 * context, `gbuf` or outputs, a non-null out->gbuf or out->palidx, undefined flag bits, a bad row range;
 * PAR_ERR_NOT_READY without sprites, entities or a light, without a retained frame, for rows not inside [r0, r1), and,
 * for par_relight_rows, when the retained frame is not a par_render / par_render_rows frame with a gbuf plane.
 * PAR_RENDER_COUNT_RAYS counts what the light kernel would count for that frame; PAR_RENDER_PIPELINED and
 * PAR_RENDER_TIMED_AS_LAUNCHED are accepted and change nothing. A relit frame does not flip the grid set and leaves
 * par_get_stats' entities, insertions and column counts as the retained frame left them.
 * Ordering: enqueue a relit frame on the retained frame's stream, or order the two yourself; the library does not
 * check it. The kernel stays inside its arrays whatever the texels hold.
 * Left out on purpose: no graph capture of relit frames, no timed variant, no par_render_device_slots counterpart. */
/* device buffers, asynchronous on `stream`, no sync */
int par_relight_device(par_context* ctx, void* stream, int row_begin, int row_end, const par_pixel* gbuf,
                       const par_outputs* device_out, unsigned flags);
/* host buffers, synchronous; reads the context's own device copy of the gbuf plane of the last par_render /
 * par_render_rows */
int par_relight_rows(par_context* ctx, int row_begin, int row_end, const par_outputs* host_out, unsigned flags);

/* hipGraph path (BASELINE config 5): capture {pinned-host AABB/light upload -> build -> fill -> render} once, replay
 * per frame. `par_graph_stage` writes the next frame's AABBs/light into the pinned staging area the graph copies
 * from; it fails with PAR_ERR_UNSUPPORTED when the staged scene needs larger launch grids than were captured (about
 * twice the bin insertions of the captured frame): capture again then. The staged AABBs are the context's scene from
 * then on: a frame that is not a graph's (par_render*, par_pick) uploads them itself before it renders, on its own
 * stream; as for any two frames on different streams, the caller orders it after a graph still in flight on another.
 * A capture with PAR_RENDER_TRACE_BACKGROUND and no lit plane keeps the rays' results in a plane of the context that
 * a capture cannot allocate: it returns PAR_ERR_NOT_READY unless a frame that is not a graph's was rendered or relit
 * with that flag, without a lit plane and with at least as many rows before. This check comes after every other one,
 * when the capture has begun: like any capture that fails then, it leaves no graph and no retained frame. A scene
 * without entities (par_set_entities with n == 0) is captured, staged and launched like any other. */
/* A context with more than one light (par_set_lights) cannot be captured: PAR_ERR_UNSUPPORTED. Two kinds of graph:
 * par_graph_capture's (the one-light path: the kernels of par_render_device with one light) and
 * par_graph_capture_lights's (the light path). Capturing either drops the graphs captured before; so does
 * par_set_sprites, after which par_graph_stage* and par_graph_launch return PAR_ERR_NOT_READY. par_graph_stage
 * replaces lights[0] (the count is kept) when `light` is not NULL. par_graph_launch renders the context's lights as
 * they are at launch time (par_set_light, par_set_lights, par_graph_stage, par_graph_stage_lights): a one-light graph
 * returns PAR_ERR_UNSUPPORTED when there are several; a light-path graph renders any count from 1 to PAR_MAX_LIGHTS. */
int par_graph_capture(par_context* ctx, void* stream, int row_begin, int row_end, const par_outputs* device_out,
                      unsigned flags);
int par_graph_stage(par_context* ctx, const par_aabb* aabbs, int first, int n, const par_light* light);
int par_graph_launch(par_context* ctx, void* stream);
/* Capture the path of several lights: {pinned AABB upload, pinned lights upload -> hash build -> [background rays]
 * -> fill -> light kernel}, one graph per grid set, like par_graph_capture. Works for a context with 1..PAR_MAX_LIGHTS
 * lights. Later launches render whatever lights the context holds at launch time, any count from 1 to PAR_MAX_LIGHTS.
 * Its argument, flag, row and readiness checks, the non-default stream, the launch grids' head-room and the stripping
 * of PAR_RENDER_COUNT_RAYS are those of par_graph_capture; a failed capture leaves no graph. A frame it replays equals,
 * bit for bit on every requested plane, what par_render_device gives for the same scene, lights, rows and flags. Each
 * launch writes the lights into the staging block of its grid set once that set's previous launch has run, so frames
 * can be staged and launched back to back without a host wait. */
int par_graph_capture_lights(par_context* ctx, void* stream, int row_begin, int row_end,
                             const par_outputs* device_out, unsigned flags);
/* par_graph_stage, plus the whole light set: lights != NULL with 1 <= n_lights <= PAR_MAX_LIGHTS replaces it (as
 * par_set_lights would); lights == NULL with n_lights == 0 keeps it. Everything is checked before anything changes: a
 * rejected call leaves the AABBs, the lights and the staging areas as they were. PAR_ERR_NOT_READY: no context or no
 * captured graph; PAR_ERR_INVALID_ARG: n_lights outside [0, PAR_MAX_LIGHTS], or `lights` and `n_lights` disagree about
 * being empty; PAR_ERR_UNSUPPORTED: n_lights >= 2 on a one-light graph (par_graph_capture); the AABB range, extent and
 * bound errors exactly as par_graph_stage. */
int par_graph_stage_lights(par_context* ctx, const par_aabb* aabbs, int first, int n,
                           const par_light* lights, int n_lights);

/* Mouse pick (alt:380-382, 698-700): the G-buffer texel under (x, y) of the last frame rendered with a gbuf
 * plane is the caller's to read; this helper renders just that pixel's row. */
int par_pick(par_context* ctx, int x, int y, par_pixel* out);

/* Statistics of the last render (blocks until it finished). PAR_ERR_DEVICE when a kernel flagged a failure since the
 * flag was last read. */
int par_get_stats(par_context* ctx, par_frame_stats* stats);

/* Read back the spatial hash of the last render in the reference's layout (`count[G]`, `map[G*8]`,
 * `bins[G*8]`, alt:503-509). Only slots below count[b] are defined; the others are zero. Parity tooling. */
int par_read_grid(par_context* ctx, int32_t* count, int32_t* map, par_aabb* bins);

/* Test hook: the reference's three arithmetic units as the DEVICE kernels compute them, on `n` host vectors
 * (tests/golden/ref_units.npz holds the reference's own answers). kind 0: AABB::intersect, alt:40-83 — in_a =
 * par_aabb[n], in_b = n x {float inv_x, inv_y, inv_z; int16 origin x, y, z; int16 pad} (`Ray`, alt:30-33), out =
 * uint8_t[n]. kind 1: Color::operator*(float), spr:8-16 — in_a = n x {float r, g, b, a, v}, out = n x uint8_t[4].
 * kind 2: Vector::normalize, spr:28-35 — in_a = n x float[3], out = n x float[3]. kinds 3 and 4: kind 0's test as the
 * render kernel runs it on the records of a shadow walk (planes as floats, packed arithmetic; 3: hardware min/max
 * where the inverse direction is finite, 4: the reference's compare-selects throughout), same arguments. */
int par_debug_units(int device, int kind, const void* in_a, const void* in_b, int n, void* out);

/* --- host-side scene helpers (C++ host code, no GPU needed) ---------------------------------------------------- */

/* `make_tile_floor` (spr:73-364). */
void par_sprite_tile_floor(par_sprite* out);
/* The graybox world of alt:517-599 for a view of width x length (480 x 320 in the reference). Returns the entity
 * count (162 308 for the reference view); writes at most `capacity` AABBs. */
int par_scene_graybox(int view_width, int view_length, par_aabb* out, int capacity);
/* Synthetic benchmark scene: n boxes of extent (20,20,20), positions from splitmix64(seed):
 * x in [-20,width), y in [-20,200), z in [-20,length). Also returns the light (5w/8, h/2, l/4). */
int par_scene_synthetic(int n, int width, int height, int length, uint64_t seed, par_aabb* out, par_light* light);
/* Row block [begin, end) of `rank` when one frame is sharded over `ranks` GPUs: contiguous, disjoint,
 * covering [0, height), cut at multiples of the bin size (a bin row of 40 screen rows never straddles two ranks), the
 * bin rows dealt as evenly as they go. */
void par_row_block(int rank, int ranks, int height, int bin_size, int* begin, int* end);
/* --- sharded frames: assembling only what can differ from the background ----------------------------
 * A frame sharded by row blocks over the GPUs of a node is assembled on one of them. Most of a sparse frame is the
 * constant background, which the assembling rank can write itself: only the screen TILES (bin footprints, bin_size x
 * bin_size pixels) that can show a primitive need to travel. Every rank holds the whole scene, so every rank derives
 * the same tile list (no exchange of metadata), sorted by bin row: a rank's row block is a contiguous run of it. */

/* The tiles that can show a primitive: the screen columns the entities reach by the cull and bin ranges of
 * alt:212-240 (a superset of the columns the spatial hash will mark occupied). Host arithmetic, no GPU needed.
 * tiles[i] = bx | by << 16, sorted by (by, bx). Returns the number of such tiles (writes at most `capacity`), or a
 * negative par_status. */
int par_scene_tiles(const par_params* params, const par_aabb* aabbs, int n, int32_t* tiles, int capacity);
/* Copy tiles d_tiles[0, n) (device array) out of a frame block -- rows [row_begin, row_end) of the frame, stored
 * at `fb_block` -- into `packed`: n slots of bin_size x bin_size pixels, slot i row-major. Pixels of a slot beyond the
 * view's right / bottom edge are not written. Asynchronous on `stream` (a hipStream_t); device pointers. */
int par_tiles_pack(const par_params* params, void* stream, const int32_t* d_tiles, int n, const par_color* fb_block,
                   int row_begin, int row_end, par_color* packed);
/* The inverse on the assembling rank: slots -> their place in the whole frame (`frame` addresses row 0). */
int par_tiles_unpack(const par_params* params, void* stream, const int32_t* d_tiles, int n, const par_color* packed,
                     par_color* frame);
/* The background (Color{background} * ambient, alt:281, 735) for n_rows whole rows starting at `rows`. */
int par_background_fill(const par_params* params, void* stream, par_color* rows, int n_rows);
/* Both of the above in one pass, for the rows the assembling rank did not render itself: rows [row_begin, row_end) of
 * the frame (`frame` addresses row 0) are written exactly once -- a packed tile's pixels where `d_map` (device array
 * of grid-x * grid-y entries: tile column + tile row * grid-x -> slot in `packed`, -1 = background) names one, the
 * background elsewhere. par_scene_tile_map makes the host copy of the map from the tile list (capacity >= grid-x *
 * grid-y entries). */
int par_tiles_assemble(const par_params* params, void* stream, const int32_t* d_map, const par_color* packed,
                       par_color* frame, int row_begin, int row_end);
int par_scene_tile_map(const par_params* params, const int32_t* tiles, int n, int32_t* map, int capacity);

/* --- changed tiles: copying back only the tiles that differ from the last frame (nothing in the reference) --------
 * A frame on the device costs tens of microseconds; the same frame copied to the host costs milliseconds, and in a
 * frame loop almost nothing on screen changes from one frame to the next. These calls compare two finished `fb` planes
 * tile by tile on the device, pack the tiles that differ by a count that never leaves the device, fetch them with one
 * small and one proportional copy, and apply them to the host's copy of the frame. Like the other passes over finished
 * planes they take no context: retained frames, graphs and statistics are not involved and do not change, and the
 * planes may come from a render, a relit frame, a graph's frame, an outlined or quantised frame, or a row block of a
 * sharded frame. par_scene_tiles cannot stand in for the comparison: it is a superset computed from the geometry and
 * knows nothing of lights, outlines or palette output, which change pixels without moving an AABB.
 * In everything below B = params->bin_size, gx = ceil(width / B), gy = ceil(height / B); params->length, the ambient,
 * the background and the palette are not read. Tile (bx, by) covers columns [bx * B, min((bx + 1) * B, width)) and rows
 * [by * B, min((by + 1) * B, height)); a tile word is bx | by << 16, a slot is B x B pixels, row-major, as
 * par_tiles_pack has them.
 * The property that ties the four calls together: take a host frame that equals `a` on the rows [r0, r1). When
 * count <= capacity, par_tiles_changed_device(a, b) -> par_tiles_pack_counted on b -> par_tiles_fetch ->
 * par_tiles_apply_host turns that frame into `b` on those rows and leaves every other row alone.
 * Left out on purpose: no comparison of planes other than 4-byte fb planes (index planes and the G-buffer have the
 * par_plane_tiles_* calls further down), no tolerance or "nearly equal", no bounding rectangle, no copy of b over a (a swap chain already holds the
 * previous frame in its other slot), no device-side apply (par_tiles_unpack is that), no graph-capture helper (the two
 * device calls are capturable as any stream-ordered launch is), and no change to par_render's own copy. */

/* Which tiles differ. Device pointers, asynchronous on `stream` (a hipStream_t): no synchronisation, no allocation, no
 * copy to the host. `a` and `b` each address (row_begin, column 0) and hold rows [r0, r1) = [row_begin, row_end), dense
 * and row-major; both are only read, and a == b is allowed (count 0). A tile is IN THE BLOCK iff its rows intersect
 * [r0, r1). A tile is CHANGED iff it is in the block and some pixel differs between a and b as a 32-bit word (the alpha
 * byte counts), among the pixels whose column is in the tile and whose row is in both the tile and the block.
 *     d_map   gx * gy entries, every one written: d_map[bx + by * gx] is the tile's rank among the changed tiles in
 *             ascending (by, bx) order -- its slot in a packed buffer -- or -1 when the tile is unchanged or not in the
 *             block (the format par_tiles_assemble reads). The rank is written whatever `capacity` is. d_map doubles as
 *             the call's work array, which is why it may not be NULL.
 *     d_tiles d_tiles[i] = bx | by << 16 of the changed tile of rank i, for i < min(count, capacity); the entries from
 *             there on are not written. May be NULL when capacity is 0.
 *     d_count d_count[0] = the number of changed tiles, which may exceed `capacity`.
 * The output is a function of the two planes alone: it does not depend on the order in which workgroups run (ordering
 * is by kernel boundaries; no flag is polled and no global atomic is used).
 * PAR_ERR_INVALID_ARG, before any device work and with nothing written (no GPU is needed to get it), for a null
 * `params`, `a`, `b`, `d_map` or `d_count`, capacity < 0, a null d_tiles with capacity > 0, width <= 0 or height <= 0,
 * a bin size outside [8, 160] (as par_tiles_pack), or rows that are not 0 <= r0 < r1 <= height; PAR_ERR_UNSUPPORTED,
 * as early, for gx or gy above 1024 (par_create's bound; the tile word depends on it). The pointers have their types'
 * alignment; the loads are of 16, 8 or 4 bytes, the largest that divides width * 4, B * 4 and both addresses (the rule of
 * the plane-tile calls below, which this call shares its kernels with), and every placement gives the same result. The
 * loads are bounded by the block's rows and the view's width whatever the planes hold. */
int par_tiles_changed_device(const par_params* params, void* stream, const par_color* a, const par_color* b,
                             int row_begin, int row_end, int32_t* d_map, int32_t* d_tiles, int capacity,
                             int32_t* d_count);
/* par_tiles_pack by a count that stays on the device. Device pointers, asynchronous on `stream`. With m =
 * min(max(d_count[0], 0), capacity) read on the device, the result is what par_tiles_pack(params, stream, d_tiles, m,
 * fb_block, row_begin, row_end, packed) writes, byte for byte: slot pixels outside the block's rows or beyond the view's
 * edge are not written, and slots from m on are not written. A list entry with bx >= gx or by >= gy is skipped, so the
 * kernel stays inside the frame whatever the list holds. capacity == 0 launches nothing. The argument checks are
 * par_tiles_pack's (PAR_ERR_INVALID_ARG for a null `params`, width or height <= 0, a bin size outside [8, 160], null
 * d_tiles, fb_block or packed with capacity > 0, or rows that are not 0 <= row_begin <= row_end <= height), plus a null
 * d_count and capacity < 0. */
int par_tiles_pack_counted(const par_params* params, void* stream, const int32_t* d_tiles, const int32_t* d_count,
                           int capacity, const par_color* fb_block, int row_begin, int row_end, par_color* packed);
/* The only call of the four that waits for the device: synchronises `stream` and copies d_count[0] to *count. If
 * 0 <= *count <= capacity then *n = *count, and *n tile words and *n * B * B pixels are copied into the host arrays
 * `tiles` and `packed` (pageable or pinned). Otherwise *n = 0 and nothing more is copied: the list is incomplete, and
 * the caller copies the frame instead. PAR_OK either way. A copy that fails returns PAR_ERR_HIP, a missing device
 * PAR_ERR_NO_DEVICE; PAR_ERR_INVALID_ARG, before any device work, for a null pointer, capacity < 0, width or
 * height <= 0 or a bin size outside [8, 160]. */
int par_tiles_fetch(const par_params* params, void* stream, const int32_t* d_count, const int32_t* d_tiles,
                    const par_color* d_packed, int capacity, int32_t* tiles, par_color* packed, int* n, int* count);
/* Host arithmetic, no GPU needed. `frame` addresses row 0 of a whole host frame. For each i < n, the pixels of slot i
 * whose row lies in both the tile and [row_begin, row_end) and whose column lies in the tile go to their place in
 * `frame`; nothing else is written. PAR_ERR_INVALID_ARG, after every entry is checked and before anything is written,
 * for a null `params`, null tiles, packed or frame with n > 0, n < 0, rows that are not 0 <= row_begin < row_end <=
 * height, width or height <= 0, a bin size outside [8, 160], or any entry with bx >= gx or by >= gy. */
int par_tiles_apply_host(const par_params* params, const int32_t* tiles, int n, const par_color* packed,
                         int row_begin, int row_end, par_color* frame);

/* --- plane tiles: the tile calls for planes of 1-, 4- and 28-byte elements (nothing in the reference) ------------
 * The calls above move `fb` planes. The plane a frame loop most wants on the host is often another one: the index
 * plane of par_quantize_device or par_finish_device (1 byte a pixel, a quarter of the copy), or the G-buffer a host picks
 * from. A tile of any plane is a run of B * E bytes per row, so these seven calls are par_tiles_pack, par_tiles_unpack,
 * par_tiles_assemble, par_tiles_changed_device, par_tiles_pack_counted, par_tiles_fetch and par_tiles_apply_host with
 * "pixel" read as "element of E = elem_bytes bytes". E is 1 (`palidx`, `lit`, index_out of par_quantize_device,
 * edge_out of par_outline_device), 4 (`fb`, `brightness`) or 28 (`gbuf`); any other value is PAR_ERR_INVALID_ARG.
 * In everything below B = params->bin_size, gx = ceil(width / B), gy = ceil(height / B); params->length (except where
 * par_plane_tiles_assemble checks it), the ambient, the background and the palette are not read. Tile (bx, by) covers
 * columns [bx * B, min((bx + 1) * B, width)) and rows [by * B, min((by + 1) * B, height)); a tile word is bx | by << 16.
 * A PLANE is dense and row-major, width * E bytes a row, and addresses (row_begin, column 0) unless a call says row 0.
 * A SLOT is B * B * E bytes: slot i starts at byte i * B * B * E of a packed buffer, and element (ry, cx) of it is at
 * byte (ry * B + cx) * E of the slot. Planes and packed buffers are void* with the alignment of their element: any
 * byte for E = 1, 4 bytes for E = 4 and E = 28. The width and B may be odd; slots of an odd B start on odd bytes.
 * The kernels move units of 16, 8, 4 or 1 bytes, the largest that divides width * E, B * E and every address involved,
 * so that a unit never spans two tiles; every placement gives the same bytes. With E = 4 (and `fill` set to the
 * background colour for assemble) every output equals the 4-byte call's, byte for byte.
 * The property that ties the changed-tiles four together holds here as there: take a host plane that equals `a` on the
 * rows [r0, r1). When count <= capacity, par_plane_tiles_changed_device(a, b) -> par_plane_tiles_pack_counted on b ->
 * par_plane_tiles_fetch -> par_plane_tiles_apply_host turns it into `b` on those rows and leaves every other row alone.
 * Left out on purpose: no union of several planes' changes in one call (a caller with `fb` and `palidx` calls twice),
 * no element sizes other than the three, no change to par_ranks or to the benchmark, and no demo flag. */

/* Which tiles differ. Device pointers, asynchronous on `stream` (a hipStream_t): no synchronisation, no allocation, no
 * copy to the host. `a` and `b` each address (row_begin, column 0) and hold rows [r0, r1) = [row_begin, row_end); both
 * are only read, and a == b is allowed (count 0). A tile is IN THE BLOCK iff its rows intersect [r0, r1). A tile is
 * CHANGED iff it is in the block and some byte differs between a and b among the elements whose column is in the tile
 * and whose row is in both the tile and the block.
 *     d_map   gx * gy entries, every one written: d_map[bx + by * gx] is the tile's rank among the changed tiles in
 *             ascending (by, bx) order -- its slot in a packed buffer -- or -1 when the tile is unchanged or not in the
 *             block (the format par_plane_tiles_assemble reads). The rank is written whatever `capacity` is. d_map
 *             doubles as the call's work array, which is why it may not be NULL.
 *     d_tiles d_tiles[i] = bx | by << 16 of the changed tile of rank i, for i < min(count, capacity); the entries from
 *             there on are not written. May be NULL when capacity is 0.
 *     d_count d_count[0] = the number of changed tiles, which may exceed `capacity`.
 * The output is a function of the two planes alone: it does not depend on the order in which workgroups run (ordering
 * is by kernel boundaries; no flag is polled and no global atomic is used).
 * PAR_ERR_INVALID_ARG, before any device work and with nothing written (no GPU is needed to get it), for an elem_bytes
 * other than 1, 4 or 28, a null `params`, `a`, `b`, `d_map` or `d_count`, capacity < 0, a null d_tiles with capacity > 0,
 * width <= 0 or height <= 0, a bin size outside [8, 160], or rows that are not 0 <= r0 < r1 <= height;
 * PAR_ERR_UNSUPPORTED, as early, for gx or gy above 1024. The loads are bounded by the block's rows and the view's width
 * whatever the planes hold. */
int par_plane_tiles_changed_device(const par_params* params, void* stream, int elem_bytes, const void* a, const void* b,
                                   int row_begin, int row_end, int32_t* d_map, int32_t* d_tiles, int capacity,
                                   int32_t* d_count);
/* Copy tiles d_tiles[0, n) (device array) out of a plane block -- rows [row_begin, row_end) of the plane, stored at
 * `block` -- into `packed`: n slots. Slot bytes outside the block's rows or beyond the view's right / bottom edge are
 * not written, and slots from n on are not written. A list entry with bx >= gx or by outside [0, gy) is skipped, so the
 * kernel stays inside the block whatever the list holds. Asynchronous on `stream`; device pointers; n == 0 launches
 * nothing. PAR_ERR_INVALID_ARG, before any device work, for an elem_bytes other than 1, 4 or 28, a null `params`, width
 * or height <= 0, a bin size outside [8, 160], n < 0, null d_tiles, block or packed with n > 0, or rows that are not
 * 0 <= row_begin <= row_end <= height. */
int par_plane_tiles_pack(const par_params* params, void* stream, int elem_bytes, const int32_t* d_tiles, int n,
                         const void* block, int row_begin, int row_end, void* packed);
/* par_plane_tiles_pack by a count that stays on the device. Device pointers, asynchronous on `stream`. With m =
 * min(max(d_count[0], 0), capacity) read on the device, the result is what par_plane_tiles_pack(params, stream,
 * elem_bytes, d_tiles, m, block, row_begin, row_end, packed) writes, byte for byte: slot bytes outside the block's rows
 * or beyond the view's edge are not written, slots from m on are not written, and a list entry with bx >= gx or by
 * outside [0, gy) is skipped. capacity == 0 launches nothing. PAR_ERR_INVALID_ARG, before any device work, for an
 * elem_bytes other than 1, 4 or 28, a null `params`, width or height <= 0, a bin size outside [8, 160], a null d_count,
 * capacity < 0, null d_tiles, block or packed with capacity > 0, or rows that are not 0 <= row_begin <= row_end <=
 * height. */
int par_plane_tiles_pack_counted(const par_params* params, void* stream, int elem_bytes, const int32_t* d_tiles,
                                 const int32_t* d_count, int capacity, const void* block, int row_begin, int row_end,
                                 void* packed);
/* The inverse of par_plane_tiles_pack on a whole plane (`frame` addresses row 0): the elements of slot i that lie in
 * the view go to their place in `frame`, for i < n; nothing else is written. A list entry with bx >= gx or by outside
 * [0, gy) is skipped, so the kernel stays inside the frame whatever the list holds. Asynchronous on `stream`; device
 * pointers. PAR_ERR_INVALID_ARG, before any device work, for an elem_bytes other than 1, 4 or 28, a null `params`, width
 * or height <= 0, a bin size outside [8, 160], n < 0, or null d_tiles, packed or frame with n > 0. */
int par_plane_tiles_unpack(const par_params* params, void* stream, int elem_bytes, const int32_t* d_tiles, int n,
                           const void* packed, void* frame);
/* Rows [row_begin, row_end) of `frame` (`frame` addresses row 0) are written exactly once: a packed tile's element
 * where `d_map` (device array of gx * gy entries: bx + by * gx -> slot in `packed`, negative = none; what
 * par_plane_tiles_changed_device and par_scene_tile_map write) names a slot >= 0, the E bytes at the HOST pointer `fill`
 * elsewhere. `fill` is read during the call and may be reused on return (it travels to the kernel by value). For the
 * palidx plane the fill is the byte PAR_PALIDX_BACKGROUND; params->ambient and background are not read. A map entry >=
 * the number of slots the caller allocated is the caller's error. Asynchronous on `stream`; row_begin == row_end launches
 * nothing. PAR_ERR_INVALID_ARG, before any device work, for an elem_bytes other than 1, 4 or 28, a null `params`, width,
 * height, length or bin size <= 0, a null d_map, packed, fill or frame, or rows that are not 0 <= row_begin <= row_end <=
 * height. */
int par_plane_tiles_assemble(const par_params* params, void* stream, int elem_bytes, const int32_t* d_map,
                             const void* packed, const void* fill, void* frame, int row_begin, int row_end);
/* The only call of the seven that waits for the device: synchronises `stream` and copies d_count[0] to *count. If
 * 0 <= *count <= capacity then *n = *count, and *n tile words and *n * B * B * E bytes of slots are copied into the host
 * arrays `tiles` and `packed` (pageable or pinned). Otherwise *n = 0 and nothing more is copied: the list is incomplete,
 * and the caller copies the plane instead. PAR_OK either way. A copy that fails returns PAR_ERR_HIP, a missing device
 * PAR_ERR_NO_DEVICE; PAR_ERR_INVALID_ARG, before any device work, for an elem_bytes other than 1, 4 or 28, a null pointer,
 * capacity < 0, width or height <= 0 or a bin size outside [8, 160]. */
int par_plane_tiles_fetch(const par_params* params, void* stream, int elem_bytes, const int32_t* d_count,
                          const int32_t* d_tiles, const void* d_packed, int capacity, int32_t* tiles, void* packed, int* n,
                          int* count);
/* Host arithmetic, no GPU needed. `frame` addresses row 0 of a whole host plane. For each i < n, the elements of slot i
 * whose row lies in both the tile and [row_begin, row_end) and whose column lies in the tile go to their place in
 * `frame`; nothing else is written. PAR_ERR_INVALID_ARG, after every entry is checked and before anything is written,
 * for an elem_bytes other than 1, 4 or 28, a null `params`, null tiles, packed or frame with n > 0, n < 0, rows that are
 * not 0 <= row_begin < row_end <= height, width or height <= 0, a bin size outside [8, 160], or any entry with bx >= gx or
 * by outside [0, gy). */
int par_plane_tiles_apply_host(const par_params* params, int elem_bytes, const int32_t* tiles, int n, const void* packed,
                               int row_begin, int row_end, void* frame);

/* --- outlines: silhouettes and creases drawn from the G-buffer (nothing in the reference) ------------------------
 * The post-process pixel-art renderers use most: a dark line where one object ends in front of another or in front of
 * the background, a highlight where a box's top face meets its front face. Everything it needs is in the G-buffer
 * plane of a frame, whatever made it. These calls are a pass over finished planes and take no context: retained
 * frames, graphs and statistics are not involved and do not change. In a frame loop the call goes directly before
 * palette output: render or relight, then outline, then quantise, so that the darkened and lightened colours snap to
 * the palette with everything else.
 * Planes and ranges. `gbuf` addresses (gbuf_row_begin, column 0) and holds rows [g0, g1) = [gbuf_row_begin,
 * gbuf_row_end); it is only read. `fb`, `fb_out` and `edge_out` address (row_begin, 0) and hold rows [r0, r1) =
 * [row_begin, row_end), dense and row-major as every plane is. Required: 0 <= g0 <= r0 < r1 <= g1 <= height. The extra
 * G-buffer rows are the halo: a caller that shades a row block passes a G-buffer plane with one more row on each side
 * that exists in the frame (par_render_device renders any row range), and the block then equals those rows of the
 * whole frame's result, byte for byte. A neighbour row outside [g0, g1) is treated exactly like a row outside the frame.
 * For the pixel at column x and absolute row y, with texel T read as seven little-endian 32-bit words w0..w6,
 * everything in integers:
 *     cov(T)  = T differs from the background texel (normal words 0, colour {bg, bg, bg, 0}, y, z and entity 0: the
 *               definition of par_relight_device)
 *     key(T)  = w4 - w5, that is y - z, in wrapping uint32 (a larger key is nearer to the viewer)
 *     d(T, N) = (int32_t)(key(T) - key(N)), the subtraction wrapping
 *     neighbours: left (x-1), right (x+1), up (y-1), down (y+1); one is present iff its column lies in [0, width) and
 *               its row in [max(0, g0), min(height, g1)); an absent neighbour contributes nothing
 *     silhouette: T is covered, and some present neighbour N either is not covered or has N.entity != T.entity with
 *               d(T, N) >= depth_step (depth_step >= 1 puts the line on the nearer object only, one pixel wide;
 *               background pixels are never outlined)
 *     crease: T is covered and is not a silhouette; the right or the down neighbour N is present and covered, does not
 *               meet the silhouette condition against T (not: T.entity != N.entity with d(N, T) >= depth_step), and
 *               its three normal words differ from T's bit for bit (-0 differs from +0; no float compare). Only right
 *               and down are looked at: the line is one pixel wide and lies on the last pixel of the upper or left
 *               face, which is a box's top edge
 *     class   = 2 for a silhouette, else 1 for a crease, else 0
 *     edge_out = (uint8_t)class                      when edge_out is not NULL
 *     fb_out  = {min(255, (r * s) >> 8), min(255, (g * s) >> 8), min(255, (b * s) >> 8), a} of the pixel's fb value
 *               when fb_out is not NULL, with s = silhouette_scale for class 2, crease_scale for class 1, 256 for class 0
 * fb_out == fb (in place) is allowed: the call reads only a pixel's own fb value; any other overlap of the arrays is
 * undefined. `fb` may be NULL only when fb_out is NULL. PAR_ERR_INVALID_ARG, before any device work and with nothing
 * written (no GPU is needed to get it), for a null `params`, `style` or `gbuf`, both outputs null, fb_out without fb,
 * params->width <= 0, depth_step < 1, a scale outside [0, 1024], or row ranges that break the inequality above. The
 * kernel stays inside its arrays whatever the texels hold. The pointers have their types' alignment (4 bytes for
 * par_pixel and par_color, any byte for edge_out); planes on 16-byte (edge_out: 4-byte) boundaries of a frame whose
 * width is a multiple of 4 take the kernel's wider accesses, every other placement gives the same bytes.
 * Left out on purpose: no 8-neighbourhood, no lines thicker than one pixel, no outline colour other than a scaled pixel
 * colour, no fusing into the render or quantise kernels, and no graph-capture helper (the device call is capturable as
 * any stream-ordered launch is). */
/* device pointers, asynchronous on `stream` (a hipStream_t), no sync: on the frame's own stream, after the render or
 * relight call and before par_quantize_device */
int par_outline_device(const par_params* params, void* stream, const par_outline_style* style,
                       const par_pixel* gbuf, int gbuf_row_begin, int gbuf_row_end,
                       const par_color* fb, int row_begin, int row_end,
                       par_color* fb_out, uint8_t* edge_out);
/* host pointers, synchronous, everything on HIP device `device` (-1: the current device, as par_create): allocates,
 * copies, launches, synchronises, copies back and frees; PAR_ERR_NO_DEVICE / PAR_ERR_OOM / PAR_ERR_HIP as
 * par_quantize_host */
int par_outline_host(const par_params* params, int device, const par_outline_style* style,
                     const par_pixel* gbuf, int gbuf_row_begin, int gbuf_row_end,
                     const par_color* fb, int row_begin, int row_end,
                     par_color* fb_out, uint8_t* edge_out);

/* --- palette output: a frame quantised to a fixed palette (nothing in the reference, which presents RGBA8) --------
 * Several lights, ranged and tinted lights give a frame thousands of colours; an indexed-colour display, a GIF or a
 * sprite sheet wants an index plane over a fixed, art-directed palette. These calls are a pass over a frame's `fb`
 * plane, whatever made it (one light, the light path, a relit frame, a graph's, a frame assembled from row blocks).
 * They take no context: retained frames, graphs and statistics are not involved and do not change.
 * `fb`, `fb_out` and `index_out` address the element of (row_begin, column 0), as every plane does, and hold
 * (row_end - row_begin) * width elements, dense and row-major; `palette` holds n_colors entries,
 * 1 <= n_colors <= PAR_MAX_PALETTE. For the pixel {r, g, b, a} at column x and ABSOLUTE frame row y (row_begin + its
 * row in the block, so a row block of a sharded frame dithers exactly as the whole frame does), in integers:
 *     t   = B4[y & 3][x & 3],  B4 = {{0, 8, 2, 10}, {12, 4, 14, 6}, {3, 11, 1, 9}, {15, 7, 13, 5}}  (ordered dither)
 *     off = floor(((2 * t - 15) * spread) / 32)     (towards minus infinity; spread == 0 gives 0 everywhere)
 *     c'  = min(255, max(0, c + off))               for c = r, g, b
 *     d_p = |r' - P[p].red| + |g' - P[p].green| + |b' - P[p].blue|   (L1, the metric of the reference's normalize;
 *                                                    the alpha of the pixel and of the entries takes no part)
 *     k   = the p with the smallest d_p, the lowest p among equals
 *     index_out = (uint8_t)k                        when index_out is not NULL
 *     fb_out    = {P[k].red, P[k].green, P[k].blue, a}   when fb_out is not NULL (the pixel's own alpha)
 * Every pixel of the rows is processed, the background too. fb_out == fb (in place) is allowed; any other overlap of
 * the arrays is undefined. PAR_ERR_INVALID_ARG, before any device work and with nothing written (no GPU is needed
 * to get it), for a null `params`, palette or `fb`, both outputs null, n_colors outside [1, PAR_MAX_PALETTE], spread
 * outside [0, 255], params->width <= 0, or rows that are not 0 <= row_begin < row_end <= params->height.
 * A palette made from the image's content comes from the fitted-palette calls below (par_palette_*_device), which go
 * directly before this call on the same stream.
 * Left out on purpose: no error-diffusion dithering (sequential by nature; its parallel substitute, pattern dithering,
 * is par_quantize_pattern_device below), no metric other than L1, no fusing into the render kernels, and no
 * graph-capture helper (the device call is capturable as any stream-ordered launch is). */
/* device pointers (`d_palette` too), asynchronous on `stream` (a hipStream_t), no sync: in a frame loop it goes on the
 * frame's own stream, after the render or relight call */
int par_quantize_device(const par_params* params, void* stream, const par_color* d_palette, int n_colors, int spread,
                        const par_color* fb, int row_begin, int row_end, par_color* fb_out, uint8_t* index_out);
/* host pointers, synchronous, everything on HIP device `device` (-1: the current device, as par_create): allocates,
 * copies, launches, synchronises, copies back and frees; PAR_ERR_NO_DEVICE / PAR_ERR_OOM / PAR_ERR_HIP as par_create */
int par_quantize_host(const par_params* params, int device, const par_color* palette, int n_colors, int spread,
                      const par_color* fb, int row_begin, int row_end, par_color* fb_out, uint8_t* index_out);
/* The natural output palette of a scene: every sprite-palette entry at `levels` brightness bands from ambient to
 * full, then the background. Host arithmetic in integers, no GPU needed. With a = (int)(ambient * 255.f), for p in
 * [0, palette_size) and k in [0, levels): s = a + ((255 - a) * k) / (levels - 1) and entry p * levels + k is
 * {(red * s) / 255, (green * s) / 255, (blue * s) / 255, palette[p].alpha} (truncating divisions); the last entry is
 * the colour par_background_fill writes, {ch, ch, ch, 0} with ch = (uint8_t)((float)background * ambient). Returns the
 * entry count palette_size * levels + 1 (writes at most `capacity` entries), or a negative par_status: a null `params`
 * or `out`, capacity < 0, levels outside [2, 255], a count above PAR_MAX_PALETTE, an ambient outside [0, 1] or a
 * palette_size outside [1, PAR_MAX_PALETTE]. */
int par_palette_ramp(const par_params* params, int levels, par_color* out, int capacity);

/* --- pattern dither: palette-aware ordered dithering (nothing in the reference) -----------------------------------
 * par_quantize_device's dither adds one offset of one strength to all three channels, which suits a regular palette
 * whose neighbouring entries lie about `spread` apart on every channel. A fitted or refined palette (below) is
 * irregular: dense where the frame has colours, sparse elsewhere, and off the gray axis under tinted lights. This call
 * is Thomas Knoll's pattern dithering, the order-free substitute for error diffusion: each pixel builds its own list of
 * `depth` palette entries whose mean approximates the pixel, and the Bayer matrix picks one of them. It reads only the
 * pixel and its absolute position.
 * The planes, the row addressing, the outputs and the in-place rule are exactly par_quantize_device's: `fb`, `fb_out`
 * and `index_out` address the element of (row_begin, column 0) and hold (row_end - row_begin) * width elements, dense
 * and row-major; fb_out == fb is allowed, any other overlap is undefined; the pixel's own alpha passes through, and
 * alpha takes no part otherwise. Every pixel of the rows is processed. For the pixel {r, g, b, a} at column x and
 * ABSOLUTE frame row y, in integers, with B4 the matrix of the quantise contract:
 *     e = (0, 0, 0)
 *     for j in 0 .. depth-1:
 *         t_c  = min(255, max(0, c + floor(e_c * strength / 256)))   for c = r, g, b  (floor towards minus infinity)
 *         k_j  = the entry par_quantize_device gives the colour t at spread 0 (L1-nearest, lowest index among equals)
 *         e_c += c - P[k_j].c                                        (the pixel's own c, not t_c; |e_c| <= 255 * depth)
 *     key_j = ((77 * P[k_j].red + 150 * P[k_j].green + 29 * P[k_j].blue) << 8) | k_j      (luma <= 65 280: 24 bits)
 *     sort the depth keys ascending   (equal keys are the same entry, so the order is total: darker first, then the
 *                                      lower index)
 *     rank = (B4[y & 3][x & 3] * depth) >> 4
 *     k    = key_sorted[rank] & 255
 *     index_out = (uint8_t)k                        when index_out is not NULL
 *     fb_out    = {P[k].red, P[k].green, P[k].blue, a}   when fb_out is not NULL (the pixel's own alpha)
 * Consequences: depth == 1 or strength == 0 gives what par_quantize_device gives at spread 0. A pixel whose colour is a
 * palette entry comes back as that entry at any depth and strength, because e stays 0. A padded copy of entry 0
 * (par_palette_emit_device's) never shows, since every k_j is the lowest index among equals. The result depends on
 * nothing but the pixel, x & 3 and y & 3, so a row block equals the whole frame's rows.
 * PAR_ERR_INVALID_ARG, before any device work and with nothing written (no GPU is needed to get it), for a null
 * `params`, palette or `fb`, both outputs null, n_colors outside [1, PAR_MAX_PALETTE], depth outside [1, 16], strength
 * outside [0, 256], params->width <= 0, or rows that are not 0 <= row_begin < row_end <= params->height.
 * In a frame loop it takes par_quantize_device's place: after the palette calls below, on the same stream.
 * Left out on purpose: no matrix other than B4, no sort key other than that luma, no fusing into par_finish_device, no
 * dither awareness in par_palette_refine_device (its assignment stays at spread 0), and no graph-capture helper (the
 * device call is capturable as any stream-ordered launch is). */
/* device pointers (`d_palette` too), asynchronous on `stream` (a hipStream_t), no sync */
int par_quantize_pattern_device(const par_params* params, void* stream, const par_color* d_palette, int n_colors,
                                int depth, int strength, const par_color* fb, int row_begin, int row_end,
                                par_color* fb_out, uint8_t* index_out);
/* host pointers, synchronous, everything on HIP device `device` (-1: the current device, as par_create): allocates,
 * copies, launches, synchronises, copies back and frees; PAR_ERR_NO_DEVICE / PAR_ERR_OOM / PAR_ERR_HIP as
 * par_quantize_host */
int par_quantize_pattern_host(const par_params* params, int device, const par_color* palette, int n_colors,
                              int depth, int strength, const par_color* fb, int row_begin, int row_end,
                              par_color* fb_out, uint8_t* index_out);

/* --- fitted palettes: a frame's palette made on the device by median cut (nothing in the reference) ---------------
 * par_palette_ramp holds every sprite-palette entry under ONE white factor. Tinted lights, ranged lights and outlines
 * scale the three channels independently, and a ramp cannot hold those colours: under a tinted light the ramp of a gray
 * sprite palette is all gray. These calls fit a palette to the colours a frame (or several) actually holds, without a
 * copy to the host. They run over finished planes as quantise, outline and present do: no context, nothing allocated,
 * asynchronous on the caller's stream, no synchronisation; retained frames, graphs and statistics are not involved. In
 * a frame loop they go after render, relight or outline and directly before par_quantize_device, on the same stream:
 * reset, count, cut, sum, emit. Everything is integer arithmetic and does not depend on the order in which the device
 * runs anything.
 * The state is a par_palette_work block (par_types.h) in device memory, 8-byte aligned. cell(p) = (p.red >> 3) |
 * (p.green >> 3) << 5 | (p.blue >> 3) << 10; alpha takes no part anywhere. `fb` addresses (row_begin, column 0) and
 * holds (row_end - row_begin) * width pixels, dense and row-major, 4-byte aligned.
 *   reset  zeroes the whole block.
 *   count  hist[cell(p)] += 1 (modulo 2^32) for every pixel of the rows. It ADDS: several frames or row blocks counted
 *          one after another give the histogram of all of them (a GIF's global palette). Reads only `fb`, writes only
 *          `hist`.
 *   cut    reads `hist`; writes all of `lut` and `n_entries` and zeroes `sums` (`hist` and `reserved` stay). With
 *          uint64 sums, a coordinate being a cell's 5-bit value on an axis, the axes in the order red, green, blue:
 *          a REGION is a box of cells given by inclusive ranges; the regions always partition the 32 x 32 x 32 cube. Its
 *          population n is the sum of `hist` over it, its tight bounds are the smallest and largest coordinate on each
 *          axis over its cells with hist > 0, its extent e is the largest hi - lo of its tight bounds.
 *          If every count is 0: n_entries = 0 and `lut` is all 0. Else region 0 is the whole cube, K = 1, and while
 *          K < n_colors:
 *            the region: among those with e >= 1 the largest e, among equals the larger n, then the lower index; none
 *              ends the cut.
 *            the axis: the first of red, green, blue whose tight hi - lo equals e.
 *            the split point: with m[v] the region's population at coordinate v on that axis, s is the smallest v in
 *              [lo, hi - 1] with 2 * (m[lo] + ... + m[v]) >= n, and hi - 1 if there is none (lo, hi: the tight bounds).
 *            the split: the region keeps its index with its range on that axis cut to [its lo, s]; region K gets
 *              [s + 1, its hi]; K += 1. Both halves hold an occupied cell.
 *          n_entries = K, and lut[c] is the index of the region that holds cell c, the empty cells too, so that a later
 *          frame's new colours map somewhere. A histogram with C occupied cells gives n_entries = min(n_colors, C).
 *   sum    sums[lut[cell(p)]] += {red, green, blue, 1} for every pixel of the rows; it adds, as count does. `lut` is
 *          read as it is found: every byte value names one of the 256 rows of `sums`.
 *   emit   writes exactly n_colors entries to d_palette. With m = min(n_entries, n_colors): entry k < m with count
 *          n_k > 0 is {R, G, B, 255}, a channel being the low 8 bits of (2 * sum + n_k) / (2 * n_k) in uint64 (truncating:
 *          the rounded mean); entry k < m with n_k == 0 is {0, 0, 0, 0}; an entry k >= m is a copy of entry 0 when
 *          m > 0, else {0, 0, 0, 0}. par_quantize_device takes the lowest index among equals, so a padded entry never
 *          shows in an index plane and the caller passes n_colors on to it without learning n_entries: no host wait.
 * A frame whose colours lie one per cell, at most n_colors of them, gets exactly those colours, and quantised with them
 * at spread 0 it comes back as it is.
 * PAR_ERR_INVALID_ARG, before any device work and with nothing written (no GPU is needed to get it), for a null
 * pointer, n_colors outside [1, PAR_MAX_PALETTE], params->width <= 0, rows that are not
 * 0 <= row_begin < row_end <= params->height, or a `work` that is not 8-byte aligned.
 * Left out on purpose: no finer cells than 5 bits a channel (a frame gets at most one entry per occupied cell), no
 * k-means iterations beyond the one mean per region, no weighting by perception, no dither awareness, no fusing into
 * the quantise or finish kernels, and no graph-capture helper (the calls are capturable as any stream-ordered launch
 * is). */
/* device pointers, asynchronous on `stream` (a hipStream_t), no sync */
int par_palette_reset_device(void* stream, par_palette_work* work);
int par_palette_count_device(const par_params* params, void* stream, const par_color* fb, int row_begin, int row_end,
                             par_palette_work* work);
int par_palette_cut_device(void* stream, par_palette_work* work, int n_colors);
int par_palette_sum_device(const par_params* params, void* stream, const par_color* fb, int row_begin, int row_end,
                           par_palette_work* work);
int par_palette_emit_device(void* stream, const par_palette_work* work, int n_colors, par_color* d_palette);
/* One frame on host pointers, synchronous, everything on HIP device `device` (-1: the current device, as par_create):
 * allocates, copies, runs reset, count, cut, sum and emit, synchronises, copies back the n_colors entries and
 * n_entries, and frees; PAR_ERR_NO_DEVICE / PAR_ERR_OOM / PAR_ERR_HIP as par_quantize_host */
int par_palette_fit_host(const par_params* params, int device, const par_color* fb, int row_begin, int row_end,
                         int n_colors, par_color* palette_out, int* n_entries_out);

/* --- refined palettes: k-medians rounds over a palette on the device (nothing in the reference) --------------------
 * The fit above stops at one mean per box of cells. par_quantize_device assigns by L1 distance, and the refinement
 * that matches it is k-medians: assign every pixel to its L1-nearest entry, then move each entry to the per-channel
 * median of its pixels. Either step lowers the summed L1 error or leaves it as it is, which per-channel means do not.
 * The call runs over finished planes as the fit does: no context, nothing allocated, asynchronous on the caller's
 * stream, no synchronisation and no host copy. In a frame loop it goes after par_palette_emit_device and before
 * par_quantize_device, on the same stream; any palette will do, a ramp or a hand-made one too.
 * `fb` addresses (row_begin, column 0) and holds (row_end - row_begin) * width pixels, dense and row-major, 4-byte
 * aligned; `d_palette` holds n_colors entries and is read and written. For each of `iterations` rounds, in integers:
 *   assign  k(p) is the index par_quantize_device gives pixel p against the palette as it stands now, at spread 0:
 *           the L1-nearest entry over red, green and blue, the lowest index among equals; alpha takes no part.
 *   update  for every entry k with n_k > 0 assigned pixels, and for each of red, green and blue, the new channel value
 *           is the LOWER MEDIAN of that channel over its pixels: element (n_k - 1) / 2 (truncating) of the values
 *           sorted in ascending order. The entry's alpha becomes 255. An entry with n_k == 0 keeps all four bytes.
 *           All entries are updated from the same assignment.
 * `d_index` holds (row_end - row_begin) * width bytes, may sit on any byte and is scratch the caller supplies. On return
 * it holds the assignment of the LAST round: the index plane against the palette as it was BEFORE the last update (not
 * against the palette the call leaves, unless that round changed nothing). `d_changed` is nullable; when given,
 * d_changed[0] is the number of entries of which a red, green, blue or alpha byte changed in the last round. 0 means a
 * fixed point, which further rounds leave alone; a caller may read it whenever it next waits anyway.
 * `work` is a par_palette_refine_work block (par_types.h) in device memory, 8-byte aligned. The call initialises
 * whatever it needs in it; between calls its content is the library's. Nothing but it, d_palette, d_index and
 * d_changed[0] is written.
 * Consequences: the summed L1 error of the frame quantised at spread 0 never rises from round to round (the largest
 * error of a single pixel may). Padded copies of entry 0 (par_palette_emit_device's) receive no pixel in the first
 * round, keep the old entry 0, and may pick up pixels in later rounds. A frame whose colours are all palette entries is
 * a fixed point. The result does not depend on the order in which the device runs anything.
 * PAR_ERR_INVALID_ARG, before any device work and with nothing written (no GPU is needed to get it), for a null
 * `params`, `fb`, `d_palette`, `d_index` or `work`, n_colors outside [1, PAR_MAX_PALETTE], iterations outside [1, 16],
 * params->width <= 0, rows that are not 0 <= row_begin < row_end <= params->height, or a `work` that is not 8-byte
 * aligned. PAR_ERR_UNSUPPORTED, as early, when (row_end - row_begin) * width >= 2^32: the tallies are 32-bit.
 * Left out on purpose: several frames in one refinement (a GIF's global palette), dither awareness (the assignment is
 * at spread 0), any metric or centre other than L1 and the median, early exit on the device, and fusing into the
 * quantise or finish kernels. */
/* device pointers, asynchronous on `stream` (a hipStream_t), no sync */
int par_palette_refine_device(const par_params* params, void* stream, const par_color* fb, int row_begin, int row_end,
                              par_color* d_palette, int n_colors, int iterations,
                              uint8_t* d_index, par_palette_refine_work* work, int32_t* d_changed);
/* One frame on host pointers, synchronous, everything on HIP device `device` (-1: the current device, as par_create):
 * allocates, copies `palette` in, runs the rounds, synchronises, copies back the n_colors entries and, where
 * `changed_out` is not NULL, the changed count, and frees; the same argument checks (`palette` for d_palette; there is
 * no d_index or work), and PAR_ERR_NO_DEVICE / PAR_ERR_OOM / PAR_ERR_HIP as par_palette_fit_host */
int par_palette_refine_host(const par_params* params, int device, const par_color* fb, int row_begin, int row_end,
                            par_color* palette, int n_colors, int iterations, int* changed_out);

/* --- present: a frame or an index plane scaled onto a surface (the reference's present, alt:774-788) ---------------
 * The last step of a frame loop: render or relight, then outline, then quantise, then present. The reference copies its
 * frame row by row into a locked SDL texture, honouring the texture's pitch (alt:776-780); the texture is
 * SDL_PIXELFORMAT_RGB888, which shows a par_color's red byte as blue. These calls do that on the device and at an integer
 * scale, nearest neighbour, and they turn an index plane (par_quantize_device's) back into colour through a palette:
 * presenting one index plane with a rotated palette frame after frame is palette cycling, with no render and no
 * quantise. They are a pass over finished planes and take no context: retained frames, graphs and statistics are not
 * involved and do not change. Everything is in integers; sx = desc->scale_x, sy = desc->scale_y.
 * Sources. Exactly one of `fb` and `index` is non-null. Each addresses (row_begin, column 0) and holds rows [r0, r1) =
 * [row_begin, row_end), dense and row-major as every plane is. With `index`, the palette holds n_colors entries,
 * 1 <= n_colors <= PAR_MAX_PALETTE; with `fb`, the palette must be NULL and n_colors 0.
 * Output. `out` addresses output row r0 * sy, byte 0, and holds output rows [r0 * sy, r1 * sy) of W' = width * sx pixels
 * each, desc->pitch bytes from row to row. For the output pixel (X, Y), 0 <= X < W' and r0 * sy <= Y < r1 * sy:
 *     s = the source element at column X / sx and absolute row Y / sy (truncating divisions)
 *     c = fb[s]                                     with an fb source
 *     c = palette[min(index[s], n_colors - 1)]      with an index source: all four bytes, the entry's alpha included
 *         (the clamp defines the out-of-range index, PAR_PALIDX_BACKGROUND among them, and keeps the kernel inside the
 *         palette whatever the plane holds)
 *     under PAR_PRESENT_BGRA the red and blue bytes of c are exchanged
 *     the 4 bytes of c go to (char*)out + (Y - r0 * sy) * pitch + 4 * X
 * The bytes of a row from 4 * W' up to pitch are NOT written (a letterboxed or larger surface: the caller offsets
 * `out`); that holds for the host form's `out` too, which is copied back with a pitched copy. A row block's output is,
 * by the formula, those output rows of the whole frame's: no halo is needed. No overlap of `out` with a source is
 * defined. `fb`, the palette and `out` must be 4-byte aligned; `index` may sit on any byte. `out` on a 16-byte boundary
 * with a pitch that is a multiple of 16 takes the kernel's wider stores; every other placement gives the same bytes.
 * PAR_ERR_INVALID_ARG, before any device work and with nothing written (no GPU is needed to get it), for a null
 * `params`, `desc` or `out`; both sources or neither; an index source without a palette or with n_colors outside
 * [1, PAR_MAX_PALETTE]; an fb source with a palette or n_colors != 0; params->width <= 0; rows that are not
 * 0 <= r0 < r1 <= params->height; a scale outside [1, PAR_MAX_SCALE]; an order that is neither of the two; a pitch that
 * is not a multiple of 4 or is below 4 * width * sx (formed in 64 bits: a product that does not fit an int32 is thereby
 * refused).
 * Left out on purpose: no filtering other than nearest, no fractional scale, no scaled INDEX output, no fusing into the
 * quantise kernel, no 24-bit or 16-bit surface formats, and no graph-capture helper (the device call is capturable as
 * any stream-ordered launch is). */
/* device pointers (`d_palette` too), asynchronous on `stream` (a hipStream_t), no sync: on the frame's own stream, after
 * the last call that writes the source */
int par_present_device(const par_params* params, void* stream, const par_present_desc* desc,
                       const par_color* fb, const uint8_t* index, const par_color* d_palette, int n_colors,
                       int row_begin, int row_end, void* out);
/* host pointers, synchronous, everything on HIP device `device` (-1: the current device, as par_create): allocates,
 * copies, launches, synchronises, copies back and frees; PAR_ERR_NO_DEVICE / PAR_ERR_OOM / PAR_ERR_HIP as
 * par_quantize_host */
int par_present_host(const par_params* params, int device, const par_present_desc* desc,
                     const par_color* fb, const uint8_t* index, const par_color* palette, int n_colors,
                     int row_begin, int row_end, void* out);

/* --- finish: outline, quantise and present a frame in one launch (nothing in the reference) ----------------------
 * The tail of a frame loop as one call: render or relight, then finish. It takes the G-buffer and `fb` in and writes the
 * scaled surface; the outlined frame and the index plane that the three calls above pass from one to the next are never
 * written (the index plane only when asked for). It is a pass over finished planes and takes no context: retained
 * frames, graphs and statistics are not involved and do not change. The contract is the three contracts above and
 * nothing else, and it holds byte for byte.
 * Stage 1, outlines, runs iff `style` is not NULL; `style` and `gbuf` are both given or both NULL. A = the fb_out of
 * par_outline_device(params, style, gbuf, g0, g1, fb, r0, r1) with [g0, g1) = [gbuf_row_begin, gbuf_row_end) and
 * [r0, r1) = [row_begin, row_end): the halo rule is that call's, 0 <= g0 <= r0 < r1 <= g1 <= height, a neighbour row
 * outside [g0, g1) being absent. Without a style A = fb, and gbuf_row_begin and gbuf_row_end are not read.
 * Stage 2, quantise, runs iff `d_palette` (`palette`) is not NULL; then 1 <= n_colors <= PAR_MAX_PALETTE and
 * 0 <= spread <= 255. I = the index_out of par_quantize_device on A, the dither on the absolute row and column.
 * `index_out` is nullable and gets I (rows [r0, r1), dense): it is what a later par_present_device needs for palette
 * cycling. Without a palette n_colors and spread must be 0 and index_out NULL.
 * Stage 3, present. With a palette `out` is what par_present_device(index = I, d_palette, n_colors) writes: all four
 * bytes of the entry, its alpha included (I < n_colors always: the clamp never acts). Without a palette `out` is what
 * par_present_device(fb = A) writes. Scale, order, pitch, the unwritten gap bytes [4 * W', pitch) and the addressing of
 * `out` (output row r0 * sy, byte 0) are that call's.
 * At least one of stages 1 and 2 must run: neither is PAR_ERR_INVALID_ARG, because that call is par_present_device.
 * With a G-buffer halo a row block's surface (and index plane) equals those output rows of the whole frame's.
 * PAR_ERR_INVALID_ARG, before any device work and with nothing written (no GPU is needed to get it), for a null
 * `params`, `desc`, `fb` or `out`; the pairings above broken; and every range check of the three calls on the arguments
 * in use: the style's fields and the row inequality with a style, 0 <= r0 < r1 <= height without one, n_colors and
 * spread with a palette, a scale outside [1, PAR_MAX_SCALE], an order that is neither of the two, a pitch that is not a
 * multiple of 4 or is below 4 * width * sx (formed in 64 bits), params->width <= 0.
 * No overlap of `out` or `index_out` with any input is defined; `fb` and `gbuf` are only read. `gbuf`, `fb`, the palette
 * and `out` must be 4-byte aligned, `index_out` may sit on any byte; `out` on a 16-byte boundary with a pitch that is a
 * multiple of 16, and `index_out` on a 4-byte boundary of a frame whose width is a multiple of 4, take the kernel's wider
 * stores, every other placement gives the same bytes. The kernel stays inside its arrays whatever the texels and pixels
 * hold.
 * Left out on purpose: no fb_out or edge_out planes (a caller who wants the intermediates has the three calls), no second
 * palette for the present stage, no fusing into the render or light kernels, no graph-capture helper (the device call is
 * capturable as any stream-ordered launch is), and no change to what the three calls above do. */
/* device pointers (`d_palette` too), asynchronous on `stream` (a hipStream_t), no sync: on the frame's own stream, after
 * the render or relight call */
int par_finish_device(const par_params* params, void* stream,
                      const par_outline_style* style, const par_pixel* gbuf, int gbuf_row_begin, int gbuf_row_end,
                      const par_color* d_palette, int n_colors, int spread,
                      const par_present_desc* desc,
                      const par_color* fb, int row_begin, int row_end,
                      void* out, uint8_t* index_out);
/* host pointers, synchronous, everything on HIP device `device` (-1: the current device, as par_create): allocates,
 * copies, launches, synchronises, copies back (`out` with a pitched copy: the caller's gap bytes stay) and frees;
 * PAR_ERR_NO_DEVICE / PAR_ERR_OOM / PAR_ERR_HIP as par_present_host */
int par_finish_host(const par_params* params, int device,
                    const par_outline_style* style, const par_pixel* gbuf, int gbuf_row_begin, int gbuf_row_end,
                    const par_color* palette, int n_colors, int spread,
                    const par_present_desc* desc,
                    const par_color* fb, int row_begin, int row_end,
                    void* out, uint8_t* index_out);

/* --- upscale: a frame or an index plane through a pixel-art scaler (nothing in the reference) ----------------------
 * At an integer scale of 2 to 4 a pixel-art frame is normally shown through an EPX-family scaler: Scale2x (AdvMAME2x),
 * Scale3x, Scale4x. For every output pixel such a scaler SELECTS the source pixel under it or one of that pixel's four
 * neighbours: hard edges and the palette stay, the staircase on the diagonals goes. It never makes a colour, so it
 * works on an index plane too, and the scaled index plane can be palette-cycled with par_present_device. These calls
 * are a pass over finished planes and take no context: retained frames, graphs and statistics are not involved and do
 * not change. Everything is in integers and byte for byte; k = desc->scaler is the factor, W = params->width.
 * Sources. Exactly one of `fb` and `index` is non-null. It addresses (src_row_begin, column 0) and holds rows [s0, s1) =
 * [src_row_begin, src_row_end), dense and row-major as every plane is, and is only read. The output rows are [r0, r1) =
 * [row_begin, row_end) with 0 <= s0 <= r0 < r1 <= s1 <= height, the halo rule of par_outline_device. Two elements are
 * EQUAL iff their 32-bit words are equal with an fb source (the alpha byte counts, as in the changed-tiles calls), or
 * their raw bytes with an index source: the comparison comes before any palette clamp, so the indices 200 and 255 over
 * a 4-entry palette are different elements that show the same colour.
 * Neighbourhood. For the source element E at column x and absolute row y, the element at offset (dx, dy) is read at
 * column clamp(x + dx, 0, W - 1) and row clamp(y + dy, s0, s1 - 1). The nine, row by row, are A B C / D E F / G H I:
 * B above E, D left, F right, H below.
 * Scale2x (k = 2). With g = (B != H && D != F), the 2 x 2 block of E, row by row:
 *     E0 = g && D == B ? D : E        E1 = g && B == F ? F : E
 *     E2 = g && D == H ? D : E        E3 = g && H == F ? F : E
 * Scale3x (k = 3). With the same g, the 3 x 3 block of E, row by row:
 *     E0 = g && D == B ? D : E
 *     E1 = g && ((D == B && E != C) || (B == F && E != A)) ? B : E
 *     E2 = g && B == F ? F : E
 *     E3 = g && ((D == B && E != G) || (D == H && E != A)) ? D : E
 *     E4 = E
 *     E5 = g && ((B == F && E != I) || (H == F && E != C)) ? F : E
 *     E6 = g && D == H ? D : E
 *     E7 = g && ((D == H && E != I) || (H == F && E != G)) ? H : E
 *     E8 = g && H == F ? F : E
 * Scale4x (k = 4). T is the Scale2x result of the source rows [s0, s1): a plane of 2 * W columns and rows
 * [2 * s0, 2 * s1). The output is the Scale2x result of T, with T's own column clamp to [0, 2 * W - 1] and row clamp to
 * [2 * s0, 2 * s1 - 1]. T is never written to memory.
 * Output. The output element (X, Y), 0 <= X < k * W and k * r0 <= Y < k * r1, is sub-element (X % k, Y % k) of the block
 * of the source element (X / k, Y / k): call it e; it is always one of the source's elements.
 *     index_out (an index source only; nullable; dense, k * W bytes a row; addresses output row k * r0) gets the raw byte e
 *     out (nullable; a surface exactly as par_present_device's: it addresses output row k * r0, byte 0, rows desc->pitch
 *         bytes apart, pixel X at byte 4 * X; the bytes from 4 * k * W up to the pitch are NOT written) gets the 4 bytes of
 *         c, red and blue exchanged under PAR_PRESENT_BGRA: c = e with an fb source, c = palette[min(e, n_colors - 1)]
 *         with an index source, all four bytes, as present does
 * At least one of `out` and `index_out` is non-null. The palette is required (1 <= n_colors <= PAR_MAX_PALETTE) exactly
 * when the source is `index` and `out` is non-null; otherwise it must be NULL with n_colors 0.
 * Row blocks. A block's output equals those output rows of the whole frame's, byte for byte, when the source block
 * carries a halo wherever those rows exist in the frame: 1 row on each side for k = 2 and 3, 2 rows for k = 4
 * (s0 = max(0, r0 - halo), s1 = min(height, r1 + halo)). A shorter halo is defined behaviour, the clamp, not an error.
 * PAR_ERR_INVALID_ARG, before any device work and with nothing written (no GPU is needed to get it), for a null
 * `params` or `desc`; both sources or neither; both outputs null; index_out with an fb source; the palette pairing above
 * broken; a scaler that is none of the three; params->width <= 0; rows that are not 0 <= s0 <= r0 < r1 <= s1 <= height;
 * and, when `out` is non-null (otherwise the pitch and the order are not read), an order that is neither of the two or a
 * pitch that is not a multiple of 4 or is below 4 * W * k (formed in 64 bits: a product that does not fit an int32 is
 * thereby refused).
 * No overlap of an output with a source is defined. `fb`, the palette and `out` must be 4-byte aligned; `index` and
 * `index_out` may sit on any byte. `out` on a 16-byte boundary with a pitch that is a multiple of 16, and `index_out` on
 * a 4-byte boundary with k * W a multiple of 4, take the kernel's wider stores; every placement gives the same bytes. The
 * kernel stays inside its arrays whatever the planes hold.
 * Left out on purpose: no other scalers (hqx, xBR, Eagle: they blend colours, which an index plane cannot hold), no
 * factor above 4, no nearest-neighbour magnification on top in the same call (the caller presents index_out, or a
 * surface, with a par_params of the scaled width), no fusing into par_finish_device, no graph-capture helper (the device
 * call is capturable as any stream-ordered launch is), and no change to what present or finish do. */
/* device pointers (`d_palette` too), asynchronous on `stream` (a hipStream_t), no sync: on the frame's own stream, after
 * the last call that writes the source */
int par_upscale_device(const par_params* params, void* stream, const par_upscale_desc* desc,
                       const par_color* fb, const uint8_t* index, const par_color* d_palette, int n_colors,
                       int src_row_begin, int src_row_end, int row_begin, int row_end,
                       void* out, uint8_t* index_out);
/* host pointers, synchronous, everything on HIP device `device` (-1: the current device, as par_create): allocates,
 * copies, launches, synchronises, copies back (`out` with a pitched copy: the caller's gap bytes stay) and frees;
 * PAR_ERR_NO_DEVICE / PAR_ERR_OOM / PAR_ERR_HIP as par_present_host */
int par_upscale_host(const par_params* params, int device, const par_upscale_desc* desc,
                     const par_color* fb, const uint8_t* index, const par_color* palette, int n_colors,
                     int src_row_begin, int src_row_end, int row_begin, int row_end,
                     void* out, uint8_t* index_out);

/* Debug overlay of alt:763-772 (Bresenham line from the picked pixel to the light) drawn into a host frame. */
void par_debug_line(const par_params* params, const par_pixel* pick, int mouse_x, const par_light* light,
                    par_color* fb);

#ifdef __cplusplus
}
#endif
#endif /* PAR_RAYTRACER_H */

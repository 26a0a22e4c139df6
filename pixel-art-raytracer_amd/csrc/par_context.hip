// par_context.hip — the renderer context and the C ABI (include/par_raytracer.h) over the HIP kernels.
//
// Host-side mirror of what the reference's `main` does around its render call (alt = src/alternative.cpp):
// it owns the work arrays (alt:503-517), takes the scene the caller built (alt:517-599, 619-626), and runs one
// frame = bin + trace + shade (alt:690-760) per render call. There is no CPU rendering path in this library.
#include <algorithm>
#include <array>
#include <cmath>
#include <new>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "par_book.h"
#include "par_hostcall.h"
#include "par_internal.h"

struct par_context {
    par_params params{};
    int device = 0;
    int gx = 0, gy = 0, gz = 0, volume = 0;
    hipStream_t stream = nullptr;   // used by the synchronous host-buffer entry points

    par_book book;  // the host's copy of the scene and what frames are sized by (par_book.h)
    int n_entities = 0, n_sprites = 0, max_sprite_id = 0;
    bool have_entities = false;
    par_light lights[PAR_MAX_LIGHTS]{};  // set_lights; n_lights >= 2 (or the test hook) takes the light kernel
    int n_lights = 0;                    // 0 until a light is set
    int depth_min = 0, depth_max = 0;    // least and largest texel depth of the sprite table (par_set_sprites)
    int light_model = PAR_LIGHTS_UNBOUNDED;  // par_set_light_model; PAR_LIGHTS_RANGED always takes the light kernel
    bool tinted = false;                 // par_set_light_tints; a tinted context always takes the light kernel
    par_light_tints tints{};             // by light index (white beyond those the call named); read while `tinted`
    int set = 0;  // head/count/node set the NEXT frame uses
    // The retained frame (par_relight_device, the contract beside it): the rows of the last frame whose hash build is
    // still what the device holds, its grid set, and whether it was a par_render / par_render_rows frame with a gbuf
    // plane (which d_out[1] then still holds: par_relight_rows). Nothing of the frame itself is stored.
    struct {
        bool valid = false;
        int r0 = 0, r1 = 0, set = 0;
        bool host_gbuf = false;
    } kept;
    // The drawn-into record (PAR_RENDER_KEPT_OUTPUTS): the frame and palette-index planes, the rows and the grid set of
    // the last frame par_render_device[_timed] enqueued as a production frame makes its launches, while the other grid
    // set still holds that frame's node list. Unlike `kept` it outlives a change of the scene: the next build's wipe
    // walks the nodes of the frame that was drawn, whatever the scene has become since.
    struct {
        bool valid = false;
        const void* fb = nullptr;
        const void* palidx = nullptr;
        int r0 = 0, r1 = 0, set = 0;
    } drawn;
    // What a kept frame clears by: book.dirty holds the entities rewritten since the last enqueued frame (fed by every
    // scene change that goes through the book, marked whole by drop_drawn and par_set_sprites, emptied by enqueue_frame),
    // and every frame takes the next sequence number (par_dirty_dev::seq; from 1, never 0).
    uint32_t frame_seq = 0;
    hipStream_t last_stream = nullptr;  // stream of the most recent asynchronous render (scene updates wait for it)
    bool has_last_stream = false;

    // device
    par_aabb* d_aabbs = nullptr;
    int32_t* d_sprite_ids = nullptr;
    par_sprite* d_sprites = nullptr;
    par_color* d_palette = nullptr;
    par_texel* d_texinfo = nullptr;
    unsigned long long* d_ray_counter = nullptr;
    uint8_t* d_scratch_lit = nullptr;  // lit plane when every ray is traced but the caller wants no lit plane
    size_t scratch_lit_bytes = 0;
    par_grid_dev grid{};
    int aabb_capacity = 0;

    // device output planes for the host-buffer entry points
    uint8_t* d_out[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    size_t d_out_bytes[5] = {0, 0, 0, 0, 0};

    // hipGraph path: one executable graph per grid set, a pinned staging area they copy from
    hipGraphExec_t graph_exec[2] = {nullptr, nullptr};
    hipGraph_t graph[2] = {nullptr, nullptr};
    // Each graph copies the scene (AABBs into d_aabbs, the lights into d_lights) from a pinned staging area of its own
    // (the copy nodes read it when the graph RUNS, which may be long after it was launched): the area of set s is
    // rewritten only after the event recorded behind set s's last launch. `stage_lo/hi`: entities changed since the
    // area last matched the host mirror.
    par_aabb* pin_aabbs[2] = {nullptr, nullptr};
    int pin_aabbs_capacity[2] = {0, 0};  // entities each holds: they grow with aabb_capacity when a graph is captured
    par_lights_block* pin_lights[2] = {nullptr, nullptr};
    hipEvent_t ev_graph[2] = {nullptr, nullptr};
    bool ev_graph_pending[2] = {false, false};
    int stage_lo[2] = {0, 0}, stage_hi[2] = {0, 0};
    // Entities par_graph_stage changed that d_aabbs does not hold yet: the next graph launch uploads the whole scene; a
    // frame that is not a graph's uploads them itself first (its launches are sized by the staged scene).
    int dev_lo = 0, dev_hi = 0;
    par_aabb* pin_update = nullptr;   // staging of par_update_aabbs_async
    int pin_update_capacity = 0;
    hipEvent_t ev_update = nullptr;   // its last copy
    bool ev_update_pending = false;
    hipStream_t update_stream = nullptr;
    // The captured kernels read the frame's lights from d_lights (a one-light graph's from the first light alone).
    bool graph_lights = false;  // which kernels were captured: false one-light (par_graph_capture), true light path
                                // (then of the light model and the tinted state the context had, which only change
                                // with the graphs dropped)
    par_lights_block* d_lights = nullptr;

    bool timed_tiles = false, timed_overflow = false, timed_both = false;  // the last timed frame launched these kernels
    hipEvent_t ev[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};  // EV_START .. EV_END
    par_frame_stats stats{};
    unsigned last_flags = 0;
    std::string err;
    // test hooks (par_debug_set_hooks), read when a frame is enqueued; 0 and 0 in production
    unsigned hooks = 0;
    int col_roles = 0;  // wavefronts per column of the column launch, 0 = its own choice
};

// par_debug_set_hooks's bits
enum : unsigned {
    PAR_HOOK_FORCE_GENERIC = 1u << 0,  // every column through render_overflow_kernel (par_render_args::dense)
    PAR_HOOK_TWO_LAUNCHES = 1u << 1,   // the hash build always takes two launches
    PAR_HOOK_RECORD_ITEMS = 1u << 2,   // columns emit no self-contained and no alone work items (PAR_FLAG_RECORD_ITEMS)
    PAR_HOOK_LOSE_BUILD_WG = 1u << 3,  // build workgroup 0 never arrives at the one-launch build's barrier
    PAR_HOOK_BAD_ALLOC = 1u << 4,      // the guarded host-allocating bodies fail as an exhausted heap would
    PAR_HOOK_LIGHTS_PATH = 1u << 5,    // a one-light frame takes the path of several lights (render_lights_kernel)
    PAR_HOOKS_ALL = (1u << 6) - 1
};

// The events of a timed frame (par_context::ev), in the order a frame records them.
enum : int {
    EV_START,
    EV_BUILT,     // after the hash build
    EV_COLUMNS,   // after the column launch (a frame with several lights has none: with EV_BUILT)
    EV_FILLED,    // after the background fill
    EV_ITEMS,     // after the render launch of the work items (or of all render kernels, or the light kernel)
    EV_RENDERED,  // after the render launches
    EV_END        // after the launch for the overflow list
};

namespace {

constexpr size_t kPlaneElem[5] = {sizeof(par_color), sizeof(par_pixel), 1, sizeof(float), 1};
// A frame takes the kept path (PAR_RENDER_KEPT_OUTPUTS) only while its column bound is at most this share of the tiles
// of its rows (measured).
constexpr int64_t kKeptMaxTilesPct = 50;

int fail(par_context* c, int status, const std::string& msg) {
    if (c) {
        try {
            c->err = msg;
        } catch (...) {  // (the message is a convenience; the status is the contract)
        }
    }
    return status;
}

// No exception crosses the C boundary (par_raytracer.h): every entry point that allocates on the host runs its
// body through this. PAR_HOOK_BAD_ALLOC (tests) makes the guarded bodies fail as an exhausted heap would.
void test_alloc_hook(const par_context* c) {
    if (c->hooks & PAR_HOOK_BAD_ALLOC) throw std::bad_alloc();
}

template <class F>
int guarded(par_context* ctx, F&& body) noexcept {
    try {
        return body();
    } catch (const std::bad_alloc&) {
        return fail(ctx, PAR_ERR_OOM, "host allocation failed");
    } catch (...) {
        return fail(ctx, PAR_ERR_HIP, "unexpected C++ exception");
    }
}

// The retained frame: `set` is the grid set the frame that just returned PAR_OK was built in; and its end (a hash build
// was enqueued or the scene changed, see par_raytracer.h).
void retain_frame(par_context* c, int row_begin, int row_end, int set, bool host_gbuf) {
    c->kept.valid = true;
    c->kept.r0 = row_begin;
    c->kept.r1 = row_end;
    c->kept.set = set;
    c->kept.host_gbuf = host_gbuf;
}
void drop_retained(par_context* c) { c->kept.valid = false; }

// The drawn-into record: made where a frame is retained (the frame of grid set `set` was enqueued whole, into `out`),
// dropped wherever something else may have written the planes or the other set's node list is no longer that frame's.
void record_drawn(par_context* c, const par_outputs& out, int row_begin, int row_end, int set) {
    c->drawn.valid = true;
    c->drawn.fb = out.fb;
    c->drawn.palidx = out.palidx;
    c->drawn.r0 = row_begin;
    c->drawn.r1 = row_end;
    c->drawn.set = set;
}
// (whatever ends the record may have changed the planes or the node list: the next frame treats every entity as rewritten)
void drop_drawn(par_context* c) {
    c->drawn.valid = false;
    c->book.dirty.mark_all();
}

int hip_fail(par_context* c, hipError_t e, const char* what) {
    return fail(c, e == hipErrorOutOfMemory ? PAR_ERR_OOM : PAR_ERR_HIP,
                std::string(what) + ": " + hipGetErrorString(e));
}

#define PAR_HIP(call)                                        \
    do {                                                     \
        hipError_t e_ = (call);                              \
        if (e_ != hipSuccess) return hip_fail(ctx, e_, #call); \
    } while (0)

bool extent_ok(const par_aabb& a) {
    // The sprite is 20 wide and 40 tall (alt:330, spr:67-71): texel row = (ey + ez) - 1 at most, column < ex.
    return a.ex >= 0 && a.ey >= 0 && a.ez >= 0 && a.ex <= PAR_SPRITE_W && (int)a.ey + (int)a.ez <= PAR_SPRITE_H;
}

// The checks of an update of entities [first, first + n) (par_update_aabbs[_async], par_graph_stage): a range outside
// the uploaded entities or no AABBs is PAR_ERR_INVALID_ARG (the stage takes NULL with n == 0: `null_ok`), then an
// extent the sprite cannot take PAR_ERR_EXTENT.
int check_update(par_context* ctx, const par_aabb* aabbs, int first, int n, bool null_ok) {
    if (first < 0 || n < 0 || !ctx->have_entities || first + n > ctx->n_entities || (!aabbs && !(null_ok && n == 0))) {
        return fail(ctx, PAR_ERR_INVALID_ARG, null_ok ? "stage range" : "update range outside the uploaded entities");
    }
    for (int i = 0; i < n; i++) {
        if (!extent_ok(aabbs[i])) return fail(ctx, PAR_ERR_EXTENT, "extent needs 0<=ex<=20, ey,ez>=0, ey+ez<=40");
    }
    return PAR_OK;
}

// *p replaced by a fresh buffer of n elements, in device memory or (`pinned`) pinned host memory; the old contents
// are not kept. *p is null until the new buffer is there.
template <class T>
hipError_t reallocate(T** p, size_t n, bool pinned = false) {
    if (*p) {
        const hipError_t e = pinned ? hipHostFree(*p) : hipFree(*p);
        if (e != hipSuccess) return e;
    }
    *p = nullptr;
    const size_t bytes = n * sizeof(T);
    return pinned ? hipHostMalloc((void**)p, bytes, hipHostMallocDefault) : hipMalloc((void**)p, bytes);
}

// Grow-on-demand memory: reallocate, with the capacity the caller keeps for the buffer (*cap) 0 until the new one of
// n elements is there.
template <class T, class N>
hipError_t grow(T** p, N* cap, N n, bool pinned = false) {
    *cap = 0;
    const hipError_t e = reallocate(p, (size_t)n, pinned);
    if (e == hipSuccess) *cap = n;
    return e;
}

void free_pool(par_context* c) {
    for (int s = 0; s < 2; s++) {
        if (c->grid.node_entity[s]) (void)hipFree(c->grid.node_entity[s]);
        if (c->grid.node_next[s]) (void)hipFree(c->grid.node_next[s]);
        if (c->grid.node_bin[s]) (void)hipFree(c->grid.node_bin[s]);
        c->grid.node_entity[s] = c->grid.node_next[s] = c->grid.node_bin[s] = nullptr;
    }
    if (c->grid.colrec) (void)hipFree(c->grid.colrec);
    c->grid.colrec = nullptr;
    c->grid.col_capacity = 0;
    c->grid.capacity = 0;
}

// Wipe both head/count sets and the node counters (context creation, and whenever the node pool is replaced and
// the record of which bins the previous frame touched is lost with it).
int reset_grid(par_context* ctx) {
    for (int s = 0; s < 2; s++) {
        PAR_HIP(hipMemsetAsync(ctx->grid.head[s], 0, (size_t)ctx->volume * sizeof(int32_t), ctx->stream));
        PAR_HIP(hipMemsetAsync(ctx->grid.count[s], 0, (size_t)ctx->volume, ctx->stream));
        PAR_HIP(hipMemsetAsync(ctx->grid.colflag[s], 0, (size_t)ctx->gx * ctx->gy * sizeof(int32_t), ctx->stream));
    }
    PAR_HIP(hipMemsetAsync(ctx->grid.counters, 0, PAR_CNT_TOTAL * sizeof(int32_t), ctx->stream));
    PAR_HIP(hipMemsetAsync(ctx->grid.node_counter, 0, 2 * sizeof(int32_t), ctx->stream));
    PAR_HIP(hipStreamSynchronize(ctx->stream));
    ctx->set = 0;
    drop_drawn(ctx);  // (the node list of the last frame is gone: nothing says which tiles it drew into)
    return PAR_OK;
}

int ensure_pool(par_context* ctx, int64_t pairs) {
    if (pairs <= ctx->grid.capacity) return PAR_OK;
    if (ctx->graph_exec[0]) return fail(ctx, PAR_ERR_UNSUPPORTED, "node pool would grow under a captured graph; capture again");
    int64_t cap = std::max<int64_t>(pairs + pairs / 2, 1 << 16);
    if (cap > 0x3FFFFFFF) return fail(ctx, PAR_ERR_UNSUPPORTED, "too many (entity, bin) pairs");
    PAR_HIP(hipDeviceSynchronize());
    free_pool(ctx);
    for (int s = 0; s < 2; s++) {
        PAR_HIP(hipMalloc(&ctx->grid.node_entity[s], (size_t)cap * sizeof(int32_t)));
        PAR_HIP(hipMalloc(&ctx->grid.node_next[s], (size_t)cap * sizeof(int32_t)));
        PAR_HIP(hipMalloc(&ctx->grid.node_bin[s], (size_t)cap * sizeof(int32_t)));
    }
    // occupied columns <= (entity, bin) pairs: one column record each
    const int64_t col_cap = std::min<int64_t>((int64_t)ctx->gx * ctx->gy, cap);
    PAR_HIP(hipMalloc(&ctx->grid.colrec, (size_t)col_cap * sizeof(par_colrec)));
    ctx->grid.col_capacity = (int32_t)col_cap;
    ctx->grid.capacity = (int32_t)cap;
    return reset_grid(ctx);
}

// Device memory for a frame of `b`: the node pool, then the render work-item list (par_book::items_per_shard).
int ensure_room(par_context* ctx, const par_bound& b) {
    const int rc = ensure_pool(ctx, b.pairs);
    if (rc != PAR_OK) return rc;
    const int64_t need = ctx->book.items_per_shard(b.items, b.cols);
    if (need <= ctx->grid.item_capacity) return PAR_OK;
    if (ctx->graph_exec[0]) return fail(ctx, PAR_ERR_UNSUPPORTED, "work-item list would grow under a captured graph; capture again");
    const int64_t cap = std::max<int64_t>(need + need / 2, 1 << 10);
    if (cap > 0x3FFFFFFF / (PAR_ITEM_LISTS * PAR_ITEM_SHARDS)) return fail(ctx, PAR_ERR_UNSUPPORTED, "too many render work items");
    PAR_HIP(hipDeviceSynchronize());
    if (ctx->grid.items) PAR_HIP(hipFree(ctx->grid.items));
    ctx->grid.items = nullptr;
    ctx->grid.item_capacity = 0;
    PAR_HIP(hipMalloc(&ctx->grid.items, (size_t)cap * PAR_ITEM_LISTS * PAR_ITEM_SHARDS * sizeof(par_item)));
    ctx->grid.item_capacity = (int32_t)cap;
    return PAR_OK;
}

void drop_graphs(par_context* c) {
    for (int s = 0; s < 2; s++) {
        if (c->graph_exec[s]) (void)hipGraphExecDestroy(c->graph_exec[s]);
        if (c->graph[s]) (void)hipGraphDestroy(c->graph[s]);
        c->graph_exec[s] = nullptr;
        c->graph[s] = nullptr;
    }
}

// Entities [first, first + n) changed on the host: both graphs' staging areas are stale there.
void mark_staged(par_context* c, int first, int n) {
    if (n <= 0) return;
    for (int s = 0; s < 2; s++) {
        if (c->stage_hi[s] <= c->stage_lo[s]) {
            c->stage_lo[s] = first;
            c->stage_hi[s] = first + n;
        } else {
            c->stage_lo[s] = std::min(c->stage_lo[s], first);
            c->stage_hi[s] = std::max(c->stage_hi[s], first + n);
        }
    }
}

par_frame_dyn make_dyn(const par_context* c, const par_light& l) {
    const int B = c->params.bin_size, H = c->params.height;
    par_frame_dyn d;
    d.lx = l.x; d.ly = l.y; d.lz = l.z;
    d.lbx = l.x / B;                // alt:729
    d.lby = (H - l.y - l.z) / B;    // alt:730-731
    d.lbz = l.z / B;                // alt:732
    return d;
}

// The context's light set: lights[0, n) replaced, `count` lights in all (par_graph_stage replaces the first alone and
// keeps the count).
void set_lights(par_context* c, const par_light* lights, int n, int count) {
    for (int l = 0; l < n; l++) c->lights[l] = lights[l];
    c->n_lights = count;
}

// What every entry point that renders or captures a frame checks first, in this order, then the context's device.
int frame_prologue(par_context* ctx, const par_outputs* out, int row_begin, int row_end, unsigned flags) {
    if (!ctx || !out) return fail(ctx, PAR_ERR_INVALID_ARG, "null argument");
    if (flags & ~PAR_ACCEPTED_FLAGS) return fail(ctx, PAR_ERR_INVALID_ARG, "undefined render flag bits");
    if (row_begin < 0 || row_end > ctx->params.height || row_begin >= row_end) {
        return fail(ctx, PAR_ERR_INVALID_ARG, "rows must satisfy 0 <= row_begin < row_end <= height");
    }
    if (ctx->n_sprites <= 0) return fail(ctx, PAR_ERR_NOT_READY, "par_set_sprites has not been called");
    if (!ctx->have_entities) return fail(ctx, PAR_ERR_NOT_READY, "par_set_entities has not been called");
    if (ctx->n_lights <= 0) return fail(ctx, PAR_ERR_NOT_READY, "par_set_light has not been called");
    if (ctx->max_sprite_id >= ctx->n_sprites) return fail(ctx, PAR_ERR_SPRITE_ID, "an entity names a sprite that was not uploaded");
    PAR_HIP(hipSetDevice(ctx->device));
    return PAR_OK;
}

par_render_args make_render_args(const par_context* c, int set, int row_begin, int row_end, const par_outputs& out,
                                 unsigned flags, bool dyn_from_device) {
    par_render_args a{};
    const int B = c->params.bin_size;
    a.W = c->params.width; a.H = c->params.height; a.B = B;
    a.row_begin = row_begin; a.row_end = row_end;
    a.by_lo = row_begin / B;
    a.by_hi = (row_end - 1) / B;
    a.set = set;
    // every ray traced (as the reference does), or the lit plane requested
    a.trace_bg = ((flags & PAR_RENDER_TRACE_BACKGROUND) || out.lit) ? 1 : 0;
    a.dense = (c->hooks & PAR_HOOK_FORCE_GENERIC) ? 1 : 0;
    a.magic_b = (uint32_t)((1ull << 32) / (uint64_t)B + 1ull);
    a.ambient = c->params.ambient;
    a.background = c->params.background;
    a.flags = flags | ((c->hooks & PAR_HOOK_RECORD_ITEMS) ? PAR_FLAG_RECORD_ITEMS : 0u);
    // Columns are visited as whole tiles only in DENSE frames, which get a launch for the tile items: enough columns
    // (a 64th of the grid, at least 16) whose entities' rectangles add up to the tile (the column kernel's own
    // criterion, over the visible entries). A frame with fewer visits every column entry by entry (tile_k 0) and keeps
    // its three launches. A captured graph serves later frames too: it always has the launch. Then: how many chunks
    // per tile item -- a frame with many lets a wavefront read what a column's chunks share once for several of them,
    // a frame with few needs every wavefront it can get. (Both can lag behind the scene, see par_book::dense.)
    const bool dense_frame = dyn_from_device || c->book.dense();
    const int64_t chunks = c->book.chunks();
    a.tile_k = !dense_frame ? 0 : (chunks >= 65536 ? 5 : (chunks >= 16384 ? 3 : (chunks >= 8192 ? 2 : 1)));
    a.tile_k_magic = a.tile_k > 0 ? (uint32_t)(65536 / a.tile_k + 1) : 65537u;
    a.dyn = make_dyn(c, c->lights[0]);
    a.dyn_ptr = dyn_from_device ? &c->d_lights->lights.l[0] : nullptr;
    a.count = c->grid.count[set];
    a.slots = c->grid.slots;
    a.sprites = c->d_sprites;
    a.texinfo = c->d_texinfo;
    a.sprite_ids = c->d_sprite_ids;
    a.palette = c->d_palette;
    a.out = out;
    a.ray_counter = c->d_ray_counter;
    return a;
}

par_bin_args make_bin_args(const par_context* c, int set, int row_begin, int row_end, unsigned flags) {
    par_bin_args b{};
    b.flags = flags;
    b.by_lo = row_begin / c->params.bin_size;
    b.by_hi = (row_end - 1) / c->params.bin_size;
    b.W = c->params.width; b.H = c->params.height; b.L = c->params.length; b.B = c->params.bin_size;
    b.n = c->n_entities;
    b.set = set;
    b.aabbs = c->d_aabbs;
    b.magic_b = (uint32_t)((1ull << 32) / (uint64_t)c->params.bin_size + 1ull);
    // tests: a build workgroup that never arrives at the one-launch hash build's barrier (PAR_ERR_DEVICE)
    b.test_lose_wg = (c->hooks & PAR_HOOK_LOSE_BUILD_WG) ? 1 : 0;
    return b;
}

// The kernels' sticky failure word (PAR_CNT_ERROR), read after a wait for the device: reported once (PAR_ERR_DEVICE)
// and cleared. The caller has synchronised with the frames it is asking about.
int check_device_error(par_context* ctx) {
    int32_t word = 0;
    PAR_HIP(hipMemcpy(&word, ctx->grid.counters + PAR_CNT_ERROR, sizeof(word), hipMemcpyDeviceToHost));
    if (word == 0) return PAR_OK;
    PAR_HIP(hipMemset(ctx->grid.counters + PAR_CNT_ERROR, 0, sizeof(word)));
    drop_retained(ctx);
    drop_drawn(ctx);
    std::string what;
    if (word & PAR_DEVERR_BARRIER) {
        what += "the hash build's barrier timed out (a build workgroup never arrived); ";
    }
    if (word & PAR_DEVERR_OVERFLOW) {
        what += "a column overflowed its record in a frame enqueued without a launch for the overflow list; ";
    }
    return fail(ctx, PAR_ERR_DEVICE, what + "a frame rendered since the last check is not valid");
}

// A frame takes the light kernel when it has several lights, or ranged or tinted ones (or the test hook asks for it with
// one).
bool ranged(const par_context* c) { return c->light_model == PAR_LIGHTS_RANGED; }
bool lights_path(const par_context* c) {
    return c->n_lights > 1 || ranged(c) || c->tinted || (c->hooks & PAR_HOOK_LIGHTS_PATH);
}

// The context's lights as they are now: positions and bins, radii (<= 0: unbounded; the lights the context does not have
// read as that) and tints.
par_lights_block make_lights_block(const par_context* c) {
    par_lights_block b{};
    b.lights.n = c->n_lights;
    for (int l = 0; l < c->n_lights; l++) {
        b.lights.l[l] = make_dyn(c, c->lights[l]);
        b.radii.r[l] = c->lights[l].radius;
    }
    b.radii.depth_min = c->depth_min;
    b.radii.depth_max = c->depth_max;
    b.tints = c->tints;
    return b;
}

// What the light kernels of a frame enqueued now read: a ranged context (PAR_LIGHTS_RANGED) takes the ranged kernels, a
// tinted one (par_set_light_tints) the tinted light kernel, and in graph mode they read the lights from d_lights, which
// the graph's copy node fills before them.
par_light_state make_light_state(const par_context* c, bool graph_mode) {
    return {make_lights_block(c), ranged(c), c->tinted, graph_mode ? c->d_lights : nullptr};
}

// Staging area `s` of the captured graphs: the context's lights as they are now.
void stage_lights(par_context* c, int s) { *c->pin_lights[s] = make_lights_block(c); }

// The hash build: small scenes in one launch, large ones in two (and frames that keep their kernels `apart`, and the
// test hook). `fa`, `fill`: the share of the background fill that rides along, if any.
int enqueue_build(par_context* ctx, hipStream_t stream, const par_bin_args& b, int64_t pair_bound,
                  const par_render_args* fa, const par_fill_plan* fill, bool apart) {
    const bool two_launches = apart || (ctx->hooks & PAR_HOOK_TWO_LAUNCHES);
    const hipError_t be = two_launches ? hipErrorNotSupported : par_launch_build(ctx->grid, b, pair_bound, fa, fill, stream);
    if (be == hipErrorNotSupported) {
        PAR_HIP(par_launch_bin_insert(ctx->grid, b, fa, fill, stream));
        PAR_HIP(par_launch_bin_resolve(ctx->grid, b, pair_bound, fa, fill, stream));
    } else if (be != hipSuccess) {
        return hip_fail(ctx, be, "par_launch_build");
    }
    return PAR_OK;
}

// A frame with several lights: the hash build, the background fill (after the background rays when they are wanted)
// and one launch of the light kernel over the occupied columns. No column records, no work items, no overflow list.
// Timed frames bracket the launches with the same events as enqueue_frame: the light kernel is ms_render and
// ms_launch[2]; the other render launches it does not have are 0. In graph mode (par_graph_capture_lights) the
// launches are sized by what the graph accepts (par_book::graph) and the kernels read the lights from d_lights, which
// the graph's copy node fills before them: one graph serves any count of lights. A ranged context (PAR_LIGHTS_RANGED)
// launches the ranged kernels, with the radii beside the lights; a tinted one (par_set_light_tints) the tinted light
// kernel, with the tints behind them.
int enqueue_lights_frame(par_context* ctx, hipStream_t stream, const par_bin_args& b, const par_render_args& r,
                         const par_bound& bound, bool graph_mode, bool apart, hipEvent_t* ev) {
    const par_light_state lights = make_light_state(ctx, graph_mode);
    const int rc = enqueue_build(ctx, stream, b, bound.pairs, &r, nullptr, apart);
    if (rc != PAR_OK) return rc;
    if (ev) {
        PAR_HIP(hipEventRecord(ev[EV_BUILT], stream));
        PAR_HIP(hipEventRecord(ev[EV_COLUMNS], stream));
    }
    if (r.trace_bg) PAR_HIP(par_launch_bglights(ctx->grid, r, lights, stream));
    PAR_HIP(par_launch_fill(ctx->grid, r, stream));
    if (ev) PAR_HIP(hipEventRecord(ev[EV_FILLED], stream));
    PAR_HIP(par_launch_render_lights(ctx->grid, r, lights, bound.cols, stream));
    if (ev) {
        PAR_HIP(hipEventRecord(ev[EV_ITEMS], stream));
        PAR_HIP(hipEventRecord(ev[EV_RENDERED], stream));
        PAR_HIP(hipEventRecord(ev[EV_END], stream));
        ctx->timed_tiles = false;
        ctx->timed_overflow = false;
        ctx->timed_both = false;
    }
    return PAR_OK;
}

// Enqueue one frame (alt:690-760) on `stream` using grid set `set`.
int enqueue_frame(par_context* ctx, hipStream_t stream, int set, int row_begin, int row_end, const par_outputs& out,
                  unsigned flags, bool graph_mode, hipEvent_t* ev) {
    // PAR_RENDER_KEPT_OUTPUTS holds only against the record of this context's last frame: the same frame and
    // palette-index planes (given or not), the same rows, drawn by the frame whose nodes this frame's build wipes.
    const bool drawn_match = ctx->drawn.valid && ctx->drawn.fb == out.fb && ctx->drawn.palidx == out.palidx &&
                             ctx->drawn.r0 == row_begin && ctx->drawn.r1 == row_end && ctx->drawn.set == (set ^ 1);
    drop_retained(ctx);  // (a hash build follows; the entry point retains the new frame once it has returned PAR_OK)
    if (ctx->dev_hi > ctx->dev_lo && !graph_mode) ctx->book.dirty.add(ctx->dev_lo, ctx->dev_hi - ctx->dev_lo);  // (staged, copied below)
    // The entities rewritten since the context's last frame; the set starts again with this frame, whichever path it takes.
    const par_dirty_set dirty = ctx->book.dirty;
    drop_drawn(ctx);
    ctx->book.dirty.clear();
    if (++ctx->frame_seq == 0) ctx->frame_seq = 1;
    par_outputs outs = out;
    if ((flags & PAR_RENDER_TRACE_BACKGROUND) && !outs.lit) {
        // every ray is to be traced but the caller wants no lit plane: the results still go to memory (a scratch
        // plane of the context), so the work is real and can be inspected
        const size_t need = (size_t)(row_end - row_begin) * ctx->params.width;
        if (ctx->scratch_lit_bytes < need) {
            if (graph_mode) return fail(ctx, PAR_ERR_NOT_READY, "render once with PAR_RENDER_TRACE_BACKGROUND before capturing it");
            PAR_HIP(grow(&ctx->d_scratch_lit, &ctx->scratch_lit_bytes, need));
        }
        outs.lit = ctx->d_scratch_lit;
    }
    // an asynchronous scene update on another stream: this frame comes after it
    if (ctx->ev_update_pending && ctx->update_stream != stream && !graph_mode) {
        PAR_HIP(hipStreamWaitEvent(stream, ctx->ev_update, 0));
    }
    if (ctx->dev_hi > ctx->dev_lo && !graph_mode) {  // staged for a graph, but this frame is none
        PAR_HIP(hipMemcpyAsync(ctx->d_aabbs + ctx->dev_lo, ctx->book.aabbs.data() + ctx->dev_lo,
                               (size_t)(ctx->dev_hi - ctx->dev_lo) * sizeof(par_aabb), hipMemcpyHostToDevice, stream));
        ctx->dev_lo = ctx->dev_hi = 0;
    }
    par_bin_args b = make_bin_args(ctx, set, row_begin, row_end, flags);
    par_render_args r = make_render_args(ctx, set, row_begin, row_end, outs, flags, graph_mode);
    r.seq = ctx->frame_seq;
    // (a timed frame keeps its kernels apart unless it is asked to time the launches as a production frame makes them)
    const bool apart = ev && !(flags & PAR_RENDER_TIMED_AS_LAUNCHED);
    const par_bound bound = ctx->book.frame_bounds(graph_mode);
    if ((flags & PAR_RENDER_COUNT_RAYS) && !graph_mode) {
        PAR_HIP(hipMemsetAsync(ctx->d_ray_counter, 0, 3 * sizeof(unsigned long long), stream));
    }
    if (ev) PAR_HIP(hipEventRecord(ev[EV_START], stream));
    // (a captured graph takes the path of its kind, chosen when it is captured)
    if (graph_mode ? ctx->graph_lights : lights_path(ctx)) {
        return enqueue_lights_frame(ctx, stream, b, r, bound, graph_mode, apart, ev);
    }
    // The overflow list is empty for sure while no column has more pairs than a record holds (a captured graph also
    // serves later frames, whose columns nobody knows yet): then the frame has no launch for it, and the column
    // kernel flags the frame should a column overflow all the same.
    const bool may_overflow = graph_mode || ctx->book.may_overflow() || r.dense || apart;
    r.overflow_launched = may_overflow ? 1 : 0;
    // The background fill depends on nothing earlier in the frame and the render kernels come after all of it: when
    // it is the plain streaming one it rides along with the first three launches (timed runs keep all kernels apart
    // so that the event pairs bracket single ones).
    par_fill_plan plan;
    const bool ride = !apart && par_plan_fill(r, &plan);
    // A kept frame (PAR_RENDER_KEPT_OUTPUTS with a matching record, never a graph's frame): the planes hold this
    // context's last frame, so the build lists the tiles that frame can have drawn into and the column launch's riding
    // workgroups clear those alone; the build launches carry no fill. Only where the fill would ride and tiles are whole
    // 16-byte runs (B % 8 == 0), and while the book's column bound says the tiles are a minority of the rendered rows
    // (kKeptMaxTilesPct): a dense frame clears every tile in short rows and loses to the streaming
    // fill. The bound only chooses; what is cleared is the device's own list.
    // Of the listed tiles only those are cleared whose column holds a node of an entity rewritten since the context's
    // previous frame, in that frame's build or in this one's: the covered pixels of every other tile are the same set
    // as before, and the render launches store each of them. With NO entity rewritten (an
    // unchanged frame) nothing is listed and nothing rides: the build wipes as an unkept frame's does and the column
    // launch is the plain one, whatever the threshold says -- the alternative is a whole fill for nothing.
    const int64_t tiles_in_rows = (int64_t)ctx->gx * (r.by_hi - r.by_lo + 1);
    const bool keepable = (flags & PAR_RENDER_KEPT_OUTPUTS) && drawn_match && !graph_mode && ride && r.B % 8 == 0;
    const bool unchanged_frame = keepable && dirty.empty();
    const bool kept_frame = keepable && !unchanged_frame &&
                            std::min(bound.cols, tiles_in_rows) * 100 <= tiles_in_rows * kKeptMaxTilesPct;
    b.kept = kept_frame ? 1 : 0;
    static_assert(par_dirty_set::MAX == 4, "par_dirty_dev holds four ranges");
    if (kept_frame) {
        b.dirty.seq = r.seq;
        b.dirty.n = dirty.n;
        for (int i = 0; i < dirty.n && i < 4; i++) {
            b.dirty.lo[i] = dirty.lo[i];
            b.dirty.len[i] = (uint32_t)(dirty.hi[i] - dirty.lo[i]);
        }
    }
    par_render_args rf = r;  // what rides along: the frame and palette-index planes
    rf.out.lit = nullptr;
    const bool fills = ride && !kept_frame && !unchanged_frame;
    const int rc = enqueue_build(ctx, stream, b, bound.pairs, &rf, fills ? &plan : nullptr, apart);
    if (rc != PAR_OK) return rc;
    if (ev) PAR_HIP(hipEventRecord(ev[EV_BUILT], stream));
    if (unchanged_frame) {
        PAR_HIP(par_launch_columns(ctx->grid, rf, bound.cols, ctx->col_roles, stream));
    } else if (ride) {
        PAR_HIP(par_launch_columns_fill(ctx->grid, rf, bound.cols, plan, kept_frame, ctx->col_roles, stream));
    } else {
        PAR_HIP(par_launch_columns(ctx->grid, r, bound.cols, ctx->col_roles, stream));
    }
    if (ev) PAR_HIP(hipEventRecord(ev[EV_COLUMNS], stream));
    // Otherwise the fill follows on the same stream. (Forking it onto a second stream beside the build was measured
    // slower, alone and with several frames in flight: the cross-stream events cost more than the overlap gains.)
    // It follows the column kernels because, when background rays are traced, it copies their results into the lit
    // plane.
    if (!ride) {
        PAR_HIP(par_launch_fill(ctx->grid, r, stream));
    } else if (r.out.lit) {  // the lit plane of the background: after the background rays
        par_render_args rl = r;
        rl.out.fb = nullptr;
        rl.out.palidx = nullptr;
        PAR_HIP(par_launch_fill(ctx->grid, rl, stream));
    }
    if (ev) PAR_HIP(hipEventRecord(ev[EV_FILLED], stream));
    // work items <= what the entities can cause one by one, and <= every column of the rendered rows as a whole tile
    const int64_t item_cap_rows = ctx->book.max_items() / ctx->gy * (r.by_hi - r.by_lo + 1);
    const int64_t item_bound = std::min(bound.items, item_cap_rows);
    bool both = false;
    if (!apart) {  // small frames: one launch for both render kernels
        const hipError_t e = par_launch_render_both(ctx->grid, r, bound.cols, item_bound, may_overflow, stream);
        if (e == hipSuccess) {
            both = true;
        } else if (e != hipErrorNotSupported) {
            return hip_fail(ctx, e, "par_launch_render_both");
        }
    }
    if (!both) {
        PAR_HIP(par_launch_render(ctx->grid, r, item_bound, stream));
        if (ev) PAR_HIP(hipEventRecord(ev[EV_ITEMS], stream));
        PAR_HIP(par_launch_render_tiles(ctx->grid, r, item_bound, stream));  // (dense frames only: r.tile_k > 0)
    } else if (ev) {
        PAR_HIP(hipEventRecord(ev[EV_ITEMS], stream));
    }
    if (ev) PAR_HIP(hipEventRecord(ev[EV_RENDERED], stream));
    if (!both && may_overflow) PAR_HIP(par_launch_render_overflow(ctx->grid, r, bound.cols, stream));
    if (ev) PAR_HIP(hipEventRecord(ev[EV_END], stream));
    if (ev) {  // which of the optional launches this frame had (par_frame_stats::ms_launch)
        ctx->timed_tiles = !both && r.tile_k > 0;
        ctx->timed_overflow = !both && may_overflow;
        ctx->timed_both = both;
    }
    return PAR_OK;
}

int render_to_host(par_context* ctx, int row_begin, int row_end, const par_outputs* host_out, unsigned flags) {
    int rc = frame_prologue(ctx, host_out, row_begin, row_end, flags);
    if (rc != PAR_OK) return rc;
    void* host[5] = {host_out->fb, host_out->gbuf, host_out->palidx, host_out->brightness, host_out->lit};
    const size_t n = (size_t)(row_end - row_begin) * ctx->params.width;
    void* dev[5];
    for (int i = 0; i < 5; i++) {
        dev[i] = nullptr;
        if (!host[i]) continue;
        const size_t bytes = n * kPlaneElem[i];
        if (ctx->d_out_bytes[i] < bytes) PAR_HIP(grow(&ctx->d_out[i], &ctx->d_out_bytes[i], bytes));
        dev[i] = ctx->d_out[i];
    }
    par_outputs d{(par_color*)dev[0], (par_pixel*)dev[1], (uint8_t*)dev[2], (float*)dev[3], (uint8_t*)dev[4]};
    rc = enqueue_frame(ctx, ctx->stream, ctx->set, row_begin, row_end, d, flags, false, nullptr);
    if (rc != PAR_OK) return rc;
    ctx->set ^= 1;
    ctx->last_flags = flags;
    for (int i = 0; i < 5; i++) {
        if (host[i]) PAR_HIP(hipMemcpyAsync(host[i], dev[i], n * kPlaneElem[i], hipMemcpyDeviceToHost, ctx->stream));
    }
    PAR_HIP(hipStreamSynchronize(ctx->stream));
    rc = check_device_error(ctx);
    if (rc == PAR_OK) retain_frame(ctx, row_begin, row_end, ctx->set ^ 1, host_out->gbuf != nullptr);
    return rc;
}

// The context's fixed device buffers: par_create allocates those of more than 0 bytes and sets every byte of those
// with a fill, par_destroy frees them all. (What grows on demand is freed beside them.)
struct par_dev_buffer {
    void** ptr;
    size_t bytes;
    int fill;  // the byte the buffer starts with, or -1
};

std::array<par_dev_buffer, 21> dev_buffers(par_context* c, bool stamps) {
    par_grid_dev& g = c->grid;
    const size_t vol = (size_t)c->volume, cols = (size_t)c->gx * c->gy, i32 = sizeof(int32_t);
    return {{
        {(void**)&g.head[0], vol * i32, -1},
        {(void**)&g.head[1], vol * i32, -1},
        {(void**)&g.count[0], vol, -1},
        {(void**)&g.count[1], vol, -1},
        {(void**)&g.colflag[0], cols * i32, -1},
        {(void**)&g.colflag[1], cols * i32, -1},
        {(void**)&g.col_list, cols * i32, -1},
        {(void**)&g.slow_list, cols * i32, -1},
        {(void**)&g.clear_list, cols * i32, -1},
        {(void**)&g.coldirty, cols * i32, 0},
        {(void**)&g.counters, PAR_CNT_TOTAL * i32, -1},
        {(void**)&g.node_counter, 2 * i32, -1},
        {(void**)&g.build_sync, 64 * i32, 0},
        {(void**)&g.item_counters, (size_t)PAR_ITEM_LISTS * PAR_ITEM_SHARDS * PAR_ITEM_COUNTER_STRIDE * i32, 0},
        {(void**)&g.stamps, stamps ? (size_t)PAR_STAMP_ROWS * PAR_STAMP_WGS * PAR_STAMP_SLOTS * sizeof(unsigned long long) : 0, 0},
        {(void**)&g.bgwalk, (size_t)c->gx * sizeof(par_bgwalk), -1},
        {(void**)&g.bglit, (size_t)c->params.width + 64, 1},
        {(void**)&g.slots, vol * PAR_SLOTS * sizeof(par_slot), 0},
        {(void**)&c->d_palette, PAR_MAX_PALETTE * sizeof(par_color), -1},  // (par_create copies the palette in)
        {(void**)&c->d_ray_counter, 3 * sizeof(unsigned long long), -1},  // (par_render_args::ray_counter)
        {(void**)&c->d_lights, sizeof(par_lights_block), -1},
    }};
}

}  // namespace

extern "C" {

const char* par_last_error(const par_context* ctx) { return ctx ? ctx->err.c_str() : ""; }

int par_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

static int par_create_impl(const par_params* params, int device, par_context** out) {
    if (!params || !out) return PAR_ERR_INVALID_ARG;
    *out = nullptr;
    const par_params& p = *params;
    if (p.width <= 0 || p.height <= 0 || p.length <= 0 || p.bin_size <= 0 || p.width > 32767 || p.height > 32767 ||
        p.length > 32767 || !(p.ambient >= 0.f && p.ambient <= 1.f) || p.palette_size <= 0 ||
        p.palette_size > PAR_MAX_PALETTE) {
        return PAR_ERR_INVALID_ARG;  // coordinates are `short` in the reference (alt:12-38); Color*ambient must fit u8
    }
    int gx, gy, gz;
    par_grid_dims(&p, &gx, &gy, &gz);
    if (p.bin_size < PAR_MIN_BIN || p.bin_size > PAR_MAX_BIN || gx > PAR_MAX_GRID_DIM || gy > PAR_MAX_GRID_DIM ||
        gz > PAR_MAX_GRID_DIM || (int64_t)gx * gy * gz > 0x3FFFFFFF) {
        return PAR_ERR_UNSUPPORTED;
    }
    const int rc = par_select_device(&device);
    if (rc != PAR_OK) return rc;

    par_context* ctx = new (std::nothrow) par_context;
    if (!ctx) return PAR_ERR_OOM;
    ctx->params = p;
    ctx->device = device;
    ctx->gx = gx; ctx->gy = gy; ctx->gz = gz; ctx->volume = gx * gy * gz;
    ctx->book.init(p, gx, gy, gz);
    ctx->grid.gx = gx; ctx->grid.gy = gy; ctx->grid.gz = gz; ctx->grid.volume = ctx->volume;
    ctx->stats.shadow_rays = -1; ctx->stats.ms_bin = -1.f; ctx->stats.ms_fill = -1.f; ctx->stats.ms_render = -1.f;
    ctx->stats.ms_overflow = -1.f;
    for (float& v : ctx->stats.ms_launch) v = -1.f;
    auto bail = [&](hipError_t e) {
        int rc = e == hipErrorOutOfMemory ? PAR_ERR_OOM : PAR_ERR_HIP;
        par_destroy(ctx);
        return rc;
    };
    hipError_t e;
    if ((e = hipSetDevice(device)) != hipSuccess) return bail(e);
    if ((e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking)) != hipSuccess) return bail(e);
    const char* dbg = std::getenv("PAR_DEBUG_STAMPS");
    for (const par_dev_buffer& b : dev_buffers(ctx, dbg && dbg[0] == '1')) {
        if (b.bytes == 0) continue;
        if ((e = hipMalloc(b.ptr, b.bytes)) != hipSuccess) return bail(e);
        if (b.fill >= 0 && (e = hipMemset(*b.ptr, b.fill, b.bytes)) != hipSuccess) return bail(e);
    }
    if ((e = hipMemcpy(ctx->d_palette, p.palette, PAR_MAX_PALETTE * sizeof(par_color), hipMemcpyHostToDevice)) != hipSuccess) return bail(e);
    for (hipEvent_t& ev : ctx->ev) {
        if ((e = hipEventCreate(&ev)) != hipSuccess) return bail(e);
    }
    if (reset_grid(ctx) != PAR_OK) {
        par_destroy(ctx);
        return PAR_ERR_HIP;
    }
    if (ensure_room(ctx, par_bound{1, 1, 1}) != PAR_OK) {
        par_destroy(ctx);
        return PAR_ERR_OOM;
    }
    *out = ctx;
    return PAR_OK;
}

void par_destroy(par_context* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)hipDeviceSynchronize();
    drop_graphs(ctx);
    free_pool(ctx);
    for (const par_dev_buffer& b : dev_buffers(ctx, false)) {
        if (*b.ptr) (void)hipFree(*b.ptr);
    }
    void* grown[] = {ctx->d_scratch_lit, ctx->grid.items, ctx->d_aabbs, ctx->d_sprite_ids, ctx->d_sprites, ctx->d_texinfo,
                     ctx->d_out[0], ctx->d_out[1], ctx->d_out[2], ctx->d_out[3], ctx->d_out[4]};
    for (void* p : grown) {
        if (p) (void)hipFree(p);
    }
    if (ctx->pin_update) (void)hipHostFree(ctx->pin_update);
    if (ctx->ev_update) (void)hipEventDestroy(ctx->ev_update);
    for (int s = 0; s < 2; s++) {
        if (ctx->pin_aabbs[s]) (void)hipHostFree(ctx->pin_aabbs[s]);
        if (ctx->pin_lights[s]) (void)hipHostFree(ctx->pin_lights[s]);
        if (ctx->ev_graph[s]) (void)hipEventDestroy(ctx->ev_graph[s]);
    }
    for (hipEvent_t ev : ctx->ev) {
        if (ev) (void)hipEventDestroy(ev);
    }
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

static int par_set_sprites_impl(par_context* ctx, const par_sprite* sprites, int n_sprites) {
    if (!ctx || !sprites || n_sprites <= 0) return fail(ctx, PAR_ERR_INVALID_ARG, "sprites");
    test_alloc_hook(ctx);
    for (int s = 0; s < n_sprites; s++) {
        for (int t = 0; t < PAR_SPRITE_TEXELS; t++) {
            const int c = sprites[s].color[t];
            if (c < 0 || c >= ctx->params.palette_size) {  // color_palette[...] out of bounds is UB at alt:353
                return fail(ctx, PAR_ERR_SPRITE_ID, "sprite palette index outside the palette");
            }
        }
    }
    PAR_HIP(hipSetDevice(ctx->device));
    PAR_HIP(hipDeviceSynchronize());
    drop_graphs(ctx);  // (a captured graph bakes the table's pointers)
    drop_retained(ctx);
    ctx->book.dirty.mark_all();  // (what every entity draws may change)
    ctx->n_sprites = 0;
    PAR_HIP(reallocate(&ctx->d_sprites, (size_t)n_sprites));
    PAR_HIP(hipMemcpy(ctx->d_sprites, sprites, (size_t)n_sprites * sizeof(par_sprite), hipMemcpyHostToDevice));
    // per-texel shading record: normal + the palette colour its index resolves to (alt:349-354)
    std::vector<par_texel> tex((size_t)n_sprites * PAR_SPRITE_TEXELS);
    for (int s = 0; s < n_sprites; s++) {
        for (int t = 0; t < PAR_SPRITE_TEXELS; t++) {
            const par_color pc = ctx->params.palette[sprites[s].color[t]];
            par_texel& x = tex[(size_t)s * PAR_SPRITE_TEXELS + t];
            x.nx = sprites[s].normal[t].x; x.ny = sprites[s].normal[t].y; x.nz = sprites[s].normal[t].z;
            x.rgba = (uint32_t)pc.red | ((uint32_t)pc.green << 8) | ((uint32_t)pc.blue << 16) | ((uint32_t)pc.alpha << 24);
        }
    }
    PAR_HIP(reallocate(&ctx->d_texinfo, tex.size()));
    PAR_HIP(hipMemcpy(ctx->d_texinfo, tex.data(), tex.size() * sizeof(par_texel), hipMemcpyHostToDevice));
    // the depths' range, for the range cull of ranged lights (clamped far outside any bin: the arithmetic stays in int)
    int dmin = INT32_MAX, dmax = INT32_MIN;
    for (int s = 0; s < n_sprites; s++) {
        for (int t = 0; t < PAR_SPRITE_TEXELS; t++) {
            dmin = std::min(dmin, (int)sprites[s].depth[t]);
            dmax = std::max(dmax, (int)sprites[s].depth[t]);
        }
    }
    ctx->depth_min = std::max(dmin, -(1 << 24));
    ctx->depth_max = std::min(dmax, 1 << 24);
    ctx->n_sprites = n_sprites;
    return PAR_OK;
}

static int par_set_entities_impl(par_context* ctx, const par_aabb* aabbs, const int32_t* sprite_ids, int n) {
    if (!ctx || n < 0 || (n > 0 && !aabbs)) return fail(ctx, PAR_ERR_INVALID_ARG, "entities");
    test_alloc_hook(ctx);
    int max_id = 0;
    for (int i = 0; i < n; i++) {
        if (!extent_ok(aabbs[i])) {
            return fail(ctx, PAR_ERR_EXTENT, "entity " + std::to_string(i) + ": extent needs 0<=ex<=20, ey,ez>=0, ey+ez<=40");
        }
        if (sprite_ids) {
            if (sprite_ids[i] < 0) return fail(ctx, PAR_ERR_SPRITE_ID, "negative sprite id");
            max_id = std::max(max_id, (int)sprite_ids[i]);
        }
    }
    PAR_HIP(hipSetDevice(ctx->device));
    PAR_HIP(hipDeviceSynchronize());
    drop_graphs(ctx);
    drop_retained(ctx);
    // (pools and lists by what the extents allow too: they then hold wherever the entities move)
    const int rc = ensure_room(ctx, ctx->book.plan(par_change::SET, aabbs, 0, n).need);
    if (rc != PAR_OK) return rc;
    if (n > ctx->aabb_capacity) PAR_HIP(grow(&ctx->d_aabbs, &ctx->aabb_capacity, std::max(n, 1)));
    if (ctx->d_sprite_ids) PAR_HIP(hipFree(ctx->d_sprite_ids));
    ctx->d_sprite_ids = nullptr;
    if (n > 0) PAR_HIP(hipMemcpy(ctx->d_aabbs, aabbs, (size_t)n * sizeof(par_aabb), hipMemcpyHostToDevice));
    if (sprite_ids && n > 0 && max_id > 0) {  // all-zero ids need no table
        PAR_HIP(hipMalloc(&ctx->d_sprite_ids, (size_t)n * sizeof(int32_t)));
        PAR_HIP(hipMemcpy(ctx->d_sprite_ids, sprite_ids, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    ctx->book.commit();
    ctx->dev_lo = ctx->dev_hi = 0;
    ctx->n_entities = n;
    ctx->max_sprite_id = max_id;
    ctx->have_entities = true;
    ctx->stats.entities = n;
    return PAR_OK;
}

static int par_set_entities_ref_layout_impl(par_context* ctx, const par_aabb* aabbs, const par_sprite* sprite_per_entity, int n) {
    if (!ctx || n < 0 || (n > 0 && (!aabbs || !sprite_per_entity))) return fail(ctx, PAR_ERR_INVALID_ARG, "entities");
    // The reference stores one 16 000-byte Sprite per entity (alt:95,107). Keep each distinct sprite once: a 64-bit
    // hash of the bytes finds the candidates, memcmp decides.
    test_alloc_hook(ctx);
    std::unordered_map<uint64_t, std::vector<int32_t>> seen;
    std::vector<par_sprite> table;
    std::vector<int32_t> ids((size_t)n);
    for (int i = 0; i < n; i++) {
        const unsigned char* bytes = reinterpret_cast<const unsigned char*>(&sprite_per_entity[i]);
        uint64_t h = 1469598103934665603ull;  // FNV-1a over 8-byte words
        for (size_t k = 0; k + 8 <= sizeof(par_sprite); k += 8) {
            uint64_t w;
            std::memcpy(&w, bytes + k, 8);
            h = (h ^ w) * 1099511628211ull;
        }
        std::vector<int32_t>& bucket = seen[h];
        int32_t id = -1;
        for (int32_t cand : bucket) {
            if (std::memcmp(&table[(size_t)cand], bytes, sizeof(par_sprite)) == 0) {
                id = cand;
                break;
            }
        }
        if (id < 0) {
            id = (int32_t)table.size();
            table.push_back(sprite_per_entity[i]);
            bucket.push_back(id);
        }
        ids[(size_t)i] = id;
    }
    if (table.empty()) {
        par_sprite s;
        par_sprite_tile_floor(&s);
        table.push_back(s);
    }
    int rc = par_set_sprites(ctx, table.data(), (int)table.size());
    if (rc != PAR_OK) return rc;
    return par_set_entities(ctx, aabbs, ids.data(), n);
}

static int par_update_aabbs_impl(par_context* ctx, const par_aabb* aabbs, int first, int n) {
    if (!ctx) return PAR_ERR_INVALID_ARG;
    int rc = check_update(ctx, aabbs, first, n, false);
    if (rc != PAR_OK) return rc;
    drop_retained(ctx);
    const par_bound need = ctx->book.plan(par_change::UPDATE, aabbs, first, n).need;
    PAR_HIP(hipSetDevice(ctx->device));
    rc = ensure_room(ctx, need);
    if (rc != PAR_OK) return rc;
    // a frame enqueued asynchronously by par_render_device may still be reading the AABBs: wait for it
    if (ctx->has_last_stream) PAR_HIP(hipStreamSynchronize(ctx->last_stream));
    if (ctx->ev_update_pending) {  // ... and an asynchronous update may still be writing them
        PAR_HIP(hipEventSynchronize(ctx->ev_update));
        ctx->ev_update_pending = false;
    }
    PAR_HIP(hipMemcpyAsync(ctx->d_aabbs + first, aabbs, (size_t)n * sizeof(par_aabb), hipMemcpyHostToDevice, ctx->stream));
    PAR_HIP(hipStreamSynchronize(ctx->stream));
    ctx->book.commit();
    mark_staged(ctx, first, n);  // (a captured graph uploads the scene from its staging area)
    return PAR_OK;
}

static int par_update_aabbs_async_impl(par_context* ctx, const par_aabb* aabbs, int first, int n, void* stream_v) {
    if (!ctx) return PAR_ERR_INVALID_ARG;
    const int rc = check_update(ctx, aabbs, first, n, false);
    if (rc != PAR_OK) return rc;
    hipStream_t stream = (hipStream_t)stream_v;
    drop_retained(ctx);
    // No cull and range arithmetic here (it cost a moving scene more host time per frame than its launches): the
    // book keeps the extents alone (EXTENTS_ONLY) until a blocking call refreshes it, and the frame's launches are
    // sized by them and include the one for the overflow list whatever the columns hold.
    const par_bound need = ctx->book.plan(par_change::ASYNC, aabbs, first, n).need;
    PAR_HIP(hipSetDevice(ctx->device));
    // the node pool and the item list grow rarely (only when extents grow); that path frees device memory and has to
    // wait for everything in flight
    if (need.pairs > ctx->grid.capacity || ctx->book.items_per_shard(need.items, need.cols) > ctx->grid.item_capacity) {
        return par_update_aabbs(ctx, aabbs, first, n);
    }
    // frames enqueued on another stream are not ordered with this copy: wait for them
    if (ctx->has_last_stream && ctx->last_stream != stream) PAR_HIP(hipStreamSynchronize(ctx->last_stream));
    if (ctx->pin_update_capacity < ctx->aabb_capacity) {
        if (ctx->ev_update_pending) PAR_HIP(hipEventSynchronize(ctx->ev_update));
        ctx->ev_update_pending = false;
        PAR_HIP(grow(&ctx->pin_update, &ctx->pin_update_capacity, ctx->aabb_capacity, true));
    }
    if (!ctx->ev_update) PAR_HIP(hipEventCreateWithFlags(&ctx->ev_update, hipEventDisableTiming));
    // the staging area is free again once the previous update's copy has run (normally long ago)
    if (ctx->ev_update_pending) PAR_HIP(hipEventSynchronize(ctx->ev_update));
    std::memcpy(ctx->pin_update + first, aabbs, (size_t)n * sizeof(par_aabb));
    PAR_HIP(hipMemcpyAsync(ctx->d_aabbs + first, ctx->pin_update + first, (size_t)n * sizeof(par_aabb),
                           hipMemcpyHostToDevice, stream));
    PAR_HIP(hipEventRecord(ctx->ev_update, stream));
    ctx->ev_update_pending = true;
    ctx->update_stream = stream;
    ctx->book.commit();
    mark_staged(ctx, first, n);  // (a captured graph uploads the scene from its staging area)
    return PAR_OK;
}

static int par_set_lights_impl(par_context* ctx, const par_light* lights, int n) {
    if (!ctx) return PAR_ERR_INVALID_ARG;
    if (n < 1 || n > PAR_MAX_LIGHTS) return fail(ctx, PAR_ERR_INVALID_ARG, "lights: n must lie in [1, PAR_MAX_LIGHTS]");
    if (!lights) return fail(ctx, PAR_ERR_INVALID_ARG, "lights");
    set_lights(ctx, lights, n, n);
    return PAR_OK;
}

static int par_set_light_model_impl(par_context* ctx, int model) {
    if (!ctx) return PAR_ERR_INVALID_ARG;
    if (model != PAR_LIGHTS_UNBOUNDED && model != PAR_LIGHTS_RANGED) {
        return fail(ctx, PAR_ERR_INVALID_ARG, "light model: PAR_LIGHTS_UNBOUNDED or PAR_LIGHTS_RANGED");
    }
    if (model == ctx->light_model) return PAR_OK;
    PAR_HIP(hipSetDevice(ctx->device));
    PAR_HIP(hipDeviceSynchronize());
    drop_graphs(ctx);  // (a captured graph bakes the kernels of the model it was captured with)
    ctx->light_model = model;
    return PAR_OK;
}

static int par_set_light_tints_impl(par_context* ctx, const par_light_tint* tints, int n) {
    if (!ctx) return PAR_ERR_INVALID_ARG;
    if (n < 0 || n > PAR_MAX_LIGHTS || (tints == nullptr) != (n == 0)) {
        return fail(ctx, PAR_ERR_INVALID_ARG, "light tints: NULL with 0, or 1 <= n <= PAR_MAX_LIGHTS");
    }
    for (int l = 0; l < n; l++) {
        for (const float v : {tints[l].r, tints[l].g, tints[l].b}) {
            if (!std::isfinite(v) || v < 0.f) {
                return fail(ctx, PAR_ERR_INVALID_ARG, "light tints: every component must be finite and not negative");
            }
        }
    }
    const bool tinted = n > 0;
    if (tinted != ctx->tinted) {
        PAR_HIP(hipSetDevice(ctx->device));
        PAR_HIP(hipDeviceSynchronize());
        drop_graphs(ctx);  // (a captured graph bakes the kernels of the state it was captured in)
        ctx->tinted = tinted;
    }
    // (a graph captured in this state reads the values from its staging area, which par_graph_launch rewrites)
    for (int l = 0; l < PAR_MAX_LIGHTS; l++) {
        const par_light_tint t = l < n ? tints[l] : par_light_tint{1.f, 1.f, 1.f};
        ctx->tints.t[l][0] = t.r;
        ctx->tints.t[l][1] = t.g;
        ctx->tints.t[l][2] = t.b;
    }
    return PAR_OK;
}

static int par_set_light_impl(par_context* ctx, const par_light* light) {
    if (!ctx || !light) return fail(ctx, PAR_ERR_INVALID_ARG, "light");
    return par_set_lights_impl(ctx, light, 1);
}

static int par_render_impl(par_context* ctx, const par_outputs* host_out, unsigned flags) {
    if (!ctx) return PAR_ERR_INVALID_ARG;
    return render_to_host(ctx, 0, ctx->params.height, host_out, flags);
}

static int par_render_rows_impl(par_context* ctx, int row_begin, int row_end, const par_outputs* host_out, unsigned flags) {
    return render_to_host(ctx, row_begin, row_end, host_out, flags);
}

static int par_render_device_impl(par_context* ctx, void* stream, int row_begin, int row_end, const par_outputs* device_out,
                      unsigned flags) {
    int rc = frame_prologue(ctx, device_out, row_begin, row_end, flags);
    if (rc != PAR_OK) return rc;
    rc = enqueue_frame(ctx, (hipStream_t)stream, ctx->set, row_begin, row_end, *device_out, flags, false, nullptr);
    if (rc != PAR_OK) return rc;
    ctx->set ^= 1;
    ctx->last_flags = flags;
    ctx->last_stream = (hipStream_t)stream;
    ctx->has_last_stream = true;
    retain_frame(ctx, row_begin, row_end, ctx->set ^ 1, false);
    record_drawn(ctx, *device_out, row_begin, row_end, ctx->set ^ 1);
    return PAR_OK;
}

static int par_render_device_timed_impl(par_context* ctx, void* stream, int row_begin, int row_end,
                            const par_outputs* device_out, unsigned flags, par_frame_stats* stats) {
    int rc = frame_prologue(ctx, device_out, row_begin, row_end, flags);
    if (rc != PAR_OK) return rc;
    rc = enqueue_frame(ctx, (hipStream_t)stream, ctx->set, row_begin, row_end, *device_out, flags, false, ctx->ev);
    if (rc != PAR_OK) return rc;
    ctx->set ^= 1;
    ctx->last_flags = flags;
    const hipEvent_t* ev = ctx->ev;
    PAR_HIP(hipEventSynchronize(ev[EV_END]));
    PAR_HIP(hipEventElapsedTime(&ctx->stats.ms_bin, ev[EV_START], ev[EV_COLUMNS]));
    PAR_HIP(hipEventElapsedTime(&ctx->stats.ms_fill, ev[EV_COLUMNS], ev[EV_FILLED]));
    PAR_HIP(hipEventElapsedTime(&ctx->stats.ms_render, ev[EV_FILLED], ev[EV_RENDERED]));
    PAR_HIP(hipEventElapsedTime(&ctx->stats.ms_overflow, ev[EV_RENDERED], ev[EV_END]));
    for (float& v : ctx->stats.ms_launch) v = -1.f;
    ctx->stats.render_merged = 0;
    if (flags & PAR_RENDER_TIMED_AS_LAUNCHED) {
        ctx->stats.render_merged = ctx->timed_both ? 1 : 0;
        PAR_HIP(hipEventElapsedTime(&ctx->stats.ms_launch[0], ev[EV_START], ev[EV_BUILT]));
        PAR_HIP(hipEventElapsedTime(&ctx->stats.ms_launch[1], ev[EV_BUILT], ev[EV_FILLED]));
        PAR_HIP(hipEventElapsedTime(&ctx->stats.ms_launch[2], ev[EV_FILLED], ev[EV_ITEMS]));
        PAR_HIP(hipEventElapsedTime(&ctx->stats.ms_launch[3], ev[EV_ITEMS], ev[EV_RENDERED]));
        PAR_HIP(hipEventElapsedTime(&ctx->stats.ms_launch[4], ev[EV_RENDERED], ev[EV_END]));
        if (!ctx->timed_tiles) ctx->stats.ms_launch[3] = 0.f;  // (an empty bracket still measures the events themselves)
        if (!ctx->timed_overflow) ctx->stats.ms_launch[4] = 0.f;
    }
    rc = stats ? par_get_stats(ctx, stats) : check_device_error(ctx);
    if (rc == PAR_OK) {
        retain_frame(ctx, row_begin, row_end, ctx->set ^ 1, false);
        // (a frame timed with its kernels apart leaves no drawn-into record: par_raytracer.h)
        if (flags & PAR_RENDER_TIMED_AS_LAUNCHED) record_drawn(ctx, *device_out, row_begin, row_end, ctx->set ^ 1);
    }
    return rc;
}

// What both relight calls check, in the order par_raytracer.h gives, before any device work. `host`: par_relight_rows.
static int relight_prologue(par_context* ctx, bool gbuf_given, const par_outputs* out, int row_begin, int row_end,
                            unsigned flags, bool host) {
    if (!ctx || !gbuf_given || !out) return fail(ctx, PAR_ERR_INVALID_ARG, "null argument");
    if (out->gbuf || out->palidx) {
        return fail(ctx, PAR_ERR_INVALID_ARG, "a relit frame writes no gbuf or palidx plane: they do not depend on lights");
    }
    if (flags & ~PAR_ACCEPTED_FLAGS) return fail(ctx, PAR_ERR_INVALID_ARG, "undefined render flag bits");
    if (row_begin < 0 || row_end > ctx->params.height || row_begin >= row_end) {
        return fail(ctx, PAR_ERR_INVALID_ARG, "rows must satisfy 0 <= row_begin < row_end <= height");
    }
    if (ctx->n_sprites <= 0) return fail(ctx, PAR_ERR_NOT_READY, "par_set_sprites has not been called");
    if (!ctx->have_entities) return fail(ctx, PAR_ERR_NOT_READY, "par_set_entities has not been called");
    if (ctx->n_lights <= 0) return fail(ctx, PAR_ERR_NOT_READY, "par_set_light has not been called");
    if (!ctx->kept.valid) return fail(ctx, PAR_ERR_NOT_READY, "no retained frame: render one first");
    if (row_begin < ctx->kept.r0 || row_end > ctx->kept.r1) {
        return fail(ctx, PAR_ERR_NOT_READY, "rows outside the retained frame's");
    }
    if (host && !ctx->kept.host_gbuf) {
        return fail(ctx, PAR_ERR_NOT_READY, "the retained frame is not a par_render / par_render_rows frame with a gbuf plane");
    }
    PAR_HIP(hipSetDevice(ctx->device));
    return PAR_OK;
}

// A relit frame on `stream`: the background rays when they are wanted, the background fill, and the relight form of the
// light kernel over the retained frame's column list, under the lights the context holds now. No hash build, no flip
// of the grid set; the retained frame stays.
static int enqueue_relight(par_context* ctx, hipStream_t stream, int row_begin, int row_end, const par_pixel* gbuf,
                           const par_outputs& out, unsigned flags) {
    par_outputs outs = out;
    if ((flags & PAR_RENDER_TRACE_BACKGROUND) && !outs.lit) {  // (as enqueue_frame: the rays' results go to a scratch plane)
        const size_t need = (size_t)(row_end - row_begin) * ctx->params.width;
        if (ctx->scratch_lit_bytes < need) PAR_HIP(grow(&ctx->d_scratch_lit, &ctx->scratch_lit_bytes, need));
        outs.lit = ctx->d_scratch_lit;
    }
    const par_render_args r = make_render_args(ctx, ctx->kept.set, row_begin, row_end, outs, flags, false);
    const par_light_state lights = make_light_state(ctx, false);
    drop_drawn(ctx);
    if (flags & PAR_RENDER_COUNT_RAYS) {
        PAR_HIP(hipMemsetAsync(ctx->d_ray_counter, 0, 3 * sizeof(unsigned long long), stream));
    }
    if (r.trace_bg) PAR_HIP(par_launch_bglights(ctx->grid, r, lights, stream));
    PAR_HIP(par_launch_fill(ctx->grid, r, stream));
    // the column list is the retained frame's: bounded as its launch was, by its rows
    const int B = ctx->params.bin_size;
    const int64_t kept_cols = (int64_t)ctx->gx * ((ctx->kept.r1 - 1) / B - ctx->kept.r0 / B + 1);
    const int64_t cols = std::min(ctx->book.frame_bounds(false).cols, kept_cols);
    PAR_HIP(par_launch_relight(ctx->grid, r, gbuf, lights, cols, stream));
    ctx->last_flags = flags;
    return PAR_OK;
}

static int par_relight_device_impl(par_context* ctx, void* stream, int row_begin, int row_end, const par_pixel* gbuf,
                                   const par_outputs* device_out, unsigned flags) {
    int rc = relight_prologue(ctx, gbuf != nullptr, device_out, row_begin, row_end, flags, false);
    if (rc != PAR_OK) return rc;
    rc = enqueue_relight(ctx, (hipStream_t)stream, row_begin, row_end, gbuf, *device_out, flags);
    if (rc != PAR_OK) return rc;
    ctx->last_stream = (hipStream_t)stream;
    ctx->has_last_stream = true;
    return PAR_OK;
}

static int par_relight_rows_impl(par_context* ctx, int row_begin, int row_end, const par_outputs* host_out, unsigned flags) {
    int rc = relight_prologue(ctx, true, host_out, row_begin, row_end, flags, true);
    if (rc != PAR_OK) return rc;
    // fb, brightness, lit: the context's device planes, addressing (row_begin, 0); the gbuf plane stays as the
    // retained frame left it, addressing that frame's first row
    const int plane[3] = {0, 3, 4};
    void* host[3] = {host_out->fb, host_out->brightness, host_out->lit};
    const size_t n = (size_t)(row_end - row_begin) * ctx->params.width;
    void* dev[3] = {nullptr, nullptr, nullptr};
    for (int i = 0; i < 3; i++) {
        if (!host[i]) continue;
        const int k = plane[i];
        const size_t bytes = n * kPlaneElem[k];
        if (ctx->d_out_bytes[k] < bytes) PAR_HIP(grow(&ctx->d_out[k], &ctx->d_out_bytes[k], bytes));
        dev[i] = ctx->d_out[k];
    }
    const par_outputs d{(par_color*)dev[0], nullptr, nullptr, (float*)dev[1], (uint8_t*)dev[2]};
    const par_pixel* gbuf = (const par_pixel*)ctx->d_out[1] + (size_t)(row_begin - ctx->kept.r0) * ctx->params.width;
    rc = enqueue_relight(ctx, ctx->stream, row_begin, row_end, gbuf, d, flags);
    if (rc != PAR_OK) return rc;
    for (int i = 0; i < 3; i++) {
        if (host[i]) PAR_HIP(hipMemcpyAsync(host[i], dev[i], n * kPlaneElem[plane[i]], hipMemcpyDeviceToHost, ctx->stream));
    }
    PAR_HIP(hipStreamSynchronize(ctx->stream));
    return check_device_error(ctx);
}

// par_graph_capture (lights_kind false: the one-light path) and par_graph_capture_lights (true: the light path).
static int graph_capture(par_context* ctx, void* stream_v, int row_begin, int row_end, const par_outputs* device_out,
                         unsigned flags, bool lights_kind) {
    hipStream_t stream = (hipStream_t)stream_v;
    // (after the prologue's refusal of null arguments, before its other checks)
    if (ctx && device_out && !stream) return fail(ctx, PAR_ERR_INVALID_ARG, "graph capture needs a non-default stream");
    int rc = frame_prologue(ctx, device_out, row_begin, row_end, flags);
    if (rc != PAR_OK) return rc;
    if (!lights_kind && ranged(ctx)) {
        return fail(ctx, PAR_ERR_UNSUPPORTED, "a frame with ranged lights cannot be captured (par_graph_capture_lights)");
    }
    if (!lights_kind && ctx->tinted) {
        return fail(ctx, PAR_ERR_UNSUPPORTED, "a frame with tinted lights cannot be captured (par_graph_capture_lights)");
    }
    if (!lights_kind && lights_path(ctx)) {
        return fail(ctx, PAR_ERR_UNSUPPORTED, "a frame with several lights cannot be captured (par_graph_capture_lights)");
    }
    PAR_HIP(hipDeviceSynchronize());
    drop_graphs(ctx);
    drop_retained(ctx);
    drop_drawn(ctx);
    rc = ensure_room(ctx, ctx->book.capture());
    if (rc != PAR_OK) return rc;
    for (int s = 0; s < 2; s++) {
        // (par_set_entities may have brought more entities since the last capture; no graph reads the area now)
        if (ctx->pin_aabbs_capacity[s] < std::max(ctx->aabb_capacity, 1)) {
            PAR_HIP(grow(&ctx->pin_aabbs[s], &ctx->pin_aabbs_capacity[s], std::max(ctx->aabb_capacity, 1), true));
        }
        if (!ctx->pin_lights[s]) PAR_HIP(hipHostMalloc(&ctx->pin_lights[s], sizeof(par_lights_block), hipHostMallocDefault));
        if (!ctx->ev_graph[s]) PAR_HIP(hipEventCreateWithFlags(&ctx->ev_graph[s], hipEventDisableTiming));
        ctx->ev_graph_pending[s] = false;
        std::memcpy(ctx->pin_aabbs[s], ctx->book.aabbs.data(), (size_t)ctx->n_entities * sizeof(par_aabb));
        stage_lights(ctx, s);
        ctx->stage_lo[s] = ctx->stage_hi[s] = 0;
    }
    ctx->graph_lights = lights_kind;  // (what enqueue_frame captures; no graph is left behind should the capture fail)
    // The frame alternates between the two grid sets, and a captured kernel node bakes its pointers: one graph
    // per set, launched alternately; each uploads the scene from its own staging area (the AABBs and the lights,
    // ahead of every kernel of the frame).
    for (int s = 0; s < 2; s++) {
        PAR_HIP(hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal));
        hipError_t e = hipSuccess;
        if (ctx->n_entities > 0) {  // (a copy of no bytes is no graph node: hipErrorInvalidValue)
            e = hipMemcpyAsync(ctx->d_aabbs, ctx->pin_aabbs[s], (size_t)ctx->n_entities * sizeof(par_aabb),
                               hipMemcpyHostToDevice, stream);
        }
        if (e == hipSuccess) {
            e = hipMemcpyAsync(ctx->d_lights, ctx->pin_lights[s], sizeof(par_lights_block), hipMemcpyHostToDevice, stream);
        }
        int erc = PAR_OK;
        if (e == hipSuccess) erc = enqueue_frame(ctx, stream, s, row_begin, row_end, *device_out, flags & ~PAR_RENDER_COUNT_RAYS, true, nullptr);
        hipGraph_t g = nullptr;
        hipError_t e2 = hipStreamEndCapture(stream, &g);
        hipError_t e3 = hipSuccess;
        if (e == hipSuccess && erc == PAR_OK && e2 == hipSuccess) {
            ctx->graph[s] = g;
            e3 = hipGraphInstantiate(&ctx->graph_exec[s], g, nullptr, nullptr, 0);
            if (e3 == hipSuccess) continue;
        } else if (g) {
            (void)hipGraphDestroy(g);
        }
        drop_graphs(ctx);  // never leave one graph of the pair behind
        if (e != hipSuccess) return hip_fail(ctx, e, "graph capture memcpy");
        if (erc != PAR_OK) return erc;
        if (e2 != hipSuccess) return hip_fail(ctx, e2, "hipStreamEndCapture");
        return hip_fail(ctx, e3, "hipGraphInstantiate");
    }
    return PAR_OK;
}

// par_graph_stage (keep_count: `lights` replaces lights[0] and the count stays) and par_graph_stage_lights (the whole
// light set) for AABBs [first, first + n). A refused call changes nothing but the freshness of the book.
static int graph_stage(par_context* ctx, const par_aabb* aabbs, int first, int n, const par_light* lights, int n_lights,
                       bool keep_count) {
    if (!ctx || !ctx->graph_exec[0]) return fail(ctx, PAR_ERR_NOT_READY, "no captured graph");
    if (n_lights < 0 || n_lights > PAR_MAX_LIGHTS || (lights == nullptr) != (n_lights == 0)) {
        return fail(ctx, PAR_ERR_INVALID_ARG, "lights: NULL with 0, or 1 <= n_lights <= PAR_MAX_LIGHTS");
    }
    if (n_lights > 1 && !ctx->graph_lights) {
        return fail(ctx, PAR_ERR_UNSUPPORTED, "a one-light graph cannot render several lights (par_graph_capture_lights)");
    }
    const int rc = check_update(ctx, aabbs, first, n, true);
    if (rc != PAR_OK) return rc;
    const int64_t pairs = ctx->book.plan(par_change::STAGE, aabbs, first, n).exact.pairs;
    if (pairs > ctx->book.graph.pairs || pairs > ctx->grid.capacity) {
        return fail(ctx, PAR_ERR_UNSUPPORTED, "staged frame exceeds what the captured graph was sized for; capture again");
    }
    ctx->book.commit();
    drop_retained(ctx);
    mark_staged(ctx, first, n);  // (the staging areas are brought up to date by par_graph_launch)
    if (n > 0) {
        const bool none = ctx->dev_hi <= ctx->dev_lo;
        ctx->dev_lo = none ? first : std::min(ctx->dev_lo, first);
        ctx->dev_hi = none ? first + n : std::max(ctx->dev_hi, first + n);
    }
    if (n_lights > 0) set_lights(ctx, lights, n_lights, keep_count ? ctx->n_lights : n_lights);
    return PAR_OK;
}

static int par_graph_launch_impl(par_context* ctx, void* stream) {
    if (!ctx || !ctx->graph_exec[0]) return fail(ctx, PAR_ERR_NOT_READY, "no captured graph");
    // (the scene may also have been changed by par_update_aabbs[_async]: same limit as par_graph_stage)
    ctx->book.refresh(par_book_state::HIST_BEHIND);
    if (ctx->book.exact.pairs > ctx->book.graph.pairs) {
        return fail(ctx, PAR_ERR_UNSUPPORTED, "the scene exceeds what the captured graph was sized for; capture again");
    }
    if (ctx->n_lights > 1 && !ctx->graph_lights) {
        return fail(ctx, PAR_ERR_UNSUPPORTED, "a frame with several lights has no one-light graph (par_graph_capture_lights)");
    }
    if (ranged(ctx) && !ctx->graph_lights) {
        return fail(ctx, PAR_ERR_UNSUPPORTED, "a frame with ranged lights has no one-light graph (par_graph_capture_lights)");
    }
    if (ctx->tinted && !ctx->graph_lights) {
        return fail(ctx, PAR_ERR_UNSUPPORTED, "a frame with tinted lights has no one-light graph (par_graph_capture_lights)");
    }
    const int s = ctx->set;
    if (!ctx->graph_exec[s]) return fail(ctx, PAR_ERR_NOT_READY, "no captured graph for this grid set");
    PAR_HIP(hipSetDevice(ctx->device));
    // This graph's staging area: free once its previous launch has run (its copy nodes read the area when they
    // execute, not when the graph is launched), then brought up to date with the host mirror and the light(s).
    if (ctx->ev_graph_pending[s]) {
        if (hipEventQuery(ctx->ev_graph[s]) != hipSuccess) PAR_HIP(hipEventSynchronize(ctx->ev_graph[s]));
        ctx->ev_graph_pending[s] = false;
    }
    if (ctx->stage_hi[s] > ctx->stage_lo[s]) {
        std::memcpy(ctx->pin_aabbs[s] + ctx->stage_lo[s], ctx->book.aabbs.data() + ctx->stage_lo[s],
                    (size_t)(ctx->stage_hi[s] - ctx->stage_lo[s]) * sizeof(par_aabb));
        ctx->stage_lo[s] = ctx->stage_hi[s] = 0;
    }
    stage_lights(ctx, s);
    // an asynchronous scene update on another stream: this frame comes after it
    if (ctx->ev_update_pending && ctx->update_stream != (hipStream_t)stream) {
        PAR_HIP(hipStreamWaitEvent((hipStream_t)stream, ctx->ev_update, 0));
    }
    drop_retained(ctx);
    drop_drawn(ctx);
    PAR_HIP(hipGraphLaunch(ctx->graph_exec[s], (hipStream_t)stream));
    ctx->dev_lo = ctx->dev_hi = 0;  // (the graph's first node copies the whole scene)
    PAR_HIP(hipEventRecord(ctx->ev_graph[s], (hipStream_t)stream));
    ctx->ev_graph_pending[s] = true;
    ctx->set ^= 1;
    ctx->last_stream = (hipStream_t)stream;
    ctx->has_last_stream = true;
    return PAR_OK;
}

static int par_pick_impl(par_context* ctx, int x, int y, par_pixel* out) {
    if (!ctx || !out || x < 0 || y < 0 || x >= ctx->params.width || y >= ctx->params.height) {
        return fail(ctx, PAR_ERR_INVALID_ARG, "pick outside the view");
    }
    std::vector<par_pixel> row((size_t)ctx->params.width);
    par_outputs o{nullptr, row.data(), nullptr, nullptr, nullptr};
    int rc = render_to_host(ctx, y, y + 1, &o, 0);
    if (rc != PAR_OK) return rc;
    ctx->kept.host_gbuf = false;  // (its one row is retained, for par_relight_device alone)
    *out = row[(size_t)x];  // `mouse_pixel`, alt:380-382
    return PAR_OK;
}

static int par_get_stats_impl(par_context* ctx, par_frame_stats* stats) {
    if (!ctx || !stats) return fail(ctx, PAR_ERR_INVALID_ARG, "stats");
    PAR_HIP(hipSetDevice(ctx->device));
    PAR_HIP(hipDeviceSynchronize());
    ctx->stats.entities = ctx->n_entities;
    ctx->stats.shadow_rays = -1;
    {
        int32_t nc[2] = {0, 0};
        static_assert(PAR_CNT_COLS == 0 && PAR_CNT_SLOW == 1, "read together");
        PAR_HIP(hipMemcpy(nc, ctx->grid.counters, sizeof(nc), hipMemcpyDeviceToHost));
        ctx->stats.occupied_columns = nc[0];
        ctx->stats.overflow_columns = nc[1];
        // the insert kernel's own count of the last frame's (entity, bin) nodes (the next frame's resolve resets it)
        int32_t nodes = 0;
        PAR_HIP(hipMemcpy(&nodes, ctx->grid.node_counter + (ctx->set ^ 1), sizeof(nodes), hipMemcpyDeviceToHost));
        ctx->stats.bin_insertions = nodes;
        const int rc = check_device_error(ctx);
        if (rc != PAR_OK) return rc;
    }
    if (ctx->last_flags & PAR_RENDER_COUNT_RAYS) {
        unsigned long long v = 0;
        PAR_HIP(hipMemcpy(&v, ctx->d_ray_counter, sizeof(v), hipMemcpyDeviceToHost));
        ctx->stats.shadow_rays = (int64_t)v;
    }
    *stats = ctx->stats;
    return PAR_OK;
}

// Internal profiling aid (not part of the public header): copy the debug stamp buffer out (PAR_DEBUG_STAMPS=1).
int par_debug_read_stamps(par_context* ctx, unsigned long long* out, size_t count) {
    if (!ctx || !out || !ctx->grid.stamps) return PAR_ERR_NOT_READY;
    const size_t n = (size_t)PAR_STAMP_ROWS * PAR_STAMP_WGS * PAR_STAMP_SLOTS;
    if (hipDeviceSynchronize() != hipSuccess) return PAR_ERR_HIP;
    if (hipMemcpy(out, ctx->grid.stamps, (count < n ? count : n) * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess) return PAR_ERR_HIP;
    return PAR_OK;
}

// Internal test aid (not part of the public header either): the (start bin, light) pairs the ranged light kernel walked
// (out[0]) and culled (out[1]) in the last frame rendered with PAR_RENDER_COUNT_RAYS; -1 and -1 when the last frame
// was not. Pairs of the bins whose walks the kernel records (the first 64 occupied bins of a column).
int par_debug_read_light_walks(par_context* ctx, int64_t* out) {
    if (!ctx || !out) return PAR_ERR_INVALID_ARG;
    out[0] = out[1] = -1;
    if (!(ctx->last_flags & PAR_RENDER_COUNT_RAYS)) return PAR_OK;
    unsigned long long v[2] = {0, 0};
    if (hipSetDevice(ctx->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return PAR_ERR_HIP;
    if (hipMemcpy(v, ctx->d_ray_counter + 1, sizeof(v), hipMemcpyDeviceToHost) != hipSuccess) return PAR_ERR_HIP;
    out[0] = (int64_t)v[0];
    out[1] = (int64_t)v[1];
    return PAR_OK;
}

// Internal test aid (not part of the public header either): the work items of the last frame's entry passes (list 0 of
// par_grid_dev::items, what render_items_kernel and the entry share of render_both_kernel consume), shard after shard,
// as the column launch left them: eight 32-bit words per item (par_item). *n_items gets their number; the first
// `capacity` of them are copied to `out` (which may be null when capacity is 0).
int par_debug_read_items(par_context* ctx, uint32_t* out, size_t capacity, int* n_items) {
    if (!ctx || !n_items || (capacity && !out)) return PAR_ERR_INVALID_ARG;
    *n_items = 0;
    if (!ctx->grid.items || !ctx->grid.item_counters) return PAR_ERR_NOT_READY;
    if (hipSetDevice(ctx->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return PAR_ERR_HIP;
    std::vector<int32_t> counters((size_t)PAR_ITEM_SHARDS * PAR_ITEM_COUNTER_STRIDE);
    if (hipMemcpy(counters.data(), ctx->grid.item_counters, counters.size() * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess) {
        return PAR_ERR_HIP;
    }
    size_t done = 0;
    for (int s = 0; s < PAR_ITEM_SHARDS; s++) {
        const int32_t c = counters[(size_t)s * PAR_ITEM_COUNTER_STRIDE];
        const size_t n = (size_t)std::min(std::max(c, 0), ctx->grid.item_capacity);
        const size_t take = std::min(n, capacity - std::min(capacity, done));
        if (take && hipMemcpy(out + done * (sizeof(par_item) / sizeof(uint32_t)),
                              ctx->grid.items + (size_t)s * ctx->grid.item_capacity, take * sizeof(par_item),
                              hipMemcpyDeviceToHost) != hipSuccess) {
            return PAR_ERR_HIP;
        }
        done += n;
    }
    *n_items = (int)done;
    return PAR_OK;
}

// Internal test aid (not part of the public header either): the context's test hooks (PAR_HOOK_* bits) and a forced
// number of wavefronts per column (1, 2, 4 or 8; 0 keeps the column launch's own choice). Read when a frame is
// enqueued; 0 and 0 restore production behaviour.
int par_debug_set_hooks(par_context* ctx, unsigned hooks, int col_roles) {
    if (!ctx) return PAR_ERR_INVALID_ARG;
    if ((hooks & ~PAR_HOOKS_ALL) || !(col_roles == 0 || col_roles == 1 || col_roles == 2 || col_roles == 4 || col_roles == 8)) {
        return fail(ctx, PAR_ERR_INVALID_ARG, "test hooks");
    }
    ctx->hooks = hooks;
    ctx->col_roles = col_roles;
    return PAR_OK;
}

static int par_read_grid_impl(par_context* ctx, int32_t* count, int32_t* map, par_aabb* bins) {
    if (!ctx || !count || !map || !bins) return fail(ctx, PAR_ERR_INVALID_ARG, "grid buffers");
    PAR_HIP(hipSetDevice(ctx->device));
    PAR_HIP(hipDeviceSynchronize());
    const int last = ctx->set ^ 1;  // the set the last frame used
    std::vector<uint8_t> c((size_t)ctx->volume);
    std::vector<par_slot> s((size_t)ctx->volume * PAR_SLOTS);
    PAR_HIP(hipMemcpy(c.data(), ctx->grid.count[last], c.size(), hipMemcpyDeviceToHost));
    PAR_HIP(hipMemcpy(s.data(), ctx->grid.slots, s.size() * sizeof(par_slot), hipMemcpyDeviceToHost));
    std::memset(map, 0, (size_t)ctx->volume * PAR_SLOTS * sizeof(int32_t));
    std::memset(bins, 0, (size_t)ctx->volume * PAR_SLOTS * sizeof(par_aabb));
    for (int b = 0; b < ctx->volume; b++) {
        count[b] = c[(size_t)b];
        for (int k = 0; k < c[(size_t)b]; k++) {
            const par_slot& r = s[(size_t)b * PAR_SLOTS + k];
            map[(size_t)b * PAR_SLOTS + k] = r.entity;
            bins[(size_t)b * PAR_SLOTS + k] = par_aabb{r.px, r.py, r.pz, r.ex, r.ey, r.ez, {0, 0}};
        }
    }
    return PAR_OK;
}


// Test hook: the reference's three arithmetic units as the DEVICE computes them (slab_hit, color_scale,
// normalize_l1_and_inverse of par_kernels.hip) on host vectors. See par_raytracer.h.
static int par_debug_units_impl(int device, int kind, const void* in_a, const void* in_b, int n, void* out) {
    const bool slab = kind == 0 || kind == 3 || kind == 4;  // (3, 4: the slab test on a walk record, par_kernels.hip)
    if (kind < 0 || kind > 4 || n < 0 || !in_a || !out || (slab && !in_b)) return PAR_ERR_INVALID_ARG;
    par_context* ctx = nullptr;  // (PAR_HIP reports through it)
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return PAR_ERR_NO_DEVICE;
    if (device < 0) device = 0;
    if (device >= ndev) return PAR_ERR_INVALID_ARG;
    PAR_HIP(hipSetDevice(device));
    const size_t a_bytes = (size_t)n * (slab ? sizeof(par_aabb) : (kind == 1 ? 5 : 3) * sizeof(float));
    const size_t b_bytes = slab ? (size_t)n * 20 : 0;
    const size_t o_bytes = (size_t)n * (slab ? 1 : (kind == 1 ? 4 : 12));
    void *da = nullptr, *db = nullptr, *dout = nullptr;
    hipError_t e = hipMalloc(&da, std::max<size_t>(a_bytes, 16));
    if (e == hipSuccess) e = hipMalloc(&db, std::max<size_t>(b_bytes, 16));
    if (e == hipSuccess) e = hipMalloc(&dout, std::max<size_t>(o_bytes, 16));
    if (e == hipSuccess && a_bytes) e = hipMemcpy(da, in_a, a_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess && b_bytes) e = hipMemcpy(db, in_b, b_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = par_launch_units(kind, da, db, n, dout, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess && o_bytes) e = hipMemcpy(out, dout, o_bytes, hipMemcpyDeviceToHost);
    if (da) (void)hipFree(da);
    if (db) (void)hipFree(db);
    if (dout) (void)hipFree(dout);
    return e == hipSuccess ? PAR_OK : (e == hipErrorOutOfMemory ? PAR_ERR_OOM : PAR_ERR_HIP);
}
int par_debug_units(int device, int kind, const void* in_a, const void* in_b, int n, void* out) {
    return guarded(nullptr, [&] { return par_debug_units_impl(device, kind, in_a, in_b, n, out); });
}

static int par_render_device_slots_impl(par_context* const* ctxs, void* const* streams, const par_outputs* device_outs,
                                        int n_slots, int row_begin, int row_end, int first_frame, int n_frames,
                                        unsigned flags) {
    if (!ctxs || !streams || !device_outs || n_slots < 1 || n_frames < 0 || first_frame < 0) return PAR_ERR_INVALID_ARG;
    if (flags & ~PAR_ACCEPTED_FLAGS) return PAR_ERR_INVALID_ARG;
    if (n_slots > 1) flags |= PAR_RENDER_PIPELINED;  // several frames in flight: throughput before latency
    for (int f = first_frame; f < first_frame + n_frames; f++) {
        const int k = f % n_slots;
        const int rc = par_render_device(ctxs[k], streams[k], row_begin, row_end, &device_outs[k], flags);
        if (rc != PAR_OK) return rc;
    }
    return PAR_OK;
}
int par_render_device_slots(par_context* const* ctxs, void* const* streams, const par_outputs* device_outs, int n_slots,
                            int row_begin, int row_end, int first_frame, int n_frames, unsigned flags) {
    return guarded(nullptr, [&] {
        return par_render_device_slots_impl(ctxs, streams, device_outs, n_slots, row_begin, row_end, first_frame,
                                            n_frames, flags);
    });
}

// ---- sharded frames: the background (context-free: the parameters say all that is needed) ----------------
int par_background_fill(const par_params* p, void* stream, par_color* rows, int n_rows) {
    if (!p || n_rows < 0 || (n_rows > 0 && !rows) || p->width <= 0 || !(p->ambient >= 0.f && p->ambient <= 1.f)) {
        return PAR_ERR_INVALID_ARG;
    }
    const uint32_t ch = (uint32_t)(uint8_t)((float)p->background * p->ambient);  // Color{127,127,127,0} * ambient
    const hipError_t e = par_launch_background(rows, (size_t)n_rows * (size_t)p->width, ch | (ch << 8) | (ch << 16),
                                               (hipStream_t)stream);
    return e == hipSuccess ? PAR_OK : PAR_ERR_HIP;
}

// ---- the exported entry points of the bodies above: no exception leaves the library -----------------------
int par_set_sprites(par_context* ctx, const par_sprite* sprites, int n_sprites) {
    return guarded(ctx, [&] { return par_set_sprites_impl(ctx, sprites, n_sprites); });
}
int par_set_entities(par_context* ctx, const par_aabb* aabbs, const int32_t* sprite_ids, int n) {
    return guarded(ctx, [&] { return par_set_entities_impl(ctx, aabbs, sprite_ids, n); });
}
int par_set_entities_ref_layout(par_context* ctx, const par_aabb* aabbs, const par_sprite* sprite_per_entity, int n) {
    return guarded(ctx, [&] { return par_set_entities_ref_layout_impl(ctx, aabbs, sprite_per_entity, n); });
}
int par_update_aabbs(par_context* ctx, const par_aabb* aabbs, int first, int n) {
    return guarded(ctx, [&] { return par_update_aabbs_impl(ctx, aabbs, first, n); });
}
int par_update_aabbs_async(par_context* ctx, const par_aabb* aabbs, int first, int n, void* stream_v) {
    return guarded(ctx, [&] { return par_update_aabbs_async_impl(ctx, aabbs, first, n, stream_v); });
}
int par_pick(par_context* ctx, int x, int y, par_pixel* out) {
    return guarded(ctx, [&] { return par_pick_impl(ctx, x, y, out); });
}
int par_read_grid(par_context* ctx, int32_t* count, int32_t* map, par_aabb* bins) {
    return guarded(ctx, [&] { return par_read_grid_impl(ctx, count, map, bins); });
}
int par_graph_capture(par_context* ctx, void* stream_v, int row_begin, int row_end, const par_outputs* device_out, unsigned flags) {
    return guarded(ctx, [&] { return graph_capture(ctx, stream_v, row_begin, row_end, device_out, flags, false); });
}
int par_graph_stage(par_context* ctx, const par_aabb* aabbs, int first, int n, const par_light* light) {
    return guarded(ctx, [&] { return graph_stage(ctx, aabbs, first, n, light, light ? 1 : 0, true); });
}
int par_graph_capture_lights(par_context* ctx, void* stream, int row_begin, int row_end, const par_outputs* device_out,
                             unsigned flags) {
    return guarded(ctx, [&] { return graph_capture(ctx, stream, row_begin, row_end, device_out, flags, true); });
}
int par_graph_stage_lights(par_context* ctx, const par_aabb* aabbs, int first, int n, const par_light* lights,
                           int n_lights) {
    return guarded(ctx, [&] { return graph_stage(ctx, aabbs, first, n, lights, n_lights, false); });
}
int par_get_stats(par_context* ctx, par_frame_stats* stats) {
    return guarded(ctx, [&] { return par_get_stats_impl(ctx, stats); });
}
int par_create(const par_params* params, int device, par_context** out) {
    return guarded(nullptr, [&] { return par_create_impl(params, device, out); });
}

int par_set_light(par_context* ctx, const par_light* light) {
    return guarded(ctx, [&] { return par_set_light_impl(ctx, light); });
}
int par_set_lights(par_context* ctx, const par_light* lights, int n) {
    return guarded(ctx, [&] { return par_set_lights_impl(ctx, lights, n); });
}
int par_set_light_model(par_context* ctx, int model) {
    return guarded(ctx, [&] { return par_set_light_model_impl(ctx, model); });
}
int par_set_light_tints(par_context* ctx, const par_light_tint* tints, int n) {
    return guarded(ctx, [&] { return par_set_light_tints_impl(ctx, tints, n); });
}
int par_render(par_context* ctx, const par_outputs* host_out, unsigned flags) {
    return guarded(ctx, [&] { return par_render_impl(ctx, host_out, flags); });
}
int par_render_rows(par_context* ctx, int row_begin, int row_end, const par_outputs* host_out, unsigned flags) {
    return guarded(ctx, [&] { return par_render_rows_impl(ctx, row_begin, row_end, host_out, flags); });
}
int par_render_device(par_context* ctx, void* stream, int row_begin, int row_end, const par_outputs* device_out, unsigned flags) {
    return guarded(ctx, [&] { return par_render_device_impl(ctx, stream, row_begin, row_end, device_out, flags); });
}
int par_render_device_timed(par_context* ctx, void* stream, int row_begin, int row_end, const par_outputs* device_out, unsigned flags, par_frame_stats* stats) {
    return guarded(ctx, [&] { return par_render_device_timed_impl(ctx, stream, row_begin, row_end, device_out, flags, stats); });
}
int par_relight_device(par_context* ctx, void* stream, int row_begin, int row_end, const par_pixel* gbuf,
                       const par_outputs* device_out, unsigned flags) {
    return guarded(ctx, [&] { return par_relight_device_impl(ctx, stream, row_begin, row_end, gbuf, device_out, flags); });
}
int par_relight_rows(par_context* ctx, int row_begin, int row_end, const par_outputs* host_out, unsigned flags) {
    return guarded(ctx, [&] { return par_relight_rows_impl(ctx, row_begin, row_end, host_out, flags); });
}
int par_graph_launch(par_context* ctx, void* stream) {
    return guarded(ctx, [&] { return par_graph_launch_impl(ctx, stream); });
}

}  // extern "C"

// par_hostcall.h — what the host sides of the passes over finished planes share (par_outline.hip, par_quantize.hip,
// par_present.hip, par_finish.hip, par_upscale.hip): the surface descriptor's check and the cut of a call's rows into
// launches, and the spans of the tile storage that par_tileset_extend_host copies, in plain C++, and for units compiled
// as HIP the opening and the bookkeeping of the *_host forms: the device a call runs on, its device buffers and its
// status. Host code only; nothing here knows a par_context.
#ifndef PAR_HOSTCALL_H
#define PAR_HOSTCALL_H

#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "par_raytracer.h"

// The scales, the byte order and the pitch of a surface `width` source pixels wide.
inline bool present_desc_ok(const par_present_desc* d, int width) {
    if (d->scale_x < 1 || d->scale_x > PAR_MAX_SCALE || d->scale_y < 1 || d->scale_y > PAR_MAX_SCALE) return false;
    if (d->order != PAR_PRESENT_RGBA && d->order != PAR_PRESENT_BGRA) return false;
    // (a pitch is an int32: a row of more bytes than that has no valid pitch)
    return (d->pitch & 3) == 0 && (int64_t)d->pitch >= 4 * (int64_t)width * (int64_t)d->scale_x;
}

// rows of one launch of a kernel that takes a tile row per blockIdx.y: the grid's y extent, and the launch's pixels
// below 2^31
constexpr uint32_t PAR_MAX_TILE_ROWS = 65535u;
constexpr uint32_t PAR_MAX_LAUNCH_PX = 0x7FFFFFF0u;

// Rows [row_begin, row_end) of a frame W pixels wide in launches of whole tile rows, tile_h rows each: at most
// PAR_MAX_TILE_ROWS tile rows and at most PAR_MAX_LAUNCH_PX pixels a launch (a single tile row is never cut). One launch
// for any frame below 2^31 pixels and 65535 tile rows. Calls launch(ra, rb, tile_rows) for rows [ra, rb) in order;
// `launch` returns its status as an int, and the first that is not 0 ends the walk and is returned.
template <class Launch>
int par_tile_row_cuts(int row_begin, int row_end, uint32_t W, uint32_t tile_h, Launch launch) {
    const uint32_t by_px = std::max<uint32_t>(1u, PAR_MAX_LAUNCH_PX / W / tile_h);
    const uint32_t tile_rows_per_launch = std::min(PAR_MAX_TILE_ROWS, by_px);
    for (int ra = row_begin; ra < row_end;) {
        const uint32_t tile_rows = std::min<uint32_t>(tile_rows_per_launch, ((uint32_t)(row_end - ra) + tile_h - 1) / tile_h);
        const int rb = (int)std::min<int64_t>((int64_t)row_end, (int64_t)ra + (int64_t)tile_rows * tile_h);
        const int status = launch(ra, rb, tile_rows);
        if (status != 0) return status;
        ra = rb;
    }
    return 0;
}

// The bytes of `tiles` that par_tileset_extend_host moves for a set of `capacity` tiles of tile_bytes bytes that held
// count_in tiles before the call and count_out after it (count_in <= count_out; either may exceed the capacity): up, the
// stored tiles [0, min(count_in, capacity)); down, the added ones [min(count_in, capacity), min(count_out, capacity)).
// Nothing beyond capacity * tile_bytes is ever named, and the caller's bytes from min(count_out, capacity) tiles on stay.
struct par_tile_spans {
    size_t upload_bytes, download_offset, download_bytes;
};
inline par_tile_spans par_tileset_extend_spans(uint64_t count_in, uint64_t count_out, uint64_t capacity, size_t tile_bytes) {
    const uint64_t stored = std::min(count_in, capacity), kept = std::max(stored, std::min(count_out, capacity));
    return {(size_t)stored * tile_bytes, (size_t)stored * tile_bytes, (size_t)(kept - stored) * tile_bytes};
}

#ifdef __HIP__
#include <hip/hip_runtime.h>

#include <cstring>

// The device of a *_host call or of a context: a negative *device becomes the current device. PAR_ERR_NO_DEVICE
// without a device or when it is no gfx950 (the kernels are built for that alone), PAR_ERR_INVALID_ARG for an index
// past the last device. It does not make the device current. The one definition: the core library and every add-on
// compile it from here, and no library links another for it.
inline int par_select_device(int* device) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return PAR_ERR_NO_DEVICE;
    if (*device < 0) {
        if (hipGetDevice(device) != hipSuccess) return PAR_ERR_NO_DEVICE;
    }
    if (*device >= ndev) return PAR_ERR_INVALID_ARG;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, *device) != hipSuccess) return PAR_ERR_NO_DEVICE;
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return PAR_ERR_NO_DEVICE;  // kernels are built for gfx950 only
    return PAR_OK;
}

// (par_status itself is the enumeration of par_raytracer.h)
inline int par_status_of(hipError_t e) {
    return e == hipSuccess ? PAR_OK : (e == hipErrorOutOfMemory ? PAR_ERR_OOM : PAR_ERR_HIP);
}

// A device buffer of a *_host call, freed at the end of its scope. The buffers of a call share the call's status: a
// buffer is in use when the status is hipSuccess, `host` is not null and `bytes` is not 0, and is then allocated and,
// when `upload`, filled from `host`; else it stays null and nothing is done. The first error stays in the status.
class par_device_buffer {
public:
    par_device_buffer(hipError_t& status, const void* host, size_t bytes, bool upload) : e_(status), bytes_(bytes) {
        if (e_ != hipSuccess || !host || !bytes) return;
        e_ = hipMalloc(&p_, bytes);
        if (e_ == hipSuccess && upload) e_ = hipMemcpy(p_, host, bytes, hipMemcpyHostToDevice);
    }
    ~par_device_buffer() {
        if (p_) (void)hipFree(p_);
    }
    par_device_buffer(const par_device_buffer&) = delete;
    par_device_buffer& operator=(const par_device_buffer&) = delete;
    template <class T>
    T* as() const {
        return static_cast<T*>(p_);
    }
    // the whole buffer to `host`, where it is in use
    void download(void* host) {
        if (e_ == hipSuccess && p_) e_ = hipMemcpy(host, p_, bytes_, hipMemcpyDeviceToHost);
    }

private:
    hipError_t& e_;
    void* p_ = nullptr;
    size_t bytes_;
};
#endif

#endif

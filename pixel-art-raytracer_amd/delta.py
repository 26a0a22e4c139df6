"""A frame in host memory, kept up to date by the tiles that changed.

A window, a file writer, an encoder or a network sink wants every frame on the host, and copying a whole `fb` plane back
costs a couple of hundred times what rendering it does. In a frame loop almost nothing on screen changes from one frame
to the next, so FrameDelta compares the new frame with the previous one on the device (a swap chain holds it in its other
slot), packs the bin-sized tiles that differ, and copies only those: changed -> pack_counted -> fetch -> apply, all on
the frame's own stream, with one wait (in the fetch). When more tiles changed than the buffers were sized for, the whole
block is copied instead.

Host-side plumbing over the C ABI (par_tiles_changed_device and its neighbours in include/par_raytracer.h); a C++ host
does the same with the four calls and a pinned buffer."""
import ctypes as C
import os

import torch

from . import ParError, tiles_apply_host, tiles_changed, tiles_fetch, tiles_pack_counted
from .types import COLOR

# The changed share of the grid up to which this path beats one pinned copy of the whole plane: the largest fraction of
# the sweep in DESIGN section 8c, "Changed tiles" (4096 x 4096: 15 % 816 us and 20 % 1159 us against the copy's 1186 us,
# 25 % 2024 us) at which it still wins. The default capacity is this share of grid-x * grid-y, rounded down (at least 1).
DEFAULT_CAPACITY_SHARE = 0.2


class FrameDelta:
    """The host's copy of rows `rows` of a frame. `frame` is the whole host frame (height * width COLOR entries, pinned);
    rows outside the block are never written."""

    def __init__(self, params, rows=None, capacity=None, device=0):
        self.params = params
        self.rows = tuple(rows) if rows else (0, params.height)
        gx, gy, _ = params.grid_dims()
        self.tiles_in_grid = gx * gy
        if capacity is None:
            capacity = max(1, int(self.tiles_in_grid * DEFAULT_CAPACITY_SHARE))
        self.capacity = capacity
        slot = params.bin_size * params.bin_size
        dev = torch.device("cuda", device)
        self._d_map = torch.zeros(self.tiles_in_grid, dtype=torch.int32, device=dev)
        self._d_tiles = torch.zeros(max(capacity, 1), dtype=torch.int32, device=dev)
        self._d_count = torch.zeros(1, dtype=torch.int32, device=dev)
        self._d_packed = torch.zeros(max(capacity, 1) * slot * 4, dtype=torch.uint8, device=dev)
        # pinned staging for the list and the slots, and the pinned host frame
        self._h_tiles = torch.zeros(max(capacity, 1), dtype=torch.int32).pin_memory()
        self._h_packed = torch.zeros(max(capacity, 1) * slot * 4, dtype=torch.uint8).pin_memory()
        self._h_frame = torch.zeros(params.height * params.width * 4, dtype=torch.uint8).pin_memory()
        self.frame = self._h_frame.numpy().view(COLOR)

    def _block_bytes(self):
        r0, r1 = self.rows
        return r0 * self.params.width * 4, (r1 - r0) * self.params.width * 4

    def first(self, d_fb, stream=0):
        """The whole block, from the device plane at `d_fb` (an int; it addresses row rows[0]), into the host frame."""
        at, n = self._block_bytes()
        _copy_to_host(self._h_frame.data_ptr() + at, d_fb, n, stream)

    def update(self, d_prev, d_cur, stream=0):
        """The host frame holds the plane at `d_prev`; make it hold the one at `d_cur` (device pointers as ints, each
        addressing row rows[0]). Returns (tiles changed, whether the whole block was copied instead)."""
        p, cap = self.params, self.capacity
        tiles_changed(p, d_prev, d_cur, self.rows, self._d_map.data_ptr(), self._d_tiles.data_ptr(), cap,
                      self._d_count.data_ptr(), stream)
        tiles_pack_counted(p, self._d_tiles.data_ptr(), self._d_count.data_ptr(), cap, d_cur, self.rows,
                           self._d_packed.data_ptr(), stream)
        n, count = tiles_fetch(p, self._d_count.data_ptr(), self._d_tiles.data_ptr(), self._d_packed.data_ptr(), cap,
                               self._h_tiles.data_ptr(), self._h_packed.data_ptr(), stream)
        if count > cap:
            self.first(d_cur, stream)
            return count, True
        tiles_apply_host(p, self._h_tiles.data_ptr(), n, self._h_packed.data_ptr(), self.rows, self._h_frame.data_ptr())
        return count, False


_hip = None


def _hip_runtime():
    """The HIP runtime this process already holds (torch's own copy where it ships one)."""
    global _hip
    if _hip is None:
        bundled = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
        _hip = C.CDLL(bundled if os.path.exists(bundled) else "libamdhip64.so")
        _hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        _hip.hipStreamSynchronize.argtypes = [C.c_void_p]
    return _hip


def _copy_to_host(host, device, nbytes, stream):
    """One device-to-host copy on `stream` and a wait for it."""
    hip = _hip_runtime()
    rc = hip.hipMemcpyAsync(host, device, nbytes, 2, stream)  # hipMemcpyDeviceToHost
    if rc == 0:
        rc = hip.hipStreamSynchronize(stream)
    if rc != 0:
        raise ParError(3, f"copying the frame block to the host failed with HIP error {rc}")

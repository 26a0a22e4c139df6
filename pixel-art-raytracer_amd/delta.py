"""A frame in host memory, kept up to date by the tiles that changed.

A window, a file writer, an encoder or a network sink wants every frame on the host, and copying a whole `fb` plane back
costs a couple of hundred times what rendering it does. In a frame loop almost nothing on screen changes from one frame
to the next, so FrameDelta compares the new frame with the previous one on the device (a swap chain holds it in its other
slot), packs the bin-sized tiles that differ, and copies only those: changed -> pack_counted -> fetch -> apply, all on
the frame's own stream, with one wait (in the fetch). When more tiles changed than the buffers were sized for, the whole
block is copied instead.

Host-side plumbing over the C ABI (par_tiles_changed_device and its neighbours in include/par_raytracer.h); a C++ host
does the same with the four calls and a pinned buffer. With elem_bytes 1 or 28 the plane is an index plane (palidx, lit,
the index plane of palette output, the edge plane of outlines) or the G-buffer, through the par_plane_tiles_* calls."""
import torch

from . import (ParError, hip_runtime, plane_tiles_apply_host, plane_tiles_changed, plane_tiles_fetch,
               plane_tiles_pack_counted, tiles_apply_host, tiles_changed, tiles_fetch, tiles_pack_counted)
from .types import COLOR, PIXEL

# The changed share of the grid up to which this path beats one pinned copy of the whole plane: the largest fraction of
# the sweep in DESIGN section 8c, "Changed tiles" (4096 x 4096: 15 % 816 us and 20 % 1159 us against the copy's 1186 us,
# 25 % 2024 us) at which it still wins. The default capacity is this share of grid-x * grid-y, rounded down (at least 1).
# The share is the same for every element size. Measured since ("Plane tiles", 4096 x 4096): the
# 28-byte G-buffer breaks even where fb does (it wins at 20 %, 7569 us against 8234 us, and loses at 25 %), but a 1-byte
# plane does so between 9 % and 10 % (298 us against the copy's 303 us, then 324 us), so for elem_bytes == 1 a share of
# 0.2 is clearly too high: up to 589 us against 304 us at 20 %. A caller with such a plane passes `capacity`; a default
# share per element size is a one-line change here, backed by those rows.
DEFAULT_CAPACITY_SHARE = 0.2

# what `frame` is a view of, by element size
_FRAME_DTYPES = {1: "u1", 4: COLOR, 28: PIXEL}


class FrameDelta:
    """The host's copy of rows `rows` of a frame. `frame` is the whole host frame (height * width entries, pinned: COLOR
    for the 4-byte planes, uint8 for the 1-byte ones, PIXEL for the G-buffer); rows outside the block are never written."""

    def __init__(self, params, rows=None, capacity=None, device=0, elem_bytes=4):
        if elem_bytes not in _FRAME_DTYPES:
            raise ParError(1, f"FrameDelta: elements of {elem_bytes} bytes (1, 4 or 28)")
        self.params = params
        self.elem_bytes = elem_bytes
        # the 4-byte plane keeps the calls it always made; the other sizes take the plane calls
        if elem_bytes == 4:
            self._changed, self._pack_counted, self._fetch, self._apply = (tiles_changed, tiles_pack_counted, tiles_fetch,
                                                                           tiles_apply_host)
        else:
            self._changed, self._pack_counted, self._fetch, self._apply = (
                _sized(f, elem_bytes) for f in (plane_tiles_changed, plane_tiles_pack_counted, plane_tiles_fetch,
                                                plane_tiles_apply_host))
        self.rows = tuple(rows) if rows else (0, params.height)
        gx, gy, _ = params.grid_dims()
        self.tiles_in_grid = gx * gy
        if capacity is None:
            capacity = max(1, int(self.tiles_in_grid * DEFAULT_CAPACITY_SHARE))
        self.capacity = capacity
        slot = params.bin_size * params.bin_size * elem_bytes
        dev = torch.device("cuda", device)
        self._d_map = torch.zeros(self.tiles_in_grid, dtype=torch.int32, device=dev)
        self._d_tiles = torch.zeros(max(capacity, 1), dtype=torch.int32, device=dev)
        self._d_count = torch.zeros(1, dtype=torch.int32, device=dev)
        self._d_packed = torch.zeros(max(capacity, 1) * slot, dtype=torch.uint8, device=dev)
        # pinned staging for the list and the slots, and the pinned host frame
        self._h_tiles = torch.zeros(max(capacity, 1), dtype=torch.int32).pin_memory()
        self._h_packed = torch.zeros(max(capacity, 1) * slot, dtype=torch.uint8).pin_memory()
        self._h_frame = torch.zeros(params.height * params.width * elem_bytes, dtype=torch.uint8).pin_memory()
        self.frame = self._h_frame.numpy().view(_FRAME_DTYPES[elem_bytes])

    def _block_bytes(self):
        r0, r1 = self.rows
        return r0 * self.params.width * self.elem_bytes, (r1 - r0) * self.params.width * self.elem_bytes

    def first(self, d_fb, stream=0):
        """The whole block, from the device plane at `d_fb` (an int; it addresses row rows[0]), into the host frame."""
        at, n = self._block_bytes()
        _copy_to_host(self._h_frame.data_ptr() + at, d_fb, n, stream)

    def update(self, d_prev, d_cur, stream=0):
        """The host frame holds the plane at `d_prev`; make it hold the one at `d_cur` (device pointers as ints, each
        addressing row rows[0]). Returns (tiles changed, whether the whole block was copied instead)."""
        p, cap = self.params, self.capacity
        self._changed(p, d_prev, d_cur, self.rows, self._d_map.data_ptr(), self._d_tiles.data_ptr(), cap,
                      self._d_count.data_ptr(), stream)
        self._pack_counted(p, self._d_tiles.data_ptr(), self._d_count.data_ptr(), cap, d_cur, self.rows,
                           self._d_packed.data_ptr(), stream)
        n, count = self._fetch(p, self._d_count.data_ptr(), self._d_tiles.data_ptr(), self._d_packed.data_ptr(), cap,
                               self._h_tiles.data_ptr(), self._h_packed.data_ptr(), stream)
        if count > cap:
            self.first(d_cur, stream)
            return count, True
        self._apply(p, self._h_tiles.data_ptr(), n, self._h_packed.data_ptr(), self.rows, self._h_frame.data_ptr())
        return count, False


def _sized(call, elem_bytes):
    """A plane call with its element size filled in: the arguments that remain are its 4-byte namesake's."""
    def sized(params, *args):
        return call(params, elem_bytes, *args)
    sized.plane_call = call
    return sized


def _copy_to_host(host, device, nbytes, stream):
    """One device-to-host copy on `stream` and a wait for it."""
    hip = hip_runtime()
    rc = hip.hipMemcpyAsync(host, device, nbytes, 2, stream)  # hipMemcpyDeviceToHost
    if rc == 0:
        rc = hip.hipStreamSynchronize(stream)
    if rc != 0:
        raise ParError(3, f"copying the frame block to the host failed with HIP error {rc}")

"""GPU tests of the objects add-on (addons/include/par_objects.h): the planes drawn over, the two counts, the object table
made from two maps and its count byte for byte against the contract restated in numpy (tests/objects.py;
tests/test_objects_cpu.py holds it to a loop over objects, pixels and bits without a GPU), on buffers carved out of
guard-filled tensors (Carved of test_gpu_quantize.py). After every call the guards round every buffer are checked and the
inputs are unchanged.

The sizes, by what they cross in the implementation. The lines launch gives a wavefront a scanline and walks the table 64
records a round: n of 1, 63, 64, 65 and 130 are the edges of the rounds, and heights 37, 48 and 9 are no multiples of the
four scanlines of a workgroup. The draw launch gives a thread eight pixels at a multiple of eight: widths 61, 64 and 67
end in a partial, no and a three-pixel segment, objects at every x phase 0 .. 7 need one or two tile segments, and the
wide stores are taken at index_io phases 0 .. 7 and fb_io dword phases 0 .. 3 where all eight pixels are written.
from_maps gives a workgroup 1024 cells: 300 x 7 crosses one."""
import importlib

import numpy as np
import pytest

import objects as OB
import screen as S
import tileset as TS
import tileset_extend as TX
import vram as V
from test_gpu_quantize import GUARD, Carved
from test_gpu_tileset import upload

pytestmark = pytest.mark.gpu

OBJECTS = importlib.import_module("pixel-art-raytracer_amd.objects")  # (without the add-on's binding nothing here can run)
POISON = 0x0BADF00D
SCREENS = ((61, 37), (64, 48), (67, 9))


@pytest.fixture(scope="module")
def objects():
    return OBJECTS


def desc_struct(objects, d):
    return objects.desc(**d)


def drawn(objects, d, chr_bytes, table, pal, fb, index, bg=None, count=None, phases=(0, 0, 0, 0), with_counts=True, work=None, stream=None,
          tag=""):
    """One par_objects_draw_device on carved buffers, checked against the model. bg: None, "index" or a plane; count: None
    or the value of the device count; phases: the bytes past a 16-byte boundary of chr, pal_words, index_io and fb_io.
    Returns the model's (fb, index, bad, over)."""
    import torch
    w, h = d["width"], d["height"]
    src = {"chr": Carved(len(chr_bytes), phases[0], chr_bytes), "objects": Carved(16 * len(table), 4, table)}
    content = {"chr": chr_bytes, "objects": table}
    if pal is not None:
        src["pal_words"], content["pal_words"] = Carved(len(pal), phases[1], pal), pal
    if count is not None:
        content["count"] = np.array([count], np.uint32)
        src["count"] = Carved(4, 8, content["count"])
    if bg is not None and not isinstance(bg, str):
        src["bg_index"], content["bg_index"] = Carved(w * h, 5, bg.reshape(-1)), bg
    out = {}
    if index is not None:
        out["index_io"] = Carved(w * h, phases[2], index.reshape(-1))
    if fb is not None:
        out["fb_io"] = Carved(4 * w * h, phases[3], fb.reshape(-1))
    if with_counts:
        out["bad_out"], out["over_out"] = Carved(4, 8, np.array([POISON], np.uint32)), Carved(4, 12, np.array([POISON], np.uint32))
    work = work or Carved(objects.work_bytes(h, d["line_limit"]), 4)
    ptr = {k: v.ptr for k, v in {**src, **out}.items()}
    torch.cuda.synchronize()
    objects.draw(desc_struct(objects, d), ptr["chr"], ptr["objects"], work.ptr, pal_words=ptr.get("pal_words"), fb_io=ptr.get("fb_io"),
                 index_io=ptr.get("index_io"), count=ptr.get("count"), bg_index=ptr.get("index_io") if isinstance(bg, str) else ptr.get("bg_index"),
                 bad_out=ptr.get("bad_out"), over_out=ptr.get("over_out"), stream=stream)
    torch.cuda.synchronize()
    e_fb, e_index, e_bad, e_over = OB.draw(d, chr_bytes, table, pal, bg, fb, index, count)
    for name, buf in {**src, **out, "work": work}.items():
        assert buf.guards_intact(), f"{tag}: {name}: bytes outside the buffer were written"
    for name, buf in src.items():
        assert buf.host(np.uint8).tobytes() == np.ascontiguousarray(content[name]).view(np.uint8).tobytes(), f"{tag}: {name} was written"
    if index is not None:
        got = out["index_io"].host(np.uint8).reshape(h, w)
        wrong = np.argwhere(got != e_index)
        assert len(wrong) == 0, f"{tag}: {len(wrong)} indices differ, first at (y, x) {wrong[:3].tolist()}: {got[tuple(wrong[0])]} for {e_index[tuple(wrong[0])]}"
    if fb is not None:
        got = out["fb_io"].host(np.uint8).reshape(h, w, 4)
        wrong = np.argwhere((got != e_fb).any(axis=2))
        assert len(wrong) == 0, f"{tag}: {len(wrong)} pixels differ, first at (y, x) {wrong[:3].tolist()}"
    if with_counts:
        got = int(out["bad_out"].host(np.uint32)[0]), int(out["over_out"].host(np.uint32)[0])
        assert got == (e_bad, e_over), f"{tag}: (bad, over) is {got}, the model's {(e_bad, e_over)}"
    return e_fb, e_index, e_bad, e_over


def scene(rng, size, tile=(8, 8), fmt=V.F_4BPP_ROWS, n=40, **over):
    """A descriptor, its random tiles, table, colour words and planes: (d, chr, table, pal, fb, index)."""
    K = 1 << V.BPP[fmt]
    table_args = {k: over.pop(k) for k in ("hidden_share", "bad_share", "behind_share") if k in over}
    d = OB.desc_of(tile_w=tile[0], tile_h=tile[1], tile_format=fmt, n_tiles=9, n_objects=n, n_colors=min(256, 4 * K), sub_size=K, bg_sub_size=K,
                   width=size[0], height=size[1])
    d.update(over)
    assert set(d) == set(OB.DESC_FIELDS)
    chr_bytes = OB.random_chr(rng, d)
    table = OB.random_table(rng, d, d["n_objects"], **table_args)
    pal = rng.integers(0, 256, d["n_colors"] * S.ENTRY_BYTES[d["pal_format"]], dtype=np.uint8)
    fb = rng.integers(0, 256, (size[1], size[0], 4), dtype=np.uint8)
    index = rng.integers(0, d["n_colors"], (size[1], size[0]), dtype=np.uint8)
    return d, chr_bytes, table, pal, fb, index


# ---- 1. draw ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", V.FORMATS, ids=V.FORMAT_NAMES)
def test_draw_every_screen_tile_size_format_and_colour_format(objects, fmt):
    """The three screens, both tile sizes each way, the colour formats, both transparencies, the three limits, the null
    planes, the forms of bg_index and the ballot edges of n go round with the cases."""
    rng = np.random.default_rng(500 + fmt)
    i, seen, over = 0, set(), 0
    for size in SCREENS:
        for tile in TS.TILES:
            n = (1, 63, 64, 65, 130)[i % 5]
            d, chr_bytes, table, pal, fb, index = scene(rng, size, tile, fmt, n, line_limit=(1, 8, 128)[i % 3], pal_format=S.PAL_FORMATS[i % 4],
                                                        opaque=(i // 2) % 2, behind_share=0.3)
            want_fb, want_index = i % 5 != 3, i % 5 != 4
            bg = (None, "index", rng.integers(0, 16, (size[1], size[0]), dtype=np.uint8))[i % 3]
            if not want_index and isinstance(bg, str):
                bg = None
            e = drawn(objects, d, chr_bytes, table, pal if want_fb or i % 2 else None, fb if want_fb else None, index if want_index else None, bg,
                      with_counts=i % 7 != 6, tag=f"{V.FORMAT_NAMES[fmt]} {size} of {tile}, n {n}, case {i}")
            seen.add((want_fb, want_index))
            over += e[3]
            i += 1
    assert seen == {(True, True), (False, True), (True, False)} and over > 0


def test_draw_every_x_phase_edge_and_flip(objects):
    """One object at every x from -17 to the width + 1 and a few y round the edges, under every flip: one or two tile
    segments under the thread's pixels, clipped left and right; then a row of objects at phases 0 .. 7 side by side."""
    rng = np.random.default_rng(21)
    for tile, size in (((8, 8), (61, 9)), ((16, 16), (67, 9)), ((16, 8), (64, 9))):
        d, chr_bytes, _, pal, fb, index = scene(rng, size, tile, V.F_4BPP_PACKED_HI, 1)
        xs = list(range(-tile[0] - 1, size[0] + 2))
        d = dict(d, n_objects=len(xs), line_limit=128)
        for flips in range(4):
            for y in (-tile[1] + 1, 0, size[1] - 1):
                table = OB.objects_of([(x, y, (x + 20) % 9, flips << 8 | (x & 3)) for x in xs])
                # every object alone on the screen: draw each through a count of one? No: all at once, the lowest wins
                drawn(objects, d, chr_bytes, table, pal, fb, index, tag=f"{tile} flips {flips} y {y}")
        spaced = OB.objects_of([(k * (tile[0] + 1) + k % 8 - 3, 1 - k % 3, k % 9, (k % 4) << 8) for k in range(size[0] // (tile[0] + 1) + 1)])
        drawn(objects, dict(d, n_objects=len(spaced), opaque=1), chr_bytes, spaced, pal, fb, index, tag=f"{tile} spaced")


def test_draw_a_line_with_more_objects_than_the_limit(objects):
    rng = np.random.default_rng(22)
    for limit in (1, 8, 128):
        n = limit + 1 + (limit == 128) * 1
        d, chr_bytes, _, pal, fb, index = scene(rng, (64, 48), (8, 16), V.F_2BPP_ROWS, n, line_limit=limit)
        table = OB.objects_of([((5 * j) % 60, 10 + j % 2, j % 9, j % 4) for j in range(n)])
        e = drawn(objects, d, chr_bytes, table, pal, fb, index, tag=f"{n} on a line of {limit}")
        assert e[3] > 0
        if limit < 128:
            more = drawn(objects, dict(d, line_limit=limit + 2), chr_bytes, table, pal, fb, index, tag="a larger limit")
            assert more[3] < e[3] and more[1].tobytes() != e[1].tobytes()


def test_draw_behind_with_each_form_of_bg_index(objects):
    rng = np.random.default_rng(23)
    d, chr_bytes, table, pal, fb, index = scene(rng, (61, 37), (8, 8), V.F_4BPP_ROWS, 65, behind_share=0.6, hidden_share=0.0, bg_sub_size=4)
    index = rng.integers(0, 16, index.shape, dtype=np.uint8)
    free = drawn(objects, d, chr_bytes, table, pal, fb, index, None, tag="bg_index null")
    own = drawn(objects, d, chr_bytes, table, pal, fb, index, "index", tag="bg_index is index_io")
    other = rng.integers(0, 16, index.shape, dtype=np.uint8)
    apart = drawn(objects, d, chr_bytes, table, pal, fb, index, other, tag="bg_index apart")
    assert len({free[1].tobytes(), own[1].tobytes(), apart[1].tobytes()}) == 3
    same = drawn(objects, d, chr_bytes, table, pal, fb, index, index.copy(), tag="bg_index a copy of index_io")
    assert same[1].tobytes() == own[1].tobytes() and same[0].tobytes() == own[0].tobytes()
    drawn(objects, dict(d, bg_sub_size=1), chr_bytes, table, pal, fb, index, "index", tag="bg_sub_size 1: nothing is opaque")


def test_draw_pal_base_and_the_clamp(objects):
    rng = np.random.default_rng(24)
    for n_colors, K, base in ((13, 4, 0), (64, 16, 48), (256, 16, 255), (1, 16, 0), (200, 256, 100), (7, 3, 2)):
        d, chr_bytes, table, pal, fb, index = scene(rng, (64, 9), (8, 8), V.F_4BPP_PACKED_LO, 63, n_colors=n_colors, sub_size=K, pal_base=base,
                                                    bad_share=0.0, hidden_share=0.0)
        e = drawn(objects, d, chr_bytes, table, pal, fb, np.zeros_like(index), tag=f"{n_colors} colours of K {K} from {base}")
        assert int(e[1].max()) == n_colors - 1, "the clamp is met"


def test_draw_hidden_bad_and_the_device_count(objects):
    """A count below, equal to and above n_objects, 0 among them; tables all hidden and all bad: consequence 3 on the
    device, guards included."""
    rng = np.random.default_rng(25)
    d, chr_bytes, table, pal, fb, index = scene(rng, (67, 9), (16, 8), V.F_4BPP_ROW_PLANES, 130, hidden_share=0.3, bad_share=0.3)
    results = {}
    for count in (None, 0, 1, 64, 129, 130, 131, 1 << 31):
        results[count] = e = drawn(objects, d, chr_bytes, table, pal, fb, index, count=count, tag=f"count {count}")
        assert e[2] <= OB.judge(d, table, 130)[1].sum()
    assert results[None][2] == results[130][2] == results[131][2] == results[1 << 31][2] > results[64][2] > 0
    assert results[0][1].tobytes() == index.tobytes() and results[0][0].tobytes() == fb.tobytes() and results[0][2:] == (0, 0)
    hidden = table.copy()
    hidden["attr"] |= OB.HIDDEN
    e = drawn(objects, d, chr_bytes, hidden, pal, fb, index, tag="all hidden")
    assert e[1].tobytes() == index.tobytes() and e[2:] == (0, 0)
    wrong = table.copy()
    wrong["attr"] &= ~OB.HIDDEN
    wrong["tile"][::2], wrong["x"][1::2] = 9, 40000
    e = drawn(objects, d, chr_bytes, wrong, pal, fb, index, tag="all bad")
    assert e[1].tobytes() == index.tobytes() and e[0].tobytes() == fb.tobytes() and e[2:] == (130, 0)


def test_draw_every_byte_phase(objects):
    """chr and pal_words at every byte phase, index_io at 0 .. 7 and fb_io at every dword phase of 16 bytes, under opaque
    objects on a grid (whole segments: the wide stores) with others across them (partial segments)."""
    rng = np.random.default_rng(26)
    i = 0
    for a in range(4):
        for b in range(8):
            size = (64, 9) if i % 2 else (61, 9)
            d, chr_bytes, _, pal, fb, index = scene(rng, size, (8, 8), V.FORMATS[i % 7], 1, pal_format=S.PAL_FORMATS[i % 4], opaque=1)
            grid = [(8 * k, 0, k % 9, k % 4 | (k % 4) << 8) for k in range(0, 8, 1 + i % 2)] + [(3 + 11 * k, 4, k % 9, OB.FLIP_X) for k in range(5)]
            table = OB.objects_of(grid)
            drawn(objects, dict(d, n_objects=len(table), line_limit=128), chr_bytes, table, pal, fb, index,
                  phases=(a, (a + 2 * b + 1) % 4, b, 4 * ((a + b) % 4)), tag=f"phases {a} {b}, case {i}")
            i += 1


def test_draw_on_a_dirty_work_block_twice(objects):
    rng = np.random.default_rng(27)
    d, chr_bytes, table, pal, fb, index = scene(rng, (64, 48), (8, 8), V.F_2BPP_PLANAR, 130, line_limit=8)
    work = Carved(objects.work_bytes(48, 8), 4, rng.integers(0, 256, objects.work_bytes(48, 8), dtype=np.uint8))
    first = drawn(objects, d, chr_bytes, table, pal, fb, index, work=work, tag="a dirty block")
    again = drawn(objects, d, chr_bytes, table, pal, fb, index, work=work, tag="the same block again")
    assert first[1].tobytes() == again[1].tobytes() and first[2:] == again[2:]
    other = OB.random_table(rng, d, 130)
    drawn(objects, d, chr_bytes, other, pal, fb, index, work=work, count=3, tag="the block after a larger table")


def test_consequences_4_to_7_on_the_device(objects):
    rng = np.random.default_rng(28)
    d, chr_bytes, table, pal, fb, index = scene(rng, (61, 37), (8, 8), V.F_4BPP_ROWS, 65, line_limit=128, bad_share=0.0, hidden_share=0.0)
    _, _, most = OB.lines(d, table, 65)
    full = drawn(objects, d, chr_bytes, table, pal, fb, index, tag="limit 128")
    tight = drawn(objects, dict(d, line_limit=most), chr_bytes, table, pal, fb, index, tag="the largest line count")
    assert full[3] == tight[3] == 0 and full[1].tobytes() == tight[1].tobytes()
    # (5) a flip for tiles stored mirrored
    tiles = V.decode_tiles(chr_bytes, (8, 8), V.F_4BPP_ROWS)
    for axis, bit in ((2, OB.FLIP_X), (1, OB.FLIP_Y)):
        flipped = table.copy()
        flipped["attr"] ^= bit
        e = drawn(objects, d, V.encode_tiles(np.ascontiguousarray(np.flip(tiles, axis=axis)), (8, 8), V.F_4BPP_ROWS)[0], flipped, pal, fb, index, tag=f"axis {axis}")
        assert e[1].tobytes() == full[1].tobytes() and e[0].tobytes() == full[0].tobytes()
    # (6) colour words or their widened table
    for fmt in (S.BGR555, S.BGR333_MD, S.BGR222):
        words = rng.integers(0, 256, d["n_colors"] * S.ENTRY_BYTES[fmt], dtype=np.uint8)
        a = drawn(objects, dict(d, pal_format=fmt), chr_bytes, table, words, fb, index, tag=f"format {fmt}")
        b = drawn(objects, d, chr_bytes, table, S.palette_rgba(words, fmt).reshape(-1), fb, index, tag="its rgba")
        assert a[0].tobytes() == b[0].tobytes()
    # (7) objects on a grid share no pixel
    apart = OB.objects_of([(8 * (k % 7) + 2, 9 * (k // 7), k % 9, k % 4 | (k % 4) << 8) for k in range(28)])
    dd = dict(d, n_objects=28)
    base = drawn(objects, dd, chr_bytes, apart, pal, fb, index, tag="apart")
    e = drawn(objects, dd, chr_bytes, apart[rng.permutation(28)], pal, fb, index, tag="permuted")
    assert e[1].tobytes() == base[1].tobytes() and e[0].tobytes() == base[0].tobytes()


def test_draw_captured_and_replayed_after_the_table_and_the_planes_changed(objects):
    import torch
    rng = np.random.default_rng(29)
    d, chr_bytes, _, pal, _, _ = scene(rng, (61, 37), (8, 16), V.F_4BPP_ROWS, 65, line_limit=8)
    cases = [(OB.random_table(rng, d, 65, behind_share=0.3), rng.integers(0, 256, (37, 61, 4), dtype=np.uint8),
              rng.integers(0, 16, (37, 61), dtype=np.uint8), count) for count in (65, 7, 0, 64)]
    c_chr, c_pal, c_table, c_count = Carved(len(chr_bytes), 1, chr_bytes), Carved(len(pal), 2, pal), Carved(16 * 65, 4), Carved(4, 4)
    c_fb, c_index, c_work, c_bad, c_over = Carved(4 * 61 * 37, 4), Carved(61 * 37, 3), Carved(objects.work_bytes(37, 8), 8), Carved(4, 4), Carved(4, 8)
    stream = torch.cuda.Stream()
    ds = desc_struct(objects, d)

    def load(k):
        upload(c_table, cases[k][0])
        upload(c_fb, cases[k][1].reshape(-1))
        upload(c_index, cases[k][2].reshape(-1))
        upload(c_count, np.array([cases[k][3]], np.uint32))
        torch.cuda.synchronize()

    def launch():
        objects.draw(ds, c_chr.ptr, c_table.ptr, c_work.ptr, pal_words=c_pal.ptr, fb_io=c_fb.ptr, index_io=c_index.ptr, count=c_count.ptr,
                     bg_index=c_index.ptr, bad_out=c_bad.ptr, over_out=c_over.ptr, stream=stream.cuda_stream)

    def check(k, tag):
        table, fb, index, count = cases[k]
        e = OB.draw(d, chr_bytes, table, pal, "index", fb, index, count)
        assert all(b.guards_intact() for b in (c_chr, c_pal, c_table, c_count, c_fb, c_index, c_work, c_bad, c_over)), tag
        assert c_index.host(np.uint8).tobytes() == e[1].tobytes() and c_fb.host(np.uint8).tobytes() == e[0].tobytes(), tag
        assert (int(c_bad.host(np.uint32)[0]), int(c_over.host(np.uint32)[0])) == e[2:], tag

    load(0)
    launch()
    stream.synchronize()
    check(0, "eagerly")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        launch()
    for k in (1, 2, 3, 0):
        load(k)
        with torch.cuda.stream(stream):
            graph.replay()
        stream.synchronize()
        check(k, f"replay {k}")


# ---- 2. from_maps ----------------------------------------------------------------------------------------------------------

def maps_of(rng, n, differing):
    """Two maps of n cells and their cell bytes that differ at exactly the cells `differing` (a bool array)."""
    a = rng.integers(0, 500, n).astype(np.uint32) | rng.integers(0, 4, n).astype(np.uint32) << 30
    ca = rng.integers(0, 8, n, dtype=np.uint8)
    how = rng.integers(0, 3, n)
    b = np.where(differing & (how != 2), a ^ np.where(how == 0, np.uint32(1), np.uint32(1 << 31)), a).astype(np.uint32)
    cb = np.where(differing & (how == 2), ca ^ 1, ca).astype(np.uint8)
    return a, b, ca, cb


def made(objects, grid, tile, a, b, ca, cb, capacity, origin=(0, 0), with_cells=True, tag=""):
    import torch
    n = grid[0] * grid[1]
    src = {"map_bg": Carved(4 * n, 4, a), "map": Carved(4 * n, 8, b)}
    content = {"map_bg": a, "map": b}
    if with_cells:
        src["cells_bg"], src["cells"] = Carved(n, 1, ca), Carved(n, 3, cb)
        content["cells_bg"], content["cells"] = ca, cb
    out, count, work = Carved(16 * capacity, 4), Carved(4, 12, np.array([POISON], np.uint32)), Carved(objects.from_maps_work_bytes(n), 4)
    torch.cuda.synchronize()
    objects.from_maps(src["map_bg"].ptr, src["map"].ptr, grid, tile, capacity, work.ptr, out.ptr, count.ptr,
                      cells_bg=src["cells_bg"].ptr if with_cells else None, cells=src["cells"].ptr if with_cells else None, origin=origin)
    torch.cuda.synchronize()
    e, total = OB.from_maps(a, b, grid, tile, capacity, ca if with_cells else None, cb if with_cells else None, origin)
    for name, buf in {**src, "objects_out": out, "count_out": count, "work": work}.items():
        assert buf.guards_intact(), f"{tag}: {name}: bytes outside the buffer were written"
    for name, buf in src.items():
        assert buf.host(np.uint8).tobytes() == np.ascontiguousarray(content[name]).view(np.uint8).tobytes(), f"{tag}: {name} was written"
    assert int(count.host(np.uint32)[0]) == total, f"{tag}: D is {int(count.host(np.uint32)[0])}, the model's {total}"
    got = out.host(np.uint8)
    assert got[:16 * len(e)].tobytes() == e.tobytes(), f"{tag}: the records"
    assert (got[16 * len(e):] == GUARD).all(), f"{tag}: records beyond min(D, capacity) were written"
    return e, total


@pytest.mark.parametrize("grid", [(1, 1), (8, 6), (61, 3), (300, 7)], ids=lambda g: f"{g[0]}x{g[1]}")
def test_from_maps_every_grid_count_and_capacity(objects, grid):
    rng = np.random.default_rng(grid[0])
    n = grid[0] * grid[1]
    for k, (tag, differing) in enumerate((("none", np.zeros(n, bool)), ("one", np.arange(n) == n - 1), ("all", np.ones(n, bool)),
                                          ("some", rng.random(n) < 0.3))):
        a, b, ca, cb = maps_of(rng, n, differing)
        total = int(differing.sum())
        for capacity in sorted({1, max(1, total - 1), max(1, total), total + 1}):
            for with_cells in (True, False):
                if not with_cells:
                    differing_now = a != b
                    e, got = made(objects, grid, TS.TILES[k], a, b, ca, cb, capacity, (-7, 5), False, f"{grid} {tag} capacity {capacity}, no cells")
                    assert got == int(differing_now.sum())
                else:
                    e, got = made(objects, grid, TS.TILES[k], a, b, ca, cb, capacity, (3, -9), True, f"{grid} {tag} capacity {capacity}")
                    assert got == total and len(e) == min(total, capacity)


# ---- 3. the host forms -----------------------------------------------------------------------------------------------------

def test_host_forms(objects):
    rng = np.random.default_rng(31)
    d, chr_bytes, table, pal, fb, index = scene(rng, (67, 37), (8, 16), V.F_4BPP_PACKED_HI, 130, pal_format=S.BGR333_MD, line_limit=8,
                                                behind_share=0.4)
    keep = [a.copy() for a in (chr_bytes, table, pal, fb, index)]
    ds = desc_struct(objects, d)
    for bg, count in ((None, None), ("index", 100), (rng.integers(0, 16, index.shape, dtype=np.uint8), 0)):
        got = objects.draw_host(ds, chr_bytes, table, pal, fb=fb, index=index, count=count, bg_index=bg, device=0)
        e = OB.draw(d, chr_bytes, table, pal, bg, fb, index, count)
        assert sorted(got) == ["bad", "fb", "index", "over"] and (got["bad"], got["over"]) == e[2:]
        assert got["fb"].tobytes() == e[0].tobytes() and got["index"].tobytes() == e[1].tobytes()
    got = objects.draw_host(ds, chr_bytes, table, index=index)
    assert got["fb"] is None and got["index"].tobytes() == OB.draw(d, chr_bytes, table, None, None, None, index)[1].tobytes()
    got = objects.draw_host(ds, chr_bytes, table, pal, fb=fb)
    assert got["index"] is None and got["fb"].tobytes() == OB.draw(d, chr_bytes, table, pal, None, fb, None)[0].tobytes()
    assert all(a.tobytes() == k.tobytes() for a, k in zip((chr_bytes, table, pal, fb, index), keep))
    n = 61 * 3
    a, b, ca, cb = maps_of(rng, n, rng.random(n) < 0.4)
    for capacity, cells in ((65536, True), (5, True), (40, False)):
        got = objects.from_maps_host(a, b, (61, 3), (16, 8), capacity, cells_bg=ca if cells else None, cells=cb if cells else None, origin=(-20, 4))
        e, total = OB.from_maps(a, b, (61, 3), (16, 8), capacity, ca if cells else None, cb if cells else None, (-20, 4))
        assert got["count"] == total and got["objects"].tobytes() == e.tobytes()


# ---- 4. the chain: consequence 1 through the device calls ------------------------------------------------------------------

class Frames:
    """A kept background and a frame over it on the device: test_gpu_vram.py's Chain builds the set from the first plane and
    encodes its map; the second plane is made local and extends the set, the set is encoded again, both maps are drawn
    (par_screen_draw_device; the second one as the answer), and from_maps and the object draw turn the first screen into
    the second. The grid is 8 cells wide, so a line_limit of 8 is the largest number of objects on a line."""

    def __init__(self, objects, T, w, h, cell, K, n_sub, capacity, table):
        from test_gpu_screen import Shown
        from test_gpu_vram import Chain
        self.objects = objects
        self.vram = importlib.import_module("pixel-art-raytracer_amd.vram")
        self.screen = importlib.import_module("pixel-art-raytracer_amd.screen")
        self.tileset = importlib.import_module("pixel-art-raytracer_amd.tileset")
        self.extend = importlib.import_module("pixel-art-raytracer_amd.tileset_extend")
        self.chain = c = Chain(self.vram, self.tileset, T, w, h, cell, K, V.SNES, 3, capacity)
        self.shown, self.answer = Shown(self.screen, c, table, n_sub), Shown(self.screen, c, table, n_sub)
        self.index, self.local, self.chosen = Carved(w * h, 2), Carved(w * h, 1), Carved(c.n, 3)
        self.work = Carved(self.extend.tileset_extend_work_bytes(c.n, capacity), 0)
        self.tile_map, self.words = Carved(4 * c.n, 4), Carved(2 * c.n, 1)
        self.bad_tiles, self.bad_cells = Carved(4, 4), Carved(4, 8)
        self.table, self.count, self.maps_work = Carved(16 * c.n, 4), Carved(4, 4), Carved(objects.from_maps_work_bytes(c.n), 4)
        self.draw_work, self.bad, self.over = Carved(objects.work_bytes(h, 8), 4), Carved(4, 4), Carved(4, 12)
        self.d = OB.desc_of(tile_format=c.fmt, n_tiles=capacity, n_objects=c.n, line_limit=8, n_colors=n_sub * K, sub_size=K, bg_sub_size=K,
                            opaque=1, width=w, height=h)
        self.desc = desc_struct(objects, self.d)
        self.outputs = (self.local, self.work, self.tile_map, self.words, self.bad_tiles, self.bad_cells, self.table, self.count, self.maps_work,
                        self.draw_work, self.bad, self.over, *self.shown.outputs, *self.answer.outputs)

    def launch_background(self, stream=None):
        self.chain.launch(stream=stream)

    def launch_frame(self, stream=None):
        c, v, s = self.chain, self.vram, stream
        v.local(self.index.ptr, c.w * c.h, c.sub_size, self.local.ptr, stream=s)
        self.extend.tileset_extend(c.params, self.local.ptr, (0, c.h), (8, 8), self.work.ptr, c.tiles.ptr, c.capacity, c.count.ptr,
                                   map_out=self.tile_map.ptr, flips=c.flips, stream=s)
        v.encode_tiles(c.tiles.ptr, c.capacity, c.count.ptr, (8, 8), c.fmt, c.chr.ptr, bad_out=self.bad_tiles.ptr, stream=s)
        v.encode_map(c.layout, self.tile_map.ptr, (c.gcx, c.gcy), self.words.ptr, cells=self.chosen.ptr, bad_out=self.bad_cells.ptr, stream=s)
        self.shown.launch(stream=s)  # the kept background's screen
        self.screen.draw(self.answer.desc, c.chr.ptr, self.words.ptr, self.answer.pal.ptr, fb_out=self.answer.fb.ptr,
                         index_out=self.answer.index.ptr, bad_out=self.answer.bad.ptr, stream=s)
        self.objects.from_maps(c.tile_map.ptr, self.tile_map.ptr, (c.gcx, c.gcy), (8, 8), c.n, self.maps_work.ptr, self.table.ptr, self.count.ptr,
                               cells_bg=c.chosen.ptr, cells=self.chosen.ptr, stream=s)
        self.objects.draw(self.desc, c.chr.ptr, self.table.ptr, self.draw_work.ptr, pal_words=self.shown.pal.ptr, fb_io=self.shown.fb.ptr,
                          index_io=self.shown.index.ptr, count=self.count.ptr, bad_out=self.bad.ptr, over_out=self.over.ptr, stream=s)

    def check(self, plane, opaque, want_count, tag):
        for buf in (self.index, self.chosen, *self.outputs, *self.chain.outputs):
            assert buf.guards_intact(), f"{tag}: bytes outside a buffer were written"
        self.answer.check(plane[0], opaque[plane[0]], f"{tag}: the answer")
        assert int(self.count.host(np.uint32)[0]) == want_count, f"{tag}: D"
        assert (int(self.bad.host(np.uint32)[0]), int(self.over.host(np.uint32)[0])) == (0, 0), tag
        self.shown.check(plane[0], opaque[plane[0]], f"{tag}: the objects over the kept background")


def frames_and_planes(objects, T, seed, n_planes, capacity=8 * 5 * 2):
    from test_vram_cpu import cells_plane
    w, h, cell, K, n_sub = 59, 37, (8, 8), 16, 8
    rng = np.random.default_rng(seed)
    planes = [cells_plane(rng, w, h, cell, n_sub, K, kinds) for kinds in (5, 9, 17, 30)[:n_planes]]
    table = rng.integers(0, 256, (n_sub * K, 4), dtype=np.uint8)
    opaque = table.copy()
    opaque[:, 3] = 255
    return Frames(objects, T, w, h, cell, K, n_sub, capacity, table), planes, opaque


def differing_cells(planes, a, b, w=59, h=37, K=16):
    """D of two cells index planes under tile sets that mirror both ways: the cells whose canonical tile or sub-palette
    differ, or whose mirror code does."""
    maps = TX.sequence_model([planes[0][0] % K] + [p[0] % K for p in planes[1:]], w, h, (8, 8), 0, 3, 4096)[0]
    return int(((maps[a][1] != maps[b][1]) | (planes[a][1] != planes[b][1])).sum())


def load(frames, planes, bg, k):
    import torch
    for buf in (*frames.outputs, *frames.chain.outputs):
        buf.t.fill_(GUARD)
    upload(frames.chain.index, planes[bg][0])
    upload(frames.chain.chosen, planes[bg][1])
    upload(frames.index, planes[k][0])
    upload(frames.chosen, planes[k][1])
    torch.cuda.synchronize()


def test_the_closing_identity_on_one_stream(objects, T):
    import torch
    frames, planes, opaque = frames_and_planes(objects, T, 41, 2)
    stream = torch.cuda.Stream()
    load(frames, planes, 0, 1)
    frames.launch_background(stream.cuda_stream)
    frames.launch_frame(stream.cuda_stream)
    stream.synchronize()
    frames.check(planes[1], opaque, differing_cells(planes, 0, 1), "one stream, no host wait")


def test_the_closing_identity_captured_and_replayed(objects, T):
    """The frame is 59 x 37 and the set holds 80 tiles, so that no buffer read back between the replays is larger than those
    of test_gpu_screen.py's captured chain (see there for what the HIP runtime did to the four-byte fills of a replayed
    graph behind larger reads)."""
    import torch
    frames, planes, opaque = frames_and_planes(objects, T, 42, 3)
    stream = torch.cuda.Stream()

    def launch():
        frames.launch_background(stream.cuda_stream)
        frames.launch_frame(stream.cuda_stream)

    load(frames, planes, 0, 1)
    launch()
    stream.synchronize()
    frames.check(planes[1], opaque, differing_cells(planes[:2], 0, 1), "eagerly")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        launch()
    for bg, k in ((0, 2), (1, 0), (2, 2)):
        load(frames, planes, bg, k)
        with torch.cuda.stream(stream):
            graph.replay()
        stream.synchronize()
        order = [planes[bg], planes[k]]
        frames.check(planes[k], opaque, differing_cells(order, 0, 1), f"replay of {k} over {bg}")


def test_the_closing_identity_in_a_three_frame_loop(objects, T):
    """Frame 0 is the level; frames 1 to 3 extend the one kept set, each drawn as objects over frame 0's screen."""
    import torch
    frames, planes, opaque = frames_and_planes(objects, T, 43, 4, capacity=8 * 5 * 4)
    stream = torch.cuda.Stream()
    load(frames, planes, 0, 1)
    frames.launch_background(stream.cuda_stream)
    for k in (1, 2, 3):
        upload(frames.index, planes[k][0])
        upload(frames.chosen, planes[k][1])
        torch.cuda.synchronize()
        frames.launch_frame(stream.cuda_stream)
        stream.synchronize()
        frames.check(planes[k], opaque, differing_cells(planes[:k + 1], 0, k), f"frame {k}")

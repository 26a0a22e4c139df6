"""GPU tests of the screen add-on (addons/include/par_screen.h): the drawn framebuffer, the index plane, the decoded map and
the bad counts byte for byte against the contract restated in numpy (tests/screen.py; tests/test_screen_cpu.py holds it to
a loop over pixels and bits without a GPU), on buffers carved out of guard-filled tensors (Carved of test_gpu_quantize.py).
After every call the guards round every buffer are checked and the inputs are unchanged.

The sizes, by what they cross in the implementation. A draw takes a thread an eight-pixel segment of a tile row in map
space, (width + 14) / 8 segment slots a screen row and 256 threads a workgroup: screens 61, 64 and 67 wide over maps 32 and
40 (or 64 and 80) pixels wide wrap every row several times, clip the first and the last segment at every scroll phase
0 .. 7, and put several rows into one workgroup. A whole segment is stored as two 16-byte words and one 8-byte word where
the addresses allow: every byte phase of index_out (0 .. 7) and every dword phase of fb_out (0, 4, 8, 12) meet both paths.
The first map_w * map_h threads count the bad cells: 1, 63, 64, 65 and 4097 cells, and a map far larger than the screen."""
import importlib

import numpy as np
import pytest

import screen as S
import tileset as TS
import vram as V
from test_gpu_quantize import GUARD, Carved
from test_gpu_tileset import upload
from test_screen_cpu import LAYOUTS, random_vram

pytestmark = pytest.mark.gpu

SCREEN = importlib.import_module("pixel-art-raytracer_amd.screen")  # (without the add-on's binding nothing here can run)
VRAM = importlib.import_module("pixel-art-raytracer_amd.vram")
POISON = 0x0BADF00D
SCREENS = [(w, h) for w in (61, 64, 67) for h in (37, 48)]
MAPS = ((4, 3), (5, 2))


@pytest.fixture(scope="module")
def screen():
    return SCREEN


def desc_struct(screen, d):
    return screen.desc(d["layout"], **{f: d[f] for f in S.DESC_FIELDS})


def drawn(screen, d, chr_bytes, words, pal, attr=None, lines=None, phases=(0, 0, 0, 0, 0), fb=True, index=True, with_bad=True, stream=None,
          tag=""):
    """One par_screen_draw_device on carved buffers, checked against the model. phases: the bytes past a 16-byte boundary
    of chr, map_words, pal_words, index_out and fb_out. Returns (fb, index, bad) of the model."""
    import torch
    w, h = d["width"], d["height"]
    src = {"chr": Carved(len(chr_bytes), phases[0], chr_bytes), "map_words": Carved(len(words), phases[1], words)}
    if pal is not None:
        src["pal_words"] = Carved(len(pal), phases[2], pal)
    if attr is not None:
        src["attr"] = Carved(len(attr), 1, attr)
    if lines is not None:
        src["line_scroll"] = Carved(4 * len(lines), 4, lines)
    content = {"chr": chr_bytes, "map_words": words, "pal_words": pal, "attr": attr, "line_scroll": lines}
    out = {}
    if index:
        out["index_out"] = Carved(w * h, phases[3])
    if fb:
        out["fb_out"] = Carved(4 * w * h, phases[4])
    if with_bad:
        out["bad_out"] = Carved(4, 8, np.array([POISON], np.uint32))
    ptr = {k: v.ptr for k, v in {**src, **out}.items()}
    torch.cuda.synchronize()
    screen.draw(desc_struct(screen, d), ptr["chr"], ptr["map_words"], ptr.get("pal_words"), fb_out=ptr.get("fb_out"),
                index_out=ptr.get("index_out"), attr=ptr.get("attr"), line_scroll=ptr.get("line_scroll"), bad_out=ptr.get("bad_out"),
                stream=stream)
    torch.cuda.synchronize()
    e_fb, e_index, e_bad = S.draw(d, chr_bytes, words, pal, attr, lines)
    for name, buf in {**src, **out}.items():
        assert buf.guards_intact(), f"{tag}: {name}: bytes outside the buffer were written"
    for name, buf in src.items():
        assert buf.host(np.uint8).tobytes() == np.ascontiguousarray(content[name]).view(np.uint8).tobytes(), f"{tag}: {name} was written"
    if index:
        got = out["index_out"].host(np.uint8).reshape(h, w)
        wrong = np.argwhere(got != e_index)
        assert len(wrong) == 0, f"{tag}: {len(wrong)} indices differ, first at (y, x) {wrong[:3].tolist()}: {got[tuple(wrong[0])]} for {e_index[tuple(wrong[0])]}"
    if fb:
        got = out["fb_out"].host(np.uint8).reshape(h, w, 4)
        wrong = np.argwhere((got != e_fb).any(axis=2))
        assert len(wrong) == 0, f"{tag}: {len(wrong)} pixels differ, first at (y, x) {wrong[:3].tolist()}"
    if with_bad:
        got = int(out["bad_out"].host(np.uint32)[0])
        assert got == e_bad, f"{tag}: bad is {got}, the model's {e_bad}"
    return e_fb, e_index, e_bad


def scene(rng, L, fmt, tile, grid, size, pal_format=S.RGBA8, n_tiles=9, n_colors=None, sub_size=None, bad_share=0.0, **over):
    """A descriptor and its random VRAM: (d, chr, map_words, pal_words)."""
    sub_size = sub_size or 1 << V.BPP[fmt]
    n_colors = n_colors or min(256, sub_size << min(4, L["pal_bits"]))
    d = S.desc_of(L, tile_w=tile[0], tile_h=tile[1], tile_format=fmt, n_tiles=n_tiles, map_w=grid[0], map_h=grid[1], pal_format=pal_format,
                  n_colors=n_colors, sub_size=sub_size, width=size[0], height=size[1])
    d.update(over)
    return (d, *random_vram(rng, L, fmt, tile, n_tiles, grid[0], grid[1], n_colors, pal_format, bad_share))


# ---- 1. draw ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", V.FORMATS, ids=V.FORMAT_NAMES)
def test_draw_every_screen_map_tile_size_and_layout(screen, fmt):
    """The six screens over both maps, both tile sizes each way, the layouts, the colour words, the backdrop, attr, line
    scroll, the null outputs and n_colors that is no multiple of K go round with the cases."""
    rng = np.random.default_rng(100 + fmt)
    i, seen = 0, set()
    for size in SCREENS:
        for grid in MAPS:
            for tile in TS.TILES:
                name, L = LAYOUTS[i % len(LAYOUTS)]
                K = 1 << V.BPP[fmt]
                d, chr_bytes, words, pal = scene(rng, L, fmt, tile, grid, size, pal_format=S.PAL_FORMATS[i % 4], n_colors=(3 * K + 1, 4 * K, 256, 1)[i % 4],
                                                 sub_size=K, backdrop=(i // 2) % 2, scroll_x=int(rng.integers(-500, 500)),
                                                 scroll_y=int(rng.integers(-500, 500)), ratio_x=1 + (i // 3) % 2, ratio_y=1 + (i // 5) % 2)
                attr = rng.integers(0, 6, S.attr_cells(d), dtype=np.uint8) if i % 3 == 0 else None
                lines = rng.integers(-300, 300, 2 * size[1]).astype(np.int32) if i % 4 == 1 else None
                fb, index = i % 5 != 3, i % 5 != 4
                drawn(screen, d, chr_bytes, words, pal if fb or i % 2 else None, attr, lines, fb=fb, index=index, with_bad=i % 7 != 6,
                      tag=f"{V.FORMAT_NAMES[fmt]} {size} over {grid} of {tile}, {name}, case {i}")
                seen.add((fb, index))
                i += 1
    assert seen == {(True, True), (False, True), (True, False)}


@pytest.mark.parametrize("name,L", LAYOUTS, ids=[l[0] for l in LAYOUTS])
def test_draw_scroll_phases_and_wrap_seams(screen, name, L):
    """x phases 0 to 7, 8, one below the period, negative and several periods out, and the same in y, under both backdrops;
    then the ends of int32."""
    rng = np.random.default_rng(sum(name.encode()) + 1)
    machine = [n for n, _ in LAYOUTS].index(name)
    fmt = V.MACHINE_FORMATS[machine][0] if machine < 6 else V.F_4BPP_PACKED_HI
    for k, (tile, grid, size) in enumerate((((8, 8), (4, 3), (61, 37)), ((16, 8), (5, 2), (67, 37)))):
        d, chr_bytes, words, pal = scene(rng, L, fmt, tile, grid, size, backdrop=k)
        px, py = grid[0] * tile[0], grid[1] * tile[1]
        scrolls = [(s, 0) for s in range(9)] + [(px - 1, py - 1), (-1, 0), (0, -1), (-7, -9), (-px - 3, -py - 5), (5 * px + 3, 0), (0, 7 * py + 2),
                                               (-9 * px + 6, 11 * py - 1), (-(1 << 31), (1 << 31) - 1), ((1 << 31) - 1, -(1 << 31))]
        for sx, sy in scrolls:
            drawn(screen, dict(d, scroll_x=sx, scroll_y=sy), chr_bytes, words, pal, tag=f"{name} {tile} scroll ({sx}, {sy})")


def test_draw_line_scroll_with_another_phase_on_every_row(screen):
    rng = np.random.default_rng(7)
    for tile, grid, size in (((8, 8), (4, 3), (64, 48)), ((16, 16), (5, 2), (61, 37))):
        d, chr_bytes, words, pal = scene(rng, V.preset(V.SNES), V.F_4BPP_ROWS, tile, grid, size, scroll_x=3, scroll_y=-2)
        lines = np.zeros((size[1], 2), np.int32)
        lines[:, 0] = np.arange(size[1]) * 9 - 100  # (9 is odd: the phases 0 .. 7 go round, the wrap seam moves every row)
        lines[:, 1] = (np.arange(size[1]) * 5) % 23 - 11
        lines[3], lines[4] = ((1 << 31) - 1, -(1 << 31)), (-(1 << 31), (1 << 31) - 1)
        e = drawn(screen, d, chr_bytes, words, pal, lines=lines.reshape(-1), tag=f"{tile} line scroll")
        # consequence 3 on the device: a scroll of (s, 0) is that line scroll on every row
        for s in (5, -13):
            a = drawn(screen, dict(d, scroll_x=3 + s), chr_bytes, words, pal, tag="scrolled")
            b = drawn(screen, d, chr_bytes, words, pal, lines=np.tile(np.array([s, 0], np.int32), size[1]), tag="by lines")
            assert a[1].tobytes() == b[1].tobytes() and a[0].tobytes() == b[0].tobytes()
        assert e[1].tobytes() != a[1].tobytes()


def test_draw_attr_at_both_ratios_with_an_odd_map_width(screen):
    """The NES way: a word without a palette field under an attribute grid, whose last colour cell of a row is ragged."""
    rng = np.random.default_rng(8)
    for ratio in ((1, 1), (2, 2), (2, 1), (1, 2)):
        for L, fmt in ((V.preset(V.NES), V.F_2BPP_PLANAR), (V.preset(V.SNES), V.F_4BPP_ROWS)):
            d, chr_bytes, words, pal = scene(rng, L, fmt, (8, 8), (5, 3), (67, 37), n_colors=16, ratio_x=ratio[0], ratio_y=ratio[1], scroll_x=-5,
                                             scroll_y=4)
            attr = rng.integers(0, 4, S.attr_cells(d), dtype=np.uint8)
            with_attr = drawn(screen, d, chr_bytes, words, pal, attr=attr, tag=f"attr at ratio {ratio}")
            without = drawn(screen, d, chr_bytes, words, pal, tag="without attr")
            assert with_attr[1].tobytes() != without[1].tobytes(), "attr replaces the word's palette"


def test_draw_clamps_at_n_colors(screen):
    """n_colors that is no multiple of K, and sub-palettes past the table: the clamp of present."""
    rng = np.random.default_rng(9)
    for n_colors, K in ((13, 4), (5, 16), (1, 16), (255, 16), (256, 256), (7, 3)):
        d, chr_bytes, words, pal = scene(rng, V.preset(V.GBA), V.F_4BPP_PACKED_LO, (8, 8), (4, 3), (64, 37), n_colors=n_colors, sub_size=K, scroll_x=2)
        e = drawn(screen, d, chr_bytes, words, pal, tag=f"{n_colors} colours of K {K}")
        assert int(e[1].max()) == n_colors - 1, "the clamp is met"


def test_draw_every_byte_phase(screen):
    """chr, map_words, pal_words at every byte phase, index_out at 0 .. 7 (its whole segments are 8-byte stores where they
    can be) and fb_out at every dword phase of 16 bytes, under scroll phases that move the segments."""
    rng = np.random.default_rng(10)
    i = 0
    for a in range(4):
        for b in range(8):
            L = (V.preset(V.MEGADRIVE), V.preset(V.NES), LAYOUTS[6][1])[i % 3]
            fmt = V.FORMATS[i % 7]
            d, chr_bytes, words, pal = scene(rng, L, fmt, TS.TILES[i % 4], MAPS[i % 2], (64, 37) if i % 2 else (61, 37),
                                             pal_format=S.PAL_FORMATS[i % 4], scroll_x=i % 9, scroll_y=i)
            drawn(screen, d, chr_bytes, words, pal, phases=(a, (a + b) % 4, (a + 2 * b + 1) % 4, b, 4 * ((a + b) % 4)),
                  tag=f"phases {a} {b}, case {i}")
            i += 1


# ---- 2. bad cells ----------------------------------------------------------------------------------------------------------

def test_each_bad_condition_alone(screen):
    L = V.layout_of(tile_step=4, tile_base=16)
    chr_bytes = V.encode_tiles(np.full((3, 8, 8), 2, np.uint8), (8, 8), V.F_4BPP_ROWS)[0]
    pal = np.arange(64, dtype=np.uint8)

    def row(*cells):
        return np.frombuffer(b"".join((t | p << 10).to_bytes(2, "little") for t, p in cells), dtype=np.uint8)

    d = S.desc_of(L, n_tiles=3, map_w=6, map_h=1, width=48, height=8)
    clean = [(16, 1), (20, 1), (24, 1), (16, 0), (20, 2), (24, 3)]
    assert drawn(screen, d, chr_bytes, row(*clean), pal, tag="clean")[2] == 0
    for tag, at, t in (("below the base", 1, 12), ("a remainder", 2, 22), ("past n_tiles", 3, 28), ("t 0", 4, 0), ("far past", 5, 1020)):
        cells = list(clean)
        cells[at] = (t, 1)
        e = drawn(screen, d, chr_bytes, row(*cells), pal, tag=tag)
        assert e[2] == 1 and (e[1][:, 8 * at:8 * at + 8] == 0).all() and int((e[1] == 0).sum()) == 64, tag
    e = drawn(screen, dict(d, width=8), chr_bytes, row((16, 1), (12, 1), (22, 1), (28, 1), (24, 1), (20, 0)), pal, tag="three, off-screen")
    assert e[2] == 3 and (e[1] == 6).all()


def test_a_map_whose_bad_cells_are_mostly_off_screen(screen):
    rng = np.random.default_rng(11)
    d, chr_bytes, words, pal = scene(rng, V.preset(V.SNES), V.F_4BPP_ROWS, (8, 8), (40, 30), (64, 48), bad_share=0.8, scroll_x=-3, scroll_y=5)
    e = drawn(screen, d, chr_bytes, words, pal, tag="40 x 30 cells, most bad")
    assert 800 < e[2] < 1200 and (e[1] != 0).any()
    drawn(screen, d, chr_bytes, words, pal, with_bad=False, tag="and without a bad_out")


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_bad_count_of_map_cell_counts(screen, n):
    rng = np.random.default_rng(n)
    for k, grid in enumerate(((n, 1), (1, n))):
        name, L = LAYOUTS[(n + 3 * k) % len(LAYOUTS)]
        d, chr_bytes, words, pal = scene(rng, L, V.F_2BPP_ROWS, (8, 8), grid, (24, 16), bad_share=0.5, scroll_x=n)
        e = drawn(screen, d, chr_bytes, words, pal, fb=bool(k), tag=f"{grid} cells, {name}")
        assert e[2] > 0 or n == 1
    ones = scene(rng, V.preset(V.SNES), V.F_2BPP_ROWS, (8, 8), (n, 1), (8, 8), bad_share=1.0)
    assert drawn(screen, *ones, tag="all bad")[2] == n


# ---- 3. limits -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", [(4096, 8), (8, 4096)], ids=["4096 x 8", "8 x 4096"])
def test_the_widest_and_the_tallest_screen(screen, size):
    rng = np.random.default_rng(size[0])
    d, chr_bytes, words, pal = scene(rng, V.preset(V.GBC), V.F_2BPP_ROWS, (8, 16), (5, 2), size, pal_format=S.BGR555, scroll_x=-3, scroll_y=9)
    lines = rng.integers(-99, 99, 2 * size[1]).astype(np.int32)
    drawn(screen, d, chr_bytes, words, pal, lines=lines, phases=(1, 2, 3, 5, 4), tag=f"{size}")


def test_the_largest_map_under_a_small_screen(screen):
    rng = np.random.default_rng(12)
    d, chr_bytes, words, pal = scene(rng, LAYOUTS[6][1], V.F_4BPP_ROWS, (16, 16), (1024, 1024), (64, 64), n_tiles=1000, bad_share=0.1,
                                     scroll_x=16 * 1024 - 20, scroll_y=-(16 * 1000 + 7))
    e = drawn(screen, d, chr_bytes, words, pal, tag="1024 x 1024 cells")
    assert 90000 < e[2] < 120000


# ---- 4. decode_map ---------------------------------------------------------------------------------------------------------

def decoded(screen, L, words, n, phase=0, with_pal=True, with_bad=True, tag=""):
    import torch
    src = Carved(len(words), phase, words)
    out, pal = Carved(4 * n, 4), Carved(n, 1) if with_pal else None
    bad = Carved(4, 4, np.array([POISON], np.uint32)) if with_bad else None
    torch.cuda.synchronize()
    screen.decode_map(screen.MapLayout(*(L[f] for f in V.FIELDS)), src.ptr, n, out.ptr, pal_out=pal.ptr if pal else None,
                      bad_out=bad.ptr if bad else None)
    torch.cuda.synchronize()
    e_map, e_pal, e_bad = S.decode_map(L, words)
    for name, buf in (("map_words", src), ("map_out", out), ("pal_out", pal), ("bad_out", bad)):
        assert buf is None or buf.guards_intact(), f"{tag}: {name}: bytes outside the buffer were written"
    assert src.host(np.uint8).tobytes() == words.tobytes(), f"{tag}: the words were written"
    assert out.host(np.uint32).tobytes() == e_map.tobytes(), f"{tag}: the map"
    assert pal is None or pal.host(np.uint8).tobytes() == e_pal.tobytes(), f"{tag}: the palettes"
    assert bad is None or int(bad.host(np.uint32)[0]) == e_bad, f"{tag}: bad"
    return e_map, e_pal, e_bad


DECODE_LAYOUTS = LAYOUTS + [
    ("one byte", V.layout_of(word_bytes=1, tile_bits=4, pal_shift=4, pal_bits=2, flip_x_bit=6, flip_y_bit=7, tile_step=3, tile_base=2)),
    ("four bytes, little, a whole-word tile", V.layout_of(word_bytes=4, tile_bits=32, pal_shift=32, pal_bits=0, flip_x_bit=-1, flip_y_bit=-1,
                                                          tile_step=16, tile_base=65535)),
    ("two bytes, big, no flips", V.layout_of(big_endian=1, tile_bits=16, pal_bits=0, flip_x_bit=-1, flip_y_bit=-1))]


@pytest.mark.parametrize("name,L", DECODE_LAYOUTS, ids=[l[0] for l in DECODE_LAYOUTS])
def test_decode_map_every_layout_and_its_round_trip(screen, name, L):
    rng = np.random.default_rng(sum(name.encode()) + 2)
    for i, n in enumerate((1, 63, 64, 65, 4097)):
        noise = rng.integers(0, 256, n * L["word_bytes"], dtype=np.uint8)
        decoded(screen, L, noise, n, phase=i % 4, with_pal=i % 2 == 0, with_bad=i % 3 != 2, tag=f"{name}: {n} words of noise")
        # consequence 7: what encode_map wrote without counting comes back
        ids = rng.integers(0, 1 << min(12, L["tile_bits"]), n).astype(np.uint32)
        ids = np.minimum(ids, np.uint32(max(0, ((1 << L["tile_bits"]) - 1 - L["tile_base"]) // L["tile_step"])))
        fx = rng.integers(0, 2, n).astype(np.uint32) * np.uint32(L["flip_x_bit"] >= 0)
        fy = rng.integers(0, 2, n).astype(np.uint32) * np.uint32(L["flip_y_bit"] >= 0)
        tile_map = ids | fx << 30 | fy << 31
        cells = rng.integers(0, 1 << min(8, L["pal_bits"]), n, dtype=np.uint8)
        words, n_bad = V.encode_map(L, tile_map, n, 1, cells)
        assert n_bad == 0
        e_map, e_pal, e_bad = decoded(screen, L, words, n, phase=(i + 1) % 4, tag=f"{name}: {n} words of encode_map")
        assert e_map.tobytes() == tile_map.tobytes() and e_pal.tobytes() == cells.tobytes() and e_bad == 0


def test_decode_map_of_encode_map_on_the_device(screen):
    """par_vram_encode_map_device then par_screen_decode_map_device on one stream: the map and the cells come back."""
    import torch
    rng = np.random.default_rng(13)
    n = 9 * 7
    tile_map = (rng.integers(0, 1024, n).astype(np.uint32) | (rng.integers(0, 4, n).astype(np.uint32) << 30))
    cells = rng.integers(0, 8, n, dtype=np.uint8)
    src, chosen, words, back, pal, bad = Carved(4 * n, 4, tile_map), Carved(n, 1, cells), Carved(2 * n, 3), Carved(4 * n, 8), Carved(n, 3), Carved(4, 4)
    L = V.preset(V.SNES)
    torch.cuda.synchronize()
    VRAM.encode_map(VRAM.MapLayout(*V.PRESETS[V.SNES]), src.ptr, (9, 7), words.ptr, cells=chosen.ptr)
    screen.decode_map(screen.MapLayout(*(L[f] for f in V.FIELDS)), words.ptr, n, back.ptr, pal_out=pal.ptr, bad_out=bad.ptr)
    torch.cuda.synchronize()
    assert all(b.guards_intact() for b in (src, chosen, words, back, pal, bad))
    assert back.host(np.uint32).tobytes() == tile_map.tobytes() and pal.host(np.uint8).tobytes() == cells.tobytes()
    assert int(bad.host(np.uint32)[0]) == 0


# ---- 5. the host forms -----------------------------------------------------------------------------------------------------

def test_host_forms(screen):
    rng = np.random.default_rng(14)
    d, chr_bytes, words, pal = scene(rng, V.preset(V.MEGADRIVE), V.F_4BPP_PACKED_HI, (8, 16), (5, 2), (67, 37), pal_format=S.BGR333_MD,
                                     bad_share=0.2, scroll_x=-11, scroll_y=70, backdrop=1, ratio_x=2)
    attr = rng.integers(0, 4, S.attr_cells(d), dtype=np.uint8)
    lines = rng.integers(-50, 50, 2 * 37).astype(np.int32)
    keep = [a.copy() for a in (chr_bytes, words, pal, attr, lines)]
    for a, l in ((None, None), (attr, lines)):
        got = screen.draw_host(desc_struct(screen, d), chr_bytes, words, pal, attr=a, line_scroll=l, device=0)
        e_fb, e_index, e_bad = S.draw(d, chr_bytes, words, pal, a, l)
        assert sorted(got) == ["bad", "fb", "index"] and got["bad"] == e_bad > 0
        assert got["fb"].tobytes() == e_fb.tobytes() and got["index"].tobytes() == e_index.tobytes()
    got = screen.draw_host(desc_struct(screen, d), chr_bytes, words, fb=False)
    assert got["fb"] is None and got["index"].tobytes() == S.draw(d, chr_bytes, words)[1].tobytes()
    got = screen.draw_host(desc_struct(screen, d), chr_bytes, words, pal, index=False)
    assert got["index"] is None and got["fb"].tobytes() == S.draw(d, chr_bytes, words, pal)[0].tobytes()
    assert all(a.tobytes() == k.tobytes() for a, k in zip((chr_bytes, words, pal, attr, lines), keep))
    got = screen.decode_map_host(screen.MapLayout(*V.PRESETS[V.MEGADRIVE]), words)
    e_map, e_pal, e_bad = S.decode_map(V.preset(V.MEGADRIVE), words)
    assert got["map"].tobytes() == e_map.tobytes() and got["pal"].tobytes() == e_pal.tobytes() and got["bad"] == e_bad == 0
    # the anchors of the header through the device: tile 5, palette 3, x flip
    for machine, word in ((V.SNES, [0x05, 0x4C]), (V.MEGADRIVE, [0x68, 0x05]), (V.GBA, [0x05, 0x34])):
        got = screen.decode_map_host(screen.MapLayout(*V.PRESETS[machine]), np.array(word, np.uint8))
        assert got["map"].tolist() == [5 | 1 << 30] and got["pal"].tolist() == [3] and got["bad"] == 0, V.MACHINES[machine]


# ---- 6. captured -----------------------------------------------------------------------------------------------------------

class Shown:
    """The screen behind a Chain of test_gpu_vram.py: its export drawn at scroll 0 on a screen the size of the frame,
    through RGBA8 entries."""

    def __init__(self, screen, chain, table, n_sub):
        self.screen, self.chain = screen, chain
        self.d = S.desc_of(chain.L, tile_format=chain.fmt, n_tiles=chain.capacity, map_w=chain.gcx, map_h=chain.gcy, n_colors=n_sub * chain.sub_size,
                           sub_size=chain.sub_size, width=chain.w, height=chain.h)
        self.desc = desc_struct(screen, self.d)
        self.pal = Carved(table.size, 2, table.reshape(-1))
        self.fb, self.index, self.bad = Carved(4 * chain.w * chain.h, 4), Carved(chain.w * chain.h, 3), Carved(4, 4)
        self.outputs = (self.fb, self.index, self.bad)

    def launch(self, stream=None):
        self.screen.draw(self.desc, self.chain.chr.ptr, self.chain.words.ptr, self.pal.ptr, fb_out=self.fb.ptr, index_out=self.index.ptr,
                         bad_out=self.bad.ptr, stream=stream)

    def check(self, index, fb, tag):
        for buf in (self.pal, *self.outputs):
            assert buf.guards_intact(), f"{tag}: bytes outside a buffer were written"
        assert int(self.bad.host(np.uint32)[0]) == 0, tag
        assert self.index.host(np.uint8).tobytes() == index.tobytes(), f"{tag}: index_out is not the cells index plane"
        assert self.fb.host(np.uint8).tobytes() == fb.tobytes(), f"{tag}: fb_out is not the cells frame with alpha 255"


def test_captured_chain_replayed_on_another_plane(screen, T):
    """local -> build -> encode tiles -> encode map -> draw captured with torch.cuda.graph after one eager run, replayed on
    other planes: the closing identity holds for every replay. The frame is 59 x 37 (ragged under the 16 x 16 cells and
    the 8 x 8 tiles), so that no buffer read back between the replays is larger than those of test_gpu_vram.py's captured
    chain, which that test shows to be safe: with a read of 35 KiB before the capture and between the replays, the HIP
    runtime replayed the four-byte fills of the bad counts of that chain, without any screen call in the graph, with
    bytes of other data (0x59595959 for 0)."""
    import torch
    from test_gpu_vram import Chain
    from test_vram_cpu import cells_plane
    tileset = importlib.import_module("pixel-art-raytracer_amd.tileset")
    w, h, cell = 59, 37, (16, 16)
    rng = np.random.default_rng(61)
    planes = [cells_plane(rng, w, h, cell, 8, 16, kinds) for kinds in (3, 17, 40)]
    table = rng.integers(0, 256, (8 * 16, 4), dtype=np.uint8)
    opaque = table.copy()
    opaque[:, 3] = 255
    chain = Chain(VRAM, tileset, T, w, h, cell, 16, V.SNES, 3, 8 * 5)
    shown = Shown(screen, chain, table, 8)
    stream = torch.cuda.Stream()

    def load(k):
        for buf in (*chain.outputs, *shown.outputs):
            buf.t.fill_(GUARD)
        upload(chain.index, planes[k][0])
        upload(chain.chosen, planes[k][1])
        torch.cuda.synchronize()

    def launch():
        chain.launch(stream=stream.cuda_stream)
        shown.launch(stream=stream.cuda_stream)

    load(0)
    launch()
    stream.synchronize()
    chain.check(*planes[0], "eagerly")
    shown.check(planes[0][0], opaque[planes[0][0]], "eagerly")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        launch()
    counts = set()
    for k in (1, 2, 0):
        load(k)
        with torch.cuda.stream(stream):
            graph.replay()
        stream.synchronize()
        counts.add(chain.check(*planes[k], f"replay on plane {k}")["count"])
        shown.check(planes[k][0], opaque[planes[k][0]], f"replay on plane {k}")
    assert len(counts) == 3, "the planes differ in their tile counts"


# ---- 7. in a frame loop ----------------------------------------------------------------------------------------------------

def test_in_a_frame_loop(par, screen, oracle, T):
    """The graybox scene under two tinted ranged lights: render_device, the palette fitted at 33, the cells fitted at 8 x 4
    over 8 x 8 cells, the frame quantised under that table, the local plane, its tile set under both mirrors, the set and
    the map encoded for the SNES, and the screen drawn from those bytes, all on the frame's stream with one wait at the
    end. The screen is the cells frame (the closing identity)."""
    import torch
    import cells as CL
    import cells_fit as CF
    import palette as P
    from test_gpu_light_range import scene as light_scene
    from test_gpu_light_tints import COLOUR, TINTS, expected
    from test_gpu_lights_graph import Planes as FramePlanes
    from test_gpu_palette import Block, garbage_work
    from test_gpu_parity import ALL, assert_planes_equal
    from test_gpu_vram import Chain

    cells = importlib.import_module("pixel-art-raytracer_amd.cells")
    fit = importlib.import_module("pixel-art-raytracer_amd.cells_fit")
    tileset = importlib.import_module("pixel-art-raytracer_amd.tileset")
    sc = light_scene("graybox", par, oracle, T)
    params = sc.params
    W, H = params.width, params.height
    lights, exp, _ = expected(T, sc, [3, 6], [200, 300], TINTS[:2], COLOUR, "graybox, two tinted ranged lights")
    fb = exp["fb"]
    N, CELL, SUBS, K = 33, (8, 8), 8, 4
    master = P.fit(T, fb, N)[0]
    e_table = CF.model(fb, W, H, CELL, master, SUBS, K, 0)[0]
    e_index, e_fb, e_chosen = CL.model(params, e_table, SUBS, K, CELL, fb, None, 0)
    e_shown = np.ascontiguousarray(e_fb).view(np.uint8).reshape(-1, 4).copy()
    e_shown[:, 3] = 255

    stream = torch.cuda.Stream()
    out = FramePlanes(params, ALL)
    block = Block(T, garbage_work(T, 85))
    d_master, d_table = Carved(4 * N, 0), Carved(4 * SUBS * K, 0)
    fit_work = Carved(fit.cells_fit_work_bytes(W, H, CELL), 0)
    chain = Chain(VRAM, tileset, T, W, H, CELL, K, V.SNES, 3, 1024)
    shown = Shown(screen, chain, np.zeros((SUBS * K, 4), np.uint8), SUBS)
    torch.cuda.synchronize()
    with sc.renderer(par, par.LIGHTS_RANGED) as r:
        r.set_lights(lights)
        r.set_light_tints(T.make_tints(TINTS[:2]))
        s = stream.cuda_stream
        r.render_device(out.ptrs, flags=par.RENDER_COUNT_RAYS, stream=s)
        par.palette_reset(block.ptr, stream=s)
        par.palette_count(params, out.ptrs["fb"], (0, H), block.ptr, stream=s)
        par.palette_cut(block.ptr, N, stream=s)
        par.palette_sum(params, out.ptrs["fb"], (0, H), block.ptr, stream=s)
        par.palette_emit(block.ptr, N, d_master.ptr, stream=s)
        fit.cells_fit(out.ptrs["fb"], W, H, CELL, d_master.ptr, N, SUBS, K, 0, fit_work.ptr, d_table.ptr, stream=s)
        cells.quantize_cells(params, d_table.ptr, SUBS, K, CELL, out.ptrs["fb"], (0, H), index_out=chain.index.ptr,
                             cell_out=chain.chosen.ptr, stream=s)
        chain.launch(stream=s)
        # the fitted table is the screen's colours, where it is: no copy
        screen.draw(shown.desc, chain.chr.ptr, chain.words.ptr, d_table.ptr, fb_out=shown.fb.ptr, index_out=shown.index.ptr,
                    bad_out=shown.bad.ptr, stream=s)
        stream.synchronize()
        assert_planes_equal(out.host(T), exp, ALL, "the frame itself")
        assert d_table.guards_intact() and d_table.host(T.COLOR).tobytes() == e_table.tobytes(), "the fitted table"
        chain.check(e_index, e_chosen, "the frame loop")
        shown.check(e_index, e_shown, "the frame loop")
        r.stats()

"""GPU tests of ALONE work items (csrc/par_internal.h par_item, csrc/par_kernels.hip render_item_alone): an entry pass
whose entry no other entry of the column can overlap skips the primary pass.

Every frame is rendered through par_render_device twice, plain and under the record-items hook (which switches the
alone and the simple items off), each time into fb + palidx (the production instantiation of the entry kernel) and into
all five planes, and equals the oracle byte for byte. After every frame the item list is read back
(par_debug_read_items, exported beside par_debug_read_stamps, outside the public header) and held to the restatement of
the rule in tests/items_alone.py: the flag sits on exactly the entries the rule calls alone, every entry has the items of
all its chunks, and an alone item carries the rectangle render_item would have worked out.

Shape A (512 x 384 x 384, bin 8, a jittered lattice of 20 x 20 x 20 boxes and the special cases) has a launch of its
own for the entry items (render_merged == 0 as launched); shape B (160 x 120 x 160, bin 40) takes render_both_kernel.
At bin 8 a tile is one 64-pixel chunk, so every column of A that shows an entry is visited as a whole tile: A's frames
are held to the oracle and must have NO entry item. So shape C: A's view and cases at bin 40, its lattice wider apart,
a sparse frame. As launched it takes render_both_kernel like B; every frame of it is rendered once more as a timed
frame without PAR_RENDER_TIMED_AS_LAUNCHED, which keeps its kernels apart (par_raytracer.h): there its entries go
through render_items_kernel's two paths, and none through a tile visit (every column that shows an entry has entry
items, asserted). Shape D (1024 x 768 x 768, bin 8, two dozen narrow boxes) is a SPARSE frame at bin 8, rendered as C
is: alone entries with ez > B (three and four start bins) and alone entries whose start bin's walk list holds exactly
1, 2 and 3 records. Shape E (2048 x 2048 x 2048, bin 40, 2 601 occupied columns, fb + palidx only) is too large for the
merged launch: as launched (PAR_RENDER_TIMED_AS_LAUNCHED, render_merged == 0, no launch for tile items) its more than
5 000 alone entries go through render_items_kernel's own launch. What the scenes hold (tests/items_alone.py scene; test_the_scenes_hold_the_cases):
rectangles one pixel apart, touching and overlapping by one pixel, side by side and one above the other; one entity in
two z bins (B, C) and in three and four (A, D); entries cut by the tile's edge and by the row range of a partial-row
render; sprite depths that carry the start bin across a bin boundary; ez > B (A, D: bin 8); from start bins of alone
entries walk lists of 1, 2 and 3 records (D), of no record, of an odd and of an even number of records, and of more
than PAR_BIN_WALK records (not recorded; C);
start bins without a walk (negative world z); a light that shares its x with a column of pixels; a sprite-id table (no
alone items); a graph capture and replay of shape B."""
import collections
import ctypes as C
import functools

import numpy as np
import pytest

import items_alone as IA
from test_gpu_lights_graph import NTHREADS, Planes, replay
from test_gpu_parity import ALL, assert_planes_equal

pytestmark = pytest.mark.gpu

FAST = ("fb", "palidx")  # the planes of a production frame
ROWS = {"A": (37, 301), "B": (13, 97), "C": (37, 301), "D": (37, 701)}
SPARSE = ("C", "D", "E")  # no column is a tile visit  # partial-row renders: neither end is a multiple of the bin size


@functools.lru_cache(maxsize=None)
def frame(shape, with_ids):
    """(params, aabbs, sprites, ids, light, the oracle's planes) of a shape. Computed once, left unchanged."""
    import importlib
    from oracle.oracle import Oracle
    par = importlib.import_module("pixel-art-raytracer_amd")
    params, aabbs, light = IA.scene(shape)
    sprites = par.tile_floor()
    ids = None
    if with_ids:
        sprites = np.concatenate([sprites, sprites])
        ids = (np.arange(len(aabbs)) % 2).astype(np.int32)
    exp = Oracle().render(params, aabbs, sprites, light, ids, nthreads=NTHREADS, planes=FAST if shape == "E" else ALL)
    return params, aabbs, sprites, ids, light, exp


def read_items(par, r):
    """The entry items of the context's last frame, eight words each."""
    fn = par.lib().par_debug_read_items  # typed by the binding's table (ABI_DEBUG_HOOKS)
    n = C.c_int(0)
    assert fn(r._ctx, None, 0, C.byref(n)) == 0
    items = np.zeros((n.value, 8), dtype=np.uint32)
    assert fn(r._ctx, items.ctypes.data_as(C.c_void_p), n.value, C.byref(n)) == 0 and n.value == len(items)
    return items


def check_items(par, r, params, rows, with_ids, hook, tag, has_items=True, every_column=False):
    """The item list against the restatement. Returns the number of alone entries. every_column: no column is a tile
    visit, so every column with an entry that shows in the rows rendered must have entry items."""
    items = read_items(par, r)
    items = items[items[:, 0] != IA.ITEM_NONE]
    count, map_, bins = r.read_grid()
    cols = IA.column_entries(params, count, map_, bins)
    by_col = collections.defaultdict(lambda: collections.defaultdict(list))
    for it in items:
        where = int(it[2])
        by_col[(where & 0x3FF, (where >> 10) & 0x3FF)][int(it[7])].append(it)
    assert bool(by_col) == has_items, f"{tag}: {len(items)} entry items"
    if every_column:
        showing = {c for c, ents in cols.items() if any(v is not None for v in IA.classify(params, ents, *c, with_ids, rows))}
        assert showing == set(by_col), f"{tag}: columns without entry items {sorted(showing ^ set(by_col))[:8]}"
    n_alone = 0
    for (bx, by), groups in by_col.items():
        ents = cols[(bx, by)]
        occupied = sorted({bz for _, _, bz in ents})
        expected = IA.classify(params, ents, bx, by, with_ids, rows)
        assert set(groups) == {ents[e][0] for e, c in enumerate(expected) if c is not None}, f"{tag}: column {bx, by}"
        for e, c in enumerate(expected):
            if c is None:
                continue
            alone, chunks, rect = c
            alone = alone and not hook
            its = groups[ents[e][0]]
            where = f"{tag}: column {bx, by} entry {e} {ents[e]}"
            assert sorted(int(it[1]) & 0xFFFF for it in its) == list(range(chunks)), where
            for it in its:
                assert bool(int(it[2]) & IA.ITEM_ALONE) == alone, f"{where}: alone should be {alone}"
                assert not (hook and int(it[2]) & IA.ITEM_SIMPLE), where
                box = ents[e][1]
                entry = (int(it[4]) & 0xFFFF, int(it[4]) >> 16, int(it[5]) & 0xFFFF, int(it[5]) >> 16, int(it[6]) & 0xFFFF,
                         int(it[6]) >> 16)
                assert entry == tuple(v & 0xFFFF for v in box), where
                if alone:
                    assert (int(it[3]) & 0xFF, (int(it[3]) >> 8) & 0xFF, (int(it[3]) >> 16) & 0xFF, int(it[3]) >> 24) == rect, where
                    assert ((int(it[1]) >> 16) & 0x3FF, int(it[1]) >> 26) == (occupied[0], len(occupied)), where
                else:
                    assert int(it[1]) >> 16 == e, where
            n_alone += alone
    return n_alone


def render_and_check(par, T, shape, rows, with_ids):
    import torch
    params, aabbs, sprites, ids, light, exp = frame(shape, with_ids)
    W = params.width
    r0, r1 = rows or (0, params.height)
    want = {k: v[r0 * W:r1 * W] for k, v in exp.items()}
    stream = torch.cuda.Stream()
    counts = {}
    with par.Renderer(params) as r:
        r.set_sprites(sprites)
        r.set_entities(aabbs, ids)
        r.set_light(light)
        for hook in (False, True):
            r.set_test_hooks(record_items=hook)
            for planes in (FAST, ALL):
                tag = f"shape {shape} rows {rows} ids {with_ids} hook {hook} planes {len(planes)}"
                out = Planes(params, planes, rows)
                r.render_device(out.ptrs, rows=rows, stream=stream.cuda_stream)
                stream.synchronize()
                assert_planes_equal(out.host(T), want, planes, tag)
                counts[(hook, planes)] = check_items(par, r, params, rows, with_ids, hook, tag, shape != "A", shape in SPARSE)
                if shape not in ("C", "D"):
                    continue
                # C and D as launched are small enough for the merged launch; a timed frame keeps its kernels apart: the
                # same items through render_items_kernel itself, and no launch for tile items
                out = Planes(params, planes, rows)
                st = r.render_device(out.ptrs, rows=rows, stream=stream.cuda_stream, timed=True)
                stream.synchronize()
                assert_planes_equal(out.host(T), want, planes, f"{tag}, kernels apart")
                # (par_frame_stats: without PAR_RENDER_TIMED_AS_LAUNCHED the kernels run apart, ms_launch stays -1 and
                # ms_render is the entry kernel's time, and the tile kernel's in a dense frame; that this frame has no
                # tile visit is check_items' every_column: every column that shows an entry has entry items)
                assert st.ms_render > 0 and all(v == -1 for v in st.ms_launch), (st.ms_render, list(st.ms_launch))
                assert check_items(par, r, params, rows, with_ids, hook, f"{tag}, kernels apart", True, True) == counts[(hook, planes)]
        r.set_test_hooks()
        if shape == "A" and rows is None:  # as launched, the frame's render kernels are not merged
            out = Planes(params, FAST)
            st = r.render_device(out.ptrs, stream=stream.cuda_stream, timed=True, flags=par.RENDER_TIMED_AS_LAUNCHED)
            stream.synchronize()
            assert_planes_equal(out.host(T), want, FAST, f"shape {shape}, timed as launched")
            assert st.render_merged == 0 and st.ms_launch[2] > 0, (list(st.ms_launch), st.render_merged)
            assert st.ms_launch[3] > 0, list(st.ms_launch)  # (A's columns are whole-tile visits: the launch for them)
        r.stats()  # raises on PAR_ERR_DEVICE
    print(f"shape {shape} rows {rows} ids {with_ids}: alone entries {counts}")
    for (hook, planes), n in counts.items():
        if hook or with_ids or shape == "A":
            assert n == 0, (hook, planes, n)
        else:
            assert n > (50 if shape in ("C", "D") else 0), (hook, planes, n)
    return counts


def test_the_scenes_hold_the_cases(oracle):
    """What the docstring promises of the scenes, from the oracle's hash (no GPU work: it guards the tests below)."""
    found = {}
    for shape in ("A", "C", "D", "E"):
        params, aabbs, light = IA.scene(shape)
        g = oracle.bin(params, aabbs)
        cols = IA.column_entries(params, g.count, g.map, g.bins)
        at = tuple(int(light[0][k]) for k in "xyz")
        exact, long_walks, alone, crowded, start_bins = set(), 0, 0, 0, set()
        for (bx, by), ents in cols.items():
            assert len(ents) <= 64 and len({bz for _, _, bz in ents}) <= 32  # (no column overflows its record)
            for e, c in enumerate(IA.classify(params, ents, bx, by, False)):
                if c is None:
                    continue
                alone += c[0]
                crowded += not c[0]
                if c[0]:
                    start_bins.add((ents[e][1][2] + ents[e][1][5]) // params.bin_size - max(ents[e][1][2], 0) // params.bin_size + 1)
                    for lo, hi in IA.start_bin_walks(params, g.count, ents, bx, by, e, at).values():
                        if lo == hi:
                            exact.add(lo)
                        long_walks += lo > IA.BIN_WALK
        found[shape] = (alone, crowded, exact, long_walks)
        if shape == "D":  # alone entries at bin 8: ez > B (three and four start bins), walk lists of 1, 2 and 3 records
            assert alone > 50 and crowded > 0 and {3, 4} <= start_bins and {0, 1, 2, 3} <= exact, (found["D"], start_bins)
        if shape == "E":  # too many columns for the merged launch
            assert len(cols) >= 2048 and alone > 5000 and crowded > 1000, (len(cols), found["E"])
        assert any(b["px"] <= at[0] < b["px"] + b["ex"] for b in aabbs)  # pixels that share the light's x
        tileable, dense_from = IA.tileable_columns(params, aabbs)
        assert (tileable >= dense_from) == (shape == "A"), (shape, tileable, dense_from)
    print({k: (v[0], v[1], sorted(v[2])[:8], v[3]) for k, v in found.items()})
    alone, crowded, exact, long_walks = found["A"]
    assert {0, 1, 2, 3} <= exact and long_walks > 0, found["A"]
    alone, crowded, exact, long_walks = found["C"]
    assert alone > 50 and crowded > 50 and long_walks > 0 and 0 in exact, found["C"]
    assert any(n % 2 for n in exact) and any(n > 0 and n % 2 == 0 for n in exact), exact


@pytest.mark.parametrize("shape", ["A", "B", "C", "D"])
def test_whole_frames(par, T, shape):
    render_and_check(par, T, shape, None, False)


@pytest.mark.parametrize("shape", ["A", "B", "C", "D"])
def test_partial_rows(par, T, shape):
    render_and_check(par, T, shape, ROWS[shape], False)


@pytest.mark.parametrize("shape", ["A", "B", "C", "D"])
def test_a_sprite_id_table_leaves_no_entry_alone(par, T, shape):
    render_and_check(par, T, shape, None, True)


def test_alone_items_through_the_entry_kernels_own_launch(par, T):
    """Shape E as a production frame launches it: more than 2 048 occupied columns, so the render kernels are not merged,
    and a sparse frame, so there is no launch for tile items: render_items_kernel itself renders the alone items."""
    import torch
    params, aabbs, sprites, ids, light, exp = frame("E", False)
    stream = torch.cuda.Stream()
    with par.Renderer(params) as r:
        r.set_sprites(sprites)
        r.set_entities(aabbs)
        r.set_light(light)
        for hook in (False, True):
            r.set_test_hooks(record_items=hook)
            out = Planes(params, FAST)
            st = r.render_device(out.ptrs, stream=stream.cuda_stream, timed=True, flags=par.RENDER_TIMED_AS_LAUNCHED)
            stream.synchronize()
            assert_planes_equal(out.host(T), exp, FAST, f"shape E hook {hook}, timed as launched")
            launches = (list(st.ms_launch), st.render_merged)
            assert st.render_merged == 0 and st.ms_launch[2] > 0 and st.ms_launch[3] == 0, launches
            n = check_items(par, r, params, None, False, hook, f"shape E hook {hook}", True, True)
            print(f"shape E hook {hook}: {n} alone entries, launches {launches}")
            assert n == 0 if hook else n > 5000, n
        r.stats()


def test_graph_replay_of_shape_b(par, T):
    import torch
    params, aabbs, sprites, ids, light, exp = frame("B", False)
    stream = torch.cuda.Stream()
    with par.Renderer(params) as r:
        r.set_sprites(sprites)
        r.set_entities(aabbs)
        r.set_light(light)
        out = Planes(params, ALL)
        r.graph_capture(out.ptrs, stream=stream.cuda_stream)
        for k in range(2):  # (both grid sets' graphs)
            assert_planes_equal(replay(r, out, stream, T), exp, ALL, f"graph replay {k}")
            assert check_items(par, r, params, None, False, False, f"graph replay {k}") > 0
        r.stats()

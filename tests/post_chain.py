"""The passes over finished planes as CHAINS: several `*_device` post calls in a row on one stream with no host wait
between, which is how a frame loop issues them and what a captured graph replays. No GPU is needed to import this module;
tests/test_gpu_post_graph.py captures the chains with it and replays them on new data, tests/test_post_chain_cpu.py says
what the chains and their inputs contain and shows on a model-backed stand-in that the driver notices what a capture can
get wrong.

  Chain        an ordered list of steps over named planes. A step names one binding of pixel-art-raytracer_amd/__init__.py
               and its keyword arguments; an argument that is a plane is a Ref (plane, byte offset). Two steps are not
               bindings: "copy" (a device-to-device copy, torch's copy_ on the device) and "poison" (a fill with POISON).
               A plane is "in" (uploaded before every replay), "history" (uploaded once; the chain's closing copies carry
               it from one replay to the next), "out" (poisoned before every replay, compared after) or "scratch"
               (poisoned, its guards checked, its contents not compared: refine's work block).
  expected()   composes the models that exist (outline, palette, palette_refine, pattern, quantize, upscale, present,
               finish, delta, plane_tiles) and nothing new. A model that takes a guard byte for the bytes a call leaves
               alone is run with two guards: the bytes that differ are the ones the call does not write, and they keep
               what the plane held.
  issue()      makes the calls on a stream, in order, with no host wait.
  check()      compares every plane byte for byte, names the first plane and offset that differ, checks every guard.
  ModelBackend the bindings over host memory, computed by the same models, with four injectable faults.

chain_a is the palette tail (outline, the five fit calls, refine, pattern dither, quantize, upscale, present), chain_b
finish and the tile calls (finish, quantize, the changed-tiles pairs on three element sizes, the pack / unpack / assemble
calls on a fixed list, the background fill, and the copies that make this frame the next one's previous frame), and
chain_frame the tail of a rendered frame (chain_a and the finish step). chain_b's changed-tiles pair at the small
capacity is a capture of its own (`small`): it needs the current frame, which the chain makes, and the previous one,
which the chain's closing copies overwrite, so the driver makes the current frame eagerly (`prologue`), replays the
small pair, poisons the current frame again and then replays the chain."""
import collections
import importlib

import numpy as np

import delta as DL
import finish as F
import outline as O
import palette as P
import palette_refine as R
import pattern as D
import plane_tiles as PT
import present as PR
import quantize as Q
import upscale as U

T = importlib.import_module("pixel-art-raytracer_amd.types")

POISON = 0xA5
GUARD = 0xEE
PAD = 256  # guard bytes before and after every plane
N_FIT = 33  # entries of the fitted palette
ROUNDS, DEPTH, STRENGTH, SPREAD = 3, 8, 256, 24
SMALL = 2  # the small capacity of the changed-tiles pair
SHAPES = {"131x67 whole": (131, 67, 8, None), "37x23 rows 5..18": (37, 23, 8, (5, 18))}
ORDER = (0, 1, 2, 0)  # the input sets of the replays of one capture

Ref = collections.namedtuple("Ref", "plane offset", defaults=(0,))
Step = collections.namedtuple("Step", "binding args")
Plane = collections.namedtuple("Plane", "name nbytes shift role kind")

# the arguments of each binding that are device pointers
POINTERS = {
    "outline": ("gbuf", "fb", "fb_out", "edge_out"),
    "quantize": ("d_palette", "fb", "fb_out", "index_out"),
    "quantize_pattern": ("d_palette", "fb", "fb_out", "index_out"),
    "palette_reset": ("work",),
    "palette_count": ("fb", "work"),
    "palette_cut": ("work",),
    "palette_sum": ("fb", "work"),
    "palette_emit": ("work", "d_palette"),
    "palette_refine_device": ("fb", "d_palette", "d_index", "work", "d_changed"),
    "present": ("out", "fb", "index", "d_palette"),
    "finish": ("out", "fb", "gbuf", "d_palette", "index_out"),
    "upscale": ("out", "fb", "index", "d_palette", "index_out"),
    "tiles_changed": ("a", "b", "d_map", "d_tiles", "d_count"),
    "tiles_pack_counted": ("d_tiles", "d_count", "fb_block", "packed"),
    "tiles_pack": ("d_tiles", "fb_block", "packed"),
    "tiles_unpack": ("d_tiles", "packed", "frame"),
    "tiles_assemble": ("d_map", "packed", "frame"),
    "background_fill": ("rows_ptr",),
    "plane_tiles_changed": ("a", "b", "d_map", "d_tiles", "d_count"),
    "plane_tiles_pack_counted": ("d_tiles", "d_count", "block", "packed"),
    "plane_tiles_pack": ("d_tiles", "block", "packed"),
    "plane_tiles_unpack": ("d_tiles", "packed", "frame"),
    "plane_tiles_assemble": ("d_map", "packed", "frame"),
}
COUNTED = ("tiles_pack_counted", "plane_tiles_pack_counted")
PSEUDO = ("copy", "poison")


class Chain:
    def __init__(self, name, params, rows=None):
        self.name, self.params = name, params
        self.rows = rows or (0, params.height)
        self.grows = O.halo(self.rows, params.height)  # the G-buffer rows outline and finish take
        self.planes, self.steps, self.prologue, self.small, self.repoison = {}, [], [], [], []

    def plane(self, name, nbytes, shift=0, role="out", kind="carved"):
        assert name not in self.planes and nbytes > 0
        self.planes[name] = Plane(name, int(nbytes), shift, role, kind)
        return Ref(name)

    def step(self, binding, **args):
        self.steps.append(Step(binding, args))
        return self.steps[-1]

    def names(self, *roles):
        return [p.name for p in self.planes.values() if p.role in roles]

    def everything(self):
        """The steps in the order a replay runs them."""
        return self.prologue + self.small + [Step("poison", {"plane": n}) for n in self.repoison] + self.steps

    def captured(self):
        """The steps that run inside a capture."""
        return self.small + self.steps

    def index_of(self, binding, nth=0):
        """The position of the nth call of `binding` among the calls (pseudo-steps not counted) of a replay."""
        calls = [s.binding for s in self.everything() if s.binding not in PSEUDO]
        return [i for i, b in enumerate(calls) if b == binding][nth]


# ---- the chains ------------------------------------------------------------------------------------------------------

def params_of(shape):
    w, h, b, rows = SHAPES[shape] if isinstance(shape, str) else shape
    return T.default_params(w, h, h, b), rows


def _frame_inputs(c):
    W = c.params.width
    c.plane("gbuf", 28 * (c.grows[1] - c.grows[0]) * W, 4, "in")
    c.plane("fb", 4 * (c.rows[1] - c.rows[0]) * W, 8, "in")


def _palette_tail(c):
    p, W, H, rows = c.params, c.params.width, c.params.height, c.rows
    n = (rows[1] - rows[0]) * W
    style = T.make_outline_style(*F.STYLE)
    lined, edge = c.plane("lined", 4 * n, 12), c.plane("edge", n, 3)
    c.step("outline", params=p, style=style, gbuf=Ref("gbuf"), gbuf_rows=c.grows, fb=Ref("fb"), rows=rows, fb_out=lined,
           edge_out=edge)
    work = c.plane("fit_work", T.PALETTE_WORK.itemsize, 8, kind="block")
    pal = c.plane("palette", 4 * N_FIT, 4, kind="call.palette")
    c.step("palette_reset", work=work)
    c.step("palette_count", params=p, fb=lined, rows=rows, work=work)
    c.step("palette_cut", work=work, n_colors=N_FIT)
    c.step("palette_sum", params=p, fb=lined, rows=rows, work=work)
    c.step("palette_emit", work=work, n_colors=N_FIT, d_palette=pal)
    rwork = c.plane("refine_work", T.PALETTE_REFINE_WORK.itemsize, 8, "scratch", "call.work")
    changed, assign = c.plane("changed", 4, 4, kind="call.changed"), c.plane("assign", n, 1)
    c.step("palette_refine_device", params=p, fb=lined, rows=rows, d_palette=pal, n_colors=N_FIT, iterations=ROUNDS,
           d_index=assign, work=rwork, d_changed=changed)
    pat_index, pat_fb = c.plane("pat_index", n, 0), c.plane("pat_fb", 4 * n, 0)
    c.step("quantize_pattern", params=p, d_palette=pal, n_colors=N_FIT, fb=lined, rows=rows, depth=DEPTH, strength=STRENGTH,
           fb_out=pat_fb, index_out=pat_index)
    index2 = c.plane("index2", n, 2)
    c.step("quantize", params=p, d_palette=pal, n_colors=N_FIT, fb=lined, rows=rows, index_out=index2, spread=SPREAD)
    # Scale3x of the index plane: a row block's output rows are those whose halo the block holds
    up = rows if rows == (0, H) else (rows[0] + 1, rows[1] - 1)
    assert U.with_halo(up, H, 3) == rows
    c.up_rows = up
    udesc = T.make_upscale_desc(3, pitch=4 * W * 3 + 4, order=T.PRESENT_BGRA)
    n_up = (up[1] - up[0]) * 3
    up_index, up_surface = c.plane("up_index", n_up * 3 * W, 1), c.plane("up_surface", n_up * int(udesc["pitch"][0]), 0)
    c.step("upscale", params=p, desc=udesc, out=up_surface, rows=up, index=pat_index, d_palette=pal, n_colors=N_FIT,
           src_rows=rows, index_out=up_index)
    pdesc = T.make_present_desc(2, 3, pitch=4 * W * 2 + 12, order=T.PRESENT_RGBA)
    surface = c.plane("surface", 3 * (rows[1] - rows[0]) * int(pdesc["pitch"][0]), 4)
    c.step("present", params=p, desc=pdesc, out=surface, rows=rows, index=pat_index, d_palette=pal, n_colors=N_FIT)


def _finish(c, n_colors):
    p, W, rows = c.params, c.params.width, c.rows
    n = (rows[1] - rows[0]) * W
    fp = c.plane("fixed_palette", 4 * n_colors, 4, "in")
    desc = T.make_present_desc(3, 2, pitch=4 * W * 3 + 8, order=T.PRESENT_BGRA)
    surface = c.plane("fin_surface", 2 * (rows[1] - rows[0]) * int(desc["pitch"][0]), 0)
    index = c.plane("fin_index", n, 2)
    c.step("finish", params=p, desc=desc, out=surface, rows=rows, fb=Ref("fb"), style=T.make_outline_style(*F.STYLE),
           gbuf=Ref("gbuf"), gbuf_rows=c.grows, d_palette=fp, n_colors=n_colors, spread=F.SPREAD, index_out=index)
    c.n_fixed = n_colors


def chain_a(shape):
    """The palette tail."""
    c = Chain("A", *params_of(shape))
    _frame_inputs(c)
    _palette_tail(c)
    return c


def chain_frame(shape, n_colors=256):
    """The tail of a rendered frame: chain A and the finish step of chain B on the frame's fb and gbuf planes."""
    c = Chain("frame", *params_of(shape))
    _frame_inputs(c)
    _palette_tail(c)
    _finish(c, n_colors)
    return c


def fixed_tiles(params, rows):
    """The fixed list of chain B: the tiles of delta.flips, which hold the block's corners, a right-edge and a
    bottom-edge tile."""
    B = params.bin_size
    tiles = sorted({(y // B, x // B) for x, y, _, _ in DL.flips(params, rows)[0]})
    return np.array([bx | by << 16 for by, bx in tiles], dtype=np.int32)


def chain_b(shape, n_colors=256):
    """Finish and the tile calls."""
    c = Chain("B", *params_of(shape))
    _frame_inputs(c)
    _finish(c, n_colors)
    p, W, H, B, rows = c.params, c.params.width, c.params.height, c.params.bin_size, c.rows
    n = (rows[1] - rows[0]) * W
    gx, gy = DL.grid(p)
    cap, slot = gx * gy, B * B
    c.capacity = cap
    cur = c.plane("cur", 4 * n, 0)
    quant = c.step("quantize", params=p, d_palette=Ref("fixed_palette"), n_colors=n_colors, fb=Ref("fb"), rows=rows,
                   fb_out=cur, spread=8)
    prev = c.plane("prev", 4 * n, 4, "history")

    def changed_pair(tag, e, a, b, capacity, steps):
        m, t = c.plane(tag + "_map", 4 * gx * gy, 4), c.plane(tag + "_tiles", 4 * capacity, 8)
        k, packed = c.plane(tag + "_count", 4, 12), c.plane(tag + "_packed", capacity * slot * e, 4 if e > 1 else 1)
        if tag in ("t", "s"):
            steps.append(Step("tiles_changed", dict(params=p, a=a, b=b, rows=rows, d_map=m, d_tiles=t, capacity=capacity,
                                                    d_count=k)))
            steps.append(Step("tiles_pack_counted", dict(params=p, d_tiles=t, d_count=k, capacity=capacity, fb_block=b,
                                                         rows=rows, packed=packed)))
        else:
            steps.append(Step("plane_tiles_changed", dict(params=p, elem_bytes=e, a=a, b=b, rows=rows, d_map=m, d_tiles=t,
                                                          capacity=capacity, d_count=k)))
            steps.append(Step("plane_tiles_pack_counted", dict(params=p, elem_bytes=e, d_tiles=t, d_count=k,
                                                               capacity=capacity, block=b, rows=rows, packed=packed)))

    changed_pair("t", 4, prev, cur, cap, c.steps)
    changed_pair("s", 4, prev, cur, SMALL, c.small)
    c.prologue, c.repoison = [quant], ["cur"]
    index_prev = c.plane("index_prev", n, 3, "history")
    changed_pair("i", 1, index_prev, Ref("fin_index"), cap, c.steps)
    gbuf_prev = c.plane("gbuf_prev", 28 * n, 4, "history")
    gbuf_block = Ref("gbuf", 28 * (rows[0] - c.grows[0]) * W)
    changed_pair("g", 28, gbuf_prev, gbuf_block, cap, c.steps)
    # the calls that take a list or a map from the host, on a fixed list
    nt = len(fixed_tiles(p, rows))
    ft, fm = c.plane("fixed_tiles", 4 * nt, 4, "in"), c.plane("fixed_map", 4 * gx * gy, 8, "in")
    p1_packed, p1_frame, p1_asm = c.plane("p1_packed", nt * slot, 1), c.plane("p1_frame", W * H, 3), c.plane("p1_asm", W * H, 2)
    c.step("plane_tiles_pack", params=p, elem_bytes=1, d_tiles=ft, n=nt, block=Ref("fin_index"), rows=rows, packed=p1_packed)
    c.step("plane_tiles_unpack", params=p, elem_bytes=1, d_tiles=ft, n=nt, packed=p1_packed, frame=p1_frame)
    c.step("plane_tiles_assemble", params=p, elem_bytes=1, d_map=fm, packed=p1_packed, fill=bytes([T.PALIDX_BACKGROUND]),
           frame=p1_asm, rows=rows)
    t4_packed, t4_frame, t4_asm = c.plane("t4_packed", 4 * nt * slot, 4), c.plane("t4_frame", 4 * W * H, 8), c.plane("t4_asm", 4 * W * H, 12)
    c.step("tiles_pack", params=p, d_tiles=ft, n=nt, fb_block=cur, rows=rows, packed=t4_packed)
    c.step("tiles_unpack", params=p, d_tiles=ft, n=nt, packed=t4_packed, frame=t4_frame)
    c.step("tiles_assemble", params=p, d_map=fm, packed=t4_packed, frame=t4_asm, rows=rows)
    c.step("background_fill", params=p, rows_ptr=c.plane("bg_rows", 4 * W * 3, 4), n_rows=3)
    # this frame is the next one's previous frame
    c.step("copy", dst=prev, src=cur, nbytes=4 * n)
    c.step("copy", dst=index_prev, src=Ref("fin_index"), nbytes=n)
    c.step("copy", dst=gbuf_prev, src=gbuf_block, nbytes=28 * n)
    return c


# ---- inputs ----------------------------------------------------------------------------------------------------------

def _b(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()


def frame_inputs(c, seed):
    W = c.params.width
    rng = np.random.default_rng([c.params.width, c.params.height, seed])
    gbuf = O.random_texels(T, rng, c.params, (c.grows[1] - c.grows[0]) * W)
    fb = Q.random_colors(T, rng, (c.rows[1] - c.rows[0]) * W)
    return gbuf, fb


def inputs_a(c):
    """Three unrelated random frames (of seeds with which refine's changed count, a single number, differs too)."""
    return [dict(gbuf=_b(g), fb=_b(f)) for g, f in (frame_inputs(c, k) for k in (0, 1, 6))]


def inputs_b(c):
    """Set 0: a random frame. Set 1: the same with the tiles that delta.flips names drawn again (and its flips made), so
    that a few tiles change. Set 2: another random frame, so that every tile of the block changes."""
    p, W, B, rows = c.params, c.params.width, c.params.bin_size, c.rows
    gx, gy = DL.grid(p)
    rng = np.random.default_rng([W, p.height, 77])
    tiles = fixed_tiles(p, rows)
    fmap = np.full(gx * gy, -1, dtype=np.int32)
    for i, t in enumerate(tiles):
        fmap[(int(t) & 0xFFFF) + (int(t) >> 16) * gx] = i
    static = dict(fixed_palette=_b(PR.random_colors(T, rng, c.n_fixed, alpha=(1, 255))), fixed_tiles=_b(tiles),
                  fixed_map=_b(fmap))
    g0, f0 = frame_inputs(c, 10)
    g1, f1 = g0.copy(), f0.copy()
    inside, _ = DL.flips(p, rows)
    for x, y, mask, _ in inside:
        bx, by = x // B, y // B
        lo, hi = DL.tile_rows(p, by, rows)
        c0, c1 = bx * B, min((bx + 1) * B, W)
        for r in range(lo, hi):
            f1[(r - rows[0]) * W + c0:(r - rows[0]) * W + c1] = Q.random_colors(T, rng, c1 - c0)
            g1[(r - c.grows[0]) * W + c0:(r - c.grows[0]) * W + c1] = O.random_texels(T, rng, p, c1 - c0)
        f1.view(np.uint32)[(y - rows[0]) * W + x] ^= np.uint32(mask)
    g2, f2 = frame_inputs(c, 12)
    return [dict(static, gbuf=_b(g), fb=_b(f)) for g, f in ((g0, f0), (g1, f1), (g2, f2))]


def inputs_of(c):
    return inputs_a(c) if c.name == "A" else inputs_b(c)


def initial_history(c, first, models=None):
    """The history planes with which the first replay of the set `first` sees an identical previous frame."""
    names = c.names("history")
    if not names:
        return {}
    zero = {n: np.zeros(c.planes[n].nbytes, dtype=np.uint8) for n in names}
    return {n: v for n, v in expected(c, dict(first, **zero), models).items() if n in names}


# ---- the models ------------------------------------------------------------------------------------------------------

class Models:
    """The arithmetic expected() composes: the numpy models of the helper modules."""
    outline = staticmethod(O.model)
    quantize = staticmethod(lambda params, palette, fb, rows, spread: Q.model(params, palette, fb, rows, spread))
    pattern = staticmethod(D.model)
    upscale = staticmethod(U.model)
    present = staticmethod(PR.model)
    finish = staticmethod(F.model)
    refine = staticmethod(lambda params, fb, rows, palette, iterations: R.refine(T, params, fb, rows, palette, iterations))
    count, cut, sums = staticmethod(P.count), staticmethod(P.cut), staticmethod(P.sums)
    emit = staticmethod(lambda work, n_colors: P.emit(T, work, n_colors))
    changed4, pack4 = staticmethod(DL.changed), staticmethod(DL.pack)
    changed, pack, unpack, assemble = (staticmethod(PT.changed), staticmethod(PT.pack), staticmethod(PT.unpack),
                                       staticmethod(PT.assemble))


def background(params):
    """The four bytes par_background_fill writes: the last entry of the ramp."""
    return bytes(Q.ramp(params, 2)[-1])


def _px(params, rows):
    return (rows[1] - rows[0]) * params.width


def _unwritten_kept(mem, ref, make):
    """Writes what `make(guard)` gives, except the bytes that are the guard's: those keep what the plane holds."""
    a, b = _b(make(0x00)), _b(make(0xFF))
    mem.write(ref, np.where(a == b, a, mem.read(ref, len(a))))


def _colors(mem, ref, n):
    return mem.read(ref, 4 * n).view(T.COLOR)


def s_outline(M, mem, params, style, gbuf, gbuf_rows, fb, rows, fb_out=None, edge_out=None):
    g = mem.read(gbuf, 28 * _px(params, gbuf_rows)).view(T.PIXEL)
    f = None if fb is None else _colors(mem, fb, _px(params, rows))
    edge, out = M.outline(params, style, g, gbuf_rows, f, rows)
    if edge_out is not None:
        mem.write(edge_out, edge)
    if fb_out is not None:
        mem.write(fb_out, out)


def s_quantize(M, mem, params, d_palette, n_colors, fb, rows, fb_out=None, index_out=None, spread=0):
    index, out = M.quantize(params, _colors(mem, d_palette, n_colors), _colors(mem, fb, _px(params, rows)), rows, spread)
    if index_out is not None:
        mem.write(index_out, index)
    if fb_out is not None:
        mem.write(fb_out, out)


def s_quantize_pattern(M, mem, params, d_palette, n_colors, fb, rows, depth, strength=256, fb_out=None, index_out=None):
    index, out = M.pattern(params, _colors(mem, d_palette, n_colors), _colors(mem, fb, _px(params, rows)), rows, depth, strength)
    if index_out is not None:
        mem.write(index_out, index)
    if fb_out is not None:
        mem.write(fb_out, out)


def _work(mem, ref):
    return mem.read(ref, T.PALETTE_WORK.itemsize).view(T.PALETTE_WORK)


def s_palette_reset(M, mem, work):
    mem.write(work, P.new_work(T))


def s_palette_count(M, mem, params, fb, rows, work):
    w = _work(mem, work)
    M.count(w, _colors(mem, fb, _px(params, rows)))
    mem.write(work, w)


def s_palette_cut(M, mem, work, n_colors):
    w = _work(mem, work)
    M.cut(w, n_colors)
    mem.write(work, w)


def s_palette_sum(M, mem, params, fb, rows, work):
    w = _work(mem, work)
    M.sums(w, _colors(mem, fb, _px(params, rows)))
    mem.write(work, w)


def s_palette_emit(M, mem, work, n_colors, d_palette):
    mem.write(d_palette, M.emit(_work(mem, work), n_colors))


def s_palette_refine_device(M, mem, params, fb, rows, d_palette, n_colors, iterations, d_index, work, d_changed=None):
    palette, index, changed = M.refine(params, _colors(mem, fb, _px(params, rows)), rows, _colors(mem, d_palette, n_colors),
                                       iterations)
    mem.write(d_palette, palette)
    mem.write(d_index, index)
    if d_changed is not None:
        mem.write(d_changed, np.array([changed], dtype=np.int32))


def s_present(M, mem, params, desc, out, rows, fb=None, index=None, d_palette=None, n_colors=0):
    f = None if fb is None else _colors(mem, fb, _px(params, rows))
    i = None if index is None else mem.read(index, _px(params, rows))
    pal = None if d_palette is None else _colors(mem, d_palette, n_colors)
    _unwritten_kept(mem, out, lambda guard: M.present(params, desc, rows, fb=f, index=i, palette=pal, guard=guard))


def s_finish(M, mem, params, desc, out, rows, fb, style=None, gbuf=None, gbuf_rows=None, d_palette=None, n_colors=0, spread=0,
             index_out=None):
    grows = gbuf_rows or rows
    g = None if gbuf is None else mem.read(gbuf, 28 * _px(params, grows)).view(T.PIXEL)
    pal = None if d_palette is None else _colors(mem, d_palette, n_colors)
    f = _colors(mem, fb, _px(params, rows))
    run = lambda guard: M.finish(params, style, g, grows, pal, spread, desc, f, rows, guard)
    _unwritten_kept(mem, out, lambda guard: run(guard)[0])
    if index_out is not None:
        mem.write(index_out, run(0)[1])


def s_upscale(M, mem, params, desc, out, rows, fb=None, index=None, d_palette=None, n_colors=0, src_rows=None, index_out=None):
    src = src_rows or rows
    f = None if fb is None else _colors(mem, fb, _px(params, src))
    i = None if index is None else mem.read(index, _px(params, src))
    pal = None if d_palette is None else _colors(mem, d_palette, n_colors)
    run = lambda guard: M.upscale(params, desc, src, rows, fb=f, index=i, palette=pal, guard=guard)
    if out is not None:
        _unwritten_kept(mem, out, lambda guard: run(guard)[0])
    if index_out is not None:
        mem.write(index_out, run(0)[1])


def _write_changed(mem, got, d_map, d_tiles, capacity, d_count):
    map_, tiles, count = got
    mem.write(d_map, np.asarray(map_, dtype=np.int32))
    m = min(count, capacity)
    if m:
        mem.write(d_tiles, np.asarray(tiles[:m], dtype=np.int32))
    mem.write(d_count, np.array([count], dtype=np.int32))


def _counted(mem, d_tiles, d_count, capacity):
    m = min(max(int(mem.read(d_count, 4).view(np.int32)[0]), 0), capacity)
    return mem.read(d_tiles, 4 * m).view(np.int32)


def s_tiles_changed(M, mem, params, a, b, rows, d_map, d_tiles, capacity, d_count):
    n = 4 * _px(params, rows)
    got = M.changed4(params, mem.read(a, n).view(np.uint32), mem.read(b, n).view(np.uint32), rows)
    _write_changed(mem, got, d_map, d_tiles, capacity, d_count)


def _pack4(M, mem, params, tiles, fb_block, rows, packed):
    if len(tiles):
        block = mem.read(fb_block, 4 * _px(params, rows)).view(np.uint32)
        _unwritten_kept(mem, packed, lambda guard: M.pack4(params, tiles, block, rows, guard))


def s_tiles_pack(M, mem, params, d_tiles, n, fb_block, rows, packed):
    _pack4(M, mem, params, mem.read(d_tiles, 4 * n).view(np.int32), fb_block, rows, packed)


def s_tiles_pack_counted(M, mem, params, d_tiles, d_count, capacity, fb_block, rows, packed):
    _pack4(M, mem, params, _counted(mem, d_tiles, d_count, capacity), fb_block, rows, packed)


def s_plane_tiles_changed(M, mem, params, elem_bytes, a, b, rows, d_map, d_tiles, capacity, d_count):
    n = elem_bytes * _px(params, rows)
    _write_changed(mem, M.changed(params, elem_bytes, mem.read(a, n), mem.read(b, n), rows), d_map, d_tiles, capacity, d_count)


def _plane_pack(M, mem, params, e, tiles, block, rows, packed):
    if len(tiles):
        src = mem.read(block, e * _px(params, rows))
        _unwritten_kept(mem, packed, lambda guard: M.pack(params, e, tiles, src, rows, guard))


def s_plane_tiles_pack(M, mem, params, elem_bytes, d_tiles, n, block, rows, packed):
    _plane_pack(M, mem, params, elem_bytes, mem.read(d_tiles, 4 * n).view(np.int32), block, rows, packed)


def s_plane_tiles_pack_counted(M, mem, params, elem_bytes, d_tiles, d_count, capacity, block, rows, packed):
    _plane_pack(M, mem, params, elem_bytes, _counted(mem, d_tiles, d_count, capacity), block, rows, packed)


def s_plane_tiles_unpack(M, mem, params, elem_bytes, d_tiles, n, packed, frame):
    e, slot = elem_bytes, params.bin_size ** 2 * elem_bytes
    whole = params.width * params.height * e
    tiles = mem.read(d_tiles, 4 * n).view(np.int32)
    mem.write(frame, M.unpack(params, e, tiles, mem.read(packed, n * slot), mem.read(frame, whole)))


def s_plane_tiles_assemble(M, mem, params, elem_bytes, d_map, packed, fill, frame, rows):
    e, slot = elem_bytes, params.bin_size ** 2 * elem_bytes
    gx, gy = DL.grid(params)
    map_ = mem.read(d_map, 4 * gx * gy).view(np.int32)
    slots = mem.read(packed, (int(map_.max()) + 1) * slot if map_.max() >= 0 else 0)
    mem.write(frame, M.assemble(params, e, map_, slots, fill, mem.read(frame, params.width * params.height * e), rows))


def s_tiles_unpack(M, mem, params, d_tiles, n, packed, frame):
    s_plane_tiles_unpack(M, mem, params, 4, d_tiles, n, packed, frame)


def s_tiles_assemble(M, mem, params, d_map, packed, frame, rows):
    s_plane_tiles_assemble(M, mem, params, 4, d_map, packed, background(params), frame, rows)


def s_background_fill(M, mem, params, rows_ptr, n_rows):
    mem.write(rows_ptr, np.frombuffer(background(params) * (n_rows * params.width), dtype=np.uint8))


SEMANTICS = {name: globals()["s_" + name] for name in POINTERS}


class State:
    """Planes by name, as expected() holds them."""

    def __init__(self, planes):
        self.p = planes

    def read(self, ref, nbytes):
        assert 0 <= ref.offset and ref.offset + nbytes <= len(self.p[ref.plane]), f"a read beyond {ref.plane}"
        return self.p[ref.plane][ref.offset:ref.offset + nbytes].copy()

    def write(self, ref, data):
        data = _b(data)
        assert 0 <= ref.offset and ref.offset + len(data) <= len(self.p[ref.plane]), f"a write beyond {ref.plane}"
        self.p[ref.plane][ref.offset:ref.offset + len(data)] = data


def run_pseudo(step, mem, planes):
    if step.binding == "copy":
        mem.write(step.args["dst"], mem.read(step.args["src"], step.args["nbytes"]))
    else:
        name = step.args["plane"]
        mem.write(Ref(name), np.full(planes[name].nbytes, POISON, dtype=np.uint8))


def expected(chain, inputs, models=None):
    """Every plane of the chain but the scratch ones after one replay: `inputs` gives the "in" and "history" planes,
    every other plane holds POISON before."""
    M = models or Models
    planes = {}
    for p in chain.planes.values():
        if p.role in ("in", "history"):
            planes[p.name] = _b(inputs[p.name])
            assert len(planes[p.name]) == p.nbytes, f"{p.name}: {len(planes[p.name])} bytes for {p.nbytes}"
        else:
            planes[p.name] = np.full(p.nbytes, POISON, dtype=np.uint8)
    mem = State(planes)
    for step in chain.everything():
        if step.binding in PSEUDO:
            run_pseudo(step, mem, chain.planes)
        else:
            SEMANTICS[step.binding](M, mem, **step.args)
    return {n: v for n, v in planes.items() if chain.planes[n].role != "scratch"}


# ---- buffers ---------------------------------------------------------------------------------------------------------

class _HostPlane:
    """Carved on the host: `nbytes` bytes that start `shift` bytes past a 16-byte boundary inside a guard-filled array."""

    def __init__(self, nbytes, shift):
        raw = np.full(nbytes + 2 * PAD + 32, GUARD, dtype=np.uint8)
        base = (-raw.ctypes.data) % 16
        self.t = raw[base:base + nbytes + 2 * PAD + 16]
        self.at, self.nbytes = PAD + shift, nbytes
        self.ptr = self.t.ctypes.data + self.at
        assert self.ptr % 16 == shift % 16


class HostBuffers:
    """The planes of a chain on the host, for ModelBackend."""

    def __init__(self, chain):
        self.chain = chain
        self.planes = {p.name: _HostPlane(p.nbytes, p.shift) for p in chain.planes.values()}

    def ptr(self, ref):
        p = self.planes[ref.plane]
        assert 0 <= ref.offset < p.nbytes
        return p.ptr + ref.offset

    def resolve(self, ptr):
        for name, p in self.planes.items():
            if p.ptr <= ptr < p.ptr + p.nbytes:
                return Ref(name, ptr - p.ptr)
        raise AssertionError(f"pointer {ptr:#x} is in no plane")

    def _view(self, name):
        p = self.planes[name]
        return p.t[p.at:p.at + p.nbytes]

    def write(self, name, data):
        self._view(name)[:] = _b(data)

    def fill(self, name, value):
        self._view(name)[:] = value

    def read(self, name):
        return self._view(name).copy()

    def whole(self, name):
        return self.planes[name].t.tobytes()

    def guards_intact(self, name):
        p = self.planes[name]
        return bool((p.t[:p.at] == GUARD).all() and (p.t[p.at + p.nbytes:] == GUARD).all())

    def copy(self, dst, src, nbytes):
        d, s = self._view(dst.plane), self._view(src.plane)
        d[dst.offset:dst.offset + nbytes] = s[src.offset:src.offset + nbytes]


class _External:
    """A plane that is someone else's tensor (a rendered frame's): no guards of its own."""

    def __init__(self, tensor):
        self.t, self.at, self.nbytes, self.ptr = tensor, 0, tensor.numel(), tensor.data_ptr()

    def guards_intact(self):
        return True


class DeviceBuffers(HostBuffers):
    """The planes of a chain on the device, every one carved out of a guard-filled tensor: Carved of
    test_gpu_quantize.py, the fit's work block a Block of test_gpu_palette.py over garbage_work, the fitted palette,
    refine's work block and its changed count those of a Call of test_gpu_palette_refine.py. Everything here runs on
    `stream` (a torch stream) and waits for nothing; read() and whole() are for after the caller's wait. `external`
    maps plane names to tensors that are used as they are."""

    def __init__(self, chain, stream, external=None):
        import torch
        from test_gpu_palette import Block, garbage_work
        from test_gpu_palette_refine import Call
        from test_gpu_quantize import Carved
        self.chain, self.stream, self.torch = chain, stream, torch
        self.planes = {}
        call = None
        for p in chain.planes.values():
            if external and p.name in external:
                assert external[p.name].numel() == p.nbytes, p.name
                self.planes[p.name] = _External(external[p.name])
            elif p.kind == "block":
                self.planes[p.name] = Block(T, garbage_work(T, 90)).c
            elif p.kind.startswith("call."):
                if call is None:
                    call = Call(T, np.zeros(1, dtype=T.COLOR), np.zeros(N_FIT, dtype=T.COLOR))
                self.planes[p.name] = getattr(call, p.kind[5:])
            else:
                self.planes[p.name] = Carved(p.nbytes, p.shift)
            got = self.planes[p.name]
            assert got.nbytes == p.nbytes and (external and p.name in external or got.ptr % 16 == p.shift % 16), p.name
        torch.cuda.synchronize()  # (the fills ran on the current stream; the chain's stream does not wait for it)

    def write(self, name, data):
        with self.torch.cuda.stream(self.stream):
            self._view(name).copy_(self.torch.from_numpy(_b(data)), non_blocking=True)

    def fill(self, name, value):
        with self.torch.cuda.stream(self.stream):
            self._view(name).fill_(value)

    def read(self, name):
        return self._view(name).cpu().numpy()

    def whole(self, name):
        return self.planes[name].t.cpu().numpy().tobytes()

    def guards_intact(self, name):
        return self.planes[name].guards_intact()

    def copy(self, dst, src, nbytes):
        with self.torch.cuda.stream(self.stream):
            d, s = self._view(dst.plane), self._view(src.plane)
            d[dst.offset:dst.offset + nbytes].copy_(s[src.offset:src.offset + nbytes], non_blocking=True)


# ---- the driver ------------------------------------------------------------------------------------------------------

def issue(par, chain, buffers, stream, steps=None):
    """The calls of `steps` (default: the chain's own) on `stream` (a hipStream_t as an int), in order, no host wait.
    Every binding raises unless its call returns PAR_OK."""
    for step in (chain.steps if steps is None else steps):
        if step.binding == "copy":
            buffers.copy(step.args["dst"], step.args["src"], step.args["nbytes"])
        elif step.binding == "poison":
            buffers.fill(step.args["plane"], POISON)
        else:
            kw = {k: (buffers.ptr(v) if isinstance(v, Ref) else v) for k, v in step.args.items()}
            getattr(par, step.binding)(stream=stream, **kw)


def upload(chain, buffers, inputs, roles=("in",)):
    for name in chain.names(*roles):
        buffers.write(name, inputs[name])


def poison(chain, buffers):
    for name in chain.names("out", "scratch"):
        buffers.fill(name, POISON)


def compare(read, exp, tag):
    """Every plane of `exp` byte for byte against read(name), the first plane and offset that differ named."""
    for name, want in exp.items():
        got = read(name)
        assert len(got) == len(want), f"{tag}: plane {name} holds {len(got)} bytes, expected {len(want)}"
        bad = np.nonzero(got != want)[0]
        assert len(bad) == 0, (f"{tag}: plane {name} differs at {len(bad)} of {len(want)} bytes, first at byte {bad[0]}: "
                               f"{got[bad[0]:bad[0] + 8].tolist()} for {want[bad[0]:bad[0] + 8].tolist()}")


def check(buffers, exp, tag):
    """compare() on the buffers' planes, and every guard."""
    compare(buffers.read, exp, tag)
    for name in buffers.planes:
        assert buffers.guards_intact(name), f"{tag}: bytes outside plane {name} were written"


def replays(chain, buffers, sets, launch, wait=lambda: None, after=None, order=ORDER, models=None):
    """The replays of one capture: for each input set of `order` upload the inputs, poison every output, launch() (every
    call of chain.everything(), however the caller runs them), wait() once and check against expected(). The history
    planes are uploaded once, before the first replay. after(k, exp) runs behind each check. Returns the expected planes
    of every replay."""
    history = initial_history(chain, sets[order[0]], models)
    upload(chain, buffers, history, ("history",))
    seen = []
    for i, k in enumerate(order):
        upload(chain, buffers, sets[k])
        poison(chain, buffers)
        launch()
        wait()
        exp = expected(chain, dict(sets[k], **history), models)
        check(buffers, exp, f"chain {chain.name}, replay {i} of input set {k}")
        history = {n: exp[n] for n in history}
        if after:
            after(k, exp)
        seen.append(exp)
    return seen


# ---- a stand-in for the library ----------------------------------------------------------------------------------------

FAULTS = ("stale replay", "skipped step", "count baked in", "wrong stream order")


class _Recording:
    def __init__(self, buffers, log):
        self.buffers, self.log = buffers, log

    def read(self, ref, nbytes):
        return self.buffers.read(ref.plane)[ref.offset:ref.offset + nbytes]

    def write(self, ref, data):
        data = _b(data)
        view = self.buffers._view(ref.plane)
        assert ref.offset + len(data) <= len(view), f"a write beyond {ref.plane}"
        view[ref.offset:ref.offset + len(data)] = data
        self.log.append((ref, data))


class ModelBackend:
    """The post bindings over a HostBuffers, computed with the models, pointers in and out as the library takes them.
    `fault` (one of FAULTS) strikes call number `at` of a replay (begin_replay() starts one):
      stale replay        the call writes what it wrote in the replay before
      skipped step        the call does nothing
      count baked in      the counted pack uses the count of the first replay
      wrong stream order  the call runs behind the next one"""

    def __init__(self, buffers, fault=None, at=None):
        assert fault is None or fault in FAULTS
        self.buffers, self.fault, self.at = buffers, fault, at
        self.replay, self.call, self.writes, self.before, self.baked, self.deferred = -1, 0, [], [], None, None

    def begin_replay(self):
        assert self.deferred is None
        self.replay, self.call, self.before, self.writes = self.replay + 1, 0, self.writes, []

    def __getattr__(self, name):
        if name not in SEMANTICS:
            raise AttributeError(name)
        return lambda stream=0, **kw: self._call(name, kw)

    def _call(self, name, kw):
        i, self.call = self.call, self.call + 1
        kw = {k: (self.buffers.resolve(v) if k in POINTERS[name] and v is not None else v) for k, v in kw.items()}
        log = []
        self.writes.append(log)
        mem = _Recording(self.buffers, log)
        run = lambda: SEMANTICS[name](Models, mem, **kw)
        struck = self.fault is not None and i == self.at
        if struck and self.fault == "skipped step":
            return
        if struck and self.fault == "stale replay" and self.replay > 0:
            for ref, data in self.before[i]:
                mem.write(ref, data)
            return
        if struck and self.fault == "wrong stream order":
            self.deferred = run
            return
        if struck and self.fault == "count baked in":
            assert name in COUNTED
            true = mem.read(kw["d_count"], 4).copy()
            if self.baked is None:
                self.baked = true
            self.buffers._view(kw["d_count"].plane)[kw["d_count"].offset:kw["d_count"].offset + 4] = self.baked
            run()
            self.buffers._view(kw["d_count"].plane)[kw["d_count"].offset:kw["d_count"].offset + 4] = true
            return
        run()
        if self.deferred is not None:
            deferred, self.deferred = self.deferred, None
            deferred()

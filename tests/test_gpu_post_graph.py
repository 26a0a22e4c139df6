"""GPU tests of the passes over finished planes under stream capture and behind graph replays: the chains of
tests/post_chain.py (between them every `*_device` post entry point and every tile call that takes a stream) captured
with torch.cuda.graph in its default, global capture-error mode, and replayed on new inputs with one wait a replay. Every
plane is compared byte for byte with post_chain.expected(), the composition of the numpy models
(tests/test_post_chain_cpu.py holds it to the slow restatements, says what the input sets reach, and shows that the
driver notices a stale replay, a skipped step, a baked-in count and a wrong order). Every buffer is carved out of a
guard-filled tensor before any capture and every output is poisoned before every replay.

The header's claim of each call is "no allocation, no synchronisation, no copy to the host" and "capturable as any
stream-ordered launch is": a call that returns an error under capture, ends the capture invalid or does not follow new
inputs when replayed fails here.

Chain B's changed-tiles pair at the small capacity is a capture of its own. It compares the previous frame with the
current one, which the chain itself makes and at its end copies over the previous one; so each replay first makes the
current frame with an eager par_quantize_device, replays the small pair, poisons the current frame again, and then
replays the chain: all on the one stream, with no wait between."""
import numpy as np
import pytest

import post_chain as PC
from post_chain import T

pytestmark = pytest.mark.gpu


def make(chain, shape):
    # (the palette of finish and of the tiles' frame: 256 entries on the larger shape, 33 on the smaller)
    return PC.chain_a(shape) if chain == "A" else PC.chain_b(shape, 256 if shape.startswith("131") else 33)


def capture(par, c, bufs, stream, steps):
    """A graph of `steps` captured on `stream`. Every binding raises unless its call returns PAR_OK, and leaving the
    capture raises unless it ends valid."""
    import torch
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        PC.issue(par, c, bufs, stream.cuda_stream, steps)
    return graph


class Rig:
    """A chain's buffers on a fresh stream, the chain run once eagerly and checked (so that every code object is loaded
    before a capture), then its captures."""

    def __init__(self, par, c, sets):
        import torch
        self.par, self.c, self.sets, self.torch = par, c, sets, torch
        self.stream = torch.cuda.Stream()
        self.bufs = PC.DeviceBuffers(c, self.stream)
        PC.replays(c, self.bufs, sets, self.eager, self.stream.synchronize, order=(0,))
        self.small = capture(par, c, self.bufs, self.stream, c.small) if c.small else None
        self.graph = capture(par, c, self.bufs, self.stream, c.steps)

    def eager(self):
        PC.issue(self.par, self.c, self.bufs, self.stream.cuda_stream, self.c.everything())

    def replay(self):
        c, s = self.c, self.stream.cuda_stream
        PC.issue(self.par, c, self.bufs, s, c.prologue)  # (eager: the current frame, for the small pair alone)
        with self.torch.cuda.stream(self.stream):
            if self.small is not None:
                self.small.replay()
        PC.issue(self.par, c, self.bufs, s, [PC.Step("poison", {"plane": n}) for n in c.repoison])
        with self.torch.cuda.stream(self.stream):
            self.graph.replay()


class Mirrors:
    """The host's copies of chain B's three planes, kept up to date by fetch and apply alone."""

    def __init__(self, par, c, history):
        p, W, H = c.params, c.params.width, c.params.height
        self.par, self.c = par, c
        r0, r1 = c.rows
        # (tag, element bytes, the plane that holds the current frame's block, its byte offset, the history plane)
        self.planes = (("t", 4, "cur", 0, "prev"), ("i", 1, "fin_index", 0, "index_prev"),
                       ("g", 28, "gbuf", 28 * (r0 - c.grows[0]) * W, "gbuf_prev"))
        self.host = {}
        for tag, e, _, _, hist in self.planes:
            whole = np.full(W * H * e, 0x11, dtype=np.uint8)  # (the rows outside the block must stay as they are)
            whole[r0 * W * e:r1 * W * e] = history[hist]
            self.host[tag] = whole

    def fetch_and_apply(self, bufs, stream, exp, tag_of_replay):
        par, c = self.par, self.c
        p, W, H, B = c.params, c.params.width, c.params.height, c.params.bin_size
        r0, r1 = c.rows
        s = stream.cuda_stream
        for tag, e, cur, at, _ in self.planes:
            cap, slot = c.capacity, B * B * e
            tiles, packed = np.full(cap, -1, dtype=np.int32), np.full(cap * slot, 0x22, dtype=np.uint8)
            ptrs = [bufs.ptr(PC.Ref(f"{tag}_{k}")) for k in ("count", "tiles", "packed")]
            if tag == "t":
                n, count = par.tiles_fetch(p, *ptrs, cap, tiles, packed.view(T.COLOR), stream=s)
                par.tiles_apply_host(p, tiles, n, packed.view(T.COLOR), (r0, r1), self.host[tag].view(T.COLOR))
            else:
                n, count = par.plane_tiles_fetch(p, e, *ptrs, cap, tiles, packed, stream=s)
                par.plane_tiles_apply_host(p, e, tiles, n, packed, (r0, r1), self.host[tag])
            model = int(exp[f"{tag}_count"].view(np.int32)[0])
            assert n == count == model, f"{tag_of_replay}: {tag}: fetched {n} of {count}, the model has {model}"
            want = exp[cur][at:at + (r1 - r0) * W * e]
            got = self.host[tag]
            assert got[r0 * W * e:r1 * W * e].tobytes() == want.tobytes(), f"{tag_of_replay}: {tag}: the mirror is not the frame"
            assert (got[:r0 * W * e] == 0x11).all() and (got[r1 * W * e:] == 0x11).all(), f"{tag_of_replay}: {tag}: other rows"
        # the small pair: an incomplete list is not fetched
        tiles, packed = np.full(PC.SMALL, -1, dtype=np.int32), np.full(PC.SMALL * 4 * B * B, 0x22, dtype=np.uint8)
        ptrs = [bufs.ptr(PC.Ref(f"s_{k}")) for k in ("count", "tiles", "packed")]
        n, count = par.tiles_fetch(p, *ptrs, PC.SMALL, tiles, packed.view(T.COLOR), stream=s)
        model = int(exp["s_count"].view(np.int32)[0])
        assert count == model and n == (model if model <= PC.SMALL else 0), f"{tag_of_replay}: small: {n} of {count} for {model}"
        if n == 0:
            assert (tiles == -1).all() and (packed == 0x22).all(), f"{tag_of_replay}: small: nothing is copied"


# ---- 1. capture, then replays on new inputs ----------------------------------------------------------------------------

@pytest.mark.parametrize("shape", list(PC.SHAPES))
@pytest.mark.parametrize("chain", ["A", "B"])
def test_chain_captures_and_replays(par, chain, shape):
    c = make(chain, shape)
    sets = PC.inputs_of(c)
    rig = Rig(par, c, sets)
    after = None
    if chain == "B":
        mirrors = Mirrors(par, c, PC.initial_history(c, sets[PC.ORDER[0]]))
        seen = []

        def after(k, exp):
            seen.append(k)
            mirrors.fetch_and_apply(rig.bufs, rig.stream, exp, f"replay {len(seen) - 1} of input set {k}")

    exps = PC.replays(c, rig.bufs, sets, rig.replay, rig.stream.synchronize, after)
    assert len(exps) == len(PC.ORDER) == 4
    if chain == "B":
        counts = [int(e["s_count"].view(np.int32)[0]) for e in exps]
        assert counts[0] == 0 and counts[1] >= 1 and counts[2] > PC.SMALL and counts[3] > PC.SMALL, counts


# ---- 2. a replay writes what the eager run writes ----------------------------------------------------------------------

@pytest.mark.parametrize("chain", ["A", "B"])
def test_captured_equals_eager(par, chain):
    shape = "131x67 whole"
    c = make(chain, shape)
    sets = PC.inputs_of(c)
    rig = Rig(par, c, sets)
    history = PC.initial_history(c, sets[0])

    def run(launch):
        PC.upload(c, rig.bufs, history, ("history",))
        PC.upload(c, rig.bufs, sets[1])
        PC.poison(c, rig.bufs)
        launch()
        rig.stream.synchronize()
        return {name: rig.bufs.whole(name) for name in c.planes}  # (whole tensors: the guards and the scratch planes too)

    eager, replayed = run(rig.eager), run(rig.replay)
    for name in c.planes:
        assert eager[name] == replayed[name], f"chain {chain}: plane {name} after a replay is not what the eager run leaves"
    PC.check(rig.bufs, PC.expected(c, dict(sets[1], **history)), f"chain {chain}, captured")


# ---- 3. behind graph-replayed frames -------------------------------------------------------------------------------------

def test_post_graph_behind_graph_replayed_frames(par, oracle):
    """333 x 170 x 150 at bin size 16 under two tinted ranged lights: the frame's graph (par_graph_capture_lights), then
    a second graph of chain A and the finish step on the frame's fb and gbuf planes, then copies into a ring slot, six
    frames with moving boxes and lights on one stream and one wait at the end."""
    import torch
    import light_tints as LT
    import sequences as S
    from test_gpu_light_range import lights_with
    from test_gpu_light_tints import TINTS
    from test_gpu_lights import oracle_planes
    from test_gpu_lights_graph import BYTES, Planes
    from test_gpu_parity import ALL, assert_planes_equal

    w, h, l, b = S.VIEWS["333x170x150 bin 16"]
    assert w % 4 != 0
    params = T.default_params(w, h, l, b)
    frames, n_boxes = 6, 96
    aabbs, _ = par.scene_synthetic(n_boxes, w, h, l, 5)
    sprite = par.tile_floor()
    tints = TINTS[:2]
    lights = lights_with(T, [(300, 60, 40), (40, 120, 100)], [260, 220])
    rng = np.random.default_rng(29)
    vel = rng.choice([-5, 0, 5], size=(n_boxes, 3)).astype(np.int16)
    lvel = np.array([[-15, 5, 10], [20, -5, -10]], dtype=np.int16)

    c = PC.chain_frame((w, h, b, None), n_colors=64)
    palette = PC._b(PC.PR.random_colors(T, rng, 64, alpha=(1, 255)))
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    out = Planes(params, ALL)
    bufs = PC.DeviceBuffers(c, stream, external={"fb": out.bufs["fb"], "gbuf": out.bufs["gbuf"]})
    bufs.write("fixed_palette", palette)
    outputs = c.names("out")
    ring = {k: torch.zeros(frames, w * h * BYTES[k], dtype=torch.uint8, device="cuda") for k in ALL}
    ring.update({n: torch.zeros(frames, c.planes[n].nbytes, dtype=torch.uint8, device="cuda") for n in outputs})
    torch.cuda.synchronize()

    def oracle_frame(a, ls):
        plain = ls.copy()
        plain["radius"] = 10  # (the oracle's planes do not depend on it; the composer applies the ranges)
        exp, _ = LT.compose_tinted(params, oracle_planes(oracle, params, a, sprite, plain), ls, tints, ranged=True)
        return exp

    def post_of(exp):
        return PC.expected(c, {"gbuf": PC._b(exp["gbuf"]), "fb": PC._b(exp["fb"]), "fixed_palette": palette})

    scenes = []
    with par.Renderer(params) as r:
        r.set_sprites(sprite)
        r.set_entities(aabbs)
        r.set_light_model(par.LIGHTS_RANGED)
        r.set_lights(lights)
        r.set_light_tints(T.make_tints(tints))
        r.graph_capture_lights(out.ptrs, stream=s)
        # the chain once eagerly behind a frame, checked, before its capture
        first = oracle_frame(aabbs, lights)
        r.graph_launch(s)
        PC.poison(c, bufs)
        PC.issue(par, c, bufs, s)
        stream.synchronize()
        assert_planes_equal(out.host(T), first, ALL, "the first frame")
        PC.check(bufs, post_of(first), "the chain behind the first frame, eagerly")
        graph = capture(par, c, bufs, stream, c.steps)
        cur = lights.copy()
        for f in range(frames):
            if f:
                for k, ax in enumerate(("px", "py", "pz")):
                    aabbs[ax] += vel[:, k]
                for k, ax in enumerate("xyz"):
                    cur[ax] += lvel[:, k]
                r.graph_stage(aabbs, 0, lights=cur)
            r.graph_launch(s)
            PC.poison(c, bufs)
            with torch.cuda.stream(stream):
                graph.replay()
                for k in ALL:
                    ring[k][f].copy_(out.bufs[k], non_blocking=True)
                for n in outputs:
                    ring[n][f].copy_(bufs._view(n), non_blocking=True)
            scenes.append((aabbs.copy(), cur.copy()))
        stream.synchronize()
        r.stats()  # raises on PAR_ERR_DEVICE
    for name in bufs.planes:
        assert bufs.guards_intact(name), f"bytes outside plane {name} were written"
    got = {k: v.cpu().numpy() for k, v in ring.items()}
    posts = []
    for f, (a, ls) in enumerate(scenes):
        exp = first if f == 0 else oracle_frame(a, ls)
        frame = {k: got[k][f].view(S.DTYPE[k]) for k in ALL}
        assert (exp["palidx"] != 0xFF).sum() > w * h // 20, f"frame {f} shows something"
        assert_planes_equal(frame, exp, ALL, f"frame {f}: the graph's frame against the composed oracle")
        post = post_of(exp)
        PC.compare(lambda n: got[n][f], {n: post[n] for n in outputs}, f"frame {f}: the post graph")
        posts.append(post)
    for n in outputs:
        assert len({posts[f][n].tobytes() for f in range(frames)}) >= 2, f"{n}: at least two frames differ"

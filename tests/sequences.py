"""Long call sequences on ONE context, checked after every step against the pinned oracle. No GPU is needed to import
this module; tests/test_gpu_sequences.py drives a Renderer with it, tests/test_sequences_cpu.py says what the
sequences contain and shows on an oracle-backed stand-in that the driver notices state that leaks between frames.

  Mirror         the host-side truth of one context: scene, lights, light model and tints; the retained frame and the
                 captured graph as include/par_raytracer.h words them; and, restated from csrc/par_book.cpp and
                 par_context.hip for the coverage counts alone, the grid set in use and the node pool's capacity.
                 expected() composes a frame from scratch from the oracle's per-light planes (test_gpu_lights.compose,
                 light_range.compose_ranged, light_tints.compose_tinted); predicted_status() is PAR_OK or the error the
                 header promises, in the header's checking order.
  generate()     a seeded list of ops (np.random.default_rng([view index, seed])), drawn with a Mirror in the loop so
                 that most ops are accepted and some are refused on purpose.
  run()          issues the ops on anything with the Renderer surface. Every frame is compared byte for byte on every
                 requested plane; device planes are poisoned (0xA5) before the call and have one guard row on either
                 side that must keep the poison; stats() follows every step (it surfaces PAR_ERR_DEVICE).
  OracleBackend  the Renderer surface over the oracle and a Mirror, with four injectable leaks.

An op is a dict: {"kind": ..., arguments}. A refusal changes nothing, with one exception the header words: a capture
refused after its arguments and the light state were accepted (PAR_RENDER_TRACE_BACKGROUND without a lit plane, before
a plain frame of as many pixels was rendered that way) leaves no graph and no retained frame (Mirror.refuse). The
generator draws neither that capture nor one of a scene without entities; hand-written sequences issue both."""
import collections
import ctypes as C
import hashlib
import importlib
import types

import numpy as np

import light_range as LR
import light_tints as LT
from test_gpu_light_states_sweep import sprite_table
from test_gpu_lights import NTHREADS, compose
from test_gpu_lights_edges import PLANE_SETS
from test_gpu_parity import ALL, assert_planes_equal

T = importlib.import_module("pixel-art-raytracer_amd.types")

OK, INVALID_ARG, UNSUPPORTED, NOT_READY = 0, 1, 5, 8
STATUS = {OK: "PAR_OK", INVALID_ARG: "INVALID_ARG", UNSUPPORTED: "UNSUPPORTED", NOT_READY: "NOT_READY"}
TRACE_BACKGROUND, COUNT_RAYS, PIPELINED = 1, 2, 4
RANGED = 1
POISON = 0xA5
GUARD = 1  # guard rows before and after a device plane
LIT = ("fb", "brightness", "lit")
BYTES = {"fb": 4, "gbuf": 28, "palidx": 1, "brightness": 4, "lit": 1}
DTYPE = {"fb": T.COLOR, "gbuf": T.PIXEL, "palidx": np.uint8, "brightness": np.float32, "lit": np.uint8}
COL_NB, COL_ENT = 32, 64  # PAR_COL_NB, PAR_COL_ENT: occupied bins and slot records a column record holds
POOL = 65536              # the node pool of a new context; the most pairs of a one-launch hash build

VIEWS = {"480x320x320 bin 40": (480, 320, 320, 40),   # the reference view
         "256x192x192 bin 8": (256, 192, 192, 8),     # 768 columns: both sides of 256; `big` is reachable
         "333x170x150 bin 16": (333, 170, 150, 16),   # width no multiple of 4: unaligned rows, the generic fill
         "640x320x160 bin 8": (640, 320, 160, 8)}     # 3 200 columns: both sides of 1 024 and 2 048
VIEW_IDS = {v: i for i, v in enumerate(VIEWS)}
REGIMES = {v: ("empty", "culled", "sparse", "many", "dense", "overflow") for v in VIEWS}
REGIMES["256x192x192 bin 8"] += ("big",)
FRAME_KINDS = ("render", "render_device", "relight", "relight_device", "graph_launch", "pick")
KINDS = FRAME_KINDS + ("set_entities", "set_sprites", "update_aabbs", "update_aabbs_async", "set_light", "set_lights",
                       "set_light_model", "set_light_tints", "graph_capture", "graph_capture_lights", "graph_stage",
                       "read_grid", "stats")
SEEDS = tuple(range(12))
STEPS = 48
TINTS = [(1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1), (2.5, .5, 0), (0, 0, 0), (.25, .75, 1.5), (1, 1, 0)]


def package():
    return importlib.import_module("pixel-art-raytracer_amd")


# ---- the host's bookkeeping, restated (csrc/par_book.cpp) ----------------------------------------------------------

def _tdiv(a, b):
    q = np.abs(a) // b  # C's division truncates towards zero
    return np.where(a < 0, -q, q)


def footprints(params, aabbs):
    """(x0, nx, y0, ny, nz) per entity: the cull and the bin ranges of alt:202-240 (footprint_of)."""
    W, H, L, B = params.width, params.height, params.length, params.bin_size
    gx, gy, gz = params.grid_dims()
    f = {k: aabbs[k].astype(np.int64) for k in ("px", "py", "pz", "ex", "ey", "ez")}
    minx, miny, minz = f["px"], f["py"], f["pz"]
    maxx, maxy, maxz = minx + f["ex"], miny + f["ey"], minz + f["ez"]
    culled = (maxx < 0) | (minx >= W) | (maxy < -maxz) | (miny >= H - minz + B) | (maxz < -f["ez"] - B) | (minz > L + B)
    x0 = np.maximum(0, _tdiv(minx, B))
    y0 = np.maximum(0, _tdiv(H - maxy - maxz, B))
    z0 = np.maximum(0, _tdiv(minz, B))
    nx = np.minimum(gx, _tdiv(maxx + B - 1, B)) - x0
    ny = np.minimum(gy, _tdiv(H - miny - minz + B - 1, B)) - y0
    nz = np.minimum(gz, _tdiv(maxz + B - 1, B)) - z0
    live = ~culled & (nx > 0) & (ny > 0) & (nz > 0)
    return x0, np.where(live, nx, 0), y0, np.where(live, ny, 0), np.where(live, nz, 0)


def bounds(params, aabbs):
    """(pairs, cols) as the host counts them exactly, and the pairs the extents alone allow (bound_of)."""
    if len(aabbs) == 0:
        return 0, 0, 0
    _, nx, _, ny, nz = footprints(params, aabbs)
    B = params.bin_size
    gx, gy, gz = params.grid_dims()
    ex, ey, ez = (aabbs[k].astype(np.int64) for k in ("ex", "ey", "ez"))
    ext = (np.minimum(gx, (ex + B - 1) // B + 1) * np.minimum(gy, (ey + ez + B - 1) // B + 1) *
           np.minimum(gz, (ez + B - 1) // B + 1))
    return int((nx * ny * nz).sum()), int((nx * ny).sum()), int(ext.sum())


def column_histograms(params, aabbs):
    """(columns with more pairs than a record surely holds, columns that can be visited as whole tiles, book.dense()):
    par_book::col_hist over every footprint."""
    W, H, B = params.width, params.height, params.bin_size
    gx, gy, _ = params.grid_dims()
    pairs = np.zeros((gx, gy), dtype=np.int64)
    chunks = np.zeros((gx, gy), dtype=np.int64)
    x0, nx, y0, ny, nz = footprints(params, aabbs) if len(aabbs) else ([], [], [], [], [])
    for i in range(len(aabbs)):
        a = aabbs[i]
        px, ex = int(a["px"]), int(a["ex"])
        row0 = H - (int(a["py"]) + int(a["ey"]) + int(a["pz"]) + int(a["ez"]))
        rh = int(a["ey"]) + int(a["ez"])
        for x in range(int(x0[i]), int(x0[i] + nx[i])):
            tw = min(B, W - x * B)
            w = min(px + ex, x * B + tw) - max(px, x * B)
            for y in range(int(y0[i]), int(y0[i] + ny[i])):
                pairs[x, y] += int(nz[i])
                th = min(B, H - y * B)
                h = min(row0 + rh, y * B + th) - max(row0, y * B)
                if w > 0 and h > 0:
                    chunks[x, y] += (w * h + 63) // 64
    tw = np.minimum(B, W - np.arange(gx) * B)[:, None]
    th = np.minimum(B, H - np.arange(gy) * B)[None, :]
    tileable = int((chunks >= (tw * th + 63) // 64).sum())
    return int((pairs > min(COL_NB, COL_ENT)).sum()), tileable, tileable >= max(16, gx * gy // 64)


def grid_sizes(params, grid):
    """From the oracle's hash: occupied screen columns per bin row, and the most slot records and occupied bins of a
    column."""
    c = np.asarray(grid.count).reshape(params.grid_dims())
    occ = (c != 0).any(axis=2)
    return occ.sum(axis=0), int(c.sum(axis=2).max(initial=0)), int((c != 0).sum(axis=2).max(initial=0))


def grids_equal(got, grid):
    """The defined part of a hash in the reference's layout: the counts, and map / bins of the slots below count."""
    count, map_, bins = got
    if not np.array_equal(np.asarray(count, dtype=np.int32), grid.count):
        return False
    live = (np.arange(T.SLOTS)[None, :] < grid.count[:, None]).reshape(-1)
    if not np.array_equal(np.asarray(map_)[live], grid.map[live]):
        return False
    return all(np.array_equal(np.asarray(bins)[k][live], grid.bins[k][live]) for k in ("px", "py", "pz", "ex", "ey", "ez"))


# ---- scenes of the regimes ------------------------------------------------------------------------------------------

def regime_scene(view, regime, rng):
    """The AABBs of `regime` in `view`; test_sequences_cpu.py holds every scene the generator draws to its regime."""
    W, H, L, B = VIEWS[view]

    def cubes(n, x=None, s=None, z=None):
        """n 20-cubes: x, s = y + z (what places a box on the screen) and z uniform in the given ranges."""
        x, s, z = x or (0, W - 20), s or (20, H - 20), z or (0, L - 20)
        px, pz = rng.integers(x[0], x[1], n), rng.integers(z[0], z[1], n)
        return [(int(a), int(b - c), int(c), 20, 20, 20) for a, b, c in zip(px, rng.integers(s[0], s[1], n), pz)]

    def floor(y=0):
        return [(i * 20, y, j * 20, 20, 20, 20) for i in range((W + 19) // 20) for j in range(L // 20)]

    if regime == "empty":
        rows = []
    elif regime == "culled":  # left of the view, and behind it
        n = int(rng.integers(5, 40))
        rows = [(-60, int(y), 30, 20, 20, 20) for y in rng.integers(0, H // 2, n)]
        rows += [(int(x), 10, L + B + 5, 20, 20, 20) for x in rng.integers(0, W - 20, n)]
    elif regime == "sparse":
        if B == 8:  # (a 20-cube alone reaches two dozen columns of 8 x 8 pixels, each a whole tile: small boxes instead)
            n = int(rng.integers(2, 4))
            rows = [(int(x), int(s - z), int(z), int(e[0]), int(e[1]), int(e[2])) for x, s, z, e in
                    zip(rng.integers(0, W - 8, n), rng.integers(20, H - 20, n), rng.integers(0, L - 8, n),
                        rng.integers(2, 7, (n, 3)))]
        else:
            rows = cubes(int(rng.integers(2, 9)))
    elif regime == "many":
        if B == 8 and W == 640:  # a jittered lattice of cubes with disjoint footprints: between 1 024 and 2 048 columns
            rows = []
            for i in range(14):
                for j in range(5):
                    z, top = int(rng.integers(0, L - 20)), 64 * j + int(rng.integers(0, 9))
                    rows.append((45 * i + int(rng.integers(0, 9)), H - top - 40 - z, z, 20, 20, 20))
        else:
            rows = cubes(int(rng.integers(100, 140)))
    elif regime == "dense":
        rows = floor() + (floor(100) if W == 640 else []) + cubes(40, s=(60, H - 20))
    elif regime == "overflow":  # a crowd in one screen column, at every depth
        x0, s0 = int(rng.integers(20, W - 60)), int(rng.integers(H // 3, H - 30))
        rows = cubes(90, x=(x0, x0 + 12), s=(s0, s0 + 7)) + cubes(20) + floor()[::3]
    elif regime == "big":
        rows = cubes(int(rng.integers(1500, 1600)), s=(20, H + 40))
    else:
        raise ValueError(regime)
    return T.make_aabbs(rows)


# ---- ops ------------------------------------------------------------------------------------------------------------

def op(kind, **kw):
    return dict(kind=kind, **kw)


def lights_array(rows):
    a = np.zeros(len(rows), dtype=T.LIGHT)
    for i, (x, y, z, r) in enumerate(rows):
        a[i]["x"], a[i]["y"], a[i]["z"], a[i]["radius"] = x, y, z, r
    return a


def describe(o):
    parts = []
    for k, v in o.items():
        if k == "kind":
            continue
        if isinstance(v, np.ndarray):
            v = f"<{len(v)}>"
        parts.append(f"{k}={v}")
    return f"{o['kind']}({', '.join(parts)})"


def digest(ops):
    h = hashlib.sha256()
    for o in ops:
        for k in sorted(o):
            v = o[k]
            h.update(k.encode())
            h.update(np.ascontiguousarray(v).tobytes() if isinstance(v, np.ndarray) else repr(v).encode())
    return h.hexdigest()[:16]


def rows_of(o, H):
    return o.get("rows") or (0, H)


# ---- the oracle's planes per scene ----------------------------------------------------------------------------------

class Scenes:
    """The oracle's planes: per scene the planes no light changes, per (scene, light position) the lit plane. Shared by
    the Mirrors of one view; the least recently used scenes are dropped."""

    def __init__(self, oracle, keep=8):
        self.oracle, self.keep = oracle, keep
        self.entries = collections.OrderedDict()
        self.renders = 0

    def outs(self, params, key, aabbs, sprites, ids, positions):
        """What the composers take: light 0 with every plane, the others with their lit plane."""
        e = self.entries.get(key)
        if e is None:
            e = self.entries[key] = {"base": None, "lit": {}, "grid": None}
            while len(self.entries) > self.keep:
                self.entries.popitem(last=False)
        self.entries.move_to_end(key)
        for pos in positions:
            if pos not in e["lit"]:
                planes = ALL if e["base"] is None else ("lit",)
                out = self.oracle.render(params, aabbs, sprites, T.make_light(*pos), ids, nthreads=NTHREADS, planes=planes)
                self.renders += 1
                e["lit"][pos] = out.pop("lit")
                if e["base"] is None:  # (fb and brightness: only the background's values are used, which no light changes)
                    e["base"] = out
        return [dict(e["base"], lit=e["lit"][positions[0]])] + [{"lit": e["lit"][p]} for p in positions[1:]]


# ---- the mirror -----------------------------------------------------------------------------------------------------

class Mirror:
    def __init__(self, par, view, scenes=None, oracle=None):
        self.par, self.view = par, view
        self.params = T.default_params(*VIEWS[view])
        self.W, self.H = self.params.width, self.params.height
        self.scenes = scenes
        self.oracle = oracle or (scenes.oracle if scenes else None)
        self.table = None      # sprite table index (test_gpu_light_states_sweep.sprite_table), None: not set
        self.sprites = None
        self.aabbs = None      # None: par_set_entities has not been called
        self.ids = None
        self.regime = None
        self.regimes_seen = set()
        self.lights = None     # rows of (x, y, z, radius)
        self.model = 0
        self.tints = None      # rows of (r, g, b), None: untinted
        self.kept = None       # the retained frame: (r0, r1, host frame with a gbuf plane)
        self.graph = None      # {"lights": kind, "rows", "planes", "flags", "pairs"}
        self.traced = 0        # the most pixels of a plain or relit frame with TRACE_BACKGROUND and no lit plane
        # restated from par_context.hip, for the coverage counts and for what par_read_grid can still show
        self.set, self.capacity, self.sets_used, self.captures = 0, POOL, set(), 0
        self.last = None       # the last frame that built a hash: {"aabbs", "rows"}, None once the pool is replaced
        self._frames = collections.OrderedDict()

    # -- state keys
    def scene_key(self):
        ids = None if self.ids is None else hashlib.sha1(self.ids.tobytes()).hexdigest()
        return (self.table, ids, len(self.aabbs), hashlib.sha1(self.aabbs.tobytes()).hexdigest())

    def ready(self):
        return self.table is not None and self.aabbs is not None and self.lights is not None

    def lights_path(self):
        return len(self.lights) > 1 or self.model == RANGED or self.tints is not None

    # -- expected frames
    def full(self, want_rays=False):
        """(planes of the whole frame, per light the covered pixels in range or None, covered pixel indices)."""
        key = (self.scene_key(), tuple(self.lights), self.model, None if self.tints is None else tuple(self.tints))
        hit = self._frames.get(key)
        if hit is None or (want_rays and self.model == RANGED and hit[1] is None):
            lights = lights_array(self.lights)
            outs = self.scenes.outs(self.params, key[0], self.aabbs, self.sprites, self.ids,
                                    [tuple(l[:3]) for l in self.lights])
            in_range = None
            if self.model == RANGED and (want_rays or self.tints is None):
                exp, per_light, _, _ = LR.compose_ranged(self.params, outs, lights)
                in_range = [r for r, _ in per_light]
            if self.tints is not None:
                exp, _ = LT.compose_tinted(self.params, outs, lights, self.tints, ranged=self.model == RANGED)
            elif self.model != RANGED:
                exp, _ = compose(self.params, outs, lights)
            hit = self._frames[key] = (exp, in_range, np.nonzero(exp["palidx"] != 0xFF)[0])
            while len(self._frames) > 4:
                self._frames.popitem(last=False)
        return hit

    def expected(self, rows, planes):
        r0, r1 = rows or (0, self.H)
        exp = self.full()[0]
        return {k: exp[k][r0 * self.W:r1 * self.W] for k in planes}

    def rays(self, rows):
        """shadow_rays of a counted frame: the (covered pixel, light) pairs in range or unbounded, of the rows."""
        r0, r1 = rows or (0, self.H)
        _, in_range, idx = self.full(want_rays=True)
        inside = (idx >= r0 * self.W) & (idx < r1 * self.W)
        if in_range is None:
            return len(self.lights) * int(inside.sum())
        return sum(int((r & inside).sum()) for r in in_range)

    def grid(self, aabbs):
        return self.oracle.bin(self.params, aabbs)

    # -- statuses
    def _frame_status(self, rows, flags):
        r0, r1 = rows or (0, self.H)
        if flags & ~0xF:
            return INVALID_ARG
        if r0 < 0 or r1 > self.H or r0 >= r1:
            return INVALID_ARG
        return OK if self.ready() else NOT_READY

    def _update_status(self, aabbs, first):
        n = 0 if aabbs is None else len(aabbs)
        if first < 0 or self.aabbs is None or first + n > len(self.aabbs):
            return INVALID_ARG
        return OK

    def _staged(self, o):
        a = self.aabbs.copy()
        if o.get("aabbs") is not None:
            a[o["first"]:o["first"] + len(o["aabbs"])] = o["aabbs"]
        return a

    def predicted_status(self, o):
        k = o["kind"]
        if k in ("render", "render_device"):
            return self._frame_status(o.get("rows"), o.get("flags", 0))
        if k == "pick":
            if not (0 <= o["x"] < self.W and 0 <= o["y"] < self.H):
                return INVALID_ARG
            return self._frame_status((o["y"], o["y"] + 1), 0)
        if k in ("relight", "relight_device"):
            if "gbuf" in o["planes"] or "palidx" in o["planes"]:
                return INVALID_ARG
            st = self._frame_status(o.get("rows"), o.get("flags", 0))
            if st != OK:
                return st
            r0, r1 = rows_of(o, self.H)
            if self.kept is None or r0 < self.kept[0] or r1 > self.kept[1]:
                return NOT_READY
            return NOT_READY if k == "relight" and not self.kept[2] else OK
        if k in ("graph_capture", "graph_capture_lights"):
            st = self._frame_status(o.get("rows"), o.get("flags", 0))
            if st != OK:
                return st
            if k == "graph_capture" and self.lights_path():
                return UNSUPPORTED
            r0, r1 = rows_of(o, self.H)
            if o.get("flags", 0) & TRACE_BACKGROUND and "lit" not in o["planes"] and self.traced < (r1 - r0) * self.W:
                return NOT_READY  # (and the graphs captured before are gone: refuse())
            return OK
        if k == "graph_stage":
            if self.graph is None:
                return NOT_READY
            ls = o.get("lights")
            if ls is not None and not 1 <= len(ls) <= 8:
                return INVALID_ARG
            if ls is not None and len(ls) > 1 and not self.graph["lights"]:
                return UNSUPPORTED
            st = self._update_status(o.get("aabbs"), o.get("first", 0))
            if st != OK:
                return st
            pairs = bounds(self.params, self._staged(o))[0]
            return UNSUPPORTED if pairs > self.graph["pairs"] or pairs > self.capacity else OK
        if k == "graph_launch":
            if self.graph is None:
                return NOT_READY
            if bounds(self.params, self.aabbs)[0] > self.graph["pairs"]:
                return UNSUPPORTED
            return UNSUPPORTED if len(self.lights) > 1 and not self.graph["lights"] else OK
        if k in ("update_aabbs", "update_aabbs_async"):
            return self._update_status(o["aabbs"], o["first"])
        if k == "set_lights":
            return OK if 1 <= len(o["lights"]) <= 8 else INVALID_ARG
        if k == "set_light_model":
            return OK if o["model"] in (0, 1) else INVALID_ARG
        if k == "set_light_tints":
            t = o["tints"]
            if t is not None and (not 1 <= len(t) <= 8 or any(not np.isfinite(v) or v < 0 for row in t for v in row)):
                return INVALID_ARG
            return OK
        if k in ("set_entities", "set_sprites", "set_light", "read_grid", "stats"):
            return OK
        raise ValueError(k)

    # -- what an accepted op changes
    def _ensure_pool(self, pairs):
        if pairs > self.capacity:  # ensure_pool: the pool is replaced, reset_grid starts again with set 0
            self.capacity = max(pairs + pairs // 2, POOL)
            self.set, self.last = 0, None

    def _built(self, rows):
        """A frame that built a hash in the set in use."""
        self.sets_used.add(self.set)
        self.set ^= 1
        self.last = {"aabbs": self.aabbs.copy(), "rows": rows or (0, self.H)}

    def refuse(self, o, st):
        """The state after `o` was refused with `st`: as before, but for a capture that failed once it had begun."""
        if o["kind"] in ("graph_capture", "graph_capture_lights") and st == NOT_READY and self.ready():
            self.apply(o)
            self.graph = None

    def apply(self, o):
        """The state after `o` returned PAR_OK."""
        k = o["kind"]
        if k in ("render", "render_device", "relight", "relight_device"):
            if o.get("flags", 0) & TRACE_BACKGROUND and "lit" not in o["planes"]:
                r0, r1 = rows_of(o, self.H)
                self.traced = max(self.traced, (r1 - r0) * self.W)
        if k == "set_sprites":
            self.table, self.graph, self.kept = o["table"], None, None
            self.sprites = sprite_table(self.par, o["table"], 0)[0]
        elif k == "set_entities":
            self.graph, self.kept = None, None
            pairs, _, extent = bounds(self.params, o["aabbs"])
            self._ensure_pool(max(pairs, extent))
            self.aabbs, self.ids, self.regime = o["aabbs"].copy(), o.get("ids"), o.get("regime")
            if len(self.sets_used) == 2:  # (entered by a context that has rendered in both grid sets)
                self.regimes_seen.add(self.regime)
        elif k in ("update_aabbs", "update_aabbs_async"):
            self.kept = None
            self.aabbs = self._staged(o)
        elif k == "set_light":
            self.lights = [tuple(o["light"])]
        elif k == "set_lights":
            self.lights = [tuple(l) for l in o["lights"]]
        elif k == "set_light_model":
            if o["model"] != self.model:
                self.graph = None
            self.model = o["model"]
        elif k == "set_light_tints":
            if (o["tints"] is None) != (self.tints is None):
                self.graph = None
            self.tints = None if o["tints"] is None else [tuple(t) for t in o["tints"]]
        elif k in ("render", "render_device"):
            r0, r1 = rows_of(o, self.H)
            self._built((r0, r1))
            self.kept = (r0, r1, k == "render" and "gbuf" in o["planes"])
        elif k == "pick":
            self._built((o["y"], o["y"] + 1))
            self.kept = (o["y"], o["y"] + 1, False)
        elif k in ("graph_capture", "graph_capture_lights"):
            self.kept = None
            pairs = 2 * bounds(self.params, self.aabbs)[0] + 4096
            self._ensure_pool(pairs)
            self.graph = {"lights": k == "graph_capture_lights", "rows": rows_of(o, self.H), "planes": tuple(o["planes"]),
                          "flags": o.get("flags", 0) & ~COUNT_RAYS, "pairs": pairs, "serial": self.captures}
            self.captures += 1
        elif k == "graph_stage":
            self.kept = None
            self.aabbs = self._staged(o)
            if o.get("light") is not None:
                self.lights = [tuple(o["light"])] + self.lights[1:]
            if o.get("lights") is not None:
                self.lights = [tuple(l) for l in o["lights"]]
        elif k == "graph_launch":
            self.kept = None
            for _ in range(o.get("count", 1)):
                self._built(self.graph["rows"])

    def last_frame_sizes(self):
        """(bin_insertions, occupied_columns) par_get_stats reports for the last frame that built a hash."""
        L = self.last
        if "sizes" not in L:
            B = self.params.bin_size
            per_row = grid_sizes(self.params, self.grid(L["aabbs"]))[0] if len(L["aabbs"]) else np.zeros(1, dtype=int)
            r0, r1 = L["rows"]
            L["sizes"] = (bounds(self.params, L["aabbs"])[0], int(per_row[r0 // B:(r1 - 1) // B + 1].sum()))
        return L["sizes"]


# ---- the generator --------------------------------------------------------------------------------------------------

def _light(rng, view):
    W, H, L, B = VIEWS[view]
    radius = 0 if rng.random() < 0.3 else int(rng.integers(max(8, B), (W + H + L) // 2 + 1))
    return (int(rng.integers(-40, W + 41)), int(rng.integers(-20, H + 1)), int(rng.integers(-20, L + 21)), radius)


def _rows(rng, view, bad=0.0):
    W, H, L, B = VIEWS[view]
    u = rng.random()
    if u < bad:
        return [(H // 2, H // 2), (10, H + 1), (-1, 20)][int(rng.integers(0, 3))]
    if u < 0.45:
        return None
    gy = (H + B - 1) // B
    if u < 0.7:  # a block of whole bin rows
        b0 = int(rng.integers(0, gy))
        b1 = int(rng.integers(b0 + 1, gy + 1))
        return (b0 * B, min(H, b1 * B))
    r0 = int(rng.integers(0, H - 1))
    return (r0, int(rng.integers(r0 + 1, H + 1)))


def _flags(rng):
    return int(sum(f for f, p in ((TRACE_BACKGROUND, .25), (COUNT_RAYS, .25), (PIPELINED, .3)) if rng.random() < p))


def _moved(rng, aabbs, most=48):
    """A sub-range moved by -5, 0 or 5 per axis, as the reference moves things (alt:643-660)."""
    n = len(aabbs)
    first = int(rng.integers(0, n))
    cnt = int(rng.integers(1, min(n - first, most) + 1))
    a = aabbs[first:first + cnt].copy()
    d = rng.choice([-5, 0, 5], size=(cnt, 3))
    for c, f in enumerate(("px", "py", "pz")):
        a[f] += d[:, c].astype(a[f].dtype)
    return first, a


def _entities(rng, par, m, view, regime):
    aabbs = regime_scene(view, regime, rng)
    ids = None
    if m.table in (1, 2) and rng.random() < 0.6:
        ids = sprite_table(par, m.table, len(aabbs))[1]
    return op("set_entities", regime=regime, aabbs=aabbs, ids=ids)


WEIGHTS = {"render": 50, "render_device": 20, "relight": 8, "relight_device": 8, "graph_launch": 10, "pick": 3,
           "set_entities": 11, "set_sprites": 2, "update_aabbs": 5, "update_aabbs_async": 4, "set_light": 2.5,
           "set_lights": 2.5, "set_light_model": 2, "set_light_tints": 2.5, "graph_capture": 4,
           "graph_capture_lights": 5, "graph_stage": 4, "read_grid": 2, "stats": 2}


def _draw(rng, par, m, view, kind):
    """One op of `kind` in the mirror's state; now and then one that must be refused."""
    W, H, L, B = VIEWS[view]
    if kind in ("render", "render_device"):
        return op(kind, planes=PLANE_SETS[int(rng.integers(0, len(PLANE_SETS)))], rows=_rows(rng, view, bad=0.04),
                  flags=_flags(rng))
    if kind in ("relight", "relight_device"):
        planes = [("fb",), LIT, ("lit",), ("brightness", "fb")][int(rng.integers(0, 4))]
        if rng.random() < 0.04:
            planes = ("fb", "gbuf")
        rows = None
        if m.kept is not None and rng.random() < 0.85:  # rows inside the retained frame's, mostly
            r0 = int(rng.integers(m.kept[0], m.kept[1]))
            rows = (r0, int(rng.integers(r0 + 1, m.kept[1] + 1))) if rng.random() < 0.5 else (m.kept[0], m.kept[1])
        elif rng.random() < 0.5:
            rows = _rows(rng, view)
        return op(kind, planes=planes, rows=rows, flags=_flags(rng))
    if kind == "pick":
        if rng.random() < 0.1:
            return op(kind, x=W, y=0)
        return op(kind, x=int(rng.integers(0, W)), y=int(rng.integers(0, H)))
    if kind == "set_entities":
        others = [r for r in REGIMES[view] if r not in m.regimes_seen] or [r for r in REGIMES[view] if r != m.regime]
        return _entities(rng, par, m, view, others[int(rng.integers(0, len(others)))])
    if kind == "set_sprites":  # (a table with a sprite for every id in use)
        tables = [0, 1, 2] if m.ids is None else [1, 2]
        return op(kind, table=tables[int(rng.integers(0, len(tables)))])
    if kind in ("update_aabbs", "update_aabbs_async"):
        extra = {"other_stream": bool(rng.random() < 0.4)} if kind == "update_aabbs_async" else {}
        if m.aabbs is None or len(m.aabbs) == 0 or rng.random() < 0.05:  # a range outside the uploaded entities
            n = 0 if m.aabbs is None else len(m.aabbs)
            return op(kind, first=n, aabbs=T.make_aabbs([(0, 0, 0, 20, 20, 20)]), **extra)
        first, a = _moved(rng, m.aabbs)
        return op(kind, first=first, aabbs=a, **extra)
    if kind == "set_light":
        return op(kind, light=_light(rng, view))
    if kind == "set_lights":
        n = int(rng.integers(1, 9))
        if rng.random() < 0.06:
            n = [0, 9][int(rng.integers(0, 2))]
        return op(kind, lights=[_light(rng, view) for _ in range(n)])
    if kind == "set_light_model":
        return op(kind, model=2 if rng.random() < 0.08 else int(rng.integers(0, 2)))
    if kind == "set_light_tints":
        if rng.random() < 0.4:
            return op(kind, tints=None)
        rows = [TINTS[int(i)] for i in rng.integers(0, 8, int(rng.integers(1, 9)))]
        if rng.random() < 0.08:
            rows[0] = (1.0, -0.5, 1.0)
        return op(kind, tints=rows)
    if kind in ("graph_capture", "graph_capture_lights"):
        planes = PLANE_SETS[int(rng.integers(0, len(PLANE_SETS)))]
        flags = _flags(rng)
        if "lit" not in planes:
            flags &= ~TRACE_BACKGROUND
        return op(kind, planes=planes, rows=_rows(rng, view), flags=flags)
    if kind == "graph_stage":
        o = op(kind)
        if m.aabbs is not None and len(m.aabbs) and rng.random() < 0.6:
            o["first"], o["aabbs"] = _moved(rng, m.aabbs)
        u = rng.random()
        one_light = m.graph is not None and not m.graph["lights"]
        if u < 0.3:
            o["light"] = _light(rng, view)
        elif u < 0.7:
            n = 1 if one_light and rng.random() < 0.8 else int(rng.integers(1, 5 if one_light else 9))
            o["lights"] = [_light(rng, view) for _ in range(n)]
        return o
    if kind == "graph_launch":
        return op(kind, count=int(rng.integers(1, 4)))
    return op(kind)


def generate(par, view, seed, steps=STEPS):
    """(ops, trace): `steps` ops, and per op what test_sequences_cpu.py counts: the predicted status, whether a frame is
    compared, the regime, the grid set a frame's hash is built in, the retained frame and the graph at the time."""
    rng = np.random.default_rng([VIEW_IDS[view], seed])
    m = Mirror(par, view)
    ops, trace = [], []

    def emit(o):
        st = m.predicted_status(o)
        t = {"kind": o["kind"], "status": st, "frame": st == OK and o["kind"] in FRAME_KINDS, "regime": m.regime,
             "set": m.set, "kept": m.kept is not None, "graph": None if m.graph is None else m.graph["serial"],
             "sets_used": len(m.sets_used), "builds": st == OK and o["kind"] in ("render", "render_device", "pick", "graph_launch"),
             "count": o.get("count", 1)}
        if st == OK:
            m.apply(o)
        else:
            m.refuse(o, st)
        ops.append(o)
        trace.append(t)

    if rng.random() < 0.5:  # before anything is set
        emit(op("render", planes=("fb",), rows=None, flags=0))
    emit(op("set_sprites", table=int(rng.integers(0, 3))))
    regimes = REGIMES[view]
    emit(_entities(rng, par, m, view, regimes[int(rng.integers(0, len(regimes)))]))
    if rng.random() < 0.6:
        emit(op("set_light", light=_light(rng, view)))
    else:
        emit(op("set_lights", lights=[_light(rng, view) for _ in range(int(rng.integers(2, 9)))]))
    kinds = list(WEIGHTS)
    relit_under = None
    while len(ops) < steps:
        w = dict(WEIGHTS)
        for k in ("relight", "relight_device"):
            if m.kept is None or (k == "relight" and not m.kept[2]):
                w[k] *= 0.15
        if m.graph is None:
            w["graph_launch"] *= 0.08
            w["graph_stage"] *= 0.15
        else:  # (a graph lives until the scene, the sprites or the light state is replaced: let it see some frames)
            w["graph_launch"] *= 3
            for k in ("set_entities", "set_sprites", "set_light_model", "set_light_tints", "graph_capture",
                      "graph_capture_lights"):
                w[k] *= 0.5
        if m.kept is not None:  # (a retained frame is there to be relit under other lights)
            for k in ("set_light", "set_lights", "set_light_model", "set_light_tints"):
                w[k] *= 2
            if relit_under != (tuple(m.lights), m.model, None if m.tints is None else tuple(m.tints)):
                w["relight_device"] *= 4
                w["relight"] *= 4
        if m.lights_path():
            w["graph_capture"] *= 0.3
        if len(m.aabbs) == 0:
            w["graph_capture"] = w["graph_capture_lights"] = 0
            w["update_aabbs"] *= 0.3
            w["update_aabbs_async"] *= 0.3
        if m.last is None:
            w["read_grid"] = 0
        if len(m.lights) > 3:  # (every moved scene costs one oracle render per light)
            w["update_aabbs"] *= 0.4
            w["update_aabbs_async"] *= 0.4
            w["set_light"] *= 2
        if m.regime == "big":
            w["set_entities"] *= 2
        if trace[-1]["status"] == OK and not trace[-1]["frame"] and rng.random() < 0.6:
            for k in kinds:  # what an accepted change did shows in the next frame
                if k not in FRAME_KINDS:
                    w[k] = 0
        p = np.array([w[k] for k in kinds], dtype=float)
        emit(_draw(rng, par, m, view, kinds[int(rng.choice(len(kinds), p=p / p.sum()))]))
        if trace[-1]["frame"]:  # the light state the last compared frame was shaded under
            relit_under = (tuple(m.lights), m.model, None if m.tints is None else tuple(m.tints))
    return ops, trace


def cases():
    """(view, seed) of every generated sequence: the GPU tests and what test_sequences_cpu.py counts."""
    return [(view, seed) for view in VIEWS for seed in SEEDS]


# ---- memory the device frames are written to ------------------------------------------------------------------------

class HostMem:
    """Plain host memory behind the interface of TorchMem, for a backend that runs on the CPU."""

    class Buf:
        def __init__(self, n):
            self.a = np.zeros(max(n, 1), dtype=np.uint8)
            self.ptr = self.a.ctypes.data

        def fill(self, v, stream):
            self.a[:] = v

        def write(self, data, stream):
            self.a[:data.nbytes] = np.frombuffer(data.tobytes(), dtype=np.uint8)

        def snapshot(self, stream):
            return self.a.copy()

    class Stream:
        def __init__(self, handle):
            self.handle = handle

        def synchronize(self):
            pass

    def __init__(self):
        self.streams = 0

    def alloc(self, n):
        return HostMem.Buf(n)

    def stream(self):
        self.streams += 1
        return HostMem.Stream(self.streams)


class TorchMem:
    """Device memory and streams through torch."""

    class Buf:
        def __init__(self, n):
            import torch
            self.t = torch.empty(max(n, 1), dtype=torch.uint8, device="cuda")  # (no fill on another stream)
            self.ptr = self.t.data_ptr()

        def fill(self, v, stream):
            import torch
            with torch.cuda.stream(stream.s):
                self.t.fill_(v)

        def write(self, data, stream):
            import torch
            src = torch.from_numpy(np.frombuffer(data.tobytes(), dtype=np.uint8).copy())
            with torch.cuda.stream(stream.s):
                self.t[:data.nbytes].copy_(src)
            stream.s.synchronize()

        def snapshot(self, stream):
            """A copy made in stream order; .cpu() after the stream was synchronised."""
            import torch
            with torch.cuda.stream(stream.s):
                return self.t.clone()

    class Stream:
        def __init__(self):
            import torch
            self.s = torch.cuda.Stream()
            self.handle = self.s.cuda_stream

        def synchronize(self):
            self.s.synchronize()

    def alloc(self, n):
        return TorchMem.Buf(n)

    def stream(self):
        return TorchMem.Stream()


class Guarded:
    """Device planes of rows [r0, r1) with GUARD rows of poison before and after each."""

    def __init__(self, mem, W, planes, rows):
        self.W, self.planes, (self.r0, self.r1) = W, tuple(planes), rows
        self.bufs = {k: mem.alloc((self.r1 - self.r0 + 2 * GUARD) * W * BYTES[k]) for k in self.planes}
        self.ptrs = {k: b.ptr + GUARD * W * BYTES[k] for k, b in self.bufs.items()}

    def poison(self, stream):
        for b in self.bufs.values():
            b.fill(POISON, stream)

    def snapshot(self, stream):
        return {k: b.snapshot(stream) for k, b in self.bufs.items()}

    def planes_of(self, snap, tag):
        """The planes of a snapshot (taken after the stream was synchronised); the guard rows must hold the poison."""
        out = {}
        for k, s in snap.items():
            a = s if isinstance(s, np.ndarray) else s.cpu().numpy()
            g = GUARD * self.W * BYTES[k]
            body = (self.r1 - self.r0) * self.W * BYTES[k]
            for name, part in (("before", a[:g]), ("after", a[g + body:g + body + g])):
                bad = np.nonzero(part != POISON)[0]
                assert len(bad) == 0, (f"{tag}: plane {k}: {len(bad)} bytes of the guard row {name} rows "
                                       f"[{self.r0}, {self.r1}) were written; first at byte {int(bad[0])}")
            out[k] = a[g:g + body].copy().view(DTYPE[k])
        return out


# ---- the driver -----------------------------------------------------------------------------------------------------

class HipFailure(AssertionError):
    """A HIP call failed inside the library (PAR_ERR_HIP, PAR_ERR_OOM): the device's state is not known any more."""


def status_of(call):
    """(status, result) of a call of the Renderer surface; a refusal's text is kept for the failure message."""
    try:
        return OK, call()
    except Exception as e:  # ParError, or a stand-in's
        if not hasattr(e, "status"):
            raise
        status_of.detail = str(e)
        return e.status, None


status_of.detail = ""


def check_stats(backend, mirror, tag, rays=None):
    st = backend.stats()  # (raises on PAR_ERR_DEVICE)
    n = 0 if mirror.aabbs is None else len(mirror.aabbs)
    assert st.entities == n, f"{tag}: stats().entities {st.entities}, the scene has {n}"
    if mirror.last is not None:
        pairs, cols = mirror.last_frame_sizes()
        assert st.bin_insertions == pairs, f"{tag}: stats().bin_insertions {st.bin_insertions}, alt:222-240 give {pairs}"
        assert st.occupied_columns == cols, (f"{tag}: stats().occupied_columns {st.occupied_columns}, the oracle's hash has "
                                             f"{cols} in the rendered rows")
    if rays is not None:
        assert st.shadow_rays == rays, f"{tag}: stats().shadow_rays {st.shadow_rays}, the composer counts {rays}"
    return st


def run(backend, ops, mirror, mem, tag=""):
    """Issue `ops` on `backend`, checking every status, every frame and the statistics against `mirror`."""
    W, H = mirror.W, mirror.H
    frames, other = mem.stream(), mem.stream()
    graph_out = None
    held = []  # (device planes a capture baked the addresses of stay allocated while the graph may run)
    for i, o in enumerate(ops):
        where = f"{tag} step {i} {describe(o)}"
        got = OK
        try:
            want = mirror.predicted_status(o)
            k = o["kind"]
            rays = None
            rows = rows_of(o, H)
            sane = 0 <= rows[0] < rows[1] <= H  # (a refused row range still needs memory of some size behind it)
            if k == "render":
                got, out = status_of(lambda: backend.render(o["planes"], rows=o["rows"], flags=o["flags"]))
                if got == OK == want:
                    assert_planes_equal(out, mirror.expected(o["rows"], o["planes"]), o["planes"], where)
            elif k == "relight":
                got, out = status_of(lambda: backend.relight(o["planes"], rows=o["rows"], flags=o["flags"]))
                if got == OK == want:
                    assert_planes_equal(out, mirror.expected(o["rows"], o["planes"]), o["planes"], where)
            elif k in ("render_device", "relight_device", "graph_capture", "graph_capture_lights"):
                g = Guarded(mem, W, o["planes"], rows if sane else (0, 1))
                g.poison(frames)
                if k == "render_device":
                    call = lambda: backend.render_device(g.ptrs, rows=o["rows"], flags=o["flags"], stream=frames.handle)
                elif k == "relight_device":
                    gbuf = mem.alloc((rows[1] - rows[0]) * W * BYTES["gbuf"] if sane else 1)
                    if sane and mirror.ready():  # what a render of these rows puts into its gbuf plane
                        gbuf.write(mirror.expected(o["rows"], ("gbuf",))["gbuf"], frames)
                    ptrs = {p: g.ptrs[p] for p in o["planes"]}
                    call = lambda: backend.relight_device(gbuf.ptr, ptrs, rows=o["rows"], flags=o["flags"], stream=frames.handle)
                else:
                    call = lambda: getattr(backend, k)(g.ptrs, rows=o["rows"], flags=o["flags"], stream=frames.handle)
                got, _ = status_of(call)
                # (in stream order behind the frame, read once the stream has drained)
                shot = g.snapshot(frames) if got == OK else None
                frames.synchronize()
                if got == OK == want and k in ("render_device", "relight_device"):
                    out = g.planes_of(shot, where)
                    assert_planes_equal(out, mirror.expected(o["rows"], o["planes"]), o["planes"], where)
                elif got == OK == want:
                    graph_out = g
                    held.append(g)
            elif k == "graph_launch":
                shots = []
                got = OK
                for _ in range(o["count"] if want == OK else 1):
                    if graph_out is not None:
                        graph_out.poison(frames)
                    got, _ = status_of(lambda: backend.graph_launch(frames.handle))
                    if got != OK or graph_out is None:  # (no capture succeeded: the status assertion below speaks)
                        break
                    shots.append(graph_out.snapshot(frames))  # (in stream order: the next launch overwrites the planes)
                frames.synchronize()
                if got == OK == want:
                    exp = mirror.expected(mirror.graph["rows"], mirror.graph["planes"])
                    for n, s in enumerate(shots):
                        out = graph_out.planes_of(s, f"{where}, launch {n}")
                        assert_planes_equal(out, exp, mirror.graph["planes"], f"{where}, launch {n}")
            elif k == "pick":
                got, px = status_of(lambda: backend.pick(o["x"], o["y"]))
                if got == OK == want:
                    exp = mirror.expected((o["y"], o["y"] + 1), ("gbuf",))["gbuf"][o["x"]]
                    assert px.tobytes() == exp.tobytes(), f"{where}: pick {px} oracle {exp}"
            elif k == "read_grid":
                got, grid = status_of(backend.read_grid)
                if got == OK and mirror.last is not None:
                    assert grids_equal(grid, mirror.grid(mirror.last["aabbs"])), f"{where}: the hash differs from oracle.bin's"
            elif k == "stats":
                got = OK
            elif k == "set_sprites":
                got, _ = status_of(lambda: backend.set_sprites(sprite_table(mirror.par, o["table"], 0)[0]))
            elif k == "set_entities":
                got, _ = status_of(lambda: backend.set_entities(o["aabbs"], o["ids"]))
            elif k == "update_aabbs":
                got, _ = status_of(lambda: backend.update_aabbs(o["aabbs"], o["first"]))
            elif k == "update_aabbs_async":
                s = other if o["other_stream"] else frames
                got, _ = status_of(lambda: backend.update_aabbs(o["aabbs"], o["first"], stream=s.handle))
            elif k == "set_light":
                got, _ = status_of(lambda: backend.set_light(lights_array([o["light"]])))
            elif k == "set_lights":
                got, _ = status_of(lambda: backend.set_lights(lights_array(o["lights"])))
            elif k == "set_light_model":
                got, _ = status_of(lambda: backend.set_light_model(o["model"]))
            elif k == "set_light_tints":
                got, _ = status_of(lambda: backend.set_light_tints(None if o["tints"] is None else T.make_tints(o["tints"])))
            elif k == "graph_stage":
                light = None if o.get("light") is None else lights_array([o["light"]])
                lights = None if o.get("lights") is None else lights_array(o["lights"])
                got, _ = status_of(lambda: backend.graph_stage(o.get("aabbs"), o.get("first", 0), light=light, lights=lights))
            else:
                raise ValueError(k)
            assert got == want, (f"{where}: returned {STATUS.get(got, got)}, the header promises {STATUS[want]}"
                                 + (f" ({status_of.detail})" if got != OK else ""))
            if want == OK:
                if k in ("render", "render_device", "relight", "relight_device") and o["flags"] & COUNT_RAYS:
                    rays = mirror.rays(o["rows"])
                mirror.apply(o)
            else:
                mirror.refuse(o, want)
            check_stats(backend, mirror, where, rays)
        except AssertionError as e:
            last = "\n  ".join(f"{j}: {describe(p)}" for j, p in list(enumerate(ops))[max(0, i - 9):i + 1])
            kind = HipFailure if got in (3, 4) else AssertionError
            raise kind(f"{e}\n{tag}: failed at step {i}; the last ops:\n  {last}") from None
        except Exception as e:
            if hasattr(e, "status"):  # (stats() of the step: PAR_ERR_DEVICE, or a HIP call that failed)
                last = "\n  ".join(f"{j}: {describe(p)}" for j, p in list(enumerate(ops))[max(0, i - 9):i + 1])
                kind = HipFailure if e.status in (3, 4) else AssertionError
                raise kind(f"{where}: {e}\n{tag}: failed at step {i}; the last ops:\n  {last}") from None
            raise
    del held


# ---- the Renderer surface over the oracle, with leaks ---------------------------------------------------------------

LEAKS = ("partial update reaches every second frame", "relight uses the retained frame's lights",
         "lit keeps the previous traced frame's background bits", "a row block writes the rows outside it")


def _store(ptr, a):
    C.memmove(ptr, a.ctypes.data, a.nbytes)


class OracleBackend:
    """What a Renderer does, by the oracle and the composers: two Mirrors (one per "grid set", in step unless a leak
    parts them) say what every call returns and what every frame shows."""

    def __init__(self, par, view, scenes, leak=None):
        assert leak is None or leak in LEAKS
        self.par, self.leak = par, leak
        self.m = [Mirror(par, view, scenes), Mirror(par, view, scenes)]
        self.cur = 0            # whose scene the next frame shows
        self.kept_lights = None
        self.bg = None          # the lit plane of the last frame that traced the background
        self.graph_ptrs = None
        self.rays = -1

    def _do(self, o, only=None):
        st = self.m[0].predicted_status(o)
        if st != OK:
            for m in self.m:
                m.refuse(o, st)
            raise self.par.ParError(st, describe(o))
        for i, m in enumerate(self.m):
            if only is None or i == only:
                m.apply(o)

    def _frame(self, o, planes, rows, flags, relit=False):
        """The planes of a frame; `o` is applied afterwards."""
        st = self.m[0].predicted_status(o)
        if st != OK:
            raise self.par.ParError(st, describe(o))
        m = self.m[self.cur]
        saved = m.lights
        if relit and self.leak == LEAKS[1]:
            m.lights = self.kept_lights
        out = {k: v.copy() for k, v in m.expected(rows, planes).items()}
        self.rays = m.rays(rows) if flags & COUNT_RAYS else -1
        m.lights = saved
        if "lit" in planes or flags & TRACE_BACKGROUND:
            r0, r1 = rows or (0, m.H)
            if self.bg is not None and self.leak == LEAKS[2] and "lit" in planes:
                back = m.expected(rows, ("palidx",))["palidx"] == 0xFF
                out["lit"][back] = self.bg[r0 * m.W:r1 * m.W][back]
            self.bg = m.full()[0]["lit"]  # (what this frame's background rays found; never written to)
        if not relit:
            self.kept_lights = list(m.lights)
            self.cur ^= 1
        for x in self.m:
            x.apply(o)
        return out

    def close(self):
        pass

    def set_sprites(self, sprites):
        n = len(sprites)  # (the tables are told apart by what sprite_table changes in them)
        table = 0 if n == 1 else (2 if int(sprites[1]["depth"][0]) == 95 else 1)
        self._do(op("set_sprites", table=table))

    def set_entities(self, aabbs, sprite_ids=None):
        self._do(op("set_entities", aabbs=np.ascontiguousarray(aabbs, dtype=T.AABB), ids=sprite_ids,
                    regime=None))

    def update_aabbs(self, aabbs, first=0, stream=None):
        o = op("update_aabbs", aabbs=np.ascontiguousarray(aabbs, dtype=T.AABB), first=first)
        partial = self.m[0].aabbs is not None and len(aabbs) < len(self.m[0].aabbs)
        self._do(o, only=self.cur if partial and self.leak == LEAKS[0] else None)

    def set_light(self, light):
        self.set_lights(light)

    def set_lights(self, lights):
        self._do(op("set_lights", lights=[tuple(int(l[k]) for k in ("x", "y", "z", "radius")) for l in lights]))

    def set_light_model(self, model):
        self._do(op("set_light_model", model=model))

    def set_light_tints(self, tints):
        self._do(op("set_light_tints", tints=None if tints is None else [tuple(float(t[k]) for k in "rgb") for t in tints]))

    def render(self, planes=("fb",), rows=None, flags=0):
        return self._frame(op("render", planes=planes, rows=rows, flags=flags), planes, rows, flags)

    def relight(self, planes=("fb",), rows=None, flags=0):
        return self._frame(op("relight", planes=planes, rows=rows, flags=flags), planes, rows, flags, relit=True)

    def _to_device(self, out, ptrs, rows, whole):
        m = self.m[0]
        for k, a in out.items():
            _store(ptrs[k], a)
            if self.leak == LEAKS[3] and not whole:  # the rows next to the block, with what an older frame left there
                stale = np.zeros(m.W * BYTES[k], dtype=np.uint8)
                _store(ptrs[k] - stale.nbytes, stale)
                _store(ptrs[k] + a.nbytes, stale)

    def render_device(self, device_ptrs, rows=None, flags=0, stream=0, timed=False):
        planes = tuple(k for k in ALL if device_ptrs.get(k))
        out = self._frame(op("render_device", planes=planes, rows=rows, flags=flags), planes, rows, flags)
        self._to_device(out, device_ptrs, rows, rows is None or tuple(rows) == (0, self.m[0].H))

    def relight_device(self, gbuf_ptr, device_ptrs, rows=None, flags=0, stream=0):
        planes = tuple(k for k in ALL if device_ptrs.get(k))
        out = self._frame(op("relight_device", planes=planes, rows=rows, flags=flags), planes, rows, flags, relit=True)
        self._to_device(out, device_ptrs, rows, True)

    def _capture(self, kind, device_ptrs, rows, flags):
        planes = tuple(k for k in ALL if device_ptrs.get(k))
        self._do(op(kind, planes=planes, rows=rows, flags=flags))
        self.graph_ptrs = dict(device_ptrs)

    def graph_capture(self, device_ptrs, rows=None, flags=0, stream=0):
        self._capture("graph_capture", device_ptrs, rows, flags)

    def graph_capture_lights(self, device_ptrs, rows=None, flags=0, stream=0):
        self._capture("graph_capture_lights", device_ptrs, rows, flags)

    def graph_stage(self, aabbs=None, first=0, light=None, lights=None):
        o = op("graph_stage")
        if aabbs is not None:
            o["aabbs"], o["first"] = np.ascontiguousarray(aabbs, dtype=T.AABB), first
        for name, v in (("light", light), ("lights", lights)):
            if v is not None:
                rows = [tuple(int(l[k]) for k in ("x", "y", "z", "radius")) for l in v]
                o[name] = rows[0] if name == "light" else rows
        self._do(o)

    def graph_launch(self, stream=0):
        g = self.m[0].graph
        if g is None:
            self._do(op("graph_launch", count=1))
        out = self._frame(op("graph_launch", count=1), g["planes"], g["rows"], g["flags"])
        self._to_device(out, self.graph_ptrs, g["rows"], tuple(g["rows"]) == (0, self.m[0].H))

    def pick(self, x, y):
        o = op("pick", x=x, y=y)
        if self.m[0].predicted_status(o) != OK:
            self._do(o)
        return self._frame(o, ("gbuf",), (y, y + 1), 0)["gbuf"][x:x + 1]

    def stats(self):
        m = self.m[self.cur ^ 1]  # (whose scene the last frame showed)
        pairs, cols = m.last_frame_sizes() if m.last is not None else (0, 0)
        return types.SimpleNamespace(entities=0 if m.aabbs is None else len(m.aabbs), bin_insertions=pairs,
                                     occupied_columns=cols, shadow_rays=self.rays)

    def read_grid(self):
        m = self.m[self.cur ^ 1]
        g = m.grid(m.last["aabbs"])
        return g.count, g.map, g.bins


# ---- the hand-written sequences: one per hazard ---------------------------------------------------------------------

def _set(view, regime, seed):
    rng = np.random.default_rng([VIEW_IDS[view], 1000 + seed])
    return op("set_entities", regime=regime, aabbs=regime_scene(view, regime, rng), ids=None)


def _checked(frame):
    return [frame, op("read_grid"), op("stats")]


def hand_written():
    """{name: (view, ops)}: one sequence per hazard the issue names, readable step by step."""
    ref, b8, odd, wide = VIEWS
    out = {}
    A, B_, C_ = (300, 160, 80, 0), (60, 40, 200, 0), (470, 300, 20, 0)
    start = lambda view, regime, seed: [op("set_sprites", table=0), _set(view, regime, seed), op("set_light", light=A)]
    full = lambda planes=ALL, flags=0, rows=None: op("render", planes=planes, rows=rows, flags=flags)

    # 1. the wipe across row blocks and set parity
    for view, rows in ((ref, (37, 203)), (odd, (16, 48)), (wide, (5, 9))):
        first, second = _set(view, "many", 1), _set(view, "overflow", 2)
        ops = [op("set_sprites", table=0), first, op("set_light", light=A)] + _checked(full())
        ops += [second] + _checked(full(rows=rows)) + _checked(full(("fb", "palidx"), rows=rows))
        ops += [op("set_entities", regime="empty", aabbs=T.make_aabbs([]), ids=None)] + _checked(full())
        ops += [first] + _checked(full()) + _checked(full(rows=rows)) + [second] + _checked(full())
        out[f"wipe across row blocks and set parity, {view}"] = (view, ops)

    # 2. the pool grows in the middle of a context's life
    ops = start(b8, "sparse", 3) + _checked(full()) + _checked(full(("fb",))) + _checked(full(rows=(8, 120)))
    ops += [_set(b8, "big", 4)] + _checked(full()) + _checked(full(("fb", "palidx"))) + _checked(full(rows=(40, 41)))
    ops += [_set(b8, "sparse", 5)] + _checked(full()) + _checked(full())
    ops += [_set(b8, "big", 6), op("set_lights", lights=[A, B_]), op("set_light_model", model=1)]
    ops += _checked(full()) + _checked(full()) + [_set(b8, "many", 7)] + _checked(full())
    out["pool growth mid-life"] = (b8, ops)

    # 3. sparse -> dense -> sparse and <= 256 -> >= 2048 -> <= 256 columns, with and without PIPELINED
    for flags in (0, PIPELINED):
        ops = [op("set_sprites", table=0), op("set_light", light=A)]
        for n, regime in enumerate(("sparse", "dense", "sparse", "many", "dense", "overflow", "sparse", "many", "sparse")):
            ops += [_set(wide, regime, 10 + n), full(flags=flags), full(("fb", "palidx"), flags=flags),
                    full(("fb",), flags=flags, rows=(64, 200)), op("stats")]
        out[f"sparse, dense, sparse and few, many, few columns, flags {flags}"] = (wide, ops)

    # 4. the background's lit bits
    for lights_a, lights_b in (([A], [B_]), ([A, B_, C_], [C_, (20, 100, 300, 0), (240, -50, -30, 0)])):
        ops = start(ref, "dense", 20)[:2]
        ops += [op("set_lights", lights=lights_a), full(("fb", "lit")), full(("fb",)), op("set_lights", lights=lights_b),
                full(("fb",), flags=TRACE_BACKGROUND), full(("lit",)), full(("fb", "lit"), rows=(37, 251)),
                op("set_lights", lights=lights_a), full(("fb", "palidx")), full(ALL),
                _set(ref, "empty", 21), full(("fb", "lit")), op("set_lights", lights=lights_b), full(("lit",))]
        out[f"background lit bits, {len(lights_a)} lights"] = (ref, ops)

    # 5. graphs out of step with plain renders
    for kind in ("graph_capture", "graph_capture_lights"):
        view = ref
        rng = np.random.default_rng(5)
        scene = _set(view, "many", 30)
        ops = [op("set_sprites", table=0), scene, op("set_light", light=A), full()]
        ops += [op(kind, planes=ALL, rows=None, flags=0), op("graph_launch", count=1), full(("fb",)),
                op("graph_launch", count=1)]
        a = scene["aabbs"]
        for _ in range(2):
            first, moved = _moved(rng, a, most=40)
            a = a.copy()
            a[first:first + len(moved)] = moved
            ops += [op("graph_stage", first=first, aabbs=moved, light=B_), op("graph_launch", count=1)]
        ops += [op("graph_launch", count=1), full(), full(("fb", "lit")), op("graph_launch", count=3), op("read_grid")]
        if kind == "graph_capture_lights":
            ops += [op("graph_stage", lights=[A, C_, B_]), op("graph_launch", count=2), full(), op("graph_launch", count=1)]
        out[f"graphs out of step, {kind}"] = (view, ops)

    # 6. an asynchronous update on a second stream
    rng = np.random.default_rng(6)
    scene = _set(ref, "many", 40)
    first, moved = _moved(rng, scene["aabbs"], most=40)
    dev = lambda planes=ALL: op("render_device", planes=planes, rows=None, flags=0)
    ops = [op("set_sprites", table=0), scene, op("set_light", light=A), full(), dev(),
           op("graph_capture", planes=ALL, rows=None, flags=0), op("graph_launch", count=2), full(),
           op("update_aabbs_async", first=first, aabbs=moved, other_stream=True),
           op("relight", planes=LIT, rows=None, flags=0),  # NOT_READY: the update dropped the retained frame
           dev(), op("relight_device", planes=LIT, rows=None, flags=0), op("graph_launch", count=1),
           op("relight", planes=LIT, rows=None, flags=0),  # NOT_READY again: a graph launch leaves no retained frame
           op("update_aabbs_async", first=first, aabbs=scene["aabbs"][first:first + len(moved)], other_stream=False),
           op("graph_launch", count=2), dev(("fb", "palidx")), full(), op("relight", planes=LIT, rows=(40, 200), flags=0),
           op("read_grid"), op("stats")]
    out["async update on a second stream"] = (ref, ops)

    # 7. (found by a generated sequence) a graph captured again after par_set_entities brought more entities
    small, large = _set(ref, "sparse", 50), _set(ref, "many", 51)
    first, moved = _moved(np.random.default_rng(7), large["aabbs"], most=40)
    capture = op("graph_capture", planes=ALL, rows=None, flags=0)
    ops = [op("set_sprites", table=0), small, op("set_light", light=A), full(), capture, op("graph_launch", count=2),
           large, capture, op("graph_launch", count=2), op("graph_stage", first=first, aabbs=moved, light=B_),
           op("graph_launch", count=2), full(), op("read_grid"), op("stats")]
    out["a graph captured again after the scene grew"] = (ref, ops)

    # 8. a capture that traces the background without a lit plane needs a plain frame of that size, traced so, before
    #    it; refused, it leaves no graph and no retained frame
    for kind in ("graph_capture", "graph_capture_lights"):
        traced = lambda rows: op(kind, planes=("fb", "brightness"), rows=rows, flags=TRACE_BACKGROUND)
        ops = start(ref, "many", 60) + [full(), op(kind, planes=ALL, rows=None, flags=0), op("graph_launch", count=1), full(),
                                        traced((5, 300)),                                   # NOT_READY
                                        op("graph_launch", count=1),                        # NOT_READY: no graph is left
                                        op("relight", planes=LIT, rows=None, flags=0),      # NOT_READY: no retained frame
                                        full(("fb", "brightness"), flags=TRACE_BACKGROUND, rows=(5, 300)), traced((5, 300)),
                                        op("graph_launch", count=2), full(), op("graph_launch", count=1),
                                        traced(None),                                       # NOT_READY: more rows than traced
                                        op("graph_launch", count=1),                        # NOT_READY
                                        full(("fb",), flags=TRACE_BACKGROUND), traced(None), op("graph_launch", count=2),
                                        op("read_grid"), op("stats")]
        out[f"a traced background without a lit plane, {kind}"] = (ref, ops)

    # 9. a context without entities meets a graph
    empty = op("set_entities", regime="empty", aabbs=T.make_aabbs([]), ids=None)
    capture = op("graph_capture", planes=ALL, rows=None, flags=0)
    ops = [op("set_sprites", table=0), empty, op("set_light", light=A), full(), capture, op("graph_launch", count=2),
           full(("fb", "lit")), op("graph_launch", count=1), op("graph_stage", light=B_), op("graph_launch", count=1),
           _set(ref, "many", 61), op("graph_launch", count=1),  # NOT_READY: par_set_entities dropped the graph
           full(), capture, op("graph_launch", count=1), empty, full(),
           op("graph_capture_lights", planes=("fb", "lit"), rows=(37, 203), flags=TRACE_BACKGROUND),
           op("graph_launch", count=3), op("read_grid"), op("stats")]
    out["captures of a scene without entities"] = (ref, ops)

    # 10. (found by generated sequences) a plain frame or a pick right after par_graph_stage, before any launch: the staged
    #     AABBs are the scene
    scene = _set(ref, "many", 70)
    rng = np.random.default_rng(10)
    first, moved = _moved(rng, scene["aabbs"], most=40)
    later = scene["aabbs"].copy()
    later[first:first + len(moved)] = moved
    first2, moved2 = _moved(rng, later, most=40)
    ops = [op("set_sprites", table=0), scene, op("set_light", light=A), full(),
           op("graph_capture", planes=ALL, rows=None, flags=0), op("graph_launch", count=1),
           op("graph_stage", first=first, aabbs=moved), full(), op("read_grid"),
           op("graph_stage", first=first2, aabbs=moved2, light=B_), op("pick", x=240, y=160),
           op("render_device", planes=ALL, rows=(37, 203), flags=0), op("graph_launch", count=2), full(), op("stats")]
    out["a plain frame right after a stage"] = (ref, ops)
    return out

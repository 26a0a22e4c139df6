"""What tests/post_chain.py holds, without a GPU: expected() against a composition of the slow restatements of every
model, the conditions on the chains' inputs that the GPU tests rely on, the driver against a model-backed stand-in with
and without the faults a capture can have, and the list of the post entry points the chains reach."""
import inspect
import re

import numpy as np
import pytest

import delta as DL
import outline as O
import palette as P
import palette_refine as R
import pattern as D
import plane_tiles as PT
import post_chain as PC
import present as PR
import quantize as Q
import upscale as U
from post_chain import T
from test_palette_cpu import cut_loop

SMALL_SHAPE = "37x23 rows 5..18"


def make(chain, shape):
    # (the palette of finish and of the tiles' frame: 256 entries on the larger shape, 33 on the smaller)
    return PC.chain_a(shape) if chain == "A" else PC.chain_b(shape, 256 if shape.startswith("131") else 33)


def on_the_stand_in(c, fault=None, at=None, order=PC.ORDER):
    """The replays of post_chain.replays on a ModelBackend: the expected planes of every replay."""
    bufs = PC.HostBuffers(c)
    backend = PC.ModelBackend(bufs, fault, at)

    def launch():
        backend.begin_replay()
        PC.issue(backend, c, bufs, 0, c.everything())

    return PC.replays(c, bufs, PC.inputs_of(c), launch, order=order)


# ---- 1. expected() against the slow restatements ---------------------------------------------------------------------

class Slow:
    """The same arithmetic one pixel, one element or one cell at a time."""
    outline = staticmethod(O.model_loop)
    quantize = staticmethod(Q.model_loop)
    pattern = staticmethod(D.model_loop)
    upscale = staticmethod(U.slow_model)
    present = staticmethod(PR.slow_model)
    changed4, pack4 = staticmethod(DL.slow_changed), staticmethod(DL.slow_pack)
    changed, pack, unpack, assemble = (staticmethod(PT.slow_changed), staticmethod(PT.slow_pack),
                                       staticmethod(PT.slow_unpack), staticmethod(PT.slow_assemble))
    emit = staticmethod(lambda work, n_colors: P.emit(T, work, n_colors))  # (Python integers as it is)

    @staticmethod
    def finish(params, style, gbuf, grows, palette, spread, desc, fb, rows, guard=0):
        lined = O.model_loop(params, style, gbuf, grows, fb, rows)[1]
        index = Q.model_loop(params, palette, lined, rows, spread)[0]
        return PR.slow_model(params, desc, rows, index=index, palette=palette, guard=guard), index

    @staticmethod
    def refine(params, fb, rows, palette, iterations):
        palette = palette.copy()
        for _ in range(iterations):
            index = Q.model_loop(params, palette, fb, rows, 0)[0]
            palette, changed = R.update_loop(palette, fb, index)
        return palette, index, changed

    @staticmethod
    def count(work, fb):
        for px in fb:
            cell = (int(px["red"]) >> 3) | (int(px["green"]) >> 3) << 5 | (int(px["blue"]) >> 3) << 10
            work["hist"][0][cell] = (int(work["hist"][0][cell]) + 1) & 0xFFFFFFFF

    @staticmethod
    def cut(work, n_colors):
        lut, n = cut_loop(work["hist"][0], n_colors)
        work["lut"][0], work["n_entries"][0], work["sums"][0] = lut, n, 0

    @staticmethod
    def sums(work, fb):
        for px in fb:
            cell = (int(px["red"]) >> 3) | (int(px["green"]) >> 3) << 5 | (int(px["blue"]) >> 3) << 10
            k = int(work["lut"][0][cell])
            for j, v in enumerate((int(px["red"]), int(px["green"]), int(px["blue"]), 1)):
                work["sums"][0][k][j] = (int(work["sums"][0][k][j]) + v) & P.MASK64


@pytest.mark.parametrize("chain", ["A", "B"])
def test_expected_equals_the_slow_models(chain):
    c = make(chain, SMALL_SHAPE)
    sets = PC.inputs_of(c)
    history = PC.initial_history(c, sets[0])
    slow_history = PC.initial_history(c, sets[0], Slow)
    for k in (0, 1, 2):
        fast = PC.expected(c, dict(sets[k], **history))
        slow = PC.expected(c, dict(sets[k], **slow_history), Slow)
        assert set(fast) == set(slow) == set(c.names("in", "history", "out"))
        for name in fast:
            bad = np.nonzero(fast[name] != slow[name])[0]
            assert len(bad) == 0, f"chain {chain}, set {k}: plane {name} differs from the slow models first at byte {bad[0]}"
        history = {n: fast[n] for n in history}
        slow_history = {n: slow[n] for n in slow_history}


# ---- 2. the inputs exercise the mechanisms ---------------------------------------------------------------------------

def i32(plane):
    return int(plane.view(np.int32)[0])


@pytest.fixture(scope="module", params=list(PC.SHAPES))
def seen(request):
    """chain name -> (chain, expected planes of every replay) on one shape, from a run on the stand-in without a fault,
    which passes check() at every replay."""
    return {chain: (c, on_the_stand_in(c)) for chain, c in ((k, make(k, request.param)) for k in ("A", "B"))}


def test_chain_a_reaches_its_mechanisms(seen):
    c, replays = seen["A"]
    p, W, rows = c.params, c.params.width, c.rows
    changed = []
    for k, exp in zip(PC.ORDER, replays):
        work = exp["fit_work"].view(T.PALETTE_WORK)
        assert int(work["n_entries"][0]) == PC.N_FIT, "the fit reaches 33 entries"
        changed.append(i32(exp["changed"]))
        palette, lined = exp["palette"].view(T.COLOR), exp["lined"].view(T.COLOR)
        plain = Q.model(p, palette, lined, rows, 0)[0]
        assert (exp["pat_index"] != plain).sum() > len(plain) // 20, "the pattern index differs from the spread-0 index"
        assert (exp["index2"] != plain).sum() > len(plain) // 20, "so does the index at spread 24"
        assert exp["lined"].tobytes() != exp["fb"].tobytes()
        assert set(np.unique(exp["edge"])) == {0, 1, 2}, "both outline classes occur, and pixels of neither"
        up = c.up_rows
        src = exp["pat_index"].reshape(rows[1] - rows[0], W)[up[0] - rows[0]:up[1] - rows[0]]
        nearest = np.repeat(np.repeat(src, 3, axis=0), 3, axis=1).reshape(-1)
        assert (exp["up_index"] != nearest).sum() > 0, "Scale3x differs from nearest-neighbour somewhere"
        for name, pitch_of in (("up_surface", 4 * W * 3 + 4), ("surface", 4 * W * 2 + 12)):
            gap = exp[name].reshape(-1, pitch_of)[:, -4:]
            assert (gap == PC.POISON).all(), f"{name}: the pitch leaves a gap, which keeps what it held"
    assert any(changed), f"refine's last round changes an entry for some input set: {changed}"


def test_chain_b_reaches_its_regimes(seen):
    c, replays = seen["B"]
    cap = c.capacity
    for tag in ("t", "i", "g"):
        counts = [i32(exp[tag + "_count"]) for exp in replays]
        assert counts[0] == 0, f"{tag}: an identical frame"
        assert 1 <= counts[1] <= cap and counts[1] < counts[2], f"{tag}: between 1 and the capacity: {counts}"
        assert counts[2] > PC.SMALL and counts[3] > PC.SMALL, f"{tag}: above the small capacity: {counts}"
    small = [i32(exp["s_count"]) for exp in replays]
    assert small == [i32(exp["t_count"]) for exp in replays], "the small pair sees the frames the chain's pair sees"
    # at the small capacity the list and the slots end at two; the map ranks every changed tile all the same
    for exp in replays[1:]:
        assert (exp["s_tiles"].view(np.int32) == exp["t_tiles"].view(np.int32)[:PC.SMALL]).all()
        slot = 4 * c.params.bin_size ** 2
        assert exp["s_packed"].tobytes() == exp["t_packed"][:PC.SMALL * slot].tobytes()
        assert exp["s_map"].tobytes() == exp["t_map"].tobytes()
    # a replay's previous frame is the frame of the replay before
    for before, after in zip(replays, replays[1:]):
        assert before["prev"].tobytes() == before["cur"].tobytes() != after["cur"].tobytes()
    assert c.params.width % 4 != 0 and (c.rows[1] - c.rows[0]) * c.params.width % 4 != 0, "unaligned rows, an odd pixel count"


@pytest.mark.parametrize("chain", ["A", "B"])
def test_the_input_sets_differ_on_every_output_plane(seen, chain):
    c, replays = seen[chain]
    # (bg_rows is the one plane that is a function of the arguments alone: par_background_fill reads no plane)
    for name in c.names("out"):
        for a in range(3):
            for b in range(a + 1, 3):
                same = replays[a][name].tobytes() == replays[b][name].tobytes()
                assert same == (name == "bg_rows"), f"chain {chain}: plane {name} of input sets {a} and {b}"
    assert replays[3].keys() == replays[0].keys()
    for name in c.names("out"):
        assert any((r[name] != PC.POISON).any() for r in replays), f"{name} is written"


# ---- 3. the driver notices what a capture can get wrong --------------------------------------------------------------

# chain, fault, the call it strikes, which of that binding's calls in a replay
FAULT_CASES = [
    ("A", "stale replay", "quantize_pattern", 0),
    ("A", "stale replay", "palette_emit", 0),
    ("A", "skipped step", "palette_cut", 0),
    ("A", "skipped step", "present", 0),
    ("A", "wrong stream order", "palette_count", 0),
    ("A", "wrong stream order", "palette_emit", 0),
    ("B", "stale replay", "finish", 0),
    ("B", "stale replay", "tiles_changed", 1),
    ("B", "skipped step", "tiles_unpack", 0),
    ("B", "skipped step", "background_fill", 0),
    ("B", "count baked in", "tiles_pack_counted", 0),  # the small pair's
    ("B", "count baked in", "tiles_pack_counted", 1),
    ("B", "count baked in", "plane_tiles_pack_counted", 0),
    ("B", "count baked in", "plane_tiles_pack_counted", 1),
    ("B", "wrong stream order", "tiles_changed", 1),
    ("B", "wrong stream order", "plane_tiles_pack", 0),
]


@pytest.mark.parametrize("chain,fault,binding,nth", FAULT_CASES)
def test_the_driver_notices(chain, fault, binding, nth):
    c = make(chain, SMALL_SHAPE)
    with pytest.raises(AssertionError, match=f"chain {chain}, replay [0-3] of input set"):
        on_the_stand_in(c, fault, c.index_of(binding, nth))


def test_every_fault_is_among_the_cases():
    assert {f for _, f, _, _ in FAULT_CASES} == set(PC.FAULTS)


def test_check_names_the_plane_and_the_offset_and_checks_guards():
    c = make("A", SMALL_SHAPE)
    bufs = PC.HostBuffers(c)
    exp = {"edge": np.full(c.planes["edge"].nbytes, 7, dtype=np.uint8)}
    bufs.fill("edge", 7)
    PC.check(bufs, exp, "fine")
    bufs._view("edge")[11] = 8
    with pytest.raises(AssertionError, match="plane edge differs at 1 of .* first at byte 11"):
        PC.check(bufs, exp, "one byte")
    bufs._view("edge")[11] = 7
    p = bufs.planes["lined"]
    p.t[p.at + p.nbytes] = 0
    with pytest.raises(AssertionError, match="bytes outside plane lined were written"):
        PC.check(bufs, exp, "a guard byte")


# ---- 4. every post entry point is in a captured chain ----------------------------------------------------------------

def symbols_of(par, binding):
    return set(re.findall(r"lib\(\)\.(par_\w+)", inspect.getsource(getattr(par, binding))))


def test_every_device_post_entry_point_is_in_a_captured_chain(par):
    frames = ("par_render_device", "par_relight_device")  # they take a context: not passes over finished planes
    needed = {s for s in par.ABI_SYMBOLS if s.endswith("_device") and s not in frames}
    assert len(needed) == 14, sorted(needed)
    # the tile calls whose names do not end in _device, as the header lists them
    needed |= {"par_tiles_pack", "par_tiles_unpack", "par_tiles_assemble", "par_background_fill", "par_tiles_pack_counted",
               "par_plane_tiles_pack", "par_plane_tiles_pack_counted", "par_plane_tiles_unpack", "par_plane_tiles_assemble"}
    assert needed <= set(par.ABI_SYMBOLS)
    used, reached = set(), set()
    for shape in PC.SHAPES:
        for c in (make("A", shape), make("B", shape), PC.chain_frame(shape)):
            used |= {s.binding for s in c.captured() if s.binding not in PC.PSEUDO}
    for binding in used:
        got = symbols_of(par, binding)
        assert len(got) == 1, f"{binding} calls {got}"
        reached |= got
    assert reached == needed, f"not captured: {sorted(needed - reached)}; not post calls: {sorted(reached - needed)}"
    assert used == set(PC.POINTERS)


def test_the_steps_name_the_bindings_arguments(par):
    for shape in PC.SHAPES:
        for c in (make("A", shape), make("B", shape)):
            for step in c.everything():
                if step.binding in PC.PSEUDO:
                    continue
                names = set(inspect.signature(getattr(par, step.binding)).parameters)
                assert set(step.args) <= names - {"stream"}, f"{step.binding}: {set(step.args) - names}"
                assert set(PC.POINTERS[step.binding]) <= names
                refs = {k for k, v in step.args.items() if isinstance(v, PC.Ref)}
                assert refs <= set(PC.POINTERS[step.binding]), f"{step.binding}: {refs}"

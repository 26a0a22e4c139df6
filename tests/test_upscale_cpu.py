"""Upscale without a GPU: the two calls are declared, exported and bound; UPSCALE_DESC has the header's layout; every
PAR_ERR_INVALID_ARG of the contract comes back from both calls before any device work and with nothing written; the
vectorised model the GPU tests lean on (upscale.model) equals a per-pixel loop (upscale.slow_model); and the properties
the GPU tests lean on hold on the model."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import headers
import present as P
import upscale as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID_ARG = 1

DECLARATIONS = {
    "par_upscale_device": "const par_params* params, void* stream, const par_upscale_desc* desc, const par_color* fb, "
                          "const uint8_t* index, const par_color* d_palette, int n_colors, int src_row_begin, "
                          "int src_row_end, int row_begin, int row_end, void* out, uint8_t* index_out",
    "par_upscale_host": "const par_params* params, int device, const par_upscale_desc* desc, const par_color* fb, "
                        "const uint8_t* index, const par_color* palette, int n_colors, int src_row_begin, "
                        "int src_row_end, int row_begin, int row_end, void* out, uint8_t* index_out",
}


def test_declared_exported_and_bound(par, T):
    headers.assert_declared(par, "par_raytracer.h", DECLARATIONS, ("upscale", "upscale_host", "make_upscale_desc"))
    assert (par.UPSCALE_SCALE2X, par.UPSCALE_SCALE3X, par.UPSCALE_SCALE4X) == (2, 3, 4)
    assert (T.UPSCALE_SCALE2X, T.UPSCALE_SCALE3X, T.UPSCALE_SCALE4X) == (2, 3, 4)


def test_desc_layout_is_the_headers(T):
    types_h = open(os.path.join(ROOT, "include", "par_types.h")).read()
    m = re.search(r"typedef struct par_upscale_desc \{(.*?)\} par_upscale_desc;", types_h, flags=re.S)
    assert m, "par_upscale_desc is not declared"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = [f.strip() for decl in re.findall(r"int32_t\s+([^;]+);", body) for f in decl.split(",")]
    assert fields == ["scaler", "pitch", "order"]
    assert re.sub(r"int32_t\s+[^;]+;", "", body).strip() == "", "a field that is not an int32_t"
    assert T.UPSCALE_DESC.itemsize == 12
    assert [(n, T.UPSCALE_DESC.fields[n][1], T.UPSCALE_DESC.fields[n][0]) for n in T.UPSCALE_DESC.names] == \
        [(n, 4 * i, np.dtype("<i4")) for i, n in enumerate(fields)]
    assert re.search(r"enum\s*\{\s*PAR_UPSCALE_SCALE2X\s*=\s*2\s*,\s*PAR_UPSCALE_SCALE3X\s*=\s*3\s*,\s*"
                     r"PAR_UPSCALE_SCALE4X\s*=\s*4\s*\}", types_h)
    assert T.make_upscale_desc(3, width=7).tobytes() == np.array([3, 84, 0], dtype="<i4").tobytes()
    assert T.make_upscale_desc(4, pitch=200, order=T.PRESENT_BGRA).tobytes() == np.array([4, 200, 1], dtype="<i4").tobytes()
    with pytest.raises(ValueError):
        T.make_upscale_desc(2)


# ---- argument errors: no device needed, nothing written -----------------------------------------------------------

# (tag, overrides): one case per condition of the contract; each breaks that one condition alone. The good call is an
# index source of 8 x 6 at k = 3 with a pitch of 112 (a gap of 16 bytes), source rows (1, 6), output rows (2, 5), both
# outputs and a palette of 4.
W0, H0, K0, PITCH0 = 8, 6, 3, 112
BAD_CALLS = [
    ("null params", dict(params=None)),
    ("null desc", dict(desc=None)),
    ("both sources", dict(fb=True)),
    ("neither source", dict(index=None)),
    ("both outputs null", dict(out=None, index_out=None, palette=None, n_colors=0)),
    ("index_out with an fb source", dict(fb=True, index=None, palette=None, n_colors=0)),
    ("index source and a surface without a palette", dict(palette=None)),
    ("index source and a surface, n_colors 0", dict(n_colors=0)),
    ("index source and a surface, n_colors 257", dict(n_colors=257)),
    ("index source without a surface, with a palette", dict(out=None)),
    ("index source without a surface, n_colors 4", dict(out=None, palette=None)),
    ("fb source with a palette", dict(fb=True, index=None, index_out=None, n_colors=0)),
    ("fb source with n_colors 4", dict(fb=True, index=None, index_out=None, palette=None)),
    ("scaler 1", dict(scaler=1)),
    ("scaler 5", dict(scaler=5, pitch=4 * 8 * 5)),
    ("scaler 0", dict(scaler=0)),
    ("order 2", dict(order=2)),
    ("order -1", dict(order=-1)),
    ("pitch not a multiple of 4", dict(pitch=98)),
    ("pitch below 4 * width * k", dict(pitch=92)),
    ("4 * width * k beyond an int32", dict(width=1 << 27, scaler=4, pitch=0x7FFFFFFC)),
    ("width 0", dict(width=0)),
    ("width negative", dict(width=-8)),
    ("src_row_begin negative", dict(src_rows=(-1, 6))),
    ("src_row_begin > row_begin", dict(src_rows=(3, 6))),
    ("row_begin == row_end", dict(rows=(2, 2))),
    ("row_begin > row_end", dict(rows=(4, 3))),
    ("row_end > src_row_end", dict(src_rows=(1, 4))),
    ("src_row_end > height", dict(src_rows=(1, 7))),
]


def _call(par, T, call, over):
    """One call made from the good call with `over` applied: (status, every buffer still as it was filled)."""
    L = par.lib()
    fn = L.par_upscale_device if call == "device" else L.par_upscale_host
    first = C.c_void_p(0) if call == "device" else -1  # the stream / the device
    params = T.default_params(W0, H0)
    params.width = over.get("width", W0)
    palette = np.full(256 * 4, 0x5A, dtype=np.uint8).view(T.COLOR)  # host dummies: never dereferenced
    fb = np.full(W0 * H0 * 4, 0xA5, dtype=np.uint8).view(T.COLOR)
    index = np.full(W0 * H0, 0x3C, dtype=np.uint8)
    out = np.full(H0 * 4 * 4 * W0 * 5, 0xC3, dtype=np.uint8)
    index_out = np.full(H0 * 4 * W0 * 4, 0x96, dtype=np.uint8)
    desc = T.make_upscale_desc(over.get("scaler", K0), over.get("pitch", PITCH0), over.get("order", 0))
    arg = dict(params=params, desc=desc, out=out, index_out=index_out, fb=None, index=index, palette=palette, n_colors=4,
               src_rows=(1, 6), rows=(2, 5))
    arg.update({k: v for k, v in over.items() if k in arg})
    if arg["fb"] is True:
        arg["fb"] = fb
    rc = fn(None if arg["params"] is None else C.byref(arg["params"]), first, T.ptr(arg["desc"]), T.ptr(arg["fb"]),
            T.ptr(arg["index"]), T.ptr(arg["palette"]), arg["n_colors"], arg["src_rows"][0], arg["src_rows"][1],
            arg["rows"][0], arg["rows"][1], T.ptr(arg["out"]), T.ptr(arg["index_out"]))
    untouched = bool((fb.view(np.uint8) == 0xA5).all() and (index == 0x3C).all() and (out == 0xC3).all() and
                     (index_out == 0x96).all() and (palette.view(np.uint8) == 0x5A).all())
    return rc, untouched


def test_the_good_call_of_the_bad_calls_is_good(par, T):
    """What the cases start from passes every check of the contract, so each case breaks one condition alone; the
    overflow case's product wraps to a negative int32, which a 32-bit check would let through; and without a surface the
    pitch and the order are not read."""
    assert W0 > 0 and 0 <= 1 <= 2 < 5 <= 6 <= H0 and K0 in (2, 3, 4)
    assert PITCH0 % 4 == 0 and PITCH0 >= 4 * W0 * K0
    product = 4 * (1 << 27) * 4
    assert product > 0x7FFFFFFF and int(np.array(product).astype(np.int32)) < 0 and 0x7FFFFFFC % 4 == 0
    assert len({tag for tag, _ in BAD_CALLS}) == len(BAD_CALLS)
    # and the library agrees: the host form gets past its argument checks (no device here, or the outputs)
    rc, _ = _call(par, T, "host", {})
    assert rc in (0, 2), rc  # PAR_OK or PAR_ERR_NO_DEVICE
    for tag, over in (("a bad pitch", dict(pitch=98)), ("a bad order", dict(order=7)), ("a pitch of 0", dict(pitch=0))):
        rc, _ = _call(par, T, "host", dict(over, out=None, palette=None, n_colors=0))
        assert rc in (0, 2), f"index_out alone with {tag}: status {rc}"
    rc, _ = _call(par, T, "host", dict(fb=True, index=None, index_out=None, palette=None, n_colors=0))
    assert rc in (0, 2), f"the fb source: status {rc}"


@pytest.mark.parametrize("call", ["device", "host"])
def test_invalid_arguments_need_no_device_and_write_nothing(par, T, call):
    for tag, over in BAD_CALLS:
        rc, untouched = _call(par, T, call, over)
        assert rc == ERR_INVALID_ARG, f"{call}: {tag}: status {rc}"
        assert untouched, f"{call}: {tag}: something was written"


def test_binding_raises_invalid_arg(par, T):
    params = T.default_params(8, 6)
    with pytest.raises(par.ParError) as e:
        par.upscale(params, T.make_upscale_desc(2, width=8), 0, (0, 6), fb=0)
    assert e.value.status == ERR_INVALID_ARG
    with pytest.raises(par.ParError) as e:
        par.upscale_host(params, T.make_upscale_desc(5, pitch=4 * 8 * 5), fb=np.zeros(48, dtype=T.COLOR))
    assert e.value.status == ERR_INVALID_ARG
    with pytest.raises(ValueError):
        par.upscale_host(params, T.make_upscale_desc(2, width=8), index=np.zeros(47, dtype=np.uint8),
                         palette=np.zeros(4, dtype=T.COLOR))
    with pytest.raises(ValueError):  # the source holds src_rows, not rows
        par.upscale_host(params, T.make_upscale_desc(2, width=8), rows=(2, 4), src_rows=(1, 5),
                         fb=np.zeros(16, dtype=T.COLOR))


# ---- the model the GPU tests compare with --------------------------------------------------------------------------

def planes(T, rng, n):
    """A frame of the three colours, an index plane of three values (200 and 255 overrun the palette) and a palette."""
    colours = U.three_colors(T, rng)
    fb = colours[rng.integers(0, 3, n)]
    index = np.array([1, 200, 255], dtype=np.uint8)[rng.integers(0, 3, n)]
    return fb, index, P.random_colors(T, rng, 6, alpha=(1, 255))


@pytest.mark.parametrize("source", ["fb", "index"])
@pytest.mark.parametrize("k", [2, 3, 4])
@pytest.mark.parametrize("w,h", [(7, 5), (5, 7)])
def test_model_equals_the_per_pixel_loop(T, w, h, k, source):
    rng = np.random.default_rng(100 * w + k)
    params = T.default_params(w, h)
    fb, index, palette = planes(T, rng, w * h)
    assert (fb["red"] != fb["blue"]).any() and len(np.unique(index)) == 3
    fired = 0
    for rows in (None, (1, 4)):
        r0, r1 = rows or (0, h)
        s0, s1 = U.with_halo((r0, r1), h, k)
        cut = slice(s0 * w, s1 * w)
        kw = dict(fb=fb[cut]) if source == "fb" else dict(index=index[cut], palette=palette)
        for order in (U.RGBA, U.BGRA):
            for gap in (0, 12):
                desc = T.make_upscale_desc(k, 4 * w * k + gap, order)
                a, ai = U.model(params, desc, (s0, s1), (r0, r1), guard=0xEE, **kw)
                b, bi = U.slow_model(params, desc, (s0, s1), (r0, r1), guard=0xEE, **kw)
                assert a.shape == ((r1 - r0) * k, 4 * w * k + gap) and a.tobytes() == b.tobytes(), (rows, order, gap)
                assert (a[:, 4 * w * k:] == 0xEE).all()
                if source == "index":
                    assert ai.shape == ((r1 - r0) * k, w * k) and ai.dtype == np.uint8 and ai.tobytes() == bi.tobytes()
                else:
                    assert ai is None and bi is None
                nearest = P.model(params, T.make_present_desc(k, k, 4 * w * k + gap, order), (r0, r1), guard=0xEE, **{
                    key: (v if key == "palette" else v[(r0 - s0) * w:(r1 - s0) * w]) for key, v in kw.items()})
                fired += int((a != nearest).sum())
    assert fired > 0, "the rules should fire on these planes"
    if source == "index":  # without a palette: the index plane alone
        desc = T.make_upscale_desc(k, 0, 0)
        a, ai = U.model(params, desc, None, None, index=index)
        b, bi = U.slow_model(params, desc, None, None, index=index)
        assert a is None and b is None and ai.tobytes() == bi.tobytes()


def elements(T, k, plane):
    """The scaled plane of elements (the index plane of the model) of a 2-D uint8 plane."""
    h, w = plane.shape
    return U.model(T.default_params(w, h), T.make_upscale_desc(k, 0, 0), None, None, index=plane.reshape(-1))[1]


@pytest.mark.parametrize("k", [2, 3, 4])
def test_properties_of_the_model(T, k):
    rng = np.random.default_rng(7 + k)
    w, h = 37, 23
    params = T.default_params(w, h)
    plane = rng.integers(0, 3, (h, w)).astype(np.uint8)
    big = elements(T, k, plane)
    nearest = np.repeat(np.repeat(plane, k, axis=0), k, axis=1)
    assert (big != nearest).mean() > 0.05, "the rules should fire"
    # every output element is one of E, B, D, F, H
    p = np.pad(plane, 1, mode="edge")
    five = [np.repeat(np.repeat(p[1 + dy:1 + dy + h, 1 + dx:1 + dx + w], k, axis=0), k, axis=1)
            for dx, dy in ((0, 0), (0, -1), (-1, 0), (1, 0), (0, 1))]
    assert np.logical_or.reduce([big == n for n in five]).all()
    # it commutes with a left-right flip, an up-down flip and a transpose
    assert np.array_equal(elements(T, k, np.ascontiguousarray(plane[:, ::-1])), big[:, ::-1])
    assert np.array_equal(elements(T, k, np.ascontiguousarray(plane[::-1])), big[::-1])
    assert np.array_equal(elements(T, k, np.ascontiguousarray(plane.T)), big.T)
    # a constant plane stays constant
    assert (elements(T, k, np.full((h, w), 9, dtype=np.uint8)) == 9).all()
    # a plane whose 4-neighbours are all distinct is present's nearest neighbour at (k, k)
    distinct = ((np.arange(w)[None, :] + 2 * np.arange(h)[:, None]) % 5).astype(np.uint8)
    q = np.pad(distinct.astype(np.int32), 1, constant_values=-1)
    four = [q[:-2, 1:-1], q[2:, 1:-1], q[1:-1, :-2], q[1:-1, 2:]]  # up, down, left, right (-1 outside the plane)
    for i in range(4):
        for j in range(i + 1, 4):
            assert ((four[i] != four[j]) | (four[i] < 0) | (four[j] < 0)).all()
    palette = P.random_colors(T, rng, 5, alpha=(1, 255))
    for order in (U.RGBA, U.BGRA):
        got = U.model(params, T.make_upscale_desc(k, 4 * w * k + 8, order), None, None, index=distinct.reshape(-1),
                      palette=palette, guard=0xEE)[0]
        exp = P.model(params, T.make_present_desc(k, k, 4 * w * k + 8, order), None, index=distinct.reshape(-1),
                      palette=palette, guard=0xEE)
        assert np.array_equal(got, exp)
    # a block with the stated halo is those rows of the whole frame's; with no halo it is not
    rows = (5, 18)
    s0, s1 = U.with_halo(rows, h, k)
    assert (s0, s1) == (5 - U.halo(k), 18 + U.halo(k))
    desc = T.make_upscale_desc(k, 0, 0)
    block = U.model(params, desc, (s0, s1), rows, index=plane[s0:s1].reshape(-1))[1]
    assert np.array_equal(block, big[k * 5:k * 18])
    bare = U.model(params, desc, rows, rows, index=plane[5:18].reshape(-1))[1]
    assert not np.array_equal(bare, big[k * 5:k * 18]), "without a halo the block's edge rows clamp"
    if k == 4:  # and one row is not enough for Scale4x
        short = U.model(params, desc, (4, 19), rows, index=plane[4:19].reshape(-1))[1]
        assert not np.array_equal(short, big[20:72]), "a halo of one row should show at Scale4x"


def test_out_of_range_indices_are_different_elements(T):
    """200 and 255 over a 4-entry palette show the same colour and are different elements for the rules."""
    plane = np.array([[1, 200, 1], [255, 1, 1], [1, 1, 1]], dtype=np.uint8)
    same = np.where(plane == 200, 255, plane).astype(np.uint8)
    for k in (2, 3, 4):
        a, b = elements(T, k, plane), elements(T, k, same)
        assert (b[k:2 * k, k:2 * k][0, 0] == 255) and (a[k:2 * k, k:2 * k] == 1).all(), k
        assert not np.array_equal(np.where(a == 200, 255, a), b), k

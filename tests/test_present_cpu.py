"""Present without a GPU: the two calls are declared, exported and bound; PRESENT_DESC has the header's layout; every
PAR_ERR_INVALID_ARG of the contract comes back from both calls before any device work and with nothing written; and the
vectorised model the GPU tests lean on (present.model) equals a per-pixel loop (present.slow_model)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import headers
import present as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID_ARG = 1

DECLARATIONS = {
    "par_present_device": "const par_params* params, void* stream, const par_present_desc* desc, const par_color* fb, "
                          "const uint8_t* index, const par_color* d_palette, int n_colors, int row_begin, int row_end, "
                          "void* out",
    "par_present_host": "const par_params* params, int device, const par_present_desc* desc, const par_color* fb, "
                        "const uint8_t* index, const par_color* palette, int n_colors, int row_begin, int row_end, "
                        "void* out",
}


def test_declared_exported_and_bound(par, T):
    headers.assert_declared(par, "par_raytracer.h", DECLARATIONS, ("present", "present_host", "make_present_desc"))
    assert (par.PRESENT_RGBA, par.PRESENT_BGRA, par.MAX_SCALE) == (0, 1, 16) == (P.RGBA, P.BGRA, T.MAX_SCALE)


def test_desc_layout_is_the_headers(T):
    types_h = open(os.path.join(ROOT, "include", "par_types.h")).read()
    m = re.search(r"typedef struct par_present_desc \{(.*?)\} par_present_desc;", types_h, flags=re.S)
    assert m, "par_present_desc is not declared"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = [f.strip() for decl in re.findall(r"int32_t\s+([^;]+);", body) for f in decl.split(",")]
    assert fields == ["scale_x", "scale_y", "pitch", "order"]
    assert re.sub(r"int32_t\s+[^;]+;", "", body).strip() == "", "a field that is not an int32_t"
    assert T.PRESENT_DESC.itemsize == 16
    assert [(n, T.PRESENT_DESC.fields[n][1], T.PRESENT_DESC.fields[n][0]) for n in T.PRESENT_DESC.names] == \
        [(n, 4 * i, np.dtype("<i4")) for i, n in enumerate(fields)]
    assert re.search(r"#define\s+PAR_MAX_SCALE\s+16\b", types_h)
    assert re.search(r"enum\s*\{\s*PAR_PRESENT_RGBA\s*=\s*0\s*,\s*PAR_PRESENT_BGRA\s*=\s*1\s*\}", types_h)
    d = T.make_present_desc(3, width=7)
    assert d.tobytes() == np.array([3, 3, 84, 0], dtype="<i4").tobytes()
    d = T.make_present_desc(2, 5, pitch=100, order=T.PRESENT_BGRA)
    assert d.tobytes() == np.array([2, 5, 100, 1], dtype="<i4").tobytes()
    with pytest.raises(ValueError):
        T.make_present_desc(2)


# ---- argument errors: no device needed, nothing written -----------------------------------------------------------

# (tag, overrides): one case per condition of the contract; each breaks that one condition alone. The good call is an
# index source of 8 x 6 at scale (2, 3) with a pitch of 80 (a gap of 16 bytes), rows (0, 6).
BAD_CALLS = [
    ("null params", dict(params=None)),
    ("null desc", dict(desc=None)),
    ("null out", dict(out=None)),
    ("both sources", dict(fb=True, n_colors=4)),
    ("neither source", dict(index=None, palette=None, n_colors=0)),
    ("index source without a palette", dict(palette=None)),
    ("index source, n_colors 0", dict(n_colors=0)),
    ("index source, n_colors 257", dict(n_colors=257)),
    ("fb source with a palette", dict(fb=True, index=None, n_colors=0)),
    ("fb source with n_colors 4", dict(fb=True, index=None, palette=None, n_colors=4)),
    ("width 0", dict(width=0, pitch=80)),
    ("width negative", dict(width=-8)),
    ("row_begin negative", dict(rows=(-1, 4))),
    ("row_begin == row_end", dict(rows=(3, 3))),
    ("row_begin > row_end", dict(rows=(5, 2))),
    ("row_end > height", dict(rows=(0, 7))),
    ("scale_x 0", dict(scale_x=0)),
    ("scale_x 17", dict(scale_x=17, pitch=4 * 8 * 17)),
    ("scale_y 0", dict(scale_y=0)),
    ("scale_y 17", dict(scale_y=17)),
    ("order 2", dict(order=2)),
    ("order -1", dict(order=-1)),
    ("pitch not a multiple of 4", dict(pitch=82)),
    ("pitch below 4 * width * sx", dict(pitch=60)),
    ("4 * width * sx beyond an int32", dict(width=1 << 27, scale_x=16, pitch=0x7FFFFFFC)),
]


def test_the_good_call_of_the_bad_calls_is_good(par, T):
    """What the cases start from passes every check of the contract, so each case breaks one condition alone; and the
    overflow case's product wraps to a small int32, which a 32-bit check would let through."""
    w, h, sx, sy, pitch, n_colors, rows = 8, 6, 2, 3, 80, 4, (0, 6)
    assert w > 0 and 0 <= rows[0] < rows[1] <= h and 1 <= sx <= 16 and 1 <= sy <= 16 and 1 <= n_colors <= 256
    assert pitch % 4 == 0 and pitch >= 4 * w * sx
    assert 4 * (1 << 27) * 16 > 0x7FFFFFFF and ((4 * (1 << 27) * 16) & 0xFFFFFFFF) == 0 and 0x7FFFFFFC % 4 == 0
    assert len({tag for tag, _ in BAD_CALLS}) == len(BAD_CALLS)
    # and the library agrees: the host form gets past its argument checks (no device here, or the surface)
    params = T.default_params(w, h)
    out = np.full(h * sy * pitch, 0xC3, dtype=np.uint8)
    rc = par.lib().par_present_host(C.byref(params), -1, T.ptr(T.make_present_desc(sx, sy, pitch, 0)), None,
                                    T.ptr(np.zeros(w * h, dtype=np.uint8)), T.ptr(np.zeros(n_colors, dtype=T.COLOR)),
                                    n_colors, rows[0], rows[1], T.ptr(out))
    assert rc in (0, 2), rc  # PAR_OK or PAR_ERR_NO_DEVICE


@pytest.mark.parametrize("call", ["device", "host"])
def test_invalid_arguments_need_no_device_and_write_nothing(par, T, call):
    L = par.lib()
    fn = L.par_present_device if call == "device" else L.par_present_host
    first = C.c_void_p(0) if call == "device" else -1  # the stream / the device

    def status(over):
        params = T.default_params(8, 6)
        params.width = over.get("width", 8)
        palette = np.full(256 * 4, 0x5A, dtype=np.uint8).view(T.COLOR)  # host dummies: never dereferenced
        fb = np.full(8 * 6 * 4, 0xA5, dtype=np.uint8).view(T.COLOR)
        index = np.full(8 * 6, 0x3C, dtype=np.uint8)
        out = np.full(6 * 3 * 80, 0xC3, dtype=np.uint8)
        desc = T.make_present_desc(over.get("scale_x", 2), over.get("scale_y", 3), over.get("pitch", 80),
                                   over.get("order", 0))
        arg = dict(params=params, desc=desc, out=out, fb=None, index=index, palette=palette, n_colors=4, rows=(0, 6))
        arg.update({k: v for k, v in over.items() if k in arg})
        if arg["fb"] is True:
            arg["fb"] = fb
        rc = fn(None if arg["params"] is None else C.byref(arg["params"]), first, T.ptr(arg["desc"]), T.ptr(arg["fb"]),
                T.ptr(arg["index"]), T.ptr(arg["palette"]), arg["n_colors"], arg["rows"][0], arg["rows"][1],
                T.ptr(arg["out"]))
        untouched = bool((fb.view(np.uint8) == 0xA5).all() and (index == 0x3C).all() and (out == 0xC3).all() and
                         (palette.view(np.uint8) == 0x5A).all())
        return rc, untouched

    for tag, over in BAD_CALLS:
        rc, untouched = status(over)
        assert rc == ERR_INVALID_ARG, f"{call}: {tag}: status {rc}"
        assert untouched, f"{call}: {tag}: something was written"


def test_binding_raises_invalid_arg(par, T):
    params = T.default_params(8, 6)
    with pytest.raises(par.ParError) as e:
        par.present(params, T.make_present_desc(2, width=8), 0, (0, 6), fb=0)
    assert e.value.status == ERR_INVALID_ARG
    with pytest.raises(par.ParError) as e:
        par.present_host(params, T.make_present_desc(17, pitch=4 * 8 * 17), fb=np.zeros(48, dtype=T.COLOR))
    assert e.value.status == ERR_INVALID_ARG
    with pytest.raises(ValueError):
        par.present_host(params, T.make_present_desc(2, width=8), index=np.zeros(47, dtype=np.uint8),
                         palette=np.zeros(4, dtype=T.COLOR))


# ---- the model the GPU tests compare with --------------------------------------------------------------------------

SCALES = (1, 2, 3, 5, 16)


@pytest.mark.parametrize("source", ["fb", "index"])
@pytest.mark.parametrize("sx", SCALES)
def test_model_equals_the_per_pixel_loop(T, source, sx):
    rng = np.random.default_rng(100 + sx)
    params = T.default_params(7, 5)
    fb = P.random_colors(T, rng, 35)
    palette = P.random_colors(T, rng, 6, alpha=(1, 255))
    index = rng.integers(0, 9, 35).astype(np.uint8)  # 6, 7, 8 are out of range
    index[:2] = (T.PALIDX_BACKGROUND, 5)
    assert (index >= 6).sum() >= 3 and (fb["red"] != fb["blue"]).any()
    kw = dict(fb=fb) if source == "fb" else dict(index=index, palette=palette)
    for sy in SCALES:
        for order in (P.RGBA, P.BGRA):
            for gap in (0, 12):
                desc = T.make_present_desc(sx, sy, 4 * 7 * sx + gap, order)
                a = P.model(params, desc, None, guard=0xEE, **kw)
                b = P.slow_model(params, desc, None, guard=0xEE, **kw)
                assert a.shape == (5 * sy, 4 * 7 * sx + gap) and a.tobytes() == b.tobytes(), (sx, sy, order, gap)
                assert (a[:, 4 * 7 * sx:] == 0xEE).all()
    # what the model must show: the exchange, the clamp, and a row block as those rows of the whole frame
    desc = T.make_present_desc(sx, 2, 4 * 7 * sx + 12, P.RGBA)
    rgba = P.model(params, desc, None, guard=0xEE, **kw)
    bgra = P.model(params, T.make_present_desc(sx, 2, 4 * 7 * sx + 12, P.BGRA), None, guard=0xEE, **kw)
    assert rgba.tobytes() != bgra.tobytes()
    assert np.array_equal(rgba[:, 0:28 * sx:4], bgra[:, 2:28 * sx:4]) and np.array_equal(rgba[:, 3::4], bgra[:, 3::4])
    block = {k: (v[7:28] if k != "palette" else v) for k, v in kw.items()}
    assert np.array_equal(P.model(params, desc, (1, 4), guard=0xEE, **block), rgba[2:8])
    assert np.array_equal(P.slow_model(params, desc, (1, 4), guard=0xEE, **block), rgba[2:8])
    if source == "index":
        last = palette[5:6].view(np.uint8)
        assert (rgba[0, 0:4] == last).all(), "an index beyond the palette takes its last entry"

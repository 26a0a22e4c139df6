"""What the five *_host forms of the passes over finished planes have in common, on an 8 x 3 frame with a 2-entry
palette: a device index past the last device is PAR_ERR_INVALID_ARG and nothing is written; device -1 is the current
device, byte for byte; and the call makes its device the current one and leaves it so (it does not restore). That last
half shows only where there are two GPUs: with one, the current device is the same before and after either way."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H = 8, 3
GUARD = 0xC3
ERR_INVALID_ARG = 1
FORMS = ("outline", "quantize", "present", "finish", "upscale")


@pytest.fixture(scope="module")
def hip(par):
    return par.hip_runtime()


def current_device(hip):
    d = C.c_int(-1)
    assert hip.hipGetDevice(C.byref(d)) == 0
    return d.value


@pytest.fixture(scope="module")
def inputs(T):
    rng = np.random.default_rng(83)
    gbuf = rng.integers(0, 4, size=W * H * T.PIXEL.itemsize, dtype=np.uint8).view(T.PIXEL)
    fb = rng.integers(0, 256, size=4 * W * H, dtype=np.uint8).view(T.COLOR)
    palette = np.array([(10, 20, 30, 255), (200, 150, 100, 255)], dtype=T.COLOR)
    index = rng.integers(0, 2, size=W * H, dtype=np.uint8)
    return dict(params=T.default_params(W, H, H), gbuf=gbuf, fb=fb, palette=palette, index=index,
                style=T.make_outline_style(), desc=T.make_present_desc(2, 2, 4 * W * 2 + 16, 1),
                up=T.make_upscale_desc(2, 4 * W * 2 + 16, 1))


def outputs(form):
    """The form's output arrays, every byte the guard."""
    f = lambda n: np.full(n, GUARD, dtype=np.uint8)
    return {"outline": dict(fb=f(4 * W * H), edge=f(W * H)),
            "quantize": dict(fb=f(4 * W * H), index=f(W * H)),
            "present": dict(out=f(2 * H * (4 * W * 2 + 16))),
            "finish": dict(out=f(2 * H * (4 * W * 2 + 16)), index=f(W * H)),
            "upscale": dict(out=f(2 * H * (4 * W * 2 + 16)), index=f(2 * H * 2 * W))}[form]


def call(L, T, form, device, i, o):
    p, ptr = C.byref(i["params"]), T.ptr
    if form == "outline":
        return L.par_outline_host(p, device, ptr(i["style"]), ptr(i["gbuf"]), 0, H, ptr(i["fb"]), 0, H, ptr(o["fb"]),
                                  ptr(o["edge"]))
    if form == "quantize":
        return L.par_quantize_host(p, device, ptr(i["palette"]), 2, 64, ptr(i["fb"]), 0, H, ptr(o["fb"]), ptr(o["index"]))
    if form == "present":
        return L.par_present_host(p, device, ptr(i["desc"]), ptr(i["fb"]), None, None, 0, 0, H, ptr(o["out"]))
    if form == "finish":
        return L.par_finish_host(p, device, ptr(i["style"]), ptr(i["gbuf"]), 0, H, ptr(i["palette"]), 2, 64, ptr(i["desc"]),
                                 ptr(i["fb"]), 0, H, ptr(o["out"]), ptr(o["index"]))
    return L.par_upscale_host(p, device, ptr(i["up"]), None, ptr(i["index"]), ptr(i["palette"]), 2, 0, H, 0, H,
                              ptr(o["out"]), ptr(o["index"]))


@pytest.mark.parametrize("form", FORMS)
def test_the_host_forms_choose_their_device_alike(par, T, hip, inputs, form):
    L = par.lib()
    count = par.device_count()
    assert count >= 1
    before = current_device(hip)
    kept = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in inputs.items()}
    # a device past the last one: refused, nothing written, the current device as it was
    o = outputs(form)
    assert call(L, T, form, count, inputs, o) == ERR_INVALID_ARG
    assert all((v == GUARD).all() for v in o.values()), "a refused call wrote something"
    assert current_device(hip) == before
    # -1 is the current device
    by_default, by_index = outputs(form), outputs(form)
    assert call(L, T, form, -1, inputs, by_default) == 0
    assert current_device(hip) == before
    assert call(L, T, form, before, inputs, by_index) == 0
    assert current_device(hip) == before
    for k in by_default:
        assert by_default[k].tobytes() == by_index[k].tobytes(), k
        assert (by_default[k] != GUARD).any(), f"{k} was not written"
    # the call makes its device current and does not restore the one before
    if count > 1:
        other = (before + 1) % count
        try:
            elsewhere = outputs(form)
            assert call(L, T, form, other, inputs, elsewhere) == 0
            assert current_device(hip) == other
            for k in by_default:
                assert elsewhere[k].tobytes() == by_default[k].tobytes(), k
        finally:
            assert hip.hipSetDevice(before) == 0
    for k, v in inputs.items():
        assert not isinstance(v, np.ndarray) or v.tobytes() == kept[k].tobytes(), f"input {k} was written"

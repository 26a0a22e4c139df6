"""The one loader of the package (_load) on all five paths, without a GPU: the core library's lib() and the four add-on
modules' lib() refuse a missing library with the same words, and a loaded add-on library carries its module's table."""
import ctypes as C
import importlib

import pytest

ADDONS = {"tileset_reduce": "ABI_TILESET_REDUCE", "cells_fit": "ABI_CELLS_FIT", "vram": "ABI_VRAM", "screen": "ABI_SCREEN"}


def module_of(name):
    return importlib.import_module("pixel-art-raytracer_amd" + ("." + name if name else ""))


@pytest.mark.parametrize("name", ["", *ADDONS])
def test_a_missing_library_is_an_import_error_in_the_cores_words(par, monkeypatch, tmp_path, name):
    module = module_of(name)
    missing = str(tmp_path / "lib" / ("lib" + (name or "raytracer") + ".so"))
    monkeypatch.setattr(module, "LIB_PATH", missing)
    monkeypatch.setattr(module, "_lib", None)
    with pytest.raises(ImportError) as e:
        module.lib()
    assert str(e.value) == (f"{missing} is missing: build it with `make -C pixel-art-raytracer_amd/csrc` "
                            "(or __graft_entry__.build()). There is no CPU fallback.")
    assert module._lib is None


@pytest.mark.parametrize("name", list(ADDONS))
def test_a_loaded_add_on_carries_its_table_and_no_other(par, name):
    module = module_of(name)
    table = getattr(module, ADDONS[name])
    L = module.lib()
    assert L is module.lib() and L is not par.lib()
    assert table and tuple(table) == getattr(module, ADDONS[name] + "_SYMBOLS")
    for symbol, sig in table.items():
        restype, argtypes = sig if type(sig) is tuple else (C.c_int, sig)
        fn = getattr(L, symbol)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), symbol
    for other in ADDONS:
        if other != name:
            assert not any(hasattr(L, symbol) for symbol in getattr(module_of(other), ADDONS[other])), other

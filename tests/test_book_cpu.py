"""The host's scene bookkeeping (csrc/par_book.cpp) without a GPU: tests/book_check.cpp drives it through seeded random
sequences of par_set_entities, blocking and asynchronous updates, graph captures, stages and launches, over several
views and bin sizes, and checks it after every step against a book built from scratch (par_book.h has the contract)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pixel-art-raytracer_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_book_follows_its_contract(tmp_path):
    exe = tmp_path / "book_check"
    # the library's flags (csrc/Makefile), host code only
    cmd = [HIPCC, "--offload-arch=gfx950", "-std=c++17", "-O3", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wextra",
           "-Wno-unused-parameter", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
           os.path.join(ROOT, "tests", "book_check.cpp"), os.path.join(CSRC, "par_book.cpp"), "-o", str(exe)]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    assert "warning" not in p.stderr, p.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-2000:]
    assert out.stdout.strip().endswith(" checks, 0 failures"), out.stdout[-2000:]

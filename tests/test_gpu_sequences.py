"""One context, many calls: seeded random sequences of everything the C ABI offers on one Renderer per test (scene
regimes that flip every launch chooser, sprite tables, blocking and asynchronous updates, 1..8 lights, both light models,
tints, host and device frames of any rows and planes, relit frames, both kinds of captured graphs out of step with plain
renders, pick, the hash read back, the statistics), and one hand-written sequence per hazard of a long-lived context.
tests/sequences.py has the driver: after every step the frame is compared byte for byte with the pinned oracle's,
composed from scratch; every refusal must be the one the header promises; stats() must not report PAR_ERR_DEVICE.
tests/test_sequences_cpu.py says what the sequences contain. No test hooks: these frames take the paths production
picks.

Wall time per test on an MI355X, oracle included (each test prints its own, pytest -s): a generated sequence of 48 steps
0.03 to 0.54 s (480-wide view 0.11..0.19 s, 256-wide 0.06..0.17 s, 333-wide 0.03..0.08 s, 640-wide 0.12..0.54 s); a
hand-written one 0.02 to 0.13 s; the first test of a session another 12 s, which torch and HIP take to start. The module,
64 tests, runs in 20 s."""
import time

import pytest

import sequences as S

pytestmark = pytest.mark.gpu

HAND_WRITTEN = S.hand_written()


@pytest.fixture(scope="module")
def scenes(oracle):
    return {view: S.Scenes(oracle) for view in S.VIEWS}


def drive(par, scenes, view, ops, tag):
    t0 = time.perf_counter()
    with par.Renderer(S.T.default_params(*S.VIEWS[view])) as r:
        try:
            S.run(r, ops, S.Mirror(par, view, scenes[view]), S.TorchMem(), tag)
        except S.HipFailure as e:  # nothing more is started on a device whose state is not known
            pytest.exit(f"a HIP call failed inside the library: {e}", returncode=3)
    print(f"{tag}: {len(ops)} steps in {time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize("view,seed", S.cases(), ids=[f"{v}-seed{s}" for v, s in S.cases()])
def test_generated_sequence(par, scenes, view, seed):
    ops, _ = S.generate(par, view, seed)
    drive(par, scenes, view, ops, f"{view} seed {seed}")


@pytest.mark.parametrize("name", list(HAND_WRITTEN))
def test_hand_written_sequence(par, scenes, name):
    view, ops = HAND_WRITTEN[name]
    drive(par, scenes, view, ops, name)

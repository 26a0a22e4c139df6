"""What keeps tests/test_gpu_sequences.py from passing vacuously, without a GPU: over the exact (view, seed) list of that
module, what the generated sequences contain (op kinds, refusals, regimes and their sizes from the oracle's hash, graph
and relight states), that the generator gives the same ops everywhere, and that the driver bites: every sequence passes
on sequences.OracleBackend, and with each of its four leaks at least one sequence per view fails.

As measured (12 seeds x 4 views x 48 steps = 2 304 steps; every test prints its counts, pytest -s):
- 1 442 compared frames (63 %), 156 predicted refusals (7 %): 78 NOT_READY, 67 INVALID_ARG, 11 UNSUPPORTED; every op kind
  in every view (the rarest: stats once in the 256-wide view, graph_capture 3 times in the 333-wide one);
- every regime of every view entered 2 to 8 times by a context that has rendered in both grid sets; the twelve ordered
  pairs of sparse, many, dense, overflow as consecutive frames 1 (dense -> sparse) to 9 (many -> sparse) times;
- regime sizes, occupied columns / (entity, bin) pairs: 640x320x160 bin 8: sparse 3..10 / 5..16, many 1 325..1 406 /
  4 413..4 811, dense 2 849..2 956 / 27 771..28 003, overflow 1 503..1 589 / 11 336..11 748 (89 records in a column);
  256x192x192 bin 8: sparse 4..8 / 4..13, many 588..643 / 6 528..8 751, dense 768 / 7 940..8 154, overflow 602..646 /
  7 192..9 111 (117 records), big 696..704 / 71 555..77 411 (1 503..1 596 entities); 480x320x320 bin 40 and 333x170x150
  bin 16 have 96 and 231 columns in all and at most 786 and 2 675 pairs;
- graph launches in grid set 0 / 1: 40 / 35, 16 / 12, 26 / 25, 37 / 41 per view; launches that follow a plain render after
  an earlier launch of the same capture: 11, 5, 14, 12; relight calls with / without a retained frame: 45 / 3, 53 / 3,
  44 / 1, 49 / 3;
- sequences (of 12 per view) that fail with a leak: partial update 7..9, relight 4..6, the previous traced frame's
  background bits 10..11, row block 11..12.

Some of these counts are one event deep (stats as an op once in the 256-wide view, dense -> sparse once, relight without a
retained frame once in the 333-wide view). They hold because the generator is pinned: test_same_ops_everywhere fails on
any change of its output, and the assertions here then say which kind, regime or transition went missing."""
import collections

import numpy as np
import pytest

import sequences as S

ORDERED = ("sparse", "many", "dense", "overflow")


@pytest.fixture(scope="module")
def generated(par):
    return {(view, seed): S.generate(par, view, seed) for view, seed in S.cases()}


@pytest.fixture(scope="module")
def scenes(oracle):
    return {view: S.Scenes(oracle) for view in S.VIEWS}


def test_same_ops_everywhere(par, generated):
    again = {c: S.digest(S.generate(par, *c)[0]) for c in S.cases()}
    assert again == {c: S.digest(ops) for c, (ops, _) in generated.items()}
    assert all(len(ops) == S.STEPS for ops, _ in generated.values())
    whole = S.digest([S.op("case", view=c[0], seed=c[1], ops=again[c]) for c in S.cases()])
    print(f"digest of all {len(again)} sequences: {whole}")
    assert whole == PINNED_DIGEST, "the generator's output changed: the counts in the docstrings were measured on another"


def test_op_coverage(generated):
    steps = frames = refused = 0
    statuses = collections.Counter()
    for view in S.VIEWS:
        kinds = collections.Counter()
        v_steps = v_frames = v_refused = 0
        for (v, _), (_, trace) in generated.items():
            if v != view:
                continue
            for t in trace:
                kinds[t["kind"]] += 1
                v_steps += 1
                v_frames += t["frame"]
                v_refused += t["status"] != S.OK
                statuses[S.STATUS[t["status"]]] += 1
        print(f"{view}: {v_steps} steps, {v_frames} compared frames, {v_refused} predicted refusals; "
              f"{', '.join(f'{k} {kinds[k]}' for k in S.KINDS)}")
        missing = [k for k in S.KINDS if not kinds[k]]
        assert not missing, f"{view}: no sequence issues {missing}"
        steps, frames, refused = steps + v_steps, frames + v_frames, refused + v_refused
    print(f"in all {steps} steps: {frames} compared frames ({frames / steps:.0%}), {refused} predicted refusals "
          f"({refused / steps:.0%}): {dict(statuses)}")
    assert frames >= 0.6 * steps
    assert refused <= 0.15 * steps
    for name in ("NOT_READY", "UNSUPPORTED", "INVALID_ARG"):
        assert statuses[name] > 0, f"{name} is never predicted"


def test_regime_coverage(generated):
    pairs_seen = collections.Counter()
    for view in S.VIEWS:
        entered = collections.Counter()  # regime -> times entered with frames rendered in both grid sets before
        for (v, seed), (_, trace) in generated.items():
            if v != view:
                continue
            built = [t["regime"] for t in trace if t["builds"]]  # the regime of every frame that built a hash
            for a, b in zip(built, built[1:]):
                if a != b:
                    pairs_seen[(a, b)] += 1
            for i, t in enumerate(trace):
                if t["kind"] == "set_entities" and t["sets_used"] == 2:
                    # (entered: a frame is rendered in it before the next scene)
                    later = [u for u in trace[i + 1:] if u["builds"] or u["kind"] == "set_entities"]
                    if later and later[0]["builds"]:
                        entered[later[0]["regime"]] += 1
        print(f"{view}: regimes entered after frames in both grid sets: {dict(entered)}")
        missing = [r for r in S.REGIMES[view] if not entered[r]]
        assert not missing, f"{view}: {missing} never entered in a context that has rendered in both grid sets"
    wanted = [(a, b) for a in ORDERED for b in ORDERED if a != b]
    print("consecutive frames, regime a -> regime b: " + ", ".join(f"{a}->{b} {pairs_seen[(a, b)]}" for a, b in wanted))
    missing = [p for p in wanted if not pairs_seen[p]]
    assert not missing, f"no consecutive frames go {missing}"


def test_regime_sizes(par, oracle, generated):
    """From the oracle's hash and alt:202-240 restated (sequences.footprints), for every scene a sequence sets."""
    seen = collections.defaultdict(list)
    for (view, seed), (ops, _) in generated.items():
        for o in ops:
            if o["kind"] == "set_entities":
                seen[(view, o["regime"])].append(o["aabbs"])
    for view, ops in S.hand_written().values():
        for o in ops:
            if o["kind"] == "set_entities":
                seen[(view, o["regime"])].append(o["aabbs"])
    for (view, regime), scenes_ in sorted(seen.items()):
        W, H, L, B = S.VIEWS[view]
        params = S.T.default_params(W, H, L, B)
        gx, gy, _ = params.grid_dims()
        rows = []
        for aabbs in scenes_:
            pairs, host_cols, extent = S.bounds(params, aabbs)
            over, tileable, dense = S.column_histograms(params, aabbs)
            grid = oracle.bin(params, aabbs)
            per_row, entries, bins = S.grid_sizes(params, grid)
            occupied = int(per_row.sum())
            bound = min(host_cols, gx * gy)  # what the launch choosers compare (columns_in_rows of a whole frame)
            rows.append((len(aabbs), occupied, bound, pairs, extent, over, dense, entries, bins))
            tag = f"{view} {regime}: {rows[-1]}"
            assert extent >= pairs and host_cols >= occupied, tag
            for threshold in (256, 1024, 2048):  # the host's bound is never on the lower side of the scene
                assert occupied < threshold or bound >= threshold, tag
            assert (pairs > S.POOL) == (regime == "big"), tag
            if regime in ("empty", "culled"):
                assert occupied == 0 and pairs == 0 and (regime == "empty") == (len(aabbs) == 0), tag
            if regime == "sparse":
                assert 0 < occupied <= bound <= 256 and not dense and over == 0, tag
            if regime == "many":
                assert occupied > (256 if B == 8 else gx * gy // 2), tag
                if gx * gy > 2048:
                    assert 1024 <= occupied <= bound < 2048, tag
            if regime == "dense":
                assert dense, tag
                if gx * gy > 2048:
                    assert occupied >= 2048, tag
            if regime == "overflow":
                # a column with more pairs than a record surely holds: the frame has a launch for the overflow list; and,
                # where the grid is deep enough for it (a bin shows 7 records at most: alt:262-264), a column that
                # overflows its record
                assert over > 0, tag
                if B == 8:
                    assert entries > S.COL_ENT or bins > S.COL_NB, tag
        cols = list(zip(*rows))
        print(f"{view} {regime}: {len(rows)} scenes; entities {min(cols[0])}..{max(cols[0])}, occupied columns "
              f"{min(cols[1])}..{max(cols[1])}, host column bound {min(cols[2])}..{max(cols[2])}, pairs {min(cols[3])}.."
              f"{max(cols[3])}, pairs by extents {min(cols[4])}..{max(cols[4])}, most records in a column {max(cols[7])}")
    for view in S.VIEWS:
        for regime in S.REGIMES[view]:
            assert (view, regime) in seen


def test_graph_and_relight_coverage(generated):
    for view in S.VIEWS:
        parities, between, relit = collections.Counter(), 0, collections.Counter()
        for (v, seed), (_, trace) in generated.items():
            if v != view:
                continue
            since = {}  # capture -> kinds of the frames since its first launch
            for t in trace:
                if t["kind"] in ("relight", "relight_device"):
                    relit["with a retained frame" if t["kept"] else "without"] += 1
                if t["status"] != S.OK or not t["builds"]:
                    continue
                g = t["graph"]
                if t["kind"] == "graph_launch":
                    for n in range(t["count"]):
                        parities[(t["set"] + n) % 2] += 1
                    if "plain" in since.get(g, ()):
                        between += 1
                        since[g] = []
                    since.setdefault(g, []).append("launch")
                elif g in since:
                    since[g].append("plain")
        print(f"{view}: graph launches in grid set 0 / 1: {parities[0]} / {parities[1]}; launches that follow a plain render "
              f"after an earlier launch of the same capture: {between}; relight calls {dict(relit)}")
        assert parities[0] and parities[1] and between
        assert relit["with a retained frame"] and relit["without"]


@pytest.mark.parametrize("view", list(S.VIEWS))
def test_the_driver_passes_on_the_oracle_and_notices_every_leak(par, scenes, generated, view):
    caught = collections.Counter()
    for (v, seed), (ops, _) in generated.items():
        if v != view:
            continue
        tag = f"{view} seed {seed}"
        S.run(S.OracleBackend(par, view, scenes[view]), ops, S.Mirror(par, view, scenes[view]), S.HostMem(), tag)
        for leak in S.LEAKS:
            try:
                S.run(S.OracleBackend(par, view, scenes[view], leak), ops, S.Mirror(par, view, scenes[view]), S.HostMem(), tag)
            except AssertionError:
                caught[leak] += 1
    print(f"{view}: sequences (of {len(S.SEEDS)}) that fail with a leak: {dict(caught)}")
    for leak in S.LEAKS:
        assert caught[leak], f"{view}: no sequence notices the leak '{leak}'"


def test_hand_written_sequences_pass_on_the_oracle(par, scenes):
    for name, (view, ops) in S.hand_written().items():
        S.run(S.OracleBackend(par, view, scenes[view]), ops, S.Mirror(par, view, scenes[view]), S.HostMem(), name)


PINNED_DIGEST = "69e0dd692002ddfc"

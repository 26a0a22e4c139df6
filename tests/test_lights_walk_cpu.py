"""The host-side restatement of the shadow walk's bin sequence (helpers.walk_probes), pinned to the oracle: the GPU
tests of the light kernel's capacity limits compute from it how many occluder records a (start bin, light) pair
stages, so it has to be the sequence par_oracle_shadow probes."""
import numpy as np

from helpers import light_bin, shadow_walk_cases, walk_probes, walk_record_bounds


def shadow_from_probes(oracle, grid, T, start, end, start_entity, ray):
    """par_oracle_shadow's answer from walk_probes and oracle.intersect: the entries of the probed bins in slot
    order; the start bin, out-of-range indices and the start entity are skipped."""
    b0 = (start[0] * grid.gy + start[1]) * grid.gz + start[2]
    for b in walk_probes(start, end, grid.gy, grid.gz):
        if b == b0 or b < 0 or b >= grid.volume:
            continue
        for j in range(int(grid.count[b])):
            s = b * T.SLOTS + j
            if int(grid.map[s]) == start_entity:
                continue
            if oracle.intersect(grid.bins[s:s + 1], ray):
                return 0
    return 1


def test_walk_probes_give_the_oracle_shadow_answer(oracle, T):
    aabbs, walks = shadow_walk_cases()
    grid = oracle.bin(T.default_params(), aabbs)
    lit = shadowed = 0
    for i, (s, e, ent, ray) in enumerate(walks):
        exp = oracle.shadow(grid, s, e, ent, ray)
        assert shadow_from_probes(oracle, grid, T, s, e, ent, ray) == exp, (i, s, e)
        lit += exp
        shadowed += 1 - exp
    assert (lit, shadowed) == (2739, 261)  # both answers are pinned


def test_walk_probes_shape_and_record_bounds(oracle, T):
    params = T.default_params()
    gx, gy, gz = params.grid_dims()
    assert walk_probes((3, 2, 1), (3, 2, 1), gy, gz) == []
    # a walk along x: seven probes per iteration, the seventh of each is the next bin of the row
    p = walk_probes((0, 2, 2), (11, 2, 2), gy, gz)
    assert len(p) == 7 * 11
    assert p[6::7] == [(x * gy + 2) * gz + 2 for x in range(1, 12)]
    # a light bin outside the grid: the walk goes on to it, through out-of-range flat indices
    p = walk_probes((11, 7, 7), (14, 9, 7), gy, gz)
    assert len(p) == 21 and max(p) >= gx * gy * gz
    # seven boxes in each bin of that row: walking the row stages each bin at least once
    aabbs = T.make_aabbs([(40 * bx + 2 * k, 100, 100, 20, 20, 20) for bx in range(12) for k in range(7)])
    grid = oracle.bin(params, aabbs)
    row = [(bx * gy + 2) * gz + 2 for bx in range(12)]
    assert all(int(grid.count[b]) == 7 for b in row)
    lo, hi = walk_record_bounds(grid.count, (0, 2, 2), (11, 2, 2), gy, gz)
    assert lo == int(sum(int(grid.count[b]) for b in row[1:])) and hi >= lo
    lo2, hi2 = walk_record_bounds(grid.count, (5, 2, 2), (6, 2, 2), gy, gz)
    assert (lo2, hi2) == (7, 7 * 4)  # bin (6,2,2) is probed by four of the seven masks


def test_light_bin_truncates_towards_zero(T):
    params = T.default_params()  # 480x320x320, bin 40
    assert light_bin(params, (250, 150, 90)) == (6, 2, 2)
    assert light_bin(params, (-50, 120, -30)) == (-1, 5, 0)   # -50 / 40 == -1, -30 / 40 == 0 in C
    assert light_bin(params, (-39, 400, 39)) == (0, -2, 0)    # (320 - 439) / 40 == -2
    assert light_bin(params, (481, 160, 80)) == (12, 2, 2)
    assert isinstance(light_bin(params, np.array([1, 2, 3], dtype=np.int16))[0], int)

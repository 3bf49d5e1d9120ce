"""tools/debug/poll_looks_by_cu.py, the arithmetic alone: records of workgroups are paired by launch and place, the pair is
ordered by blockIdx.x, and the summary says how the first-look shares of the older and the younger workgroup compare."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location('poll_looks_by_cu', os.path.join(ROOT, 'tools', 'debug', 'poll_looks_by_cu.py'))
T = importlib.util.module_from_spec(spec)
spec.loader.exec_module(T)


def hw_id(se, sh, cu, wave=3):
    return (se << 13) | (sh << 12) | (cu << 8) | wave


def test_place_decodes_the_hardware_id():
    assert T.place(hw_id(5, 1, 9), 7) == (7, 5, 1, 9)
    assert T.place(hw_id(0, 0, 15, wave=15) | (3 << 30), 0) == (0, 0, 0, 15)


def test_pairs_are_ordered_by_block_and_split_by_launch():
    recs = []
    for launch in (200, 456):
        for cu in range(4):
            # the younger workgroup (block 100 + cu) is listed FIRST: the order of the records must not matter
            recs.append([launch, 100 + cu, hw_id(1, 0, cu), 2, 90, 5, 5, 115])
            recs.append([launch, cu, hw_id(1, 0, cu), 2, 30, 10, 60, 400])
    recs.append([200, 300, hw_id(2, 0, 0), 2, 50, 0, 0, 50])      # alone on its CU: not a pair
    pairs, s = T.summarise(recs)
    assert len(pairs) == 8 and s['cu_pairs'] == 8 and s['cus_not_paired'] == 1 and s['workgroup_records'] == 17
    for p in pairs:
        assert p['older']['block'] < 100 <= p['younger']['block']
        assert p['older']['first_look_share'] == 0.3 and p['younger']['first_look_share'] == 0.9
        assert p['older']['looks_per_poll'] == 4.0 and p['younger']['looks_per_poll'] == 1.15
    assert s['spread_within_group'] == 0. and s['share_of_cus_younger_above_older_by_more_than_spread'] == 1.
    assert s['share_of_cus_older_above_younger_by_more_than_spread'] == 0.
    assert s['share_3_or_more'] == round(65 / 200, 4) and s['share_of_the_3_or_more_on_older'] == round(60 / 65, 4)
    # per CU, the two launches summed
    rows = T.by_cu(pairs)
    assert rows == [[2, 1, 0, cu, 2, 0.3, 4.0, 0.9, 1.15] for cu in range(4)]


def test_symmetric_pairs_do_not_differ():
    recs = []
    for cu in range(6):
        a, b = 60 + cu, 65 - cu
        recs.append([7, cu, hw_id(0, 0, cu), 0, a, 0, 100 - a, 100 + 3 * (100 - a)])
        recs.append([7, 50 + cu, hw_id(0, 0, cu), 0, b, 0, 100 - b, 100 + 3 * (100 - b)])
    _, s = T.summarise(recs)
    # (as many CUs one way as the other, and only the outermost of them by more than the spread)
    assert s['share_of_cus_younger_above_older_by_more_than_spread'] == s['share_of_cus_older_above_younger_by_more_than_spread']
    assert s['share_of_cus_younger_above_older_by_more_than_spread'] < 0.2
    assert abs(s['mean_younger_minus_older']) < 1e-9
    assert s['first_look_share_older'] == s['first_look_share_younger']

"""The host rule of the per-position entries k_owner_window writes next to its owner tables (debug key pos_entries_ring), in plain
NumPy: position k of a step's occurrence list X | Y | samples holds (last + 1, R - first, count, 0) of its item over the item's table
-- the value the forward kernels would have published to occ_fl[table][item] -- and zeros where the position holds no item.  One
table over the whole list with the constrained embedding; with a separate embedding positions [0, B) are the E table and [B, R) the
Wy table, so the same id in both is two items.  tests/test_gpu_pos_entries.py checks every slot of the device's ring against it; the
self-check below runs without a GPU on a hand-made list whose expected entries are written out."""
import numpy as np


def expected_entries(occ, B, constrained):
    """[Rp][4] ints (Rp = R rounded up to a multiple of 4; the padding holds zeros) for one step's occurrence list."""
    occ = np.asarray(occ).tolist()
    R = len(occ)
    groups = {}
    for k, item in enumerate(occ):
        if item < 0:
            continue
        table = 0 if (constrained or k >= B) else 1
        groups.setdefault((table, item), []).append(k)
    out = np.zeros(((R + 3) // 4 * 4, 4), dtype=np.int32)
    for pos in groups.values():
        out[pos] = (pos[-1] + 1, R - pos[0], len(pos), 0)
    return out


def check_entries(ring_slot, occ, B, constrained):
    """ring_slot: [Rp][4] ints of one step.  Returns the number of positions whose item occurs only among the sampled negatives, more
    than once (the items the owner tables never look at)."""
    want = expected_entries(occ, B, constrained)
    np.testing.assert_array_equal(np.asarray(ring_slot).reshape(want.shape), want)
    R = len(occ)
    return int(((want[:, 2] > 1) & (R - want[:, 1] >= 2 * B)).sum())


def test_entry_rule_on_a_hand_made_list():
    B = 4
    #        X            Y            samples
    occ = [7, 3, 7, -1, 5, 5, 9, -1] + [3, 11, 11, 9] + [8] * 6
    R = len(occ)
    assert R == 18
    one = expected_entries(occ, B, True)
    assert one.shape == (20, 4)
    # one table: 7 at 0, 2; 3 at 1, 8; 5 at 4, 5; 9 at 6, 11; 11 at 9, 10; 8 at 12 .. 17
    assert one[0].tolist() == [3, R - 0, 2, 0] and one[2].tolist() == one[0].tolist()
    assert one[1].tolist() == [9, R - 1, 2, 0] and one[8].tolist() == one[1].tolist()
    assert one[4].tolist() == [6, R - 4, 2, 0]
    assert one[6].tolist() == [12, R - 6, 2, 0] and one[11].tolist() == one[6].tolist()
    assert one[9].tolist() == [11, R - 9, 2, 0]
    assert one[17].tolist() == [18, R - 12, 6, 0] and one[12].tolist() == one[17].tolist()
    # -1 positions and the padding behind R hold zeros
    assert not one[3].any() and not one[7].any() and not one[18:].any()
    # two tables: the 3 of X (position 1) and the 3 among the samples (position 8) are two items, one occurrence each
    two = expected_entries(occ, B, False)
    assert two[1].tolist() == [2, R - 1, 1, 0] and two[8].tolist() == [9, R - 8, 1, 0]
    assert two[0].tolist() == one[0].tolist() and two[17].tolist() == one[17].tolist()
    # the same id in X and in Y with counts of their own
    occ2 = list(occ)
    occ2[1] = 5
    two = expected_entries(occ2, B, False)
    assert two[1].tolist() == [2, R - 1, 1, 0] and two[4].tolist() == [6, R - 4, 2, 0]
    one = expected_entries(occ2, B, True)
    assert one[1].tolist() == [6, R - 1, 3, 0] and one[5].tolist() == one[1].tolist()
    # items all of whose occurrences are sampled negatives, repeated: 11 (twice) and 8 (six times)
    assert check_entries(expected_entries(occ, B, True), occ, B, True) == 8
    bad = expected_entries(occ, B, True)
    bad[17, 2] -= 1
    try:
        check_entries(bad, occ, B, True)
    except AssertionError:
        pass
    else:
        raise AssertionError('a wrong count passed')
    # a step with M = 0 touches nothing
    assert not expected_entries([-1] * R, B, True).any()

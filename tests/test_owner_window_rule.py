"""The host rule of the lean update's owner tables (k_owner_window / owner_prescan write them, k_update_l reads them), in plain NumPy:
the occurrence list X | Y | samples of a step from the plan and the sample store, the owners of repeated items and the rows the
table has to hold for them.  tests/test_gpu_owner_window.py checks every slot of the device's owner ring against it; the self-check
below runs without a GPU on a hand-made list whose expected rows are written out."""
import numpy as np

INLINE = 15      # G4R_OWN_INLINE: earlier occurrences an owner-table row holds; more: the row says -1 and the owner scans in k_update_l


def occurrences(plan, ST, t, row, B, ns):
    """Occurrence ids of plan step t: in_idx | out_idx (rows >= M: -1) | row `row` of the sample store (a step with M = 0: -1)."""
    M = int(plan['M'][t])
    occ = np.full(2 * B + ns, -1, dtype=np.int64)
    occ[:M] = plan['in_idx'][t, :M]
    occ[B:B + M] = plan['out_idx'][t, :M]
    if ns and M > 0:
        occ[2 * B:] = ST[row]
    return occ


def owners(occ, B, constrained):
    """Host rule of k_update_l's owners that need a list: {owner position: ascending earlier positions}."""
    groups = {}
    for k, item in enumerate(np.asarray(occ).tolist()):
        if item < 0:
            continue
        table = 0 if (constrained or k >= B) else 1
        groups.setdefault((table, item), []).append(k)
    out = {}
    for pos in groups.values():
        if len(pos) > 1 and pos[0] < 2 * B:      # (all occurrences among the sampled negatives: the shortcut, no list)
            out[pos[-1]] = pos[:-1]
    return out


def expected_rows(occ, B, constrained):
    """{owner position: (entry 0 of its row, the positions behind it)}: the count and the list, or -1 and nothing for a hot item."""
    rows = {}
    for k, want in owners(occ, B, constrained).items():
        rows[k] = (-1, []) if len(want) > INLINE else (len(want), want)
    return rows


def check_table(pos, occ, B, constrained):
    """pos: [R][16] ints of one step's owner table.  Returns the number of owners that read a list from it."""
    rows = expected_rows(occ, B, constrained)
    lists = 0
    for k, (n, want) in rows.items():
        assert pos[k, 0] == n, (k, int(pos[k, 0]), n)
        if n > 0:
            np.testing.assert_array_equal(pos[k, 1:1 + n], np.array(want, dtype=np.int32), err_msg='owner %d' % k)
            lists += 1
    return lists


def test_owner_rule_on_a_hand_made_list():
    B, ns = 4, 20
    #        X            Y            samples
    occ = [7, 3, 7, -1, 5, 5, 9, -1] + [3, 11, 11, 9] + [8] * 16
    plan = dict(M=np.array([3]), in_idx=np.array([[7, 3, 7, 99]]), out_idx=np.array([[5, 5, 9, 99]]))
    ST = np.array([occ[8:]])
    np.testing.assert_array_equal(occurrences(plan, ST, 0, 0, B, ns), occ)
    # one table (constrained embedding): 7 at 0, 2 -> owner 2; 3 at 1, 8 -> owner 8; 5 at 4, 5 -> owner 5; 9 at 6, 11 -> owner 11;
    # 11 at 9, 10 and 8 at 12 .. 27: sampled negatives only, no row
    assert owners(occ, B, True) == {2: [0], 8: [1], 5: [4], 11: [6]}
    # two tables: X is its own (7 at 0, 2); 3 is single in either table
    assert owners(occ, B, False) == {2: [0], 5: [4], 11: [6]}
    assert expected_rows(occ, B, True) == {2: (1, [0]), 8: (1, [1]), 5: (1, [4]), 11: (1, [6])}
    # a hot item: 8 also in Y -> its 17 occurrences make 16 earlier ones, one more than a row holds
    hot = list(occ)
    hot[7 - 1] = 8
    rows = expected_rows(hot, B, True)
    assert rows[27] == (-1, []) and 11 not in rows
    # ... and with 15 earlier ones the row holds them all
    hot[27] = 12
    rows = expected_rows(hot, B, True)
    assert rows[26] == (15, [6] + list(range(12, 26)))
    pos = np.zeros((len(occ), 16), dtype=np.int32)
    for k, (n, want) in rows.items():
        pos[k, 0] = n
        pos[k, 1:1 + len(want)] = want
    assert check_table(pos, hot, B, True) == len(rows)
    pos[26, 3] += 1
    try:
        check_table(pos, hot, B, True)
    except AssertionError:
        pass
    else:
        raise AssertionError('a wrong position passed')
    # a step with M = 0 touches nothing
    plan0 = dict(M=np.array([0]), in_idx=plan['in_idx'], out_idx=plan['out_idx'])
    assert (occurrences(plan0, ST, 0, 0, B, ns) == -1).all()

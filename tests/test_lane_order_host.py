"""CPU: the specification of the lane order (tests/lane_order_reference.py) holds together -- its models pass its own checkers at
every shape of tests/test_lane_order_gpu.py, each kind of wrong order is rejected with a message that names the rule broken, and
the alignment of the XCDs' lists with the eighths of xcd_unit_of is what DESIGN 4.9 says it is."""
import os
import re

import numpy as np
import pytest

import lane_order_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ models against checkers
@pytest.mark.parametrize("S,weave", R.WINDOWED_CASES)
def test_windowed_model_passes_its_checker_with_random_ties(S, weave):
    for pattern in R.WINDOWED_PATTERNS:
        keys = R.keys_of(*R.step_counts(pattern, S))
        for seed in (None, 3):
            rng = None if seed is None else np.random.default_rng(seed)
            order = R.model_windowed(keys, weave, rng)
            ranks = R.check_windowed(order, keys, weave)
            assert sorted(ranks.tolist()) == list(range(R.Layout(S, weave).nwin)), pattern
            if seed is None:                   # the decoded ranks and index order among equal keys give the same order back
                assert np.array_equal(R.build_windowed(keys, weave, ranks), order), pattern


@pytest.mark.parametrize("S", R.GLOBAL_SIZES)
def test_global_model_passes_its_checker_with_random_ties(S):
    for pattern in R.GLOBAL_PATTERNS:
        keys = R.keys_of(*R.step_counts(pattern, S))
        R.check_global(R.model_global(keys), keys)
        R.check_global(R.model_global(keys, np.random.default_rng(4)), keys)


def test_patterns_are_what_their_names_say():
    """The properties the GPU file relies on: which patterns determine the order completely, where the ties are."""
    for S, weave in R.WINDOWED_CASES:
        L = R.Layout(S, weave)
        keys = R.keys_of(*R.step_counts("window-distinct", S))
        assert R.keys_distinct_in_windows(keys), S
        assert R.window_keys_distinct(keys) == (L.nfull <= R.BINS + 1 - min(L.W, S)), S      # 1 024 bins: no more distinct window keys fit
        keys = R.keys_of(*R.step_counts("window-keys-equal", S))
        assert all(keys[lo:lo + L.W].max() == 500 for lo in range(0, S, L.W))
        keys = R.keys_of(*R.step_counts("heavy-in-short", S))
        assert np.argmax(keys) >= (L.nwin - 1) * L.W and np.sum(keys == keys.max()) == 1
        keys = R.keys_of(*R.step_counts("heavy-at-window-end", S))
        assert all(np.argmax(keys[lo:lo + L.W]) == min(L.W, S - lo) - 1 for lo in range(0, S, L.W))
    acc, rej = R.step_counts("clamped", 1025)
    assert set((acc.astype(np.int64) + rej).tolist()) == {1022, 1023, 1024, 5000} and set(R.keys_of(acc, rej).tolist()) == {1022, 1023}
    acc, rej = R.step_counts("zeros-negative", 1025)
    assert (acc.astype(np.int64) + rej).min() < 0 and R.keys_of(acc, rej).min() == 0
    for S in (255, 1023):
        assert np.unique(R.keys_of(*R.step_counts("distinct", S))).size == S
    assert [R.window_size(S) for S in (1, 128, 129, 900, 8191, 8193, 20480, 33000, 140000, 262144)] == [16, 16, 32, 128, 1024, 528, 864, 832, 976, 1024]


def test_layout_at_the_shapes_the_gpu_file_names():
    L = R.Layout(900)
    assert (L.W, L.nwin, L.n_short) == (128, 8, 4)
    L = R.Layout(33000)
    assert (L.W, L.nwin, L.n_short, L.xs, L.lens, L.nf[7], L.weave) == (832, 40, 552, 7, [5] * 8, 4, 5)
    L = R.Layout(140000)
    assert (L.nwin, L.lens, L.weave, [mg for _, _, mg in L.groups(0)], [mg for _, _, mg in L.groups(7)]) == (144, [18] * 8, 16, [16, 2], [16, 1])
    L = R.Layout(145)
    assert (L.W, L.nwin, L.lens, L.xs, L.n_short) == (32, 5, [1, 1, 1, 1, 1, 0, 0, 0], 4, 17)
    assert R.Layout(1).sizes == [1, 0, 0, 0, 0, 0, 0, 0]
    assert [R.Layout(32768, wv).weave for wv in (0, 1, 255)] == [4, 1, 255]


# ------------------------------------------------------------------------------------------------ wrong orders are rejected
S_MUT = 33000                 # W = 832, 40 windows, lists of five, list 7 = four full windows and the short one of 552


@pytest.fixture(scope="module")
def mut_keys():
    keys = R.keys_of(*R.step_counts("window-distinct", S_MUT))
    assert R.keys_distinct_in_windows(keys) and R.window_keys_distinct(keys)
    return keys


def rejected(tag, call):
    with pytest.raises(R.OrderError) as ei:
        call()
    assert "[%s]" % tag in str(ei.value), str(ei.value)
    return str(ei.value)


def kernel_formulas(keys, weave, deduct_short=True):
    """The placement written the way k_order_place / k_order_copy compute it, window by window, into an array prefilled with -1 and
    behind their `0 <= pos < S` guard -- with the one mistake a test asks for: deduct_short=False forgets that the list of the short
    window has one full window fewer."""
    S = keys.size
    L = R.Layout(S, weave)
    W, nwin, wv = L.W, L.nwin, L.weave
    wkeys = [int(keys[w * W:(w + 1) * W].max()) for w in range(L.nfull)]
    rank_of = {w: r for r, w in enumerate(sorted(range(L.nfull), key=lambda w: (-wkeys[w], w)))}
    order = np.full(S, -1, dtype=np.int64)
    for w in range(nwin):
        lo, hi = w * W, min(S, (w + 1) * W)
        local = lo + np.lexsort((np.arange(hi - lo), -keys[lo:hi]))
        short = L.has_short and w == nwin - 1
        r = nwin - 1 if short else rank_of[w]
        x, j = r % 8, r // 8
        nf = L.lens[x] - (1 if (L.has_short and x == L.xs and (deduct_short or short)) else 0)
        i = np.arange(hi - lo)
        if short:
            pos = L.starts[x] + nf * W + i
        else:
            g, m = j // wv, j % wv
            mg = min(nf - g * wv, wv)
            pos = L.starts[x] + g * wv * W + ((i >> 4) * mg + m) * 16 + (i & 15)
        keep = (pos >= 0) & (pos < S)
        order[pos[keep]] = local[keep]
    return order


@pytest.mark.parametrize("S,weave", R.WINDOWED_CASES)
def test_the_kernels_formulas_and_the_model_agree(S, weave):
    keys = R.keys_of(*R.step_counts("ten-keys", S))
    assert np.array_equal(kernel_formulas(keys, weave), R.model_windowed(keys, weave))


@pytest.mark.parametrize("weave", [0, 3])
def test_swapped_entries_inside_a_window_are_rejected(mut_keys, weave):
    order = R.model_windowed(mut_keys, weave)
    p = R.Layout(S_MUT, weave).starts[2]
    order[[p, p + 1]] = order[[p + 1, p]]
    assert order[p] // 832 == order[p + 1] // 832 and mut_keys[order[p]] != mut_keys[order[p + 1]]
    rejected("window-sorted", lambda: R.check_windowed(order, mut_keys, weave))


@pytest.mark.parametrize("weave", [0, 3])
def test_windows_that_exchange_ranks_are_rejected(mut_keys, weave):
    ranks = R.check_windowed(R.model_windowed(mut_keys, weave), mut_keys, weave)
    ranks[[2, 11]] = ranks[[11, 2]]
    msg = rejected("window-rank", lambda: R.check_windowed(R.build_windowed(mut_keys, weave, ranks), mut_keys, weave))
    assert msg.count("[") == msg.count("[window-rank]")          # nothing else is wrong with it


@pytest.mark.parametrize("weave", [0, 3])
def test_exchanged_slots_in_one_chunk_are_rejected(mut_keys, weave):
    order = R.model_windowed(mut_keys, weave)
    L = R.Layout(S_MUT, weave)
    g, p0, mg = L.groups(1)[0]
    a, b = p0 + (1 * mg + 0) * 16, p0 + (1 * mg + 1) * 16      # second row of the group: the chunks of slot 0 and slot 1
    tmp = order[a:a + 16].copy()
    order[a:a + 16] = order[b:b + 16]
    order[b:b + 16] = tmp
    msg = rejected("slot", lambda: R.check_windowed(order, mut_keys, weave))
    assert "c % mg" in msg


@pytest.mark.parametrize("weave", [0, 3, 16])
def test_a_group_size_that_forgets_the_short_window_is_rejected(mut_keys, weave):
    order = kernel_formulas(mut_keys, weave, deduct_short=False)
    msg = rejected("slot", lambda: R.check_windowed(order, mut_keys, weave))
    assert "list 7" in msg and "[permutation]" in msg          # the stretched group also leaves holes and runs over the short window


def test_a_group_size_that_forgets_the_short_window_is_harmless_only_without_one(mut_keys):
    keys = mut_keys[:32768]
    assert np.array_equal(kernel_formulas(keys, 3, deduct_short=False), R.model_windowed(keys, 3))


def test_the_short_window_first_in_its_list_is_rejected(mut_keys):
    order = R.model_windowed(mut_keys, 0)
    L = R.Layout(S_MUT)
    lo, hi = L.starts[L.xs], L.starts[L.xs] + L.sizes[L.xs]
    order[lo:hi] = np.concatenate([order[hi - L.n_short:hi], order[lo:hi - L.n_short]])
    rejected("short-window", lambda: R.check_windowed(order, mut_keys, 0))


def test_the_heaviest_window_ranked_by_its_key_when_it_is_the_short_one_is_rejected():
    """A short window holding the batch's heaviest segment still ranks last; an order that ranks it first by its key is wrong."""
    keys = R.keys_of(*R.step_counts("heavy-in-short", 900))
    L = R.Layout(900)
    good = R.model_windowed(keys)
    assert R.check_windowed(good, keys)[L.nwin - 1] == L.nwin - 1
    bad = np.concatenate([good[L.short_start():], good[:L.short_start()]])
    rejected("short-window", lambda: R.check_windowed(bad, keys))


def test_a_duplicated_entry_is_rejected(mut_keys):
    order = R.model_windowed(mut_keys, 0)
    order[5] = order[6]
    msg = rejected("permutation", lambda: R.check_windowed(order, mut_keys, 0))
    assert "1 segments missing" in msg and "1 segments more than once" in msg
    order = R.model_global(mut_keys)
    order[5] = order[6]
    rejected("permutation", lambda: R.check_global(order, mut_keys))
    rejected("permutation", lambda: R.check_global(np.full(S_MUT, -1), mut_keys))        # an output that was never written
    rejected("permutation", lambda: R.check_windowed(np.full(S_MUT, -1), mut_keys))


def test_an_ascending_global_order_is_rejected(mut_keys):
    for keys in (mut_keys, R.keys_of(*R.step_counts("ten-keys", 257)), np.array([1, 2])):
        order = R.model_global(keys)[::-1].copy()
        msg = rejected("global-sorted", lambda: R.check_global(order, keys))
        assert "[permutation]" not in msg


def test_an_entry_of_a_neighbouring_window_is_rejected(mut_keys):
    order = R.model_windowed(mut_keys, 0)
    a, b = int(np.flatnonzero(order == 3 * 832 + 5)[0]), int(np.flatnonzero(order == 4 * 832 + 9)[0])
    order[[a, b]] = order[[b, a]]
    msg = rejected("window-entries", lambda: R.check_windowed(order, mut_keys, 0))
    assert "[chunk]" in msg and "[permutation]" not in msg


def test_a_wrong_weave_is_rejected(mut_keys):
    """An order built for one group size does not pass for another (unless both are at least the list length)."""
    order = R.model_windowed(mut_keys, 2)
    rejected("slot", lambda: R.check_windowed(order, mut_keys, 3))
    R.check_windowed(R.model_windowed(mut_keys, 16), mut_keys, 255)
    R.check_windowed(R.model_windowed(mut_keys, 0), mut_keys, 5)          # weave = 0 here means min(ceil(40 / 8), 16) = 5


# ------------------------------------------------------------------------------------------------ step statistics
def test_step_stats_in_python_integers():
    assert R.step_stats([1, 2, 3], [0, 5, 1]) == [12, 7, 3]
    acc = np.full(262145, 10000, dtype=np.int32)
    assert R.step_stats(acc, np.zeros_like(acc)) == [2621450000, 10000, 262145] and 2621450000 > 2 ** 31
    assert R.step_stats([0, 0], [0, 0]) == [0, 0, 2]


# ------------------------------------------------------------------------------------------------ XCD alignment
def test_xcd_of_unit_inverts_the_kernels_map():
    for nb in (1, 7, 8, 9, 63, 64, 65, 1280, 1281):
        chunk, rem = divmod(nb, 8)
        units = [(b % 8) * chunk + min(b % 8, rem) + b // 8 for b in range(nb)]          # xcd_unit_of(b, nb)
        assert sorted(units) == list(range(nb))
        assert all(R.xcd_of_unit(u, nb) == b % 8 for b, u in enumerate(units))


@pytest.mark.parametrize("unit", [16, 32, 64])
def test_lists_are_the_eighths_at_multiples_of_8192_and_at_4096(unit):
    for S in [4096] + list(range(8192, 262144 + 1, 8192)):
        assert R.xcd_alignment(S, unit) == 0.0, S


ALIGNMENT_TABLE = {(20 * 1024, 16): 896, (20 * 1024, 32): 896, (20 * 1024, 64): 896,
                   (20000, 16): 1136, (20000, 32): 1120, (20000, 64): 928,
                   (8200, 16): 784, (8200, 32): 672, (8200, 64): 512}


def test_alignment_figures_are_the_ones_design_4_9_quotes():
    """Positions worked by another XCD than their list's, as computed; DESIGN 4.9 carries the same table (their cost in time is
    unmeasured)."""
    doc = open(os.path.join(ROOT, "DESIGN.md")).read()
    for (S, unit), count in ALIGNMENT_TABLE.items():
        assert R.xcd_misplaced(S, unit) == count, (S, unit, R.xcd_misplaced(S, unit))
    for S in (20 * 1024, 20000, 8200):
        row = "| %s | %d | %s |" % ("{:,}".format(S).replace(",", " "), R.window_size(S),
                                    " | ".join("%d (%.1f %%)" % (ALIGNMENT_TABLE[S, u], 100.0 * ALIGNMENT_TABLE[S, u] / S) for u in (16, 32, 64)))
        assert row in doc, row
    assert re.search(r"cost in time .{0,40}(unmeasured|not been measured)", doc)

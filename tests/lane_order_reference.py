"""The lane order of the adaptive sweeps and their step statistics, stated as checks.

The device builds both orders with atomics: where two segments of a window have the same key, or two windows the same window key,
the hardware decides who comes first.  So an order is not compared with "the" order: it is checked against the rules every valid
order obeys, restated here from the comments over k_order_scan, k_order_window, k_order_place and k_order_copy
(csrc/kernels_util.hip) and over order_window_size / xcd_unit_of (csrc/kernels.hpp) -- and what the device chose among the ties is
decoded and returned.  model_global / model_windowed build ONE valid order (the only one when no keys tie).

    key(s) = clamp(accepted[s] + rejected[s], 0, 1023)

Everything is integer arithmetic; nothing here has a tolerance."""
import numpy as np

BINS = 1024          # ORDER_BINS: keys are clamped to [0, BINS)
XCDS = 8             # LTO_XCDS
CHUNK = 16           # the interleave unit: 16 consecutive positions hold 16 consecutive entries of one window's local order
MAX_WINDOW = 1024    # LTO_ORDER_WINDOW


class OrderError(AssertionError):
    """An order that breaks the specification; the message carries one [tag] per rule broken."""


def keys_of(acc, rej):
    k = np.asarray(acc, dtype=np.int64) + np.asarray(rej, dtype=np.int64)
    return np.clip(k, 0, BINS - 1)


def window_size(S):
    """order_window_size: 8 k windows for k = ceil(S / 8 192), rounded up to 16 segments, 16 .. 1 024."""
    k = max(1, -(-S // 8192))
    w = -(-S // (8 * k))
    w = -(-w // CHUNK) * CHUNK
    return min(max(w, CHUNK), MAX_WINDOW)


class Layout:
    """Where the windowed order puts what, as a function of S and weave alone.
    W, nwin; has_short / n_short: the last window has fewer than W segments; nfull full windows with ranks 0 .. nfull-1, the short
    one has rank nwin-1 whatever its key.  The window of rank r is window r // 8 of list r % 8; lens[x] windows in list x; the lists
    follow one another, list x at starts[x], and list xs = (nwin-1) % 8 ends with the short window (it is `deficit` positions
    shorter).  weave: the group size in effect (0 -> min(ceil(nwin / 8), 16), at least 1)."""

    def __init__(self, S, weave=0):
        if S < 1 or not 0 <= weave <= 255:
            raise ValueError("need S >= 1 and 0 <= weave <= 255")
        self.S, self.W = S, window_size(S)
        W = self.W
        self.nwin = -(-S // W)
        self.has_short = S % W != 0
        self.n_short = S % W
        self.nfull = self.nwin - (1 if self.has_short else 0)
        self.xs = (self.nwin - 1) % XCDS
        self.deficit = self.nwin * W - S
        self.lens = [(self.nwin - x + XCDS - 1) // XCDS for x in range(XCDS)]
        self.nf = [self.lens[x] - (1 if self.has_short and x == self.xs else 0) for x in range(XCDS)]       # full windows per list
        self.sizes = [self.lens[x] * W - (self.deficit if self.has_short and x == self.xs else 0) for x in range(XCDS)]
        self.starts = [sum(self.sizes[:x]) for x in range(XCDS)]
        assert sum(self.lens) == self.nwin and sum(self.sizes) == S
        if weave == 0:
            nx = -(-self.nwin // XCDS)
            weave = min(max(nx, 1), 16)
        self.weave = weave

    def groups(self, x):
        """[(g, first position, mg)] of list x: groups of `weave` full windows, the last one of what is left."""
        out, g = [], 0
        while g * self.weave < self.nf[x]:
            out.append((g, self.starts[x] + g * self.weave * self.W, min(self.nf[x] - g * self.weave, self.weave)))
            g += 1
        return out

    def short_start(self):
        return self.starts[self.xs] + self.nf[self.xs] * self.W

    def list_of_position(self):
        """[S]: the list (= XCD) every position belongs to."""
        out = np.empty(self.S, dtype=np.int64)
        for x in range(XCDS):
            out[self.starts[x]:self.starts[x] + self.sizes[x]] = x
        return out


def _fail(problems):
    if problems:
        tags, head = set(), []
        for p in problems:                       # the first report of every rule ahead of the rest: a long list is cut short
            tag = p.split("]")[0]
            if tag not in tags:
                tags.add(tag)
                head.append(p)
        problems = head + [p for p in problems if p not in head]
        more = ["... and %d more" % (len(problems) - 12)] if len(problems) > 12 else []
        raise OrderError("lane order breaks its rules in %d place(s):\n  " % len(problems) + "\n  ".join(problems[:12] + more))


def _permutation_problem(order, S):
    if order.shape != (S,):
        return "[permutation] the order has shape %s, not (%d,)" % (order.shape, S)
    ok = (order >= 0) & (order < S)
    counts = np.bincount(order[ok], minlength=S)
    if ok.all() and (counts == 1).all():
        return None
    bad = np.flatnonzero(~ok)
    missing, twice = np.flatnonzero(counts == 0), np.flatnonzero(counts > 1)
    return ("[permutation] not a permutation of [0, %d): %d entries out of range (first at position %s: %s), %d segments missing "
            "(first %s), %d segments more than once (first %s)" %
            (S, bad.size, bad[:1], order[bad[:1]], missing.size, missing[:1], twice.size, twice[:1]))


def check_global(order, keys):
    """The global order: a permutation of [0, S), keys non-increasing along it."""
    keys = np.asarray(keys, dtype=np.int64)
    order = np.asarray(order).astype(np.int64)
    S = keys.size
    problems = []
    p = _permutation_problem(order, S)
    if p:
        problems.append(p)
    if order.shape == (S,):
        ok = (order >= 0) & (order < S)
        k = np.where(ok, keys[np.where(ok, order, 0)], -1)
        up = np.flatnonzero(np.diff(k) > 0)
        if up.size:
            i = int(up[0])
            problems.append("[global-sorted] keys must not increase along the order: %d places do, first at positions %d, %d (keys %d, %d)"
                            % (up.size, i, i + 1, k[i], k[i + 1]))
    _fail(problems)


def check_windowed(order, keys, weave=0):
    """The windowed order for `keys` and the group size `weave` (0: the kernel's choice).  Raises OrderError naming every rule
    broken; returns the rank -> window map the order encodes (int array [nwin])."""
    keys = np.asarray(keys, dtype=np.int64)
    order = np.asarray(order).astype(np.int64)
    S = keys.size
    L = Layout(S, weave)
    W = L.W
    problems = []
    p = _permutation_problem(order, S)
    if p:
        problems.append(p)
    if order.shape != (S,):
        _fail(problems)
    ok = (order >= 0) & (order < S)
    safe = np.where(ok, order, 0)
    win_of = np.where(ok, safe // W, -1)            # the window every position's entry comes from
    key_of = np.where(ok, keys[safe], -1)
    rank_to_window = np.full(L.nwin, -1, dtype=np.int64)
    seen = {}

    def window_sequence(tag_where, w, seq_e, seq_k, lo, hi):
        if not np.array_equal(np.sort(seq_e), np.arange(lo, hi)):
            problems.append("[window-entries] %s: its %d positions must hold exactly the segments [%d, %d) of window %d; %d of them do not"
                            % (tag_where, seq_e.size, lo, hi, w, int(np.sum((seq_e < lo) | (seq_e >= hi)))))
        up = np.flatnonzero(np.diff(seq_k) > 0)
        if up.size:
            i = int(up[0])
            problems.append("[window-sorted] %s (window %d): read in position order its keys must not increase; %d places do, first "
                            "between its entries %d and %d (keys %d, %d)" % (tag_where, w, up.size, i, i + 1, seq_k[i], seq_k[i + 1]))

    for x in range(XCDS):
        if L.lens[x] == 0:
            continue
        lo, hi = L.starts[x], L.starts[x] + L.sizes[x]
        distinct = np.unique(win_of[lo:hi])
        if distinct.size != L.lens[x]:
            problems.append("[lists] list %d, positions [%d, %d), must hold %d windows (the short window's deficit of %d comes off list "
                            "%d); it holds entries of %d" % (x, lo, hi, L.lens[x], L.deficit if L.has_short else 0, L.xs, distinct.size))
        for g, p0, mg in L.groups(x):
            blk = slice(p0, p0 + mg * W)
            bw = win_of[blk].reshape(W // CHUNK, mg, CHUNK)          # [row][slot][lane]: chunk c = row * mg + slot
            be = order[blk].reshape(W // CHUNK, mg, CHUNK)
            bk = key_of[blk].reshape(W // CHUNK, mg, CHUNK)
            first = bw[:, :, 0]
            mixed = np.argwhere((bw != first[:, :, None]).any(axis=2))
            if mixed.size:
                row, m = mixed[0]
                problems.append("[chunk] list %d group %d: every 16-position chunk holds entries of one window only; %d chunks mix windows, "
                                "first chunk %d (positions from %d): windows %s" %
                                (x, g, len(mixed), row * mg + m, p0 + (row * mg + m) * CHUNK, np.unique(bw[row, m]).tolist()))
            slot_w = first[0]
            wrong = np.argwhere(first != slot_w[None, :])
            if wrong.size:
                row, m = wrong[0]
                problems.append("[slot] list %d group %d: chunk c of a group of mg = %d windows belongs to slot c %% mg; %d chunks hold "
                                "another window than their slot's first chunk, first chunk %d (slot %d holds window %d, the chunk window %d)"
                                % (x, g, mg, len(wrong), row * mg + m, m, slot_w[m], first[row, m]))
            for m in range(mg):
                w, r = int(slot_w[m]), x + XCDS * (g * L.weave + m)
                where = "list %d group %d slot %d (rank %d)" % (x, g, m, r)
                if not 0 <= w < L.nfull:
                    problems.append("[window-entries] %s must hold a full window; its first entry belongs to window %d" % (where, w))
                    continue
                if w in seen:
                    problems.append("[window-entries] window %d sits at %s and at %s" % (w, seen[w], where))
                seen[w] = where
                rank_to_window[r] = w
                window_sequence(where, w, be[:, m, :].ravel(), bk[:, m, :].ravel(), w * W, (w + 1) * W)
        if L.has_short and x == L.xs:
            p0, w = L.short_start(), L.nwin - 1
            seq = order[p0:p0 + L.n_short]
            if p0 + L.n_short != hi or not np.array_equal(np.sort(seq), np.arange(w * W, S)):
                problems.append("[short-window] the short window (%d segments from %d) sits alone at the end of list %d, positions [%d, %d), "
                                "unwoven, whatever its key; %d of these positions hold other segments" %
                                (L.n_short, w * W, x, p0, p0 + L.n_short, int(np.sum(seq < w * W))))
            else:
                rank_to_window[w] = w
                window_sequence("the short window at the end of list %d" % x, w, seq, key_of[p0:p0 + L.n_short], w * W, S)
    ranked = rank_to_window[:L.nfull]
    if (ranked >= 0).all() and L.nfull > 1:
        wkeys = keys[:L.nfull * W].reshape(L.nfull, W).max(axis=1)[ranked]
        up = np.flatnonzero(np.diff(wkeys) > 0)
        if up.size:
            r = int(up[0])
            problems.append("[window-rank] with rank r = x + 8 (g * weave + m) the window keys (a window's largest key) of the full windows "
                            "must not increase in r; %d places do, first ranks %d, %d: windows %d, %d with keys %d, %d"
                            % (up.size, r, r + 1, ranked[r], ranked[r + 1], wkeys[r], wkeys[r + 1]))
    _fail(problems)
    return rank_to_window


def _descending(k, rng):
    """Indices that sort k descending; ties in index order, or in a random one."""
    tie = np.arange(k.size) if rng is None else rng.permutation(k.size)
    return np.lexsort((tie, -k))


def build_windowed(keys, weave, rank_to_window, tie_rng=None):
    """The windowed order with the full windows at the given ranks (rank_to_window[r], r < nfull) and every window's segments
    heaviest first (equal keys in index order, or shuffled by tie_rng)."""
    keys = np.asarray(keys, dtype=np.int64)
    S = keys.size
    L = Layout(S, weave)
    W = L.W
    order = np.full(S, -1, dtype=np.int64)

    def local(w):
        lo, hi = w * W, min(S, (w + 1) * W)
        return lo + _descending(keys[lo:hi], tie_rng)
    for x in range(XCDS):
        for g, p0, mg in L.groups(x):
            view = order[p0:p0 + mg * W].reshape(W // CHUNK, mg, CHUNK)
            for m in range(mg):
                w = int(rank_to_window[x + XCDS * (g * L.weave + m)])
                view[:, m, :] = local(w).reshape(W // CHUNK, CHUNK)
    if L.has_short:
        order[L.short_start():L.short_start() + L.n_short] = local(L.nwin - 1)
    return order


def model_windowed(keys, weave=0, tie_rng=None):
    """One valid windowed order: full windows ranked by their largest key, heaviest first (ties in index order or shuffled)."""
    keys = np.asarray(keys, dtype=np.int64)
    L = Layout(keys.size, weave)
    wkeys = keys[:L.nfull * L.W].reshape(L.nfull, L.W).max(axis=1) if L.nfull else np.zeros(0, dtype=np.int64)
    ranks = np.append(_descending(wkeys, tie_rng), L.nwin - 1) if L.has_short else _descending(wkeys, tie_rng)
    return build_windowed(keys, weave, ranks, tie_rng)


def model_global(keys, tie_rng=None):
    return _descending(np.asarray(keys, dtype=np.int64), tie_rng)


def keys_distinct_in_windows(keys):
    keys = np.asarray(keys, dtype=np.int64)
    W = window_size(keys.size)
    return all(np.unique(keys[lo:lo + W]).size == keys[lo:lo + W].size for lo in range(0, keys.size, W))


def window_keys_distinct(keys):
    keys = np.asarray(keys, dtype=np.int64)
    L = Layout(keys.size)
    wk = [int(keys[w * L.W:(w + 1) * L.W].max()) for w in range(L.nfull)]
    return len(set(wk)) == len(wk)


def step_stats(acc, rej):
    """[sum, max, S] of acc + rej in Python integers; the maximum is taken from 0 up, as k_step_stats takes it."""
    total, top = 0, 0
    for a, r in zip(np.asarray(acc).tolist(), np.asarray(rej).tolist()):
        total += a + r
        top = max(top, a + r)
    return [total, top, len(acc)]


def xcd_of_unit(u, nb):
    """The XCD whose workgroups work unit u of nb: the inverse of xcd_unit_of (workgroup b runs on XCD b % 8 and works unit
    x * chunk + min(x, rem) + b // 8 with chunk, rem = divmod(nb, 8))."""
    chunk, rem = divmod(nb, XCDS)
    for x in range(XCDS):
        lo = x * chunk + min(x, rem)
        if lo <= u < lo + chunk + (1 if x < rem else 0):
            return x
    raise ValueError("unit %d of %d" % (u, nb))


def xcd_alignment(S, unit):
    """Share of the S positions of a windowed order that are worked by another XCD than the one their list belongs to, when the
    sweep's workgroups cover `unit` consecutive positions each and are mapped by xcd_unit_of.  0.0 exactly when none is."""
    return xcd_misplaced(S, unit) / S


def xcd_misplaced(S, unit):
    """The count behind xcd_alignment."""
    L = Layout(S)
    nb = -(-S // unit)
    chunk, rem = divmod(nb, XCDS)
    ends = np.array([(x + 1) * chunk + min(x + 1, rem) for x in range(XCDS)])          # one past the last unit of XCD x
    worker = np.searchsorted(ends, np.arange(S) // unit, side="right")
    return int(np.sum(worker != L.list_of_position()))


# ------------------------------------------------------------------------------------------------ the cases of both test files
# Global order: 262 144 + 257 segments are more than 1 024 workgroups of 256, so histogram and scatter take a second grid-stride trip.
GLOBAL_SIZES = [1, 2, 255, 256, 257, 1025, 262144 + 257]
GLOBAL_PATTERNS = ["one-key", "ten-keys", "distinct", "clamped", "zeros-negative", "heavy-first", "heavy-last"]
# Windowed order, (S, weave).  1 .. 128: W = 16 and one to eight windows; 129, 145: W = 32 and five windows (lists of unequal
# length: some XCDs get none), with and without a short window; 900: W = 128 and a short window of 4; 32 768 / 33 000: lists of four and five windows, whole and ragged groups, a short window of
# 552; 140 000: 144 windows, lists of 18, weave 0 -> groups of 16 + 2.
WINDOWED_CASES = ([(S, 0) for S in (1, 15, 16, 17, 29, 127, 128, 129, 145, 900, 1024, 1025, 8191, 8192, 8193, 16385)] +
                  [(S, wv) for S in (32768, 33000) for wv in (0, 1, 2, 3, 5, 16, 255)] + [(140000, 0)])
WINDOWED_PATTERNS = GLOBAL_PATTERNS + ["window-distinct", "window-keys-equal", "heavy-in-short", "heavy-at-window-end"]


def step_counts(pattern, S, seed=0):
    """(accepted, rejected) int32 [S] of a named pattern; key = clamp(accepted + rejected, 0, 1023)."""
    rng = np.random.default_rng([seed, S, sorted(WINDOWED_PATTERNS).index(pattern)])
    W = window_size(S)
    if pattern == "one-key":
        total = np.full(S, 9)
    elif pattern == "ten-keys":                    # the line search: about ten distinct step counts
        total = rng.integers(20, 30, S)
    elif pattern == "distinct":                    # distinct step counts; past 1 024 segments the large ones tie in the last bin
        total = rng.permutation(S)
    elif pattern == "clamped":                     # 1 023, 1 024 and 5 000 tie in bin 1 023
        total = rng.choice([1022, 1023, 1024, 5000], S)
    elif pattern == "zeros-negative":
        total = rng.choice([0, 0, -5, 3], S)
    elif pattern in ("heavy-first", "heavy-last"):
        total = np.full(S, 3)
        total[0 if pattern == "heavy-first" else S - 1] = 900
    elif pattern == "window-distinct":             # distinct keys inside every window; distinct window keys where 1 024 bins allow
        L = Layout(S)
        room = np.arange(min(W, S) - 1, BINS)
        tops = rng.choice(room, L.nfull, replace=L.nfull > room.size)
        total = np.empty(S, dtype=np.int64)
        for w in range(L.nwin):
            lo, hi = w * W, min(S, (w + 1) * W)
            top = int(tops[w]) if w < L.nfull else BINS - 1
            total[lo:hi] = rng.permutation(np.append(rng.choice(top, hi - lo - 1, replace=False), top))
    elif pattern == "window-keys-equal":           # every window's largest key is 500
        total = rng.integers(0, 500, S)
        total[np.arange(0, S, W) + rng.integers(0, np.minimum(W, S - np.arange(0, S, W)))] = 500
    elif pattern == "heavy-in-short":              # the batch's heaviest segment in the last window only: it still ranks last
        total = rng.integers(0, 100, S)
        total[S - 1 - int(rng.integers(0, max(1, S % W)))] = 1000
    elif pattern == "heavy-at-window-end":
        total = rng.integers(0, 100, S)
        total[np.minimum(np.arange(0, S, W) + W - 1, S - 1)] = 200 + rng.integers(0, 50, -(-S // W))
    else:
        raise ValueError(pattern)
    total = np.asarray(total, dtype=np.int64)
    rej = np.minimum(rng.integers(0, 4, S), np.maximum(total, 0))
    return (total - rej).astype(np.int32), rej.astype(np.int32)

"""Host restatement of the indirect method's mesh equidistribution (lto_indirect_remesh_batch): the monitor's running
sum in the device's summation order, the new grid, and which old node each new one is propagated from over which span.  numpy only."""
import numpy as np


def scan64(w):
    """Inclusive running sum of w in the order k_remesh_grid uses: tiles of 64 consecutive entries scanned with six shift-and-add
    steps (shifts 1, 2, .. 32), the tile totals scanned the same way (recursively), then every entry adds the inclusive sum of the
    tiles before its own.  Integer-valued w: exact, equal to np.cumsum."""
    w = np.asarray(w, dtype=np.float64)
    m = w.size
    tiles = (m + 63) // 64
    x = np.zeros(tiles * 64)
    x[:m] = w
    x = x.reshape(tiles, 64)
    for off in (1, 2, 4, 8, 16, 32):
        x = np.concatenate([x[:, :off], x[:, off:] + x[:, :-off]], axis=1)
    if tiles > 1:
        inc = scan64(x[:, -1])
        x[1:] = inc[:-1, None] + x[1:]
    return x.reshape(-1)[:m]


def new_grid(t, w, n_new):
    """Step 2: C_0 = 0, C_{i+1} = C_i + w_i, W = C_{n-1}; g_k = k W / (n_new - 1), i = the largest index with C_i <= g_k,
    t'_k = t_i + (g_k - C_i) / w_i * (t_{i+1} - t_i); the end points are the old ones.  Returns (t_new, C)."""
    t = np.asarray(t, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    n = t.size
    assert w.size == n - 1 and n_new >= 2
    C = np.concatenate([[0.0], scan64(w)])
    W = C[-1]
    k = np.arange(1, n_new - 1, dtype=np.float64)
    g = k * W / np.float64(n_new - 1)
    i = np.clip(np.searchsorted(C, g, side="right") - 1, 0, n - 2)
    tk = t[i] + (g - C[i]) / w[i] * (t[i + 1] - t[i])
    return np.concatenate([[t[0]], tk, [t[-1]]]), C


def sources(t, t_new):
    """Step 3: (i, span) per new node: i = the largest index with t_i <= t'_k, span = t'_k - t_i; the last node is old node n-1
    with span 0 (a copy), never a propagation of node n-2."""
    t = np.asarray(t, dtype=np.float64)
    t_new = np.asarray(t_new, dtype=np.float64)
    i = np.clip(np.searchsorted(t, t_new, side="right") - 1, 0, t.size - 1)
    return i, t_new - t[i]


def monitor_share(t, w, t_new):
    """The monitor each new segment carries: differences of the piecewise-linear C(t) at the new nodes."""
    t = np.asarray(t, dtype=np.float64)
    C = np.concatenate([[0.0], np.cumsum(np.asarray(w, dtype=np.float64))])
    return np.diff(np.interp(t_new, t, C))

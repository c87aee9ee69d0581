"""Host restatement of the direct method's resampling (lto_direct_resample_batch), step by step: the monitor from the
estimates, the grid (remesh_reference.new_grid, scan64 order), the node rule with the CPU oracle's fixed-step RKF7(8) flow, and
the passes.  numpy and the oracle module handed in; never the device library."""
import numpy as np

import remesh_reference as rr


def weights_from_estimates(e, w_floor):
    """Step 2: r_i = e_i^(1/8) as three correctly rounded square roots, w_i = max(r_i, w_floor max_j r_j); all 1 if every r is 0.
    A NaN estimate: None (status 2)."""
    e = np.asarray(e, dtype=np.float64)
    if np.isnan(e).any():
        return None
    r = np.sqrt(np.sqrt(np.sqrt(e)))
    rmax = r.max()
    if rmax == 0.0:
        return np.ones_like(r)
    return np.maximum(r, np.float64(w_floor) * rmax)


def grid(t, w, n_new):
    """Step 3: the new times, end points bit copies."""
    return rr.new_grid(t, w, n_new)[0]


def node_rule(t, tk, last):
    """Step 4's case analysis for one new time: ("copy", i), ("forward", i, span, s) or ("backward", i, span, s); i = the largest
    index with t_i <= t'_k, s = (t'_k - t_i)/(t_{i+1} - t_i).  At t'_k == t_mid the span is the sweep's 0.5 (t_{i+1} - t_i)."""
    n = t.size
    i = n - 1 if last else int(np.clip(np.searchsorted(t, tk, side="right") - 1, 0, n - 1))
    if i == n - 1 or tk == t[i]:
        return ("copy", i)
    t0, t1 = t[i], t[i + 1]
    tm = t0 + (t1 - t0) / 2
    s = (tk - t0) / (t1 - t0)
    if tk <= tm:
        return ("forward", i, 0.5 * (t1 - t0) if tk == tm else tk - t0, s)
    return ("backward", i, t1 - tk, s)


def nodes(oracle, X, U, t, t_new, nsteps, prm):
    """Step 4: states and controls at t_new on the piecewise trajectory of (X, U, t).  prm = (MU, DU, TU, Isp)."""
    X, U, t, t_new = (np.asarray(a, dtype=np.float64) for a in (X, U, t, t_new))
    Xn = np.zeros((X.shape[0], t_new.size), order="F")
    Un = np.zeros((3, t_new.size), order="F")
    flip = np.ones(X.shape[0])
    flip[3:6] = -1.0
    for k, tk in enumerate(t_new):
        rule = node_rule(t, tk, k == t_new.size - 1)
        i = rule[1]
        if rule[0] == "copy":
            Xn[:, k], Un[:, k] = X[:, i], U[:, i]
            continue
        _, _, span, s = rule
        if rule[0] == "forward":
            Xn[:, k], _ = oracle.flow_prop_ep(X[:, i], U[:, i], 1.0, span, oracle.RKF78_FIXED, nsteps - 1, *prm)
        else:
            y, _ = oracle.flow_prop_ep(X[:, i + 1] * flip, U[:, i + 1], -1.0, span, oracle.RKF78_FIXED, nsteps - 1, *prm)
            Xn[:, k] = y * flip
        Un[:, k] = U[:, i] + s * (U[:, i + 1] - U[:, i])
    return Xn, Un


def resample(oracle, X, U, t, nsteps, prm, n_new, weights=None, w_floor=0.1, passes=1):
    """Steps 1-5 for one trajectory (its valid part).  Returns (X, U, t, status); status 2: outputs NaN."""
    assert weights is None or passes == 1
    X, U, t = (np.asarray(a, dtype=np.float64) for a in (X, U, t))
    for _ in range(passes):
        w = weights
        if w is None:
            w = weights_from_estimates(oracle.direct_defect(X, U, t, nsteps, *prm)[1], w_floor)
        if w is None:
            nan = np.full((X.shape[0], n_new), np.nan)
            return nan, nan[:3].copy(), nan[0].copy(), 2
        t_new = grid(t, w, n_new)
        X, U = nodes(oracle, X, U, t, t_new, nsteps, prm)
        t = t_new
    return X, U, t, 0

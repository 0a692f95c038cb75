"""Shared helpers of the adaptive-sampling tests (tests/test_adaptive.py on the
host, tests/test_gpu_adaptive.py and tests/test_gpu_adaptive_wide.py on the
GPU): the stop rule of
include/pt_capi.h (pt_adapt_params) evaluated in numpy with the same f64
operations in the same order, a simulation of a whole adaptive run on
per-sample colours, and the oracle's per-sample frames."""
import numpy as np


def err_numpy(S, Q, n, floor):
    """err of every pixel: S, Q (..., 3) f64, n (...) unsigned; +inf for n < 2."""
    S = np.asarray(S, dtype=np.float64)
    Q = np.asarray(Q, dtype=np.float64)
    n = np.asarray(n)
    dn = n.astype(np.float64)
    d1 = (n.astype(np.int64) - 1).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        m = S / dn[..., None]
        v = np.maximum(0.0, Q - S * S / dn[..., None]) / d1[..., None]
        num = np.sqrt(((v[..., 0] + v[..., 1]) + v[..., 2]) / dn)
        den = ((np.abs(m[..., 0]) + np.abs(m[..., 1])) + np.abs(m[..., 2])) + np.float64(floor)
        err = num / den
    return np.where(n < 2, np.inf, err)


def active_numpy(n, err, tol, min_spp, max_spp):
    n = np.asarray(n)
    return (n < min_spp) | ((err > tol) & (n < max_spp))


def k_numpy(n, min_spp, max_spp, step_spp):
    n = np.asarray(n).astype(np.int64)
    goal = np.where(n < min_spp, min_spp, max_spp)
    return np.clip(np.minimum(step_spp, goal - n), 0, None)


def simulate(samples, tol, floor, min_spp, max_spp, step_spp):
    """The adaptive run on per-sample colours samples[s] (..., 3), s <
    max_spp: sample s of a pixel is samples[s] at that pixel whichever pass
    takes it.  Returns dict(n, S, Q, err, mean, passes [(n_active, added)],
    margin: the smallest |err - tol| / tol of a stop decision at n >= 2)."""
    samples = np.asarray(samples, dtype=np.float64)
    shape = samples.shape[1:-1]
    n = np.zeros(shape, dtype=np.int64)
    S = np.zeros(shape + (3,))
    Q = np.zeros(shape + (3,))
    passes = []
    margin = np.inf
    while True:
        err = err_numpy(S, Q, n, floor)
        act = active_numpy(n, err, tol, min_spp, max_spp)
        decided = (n >= max(2, min_spp)) & (n < max_spp) & np.isfinite(err)
        if tol > 0 and decided.any():
            margin = min(margin, float(np.min(np.abs(err[decided] - tol)) / tol))
        if not act.any():
            break
        k = np.where(act, k_numpy(n, min_spp, max_spp, step_spp), 0)
        passes.append((int(act.sum()), int(k.sum())))
        for j in range(int(k.max())):
            take = act & (j < k)
            idx = np.nonzero(take)
            c = samples[(n[idx] + j,) + idx]
            S[idx] += c
            Q[idx] += c * c
        n = n + k
    mean = np.where(n[..., None] > 0, S / np.maximum(n, 1)[..., None], 0.0)
    return dict(n=n, S=S, Q=Q, err=err, mean=mean, passes=passes, margin=margin)


def oracle_samples(packed, width, height, bounces, seed, n_samples, flags=0, rr_depth=3):
    """The oracle's per-sample frames (n_samples, H, W, 3) f64 in image
    orientation: frame s is the spp = 1 render of sample index s."""
    from oracle import oracle
    from pathtracerpython_amd.render import from_list_order
    out = np.zeros((n_samples, height, width, 3))
    for s in range(n_samples):
        c, _ = oracle.render(packed, width, height, 1, bounces, seed, flags, rr_depth,
                             sample_begin=s)
        out[s] = from_list_order(c, width, height)
    return out


def moments_upto(samples, n):
    """S[e] = sum of samples[s][e] over s < n[e] and Q likewise with the
    squares, for per-pixel counts n (...) <= len(samples): what an accumulator
    holds once every pixel e has taken its first n[e] samples."""
    samples = np.asarray(samples, dtype=np.float64)
    n = np.asarray(n).astype(np.int64)
    assert n.min() >= 0 and n.max() <= len(samples)
    zero = np.zeros((1,) + samples.shape[1:])
    idx = np.broadcast_to(n[None, ..., None], (1,) + samples.shape[1:])
    S = np.take_along_axis(np.concatenate([zero, np.cumsum(samples, axis=0)]), idx, axis=0)[0]
    Q = np.take_along_axis(np.concatenate([zero, np.cumsum(samples ** 2, axis=0)]), idx, axis=0)[0]
    return S, Q


def block_counts(active, block=256):
    """Active pixels per select block: the counts k_accum_select_count leaves
    for the scan (pixel e belongs to block e // block)."""
    a = np.asarray(active).ravel().astype(np.int64)
    return np.add.reduceat(a, np.arange(0, a.size, block))


def histogram(n):
    v, c = np.unique(np.asarray(n), return_counts=True)
    return {int(a): int(b) for a, b in zip(v, c)}

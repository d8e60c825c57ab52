"""Update diagnostics, restated in numpy (include/pcc_policy.h: pcc_update_diag_pop): reference() is a member's
row of `diag` in plain float64 from the float32 inputs, bounds() what a device that follows the header's float32 operations may
differ from it by, clip_margin_ok() whether the exact clipped count is a fair demand, decide() the stop rule and hyper_live.

The bound of the log-ratio.  The header fixes the float32 operations, each rounded to nearest (unit roundoff u = 2^-24), without
contraction, on exact float32 inputs:
    inv = expf(-log_std)        libm, 1 ulp: relative error <= 2 u
    t   = act - mean_new        u
    z   = t * inv               u           -> z carries a relative error <= 4 u, z^2 <= 8 u
    p   = (-0.5f * z) * z       u (the halving is exact) -> |p + z^2 / 2| <= 9 u z^2 / 2
    q   = p - log_std           u |q|       <= u (z^2 / 2 + |log_std|)
    lp  = q - kHalfLog2Pi       u |lp|      <= u (z^2 / 2 + |log_std| + 0.919), and the float32 constant is off by <= u / 2
    d32 = lp - logp_old         u |d32|     <= u (z^2 / 2 + |log_std| + 0.919 + |logp_old|)
which adds up, to first order in u, to u (12 z^2 / 2 + 3 |log_std| + 2.34 + |logp_old|) <= 12 u (z^2 / 2 + |log_std| + 1 +
|logp_old|).  C = 13 leaves one unit for the terms of second order (each is below 1e-6 of the first).  So per sample
    delta_i = C 2^-24 (z_i^2 / 2 + |log_std| + 1 + |logp_old_i|).
k = expm1(d) - d has the derivative expm1(d): a sample's k moves by at most |expm1(d_i)| delta_i + delta_i^2 (the float64 expm1's
own ulp, 2^-53 |expm1(d)|, disappears in it), and the float64 sum of n terms adds 8 n 2^-53 max k.  The variances are held to
moment_bounds of tests/test_obs_norm_cpu.py (section 19)."""
import numpy as np

from reward_norm_model import batch_moments, moment_bounds  # noqa: F401  (section 19's restatement, as the sibling model shares it)

C = 13.0
U32 = 2.0 ** -24
U64 = 2.0 ** -53
HALF_LOG_2PI = 0.5 * np.log(2.0 * np.pi)
DIAG_NAMES = ("count", "approx_kl", "clip_fraction", "explained_variance", "max_abs_log_ratio", "var_ret", "var_resid", "nonfinite")


def selected(x, row_step):
    """The rows 0, row_step, 2 row_step, ... of x [T][n]."""
    return np.asarray(x)[::row_step]


def logp32(act, mean, log_std):
    """The Gaussian head's log-probability as the kernels compute it, float32 operation by float32 operation (for the tests'
    logp_old: what the rollout would have stored)."""
    act, mean, ls = np.asarray(act, np.float32), np.asarray(mean, np.float32), np.float32(log_std)
    inv = np.exp(-ls).astype(np.float32)
    z = ((act - mean) * inv).astype(np.float32)
    return ((np.float32(-0.5) * z) * z - ls - np.float32(HALF_LOG_2PI)).astype(np.float32)


def log_ratio(act, logp_old, mean_new, log_std):
    """(d, z) in plain float64 from the float32 inputs."""
    act, lo, mu = (np.asarray(x, np.float32).astype(np.float64) for x in (act, logp_old, mean_new))
    ls = np.float64(np.float32(log_std))
    with np.errstate(invalid="ignore", over="ignore"):
        z = (act - mu) * np.exp(-ls)
        return -0.5 * z * z - ls - HALF_LOG_2PI - lo, z


def deltas(z, logp_old, log_std):
    """delta_i of the docstring (NaN for a NaN sample)."""
    lo = np.abs(np.asarray(logp_old, np.float32).astype(np.float64))
    return C * U32 * (z * z / 2.0 + abs(np.float64(np.float32(log_std))) + 1.0 + lo)


def reference(act, logp_old, mean_new, ret, val, log_std, clip, row_step=1):
    """A member's row of diag, as a dict of DIAG_NAMES, from its [T][n_m] float32 columns: float64 numpy, two-pass variances."""
    act, logp_old, mean_new, ret, val = (selected(x, row_step) for x in (act, logp_old, mean_new, ret, val))
    d, _ = log_ratio(act, logp_old, mean_new, log_std)
    n = d.size
    with np.errstate(invalid="ignore", over="ignore"):
        r1 = np.expm1(d)
        k = r1 - d
        clipped = int((np.abs(r1) > np.float64(np.float32(clip))).sum())
    r = np.asarray(ret, np.float32).astype(np.float64).reshape(-1, 1)
    e = r - np.asarray(val, np.float32).astype(np.float64).reshape(-1, 1)
    constant = bool(np.ptp(r) == 0.0)   # (a mean of n equal numbers need not be that number: the two-pass would leave dust)
    var_ret = 0.0 if constant else float(batch_moments(r)[2][0]) / n
    var_resid = float(batch_moments(e)[2][0]) / n
    absd = np.abs(d)
    return {"count": float(n), "approx_kl": float(k.mean()), "clip_fraction": clipped / n, "clipped": clipped,
            "explained_variance": float("nan") if var_ret == 0.0 else 1.0 - var_resid / var_ret,
            "max_abs_log_ratio": float(np.fmax.reduce(absd.reshape(-1), initial=0.0)), "var_ret": var_ret, "var_resid": var_resid,
            "nonfinite": float((~np.isfinite(d)).sum())}


def bounds(act, logp_old, mean_new, ret, val, log_std, row_step=1):
    """What the device's row may differ from reference() by: a dict with approx_kl, max_abs_log_ratio, var_ret, var_resid and
    explained_variance (NaN where the reference is NaN or the samples are not finite)."""
    act, logp_old, mean_new, ret, val = (selected(x, row_step) for x in (act, logp_old, mean_new, ret, val))
    d, z = log_ratio(act, logp_old, mean_new, log_std)
    dl = deltas(z, logp_old, log_std)
    n = d.size
    with np.errstate(invalid="ignore", over="ignore"):
        r1 = np.expm1(d)
        k = r1 - d
        kl = float((np.abs(r1) * dl + dl * dl).mean() + 8.0 * n * U64 * k.max())
    r = np.asarray(ret, np.float32).astype(np.float64)
    e = r - np.asarray(val, np.float32).astype(np.float64)
    b_ret, b_resid = moment_bounds(n, float(np.abs(r).max()))[1], moment_bounds(n, float(np.abs(e).max()))[1]
    vt, vr = float(batch_moments(r.reshape(-1, 1))[2][0]) / n, float(batch_moments(e.reshape(-1, 1))[2][0]) / n
    if np.ptp(r) == 0.0 or vt <= b_ret:
        ev = float("nan")
    else:   # |vr' / vt' - vr / vt| <= (|vr' - vr| + (vr / vt) |vt' - vt|) / vt', vt' >= vt - b_ret; then a division and a subtraction
        ev = (b_resid + vr / vt * b_ret) / (vt - b_ret) + 4.0 * U64 * (1.0 + vr / vt)
    return {"approx_kl": kl, "max_abs_log_ratio": float(np.fmax.reduce(dl.reshape(-1), initial=0.0)), "var_ret": b_ret,
            "var_resid": b_resid, "explained_variance": ev}


def clip_margin_ok(act, logp_old, mean_new, log_std, clip, row_step=1):
    """True when no sample's |expm1(d)| lies within exp(d) delta_i of clip: only then does a device whose d is off by delta_i count
    the same samples as clipped."""
    act, logp_old, mean_new = (selected(x, row_step) for x in (act, logp_old, mean_new))
    d, z = log_ratio(act, logp_old, mean_new, log_std)
    dl = deltas(z, logp_old, log_std)
    ok = np.isfinite(d)
    with np.errstate(invalid="ignore", over="ignore"):
        near = np.abs(np.abs(np.expm1(d[ok])) - np.float64(np.float32(clip))) <= np.exp(d[ok]) * dl[ok]
    return not bool(near.any())


def decide(stop, approx_kl, kl_limit, epoch, hyper):
    """(stop, hyper_live) after a check, from the device's own approx_kl [K]: the header's rule, member by member."""
    stop = np.array(stop, dtype=np.int32)
    live = np.array(hyper, dtype=np.float32)
    for m in range(stop.size):
        if stop[m] == 0 and kl_limit > 0 and not (approx_kl[m] <= kl_limit):
            stop[m] = epoch
        if stop[m] != 0:
            live[m, 0] = 0.0
    return stop, live


# ---------------------------------------------------------------------------------------------- the GPU tests' table of cases
LOG_STDS = (0.0, -1.0, 0.5)
# name: (T, n_m, K, row_step, shift, ret / val kind)
CASES = {
    "one": (1, 1, 1, 1, 1e-3, "unit"),
    "three-members": (5, 257, 3, 1, 0.1, "unit"),
    "many-groups": (7, 4099, 2, 1, 1e-3, "offset"),
    "four-members": (3, 65, 4, 1, 3.0, "unit"),
    "one-wave": (3, 64, 1, 1, 0.0, "offset"),
    "episode": (400, 64, 1, 1, 0.1, "unit"),
    "every-second-row": (7, 4099, 2, 2, 0.1, "unit"),
    "step-past-T": (5, 257, 3, 9, 3.0, "offset"),
    "constant-ret": (3, 65, 4, 1, 0.1, "constant"),
}
CLIP = 0.2


def make_case(name):
    """The inputs of a case, chosen on the CPU: a dict of float32 [T][N] arrays act, logp_old, mean_new, ret, val, log_std [K] and
    the scalars.  mean_new = mean_old + shift; act = mean_old + exp(log_std) eps; logp_old by logp32."""
    T, n_m, K, row_step, shift, kind = CASES[name]
    rng = np.random.default_rng(sorted(CASES).index(name) + 23)
    N = n_m * K
    log_std = np.array([LOG_STDS[m % len(LOG_STDS)] for m in range(K)], dtype=np.float32)
    ls_cols = np.repeat(log_std, n_m)
    mean_old = rng.standard_normal((T, N)).astype(np.float32)
    act = (mean_old + np.exp(ls_cols) * rng.standard_normal((T, N))).astype(np.float32)
    logp_old = np.empty((T, N), np.float32)
    for m in range(K):
        c = slice(m * n_m, (m + 1) * n_m)
        logp_old[:, c] = logp32(act[:, c], mean_old[:, c], log_std[m])
    mean_new = (mean_old + np.float32(shift)).astype(np.float32)
    loc = -50.0 if kind == "offset" else 0.0
    ret = (loc + rng.standard_normal((T, N))).astype(np.float32)
    if kind == "constant":
        ret[:] = np.float32(0.1)
    val = (loc + rng.standard_normal((T, N))).astype(np.float32)
    return {"T": T, "n_m": n_m, "K": K, "N": N, "row_step": row_step, "shift": shift, "kind": kind, "log_std": log_std, "act": act,
            "logp_old": logp_old, "mean_new": mean_new, "ret": ret, "val": val, "clip": CLIP}


def member(case, m, key):
    n_m = case["n_m"]
    return case[key][:, m * n_m:(m + 1) * n_m]


def member_reference(case, m):
    cols = [member(case, m, k) for k in ("act", "logp_old", "mean_new", "ret", "val")]
    return (reference(*cols, case["log_std"][m], case["clip"], case["row_step"]),
            bounds(*cols, case["log_std"][m], case["row_step"]))

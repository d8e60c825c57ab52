"""A numpy restatement of the contract of csrc/pcc_streams.hip (include/pcc_policy.h: pcc_rollout_noise_pop, pcc_sample_order_pop,
pcc_adv_standardise_pop), written from the header alone: its own Philox4x32-10 on Python integers (and the
same rounds on numpy arrays, held to the integer version), the Feistel walk, Box-Muller in float64 and the standardisation with
the kernel's order of sums.  tests/test_learner_streams_cpu.py checks the model's own properties; tests/test_learner_streams.py holds
the kernels to it."""
import numpy as np

M32 = 0xFFFFFFFF
M64 = 0xFFFFFFFFFFFFFFFF
TAG_NOISE, TAG_ORDER = 0x4E4F4953, 0x4F524452   # counter word 3: "NOIS", "ORDR"
ROUNDS = 6
WEYL = 0x9E3779B9


def philox4x32_10(ctr, key):
    """Philox4x32-10 (Salmon et al. 2011) on Python integers: four counter words, two key words -> four words."""
    c0, c1, c2, c3 = (int(x) & M32 for x in ctr)
    k0, k1 = (int(x) & M32 for x in key)
    for _ in range(10):
        p0, p1 = c0 * 0xD2511F53, c2 * 0xCD9E8D57
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return [c0, c1, c2, c3]


def philox_array(c0, c1, c2, c3, key):
    """The same rounds on uint64 arrays of 32-bit words (broadcast against each other): returns [..., 4] uint32."""
    c0, c1, c2, c3 = np.broadcast_arrays(*(np.asarray(c, dtype=np.uint64) & np.uint64(M32) for c in (c0, c1, c2, c3)))
    k0, k1 = int(key) & M32, (int(key) >> 32) & M32
    m = np.uint64(M32)
    for _ in range(10):
        p0, p1 = c0 * np.uint64(0xD2511F53), c2 * np.uint64(0xCD9E8D57)
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & m, (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & m
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def key_from_seed(seed):
    """A learner's 64-bit key: the splitmix64 finaliser of seed + the golden-ratio increment (pcc_rl_amd.streams.key_from_seed)."""
    z = (int(seed) + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


# ------------------------------------------------------------------------------------------------------------------- noise
def noise_words(key, iteration, T, n_m):
    """uint32 [T][n_m]: local env e of step t takes word e & 3 of the block with counter (e >> 2, t, iteration, TAG_NOISE)."""
    q = np.arange((n_m + 3) // 4, dtype=np.uint64)
    w = philox_array(q[None, :], np.arange(T, dtype=np.uint64)[:, None], iteration, TAG_NOISE, key)   # [T][blocks][4]
    return w.reshape(T, -1)[:, :n_m]


def _sincos_2pi(b):
    """(sin, cos) of 2 pi b / 2^32 for uint32 b, the argument reduced in integers: the quadrant is b >> 30, the rest folds onto [0,
    pi / 4], where numpy's sin and cos of a rounded argument are good to an ulp or two of the RESULT (cos(2 pi u) on the unreduced
    angle is not: near its zeros the angle's rounding alone is several float32 spacings of the value)."""
    b = np.asarray(b, dtype=np.uint64)
    quad = (b >> np.uint64(30)).astype(np.int64)
    r = (b & np.uint64((1 << 30) - 1)).astype(np.int64)            # the angle within the quadrant: (pi / 2) r / 2^30
    fold = r > (1 << 29)
    rr = np.where(fold, (1 << 30) - r, r).astype(np.float64)       # <= 2^29: the angle (pi / 2) rr / 2^30 <= pi / 4
    ang = rr * (np.pi / 2.0 ** 31)
    s0, c0 = np.sin(ang), np.cos(ang)
    s, c = np.where(fold, c0, s0), np.where(fold, s0, c0)          # of the angle within the quadrant
    sin = np.choose(quad, [s, c, -s, -c])
    cos = np.choose(quad, [c, -s, -c, s])
    return sin, cos


def noise64(key, iteration, T, n_m):
    """float64 [T][n_m]: the normals before the one rounding to float32.  Per block, u1 = (w0 + 1) / 2^32 in (0, 1], r = sqrt(-2
    ln u1): envs 4 q and 4 q + 1 get r cos and r sin of 2 pi w1 / 2^32; envs 4 q + 2 and 4 q + 3 the same from (w2, w3)."""
    q = np.arange((n_m + 3) // 4, dtype=np.uint64)
    w = philox_array(q[None, :], np.arange(T, dtype=np.uint64)[:, None], iteration, TAG_NOISE, key).astype(np.float64)
    out = np.empty(w.shape, dtype=np.float64)
    for a in (0, 2):
        r = np.sqrt(-2.0 * np.log((w[..., a] + 1.0) * (1.0 / 4294967296.0)))
        s, c = _sincos_2pi(w[..., a + 1].astype(np.uint64))
        out[..., a], out[..., a + 1] = r * c, r * s
    return out.reshape(T, -1)[:, :n_m]


# ------------------------------------------------------------------------------------------------------------------- order
def half_bits(n):
    """h: the smallest even-bit domain 4^h >= n."""
    h = 0
    while (1 << (2 * h)) < n:
        h += 1
    return h


def fmix32(v):
    v = np.asarray(v, dtype=np.uint64)
    m = np.uint64(M32)
    v = v ^ (v >> np.uint64(16)); v = (v * np.uint64(0x85EBCA6B)) & m
    v = v ^ (v >> np.uint64(13)); v = (v * np.uint64(0xC2B2AE35)) & m
    return v ^ (v >> np.uint64(16))


def round_keys(key, iteration, epoch):
    w = philox4x32_10((epoch, 0, iteration, TAG_ORDER), (key & M32, (key >> 32) & M32))
    return [(w[r & 3] + r * WEYL) & M32 for r in range(ROUNDS)]


def feistel(x, h, rk):
    """The balanced 6-round network on 2 h bits, on a uint64 array."""
    mask = np.uint64((1 << h) - 1)
    L, R = x >> np.uint64(h), x & mask
    for r in range(ROUNDS):
        f = fmix32((R + np.uint64(rk[r])) & np.uint64(M32)) & mask
        L, R = R, L ^ f
    return (L << np.uint64(h)) | R


def order_local(key, iteration, epoch, n, with_walks=False):
    """int64 [n]: position i -> the local sample the walk from i ends at (the first value below n)."""
    h, rk = half_bits(n), round_keys(key, iteration, epoch)
    x = feistel(np.arange(n, dtype=np.uint64), h, rk)
    walks = np.ones(n, dtype=np.int64)
    while True:
        out = np.nonzero(x >= np.uint64(n))[0]
        if out.size == 0:
            break
        x[out] = feistel(x[out], h, rk)
        walks[out] += 1
    return (x.astype(np.int64), walks) if with_walks else x.astype(np.int64)


def order_global(keys, iteration, epoch, T, n_envs):
    """int64 [K][T n_m]: row m as indices t * n_envs + m * n_m + e into the flattened [T * n_envs] arrays."""
    K = len(keys)
    n_m = n_envs // K
    rows = []
    for m, key in enumerate(keys):
        j = order_local(key, iteration, epoch, T * n_m)
        rows.append((j // n_m) * n_envs + m * n_m + j % n_m)
    return np.stack(rows)


# ----------------------------------------------------------------------------------------------------------- standardisation
def _member_sum(cols):
    """The kernel's order for one member's float64 [T][n_m] terms: lane = env adds its T terms in step order from 0.0; a wavefront of
    64 lanes by the tree x[j] += x[j + d], j < d, d = 32 .. 1; a workgroup its 4 wavefronts in index order; then the workgroups'
    partials: sub-lane j of 256 adds [j per, j per + per), per = ceil(G / 256), in index order from 0.0, and the tree x[j] += x[j + s],
    j < s, s = 128 .. 1."""
    T, n_m = cols.shape
    G = (n_m + 255) // 256
    lane = np.zeros(G * 256, dtype=np.float64)
    for t in range(T):
        lane[:n_m] += cols[t]
    x = lane.reshape(G, 4, 64).copy()
    d = 32
    while d >= 1:
        x[..., :d] += x[..., d:2 * d]
        d >>= 1
    part = x[:, 0, 0].copy()
    for w in range(1, 4):
        part += x[:, w, 0]
    per = (G + 255) // 256
    sub = np.zeros(256, dtype=np.float64)
    for j in range(256):
        for g in range(min(j * per, G), min(j * per + per, G)):
            sub[j] += part[g]
    s = 128
    while s >= 1:
        sub[:s] += sub[s:2 * s]
        s >>= 1
    return sub[0]


def standardise(adv, n_members):
    """(out float32 [T][N], moments float64 [K][2] = {mean, var}): per member over its own columns, float64 throughout, two passes,
    out = float32((a - mean) / (sqrt(var) + 1e-8))."""
    adv = np.asarray(adv, dtype=np.float32)
    T, N = adv.shape
    n_m = N // n_members
    out, moments = np.empty((T, N), dtype=np.float32), np.empty((n_members, 2), dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        for m in range(n_members):
            a = adv[:, m * n_m:(m + 1) * n_m].astype(np.float64)
            n = float(T) * float(n_m)
            mean = _member_sum(a) / n
            d = a - mean
            var = np.float64(_member_sum(d * d)) / np.float64(n - 1.0)
            out[:, m * n_m:(m + 1) * n_m] = (d / (np.sqrt(var) + 1e-8)).astype(np.float32)
            moments[m] = mean, var
    return out, moments

"""Every on-device random draw of the library as an exact function of integers, in NumPy (uint64 / float64), written from the definitions in
csrc/ppo_kernels.hpp (splitmix64_dev, ctr_hash, ctr_normal, ctr_uniform), csrc/ppo_epoch.hpp (keyed_bijection, shuffle_row, storage_row /
storage_row_gathered, epoch_prepare_kernel) and csrc/ppo_hip.hip (ppo_seed, upload_epoch_keys, enqueue_epoch_index) -- and the comparison rules tests/test_counter_draws.py holds the device to.

Exploration noise.  A draw is keyed by (key, row, step, lane):
    ctr_hash(key, row, step, lane) = splitmix64(splitmix64(key << 32 | row) ^ (step << 32 | lane)) >> 32
    normal  column j: key ^ 0xA5A5A5A5, lanes 2j and 2j + 1;  u1 = ((h1 >> 8) + 1) / 2^24 in (0, 1],  u2 = (h2 >> 8) / 2^24 in [0, 1);  sqrt(-2 ln u1) cos(2 pi u2)
    uniform column j: key ^ 0x3C5A96C3, lane j;               ((h >> 8) + 0.5) / 2^24 in (0, 1)
ppo_step, rollout_act: key = seed_key(s) of the last seed(s), row = rank * n_envs + row, step = the handle's call counter.
collect_synthetic: key = its `seed` argument itself, row = env0 + e, step = step0 + t.

Epoch shuffle.  Epoch ep of update(.., seed) has the keys (k0, k1) = the two halves of splitmix64(seed + ep * golden); position p of the permuted order holds the
flattened env-major row r = keyed_bijection walked from p until it lands below B (cycle walking), over `bits` = the smallest value >= 1 with 2^bits >= B; the row
lies at (r % T) * E + r // T of the time-major rollout buffers.  Under dist_global_shuffle one permutation covers the B * world rows of all ranks."""
import numpy as np

U64 = np.uint64
M32 = 0xFFFFFFFF
M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
NORMAL_KEY = 0xA5A5A5A5
UNIFORM_KEY = 0x3C5A96C3
HALF_LOG_2PI = 0.9189385332046727
BOUND = 1e-3                 # |device normal - model|, elementwise (tests/test_counter_draws.py derives it)
NLP_RTOL = 2e-4
TIE = 2.0 ** -16             # a categorical row is compared only when its two largest allowed uniforms are at least this far apart


def _u64(x):
    return np.asarray(x).astype(np.uint64)


def splitmix64(x):
    """a Python int gives a Python int; anything else a uint64 array"""
    if isinstance(x, (int, np.integer)) and not isinstance(x, np.ndarray):
        x = (int(x) + GOLDEN) & M64
        x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
        x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
        return x ^ (x >> 31)
    with np.errstate(over="ignore"):
        x = _u64(x) + U64(GOLDEN)
        x = (x ^ (x >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> U64(27))) * U64(0x94D049BB133111EB)
        return x ^ (x >> U64(31))


def seed_key(s):
    """ppo_seed: the 32-bit key a handle draws under after seed(s)"""
    z = splitmix64(int(s) & M64)
    return (z ^ (z >> 32)) & M32


def ctr_hash(key, row, step, lane):
    """uint32 hashes (as uint64) of the broadcast arguments; each argument wraps to 32 bits as on the device"""
    a = (_u64(int(key) & M32) << U64(32)) | (_u64(row) & U64(M32))
    b = ((_u64(step) & U64(M32)) << U64(32)) | (_u64(lane) & U64(M32))
    return splitmix64(splitmix64(a) ^ b) >> U64(32)


def normals_from_hashes(h1, h2):
    u1 = ((h1 >> U64(8)).astype(np.float64) + 1.0) / 16777216.0
    u2 = (h2 >> U64(8)).astype(np.float64) / 16777216.0
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def uniforms_from_hash(h):
    return ((h >> U64(8)).astype(np.float64) + 0.5) / 16777216.0


def _grid(rows, step, A):
    rows = _u64(rows).reshape(-1, 1)
    step = np.broadcast_to(_u64(step).reshape(-1, 1), rows.shape) if np.ndim(step) else _u64(step)
    return rows, step, np.arange(A, dtype=np.uint64).reshape(1, -1)


def counter_normals(key, rows, step, A):
    """(eps [len(rows), A] float64, h1 >> 8 [len(rows), A]) of ctr_normal; step: one value or one per row"""
    r, s, j = _grid(rows, step, A)
    h1 = ctr_hash(key ^ NORMAL_KEY, r, s, U64(2) * j)
    h2 = ctr_hash(key ^ NORMAL_KEY, r, s, U64(2) * j + U64(1))
    return normals_from_hashes(h1, h2), h1 >> U64(8)


def counter_uniforms(key, rows, step, A):
    """u [len(rows), A] float64 of ctr_uniform"""
    r, s, j = _grid(rows, step, A)
    return uniforms_from_hash(ctr_hash(key ^ UNIFORM_KEY, r, s, j))


def gaussian_neglogp(eps):
    """neglogp of a unit-variance head whose action is the draw: 0.5 sum eps^2 + A log sqrt(2 pi)"""
    return 0.5 * (eps ** 2).sum(-1) + eps.shape[-1] * HALF_LOG_2PI


# ---- epoch shuffle ------------------------------------------------------------------------------------------------------------------------------------
def epoch_keys(seed, ep):
    """(k0, k1) of epoch ep: upload_epoch_keys"""
    z = splitmix64((int(seed) + GOLDEN * int(ep)) & M64)
    return z & M32, z >> 32


def shuffle_bits(B):
    bits = 1
    while (1 << bits) < B:
        bits += 1
    return bits


def keyed_bijection(x, bits, k0, k1):
    """a bijection of [0, 2^bits); x, k0, k1 broadcast (uint64 arrays holding 32-bit values: no product leaves 64 bits)"""
    mask = U64(M32 if bits >= 32 else (1 << bits) - 1)
    sh = U64(bits // 2 if bits > 1 else 1)
    k0, k1 = _u64(k0), _u64(k1)
    x = _u64(x)
    x = (x * (k0 | U64(1)) + k1) & mask; x = x ^ (x >> sh)
    x = (x * U64(0x9E3779B1) + (k0 >> U64(7))) & mask; x = x ^ (x >> sh)
    x = (x * (k1 | U64(1)) + U64(0x85EBCA6B)) & mask; x = x ^ (x >> sh)
    x = (x * U64(0xC2B2AE35) + k0) & mask; x = x ^ (x >> sh)
    return x


def walk(B, k0, k1):
    """[len(k0), B]: per key pair, position p -> the first iterate of the bijection below B"""
    bits = shuffle_bits(B)
    k0, k1 = _u64(k0).reshape(-1, 1), _u64(k1).reshape(-1, 1)
    x = keyed_bijection(np.broadcast_to(np.arange(B, dtype=np.uint64), (k0.shape[0], B)), bits, k0, k1)
    k0b, k1b = np.broadcast_to(k0, x.shape), np.broadcast_to(k1, x.shape)
    while True:
        out = x >= U64(B)
        if not out.any():
            return x.astype(np.int64)
        x = x.copy()
        x[out] = keyed_bijection(x[out], bits, k0b[out], k1b[out])


def epoch_perms(B, seeds, ep, keys=epoch_keys):
    ks = [keys(s, ep) for s in seeds]
    return walk(B, [k[0] for k in ks], [k[1] for k in ks])


def epoch_perm(B, seed, ep, keys=epoch_keys):
    """r[p]: the flattened env-major row (e * T + t) at position p of epoch ep's order"""
    return epoch_perms(B, [seed], ep, keys)[0]


def gidx_of(perm, E, T):
    """time-major storage row of the env-major row r"""
    perm = np.asarray(perm, np.int64)
    return (perm % T) * E + perm // T


def explicit_perm(perm):
    """the `perms` row that makes update() visit the rows in the order `perm` does: invert_perm_kernel stores inv[perms[i]] = i and position p reads inv[p], so
    perms[perm[p]] = p"""
    out = np.empty(len(perm), np.int32)
    out[np.asarray(perm)] = np.arange(len(perm), dtype=np.int32)
    return out


def global_gidx(E, T, nmb, world, rank, seed, ep, keys=epoch_keys, storage=gidx_of):
    """rank's gidx [B] under dist_global_shuffle: one permutation of the B * world rows r = e_global * T + t; global minibatch k is positions [k Mg, (k + 1) Mg), of
    which this rank trains [k Mg + rank M, k Mg + (rank + 1) M); a row lies at rs * T * E + t * E + e of the gathered [world][T][E] arrays"""
    B = E * T
    M, Mg = B // nmb, (B // nmb) * world
    perm = epoch_perm(B * world, seed, ep, keys)
    k, i = np.divmod(np.arange(B), M)
    r = perm[k * Mg + rank * M + i]
    eg, t = r // T, r % T
    rs, e = eg // E, eg % E
    return rs * T * E + storage(e * T + t, E, T)             # = rs T E + t E + e


# ---- comparison rules -----------------------------------------------------------------------------------------------------------------------------
def _where(idx, axes):
    return ", ".join("%s %d" % (n, i) for n, i in zip(axes, idx))


def compare_normals(got, model, axes=("row", "column"), what="draw", bound=BOUND, others=()):
    """|got - model| <= bound elementwise, and everything finite; returns the largest difference.  A failure names the first disagreeing index and, where one
    exists, the model index whose value the device's does match: in `model`, then in `others` [(name, array)] (the case's other steps, say)"""
    got, model = np.asarray(got, np.float64), np.asarray(model, np.float64)
    assert got.shape == model.shape, (what, got.shape, model.shape)
    assert np.isfinite(got).all(), "%s: not finite at (%s)" % (what, _where(np.argwhere(~np.isfinite(got))[0], axes))
    diff = np.abs(got - model)
    bad = np.argwhere(diff > bound)
    if bad.size:
        first = tuple(bad[0])
        src = "no value of the model in this case"
        for name, arr in ((what, model),) + tuple(others):
            hit = np.argwhere(np.abs(np.asarray(arr, np.float64) - got[first]) <= bound)
            if hit.size:
                src = "the model's value at (%s) of %s" % (_where(hit[0], axes), name)
                break
        raise AssertionError("%s: %d of %d differ by more than %g; first at (%s): device %.7g, model %.7g; the device's value is %s"
                             % (what, len(bad), diff.size, bound, _where(first, axes), got[first], model[first], src))
    return float(diff.max()) if diff.size else 0.0


def compare_neglogp(got, eps, what="neglogp"):
    np.testing.assert_allclose(got, gaussian_neglogp(np.asarray(eps, np.float64)), rtol=NLP_RTOL, atol=0, err_msg=what)


def component_offsets(A, nvec=None):
    return np.concatenate([[0], np.cumsum(nvec if nvec is not None else [A])]).astype(np.int64)


def expected_categories(u, mask=None, nvec=None):
    """equal logits: the category is argmax_j u_j over the allowed columns, per component.  (category [n, K], compared [n] bool, log of the allowed count summed over
    the components [n]); a row is left out when, in any component, its two largest allowed uniforms are closer than TIE"""
    u = np.asarray(u, np.float64)
    n, A = u.shape
    ok = np.ones((n, A), bool) if mask is None else np.asarray(mask) != 0
    off = component_offsets(A, nvec)
    cat = np.empty((n, len(off) - 1), np.int64)
    clear = np.ones(n, bool)
    nlp = np.zeros(n)
    for k in range(len(off) - 1):
        v = np.where(ok[:, off[k]:off[k + 1]], u[:, off[k]:off[k + 1]], -1.0)
        cat[:, k] = np.argmax(v, 1)
        if v.shape[1] > 1:
            top = np.sort(v, 1)[:, -2:]
            clear &= (top[:, 1] - top[:, 0] >= TIE) | (top[:, 0] < 0)
        nlp += np.log(ok[:, off[k]:off[k + 1]].sum(1))
    return cat, clear, nlp


def compare_categories(got, got_nlp, u, mask=None, nvec=None, what="category"):
    """integer equality on the compared rows, neglogp = log(allowed count) to 1e-5 on every row; returns the share of rows left out (at most 1 %)"""
    cat, clear, nlp = expected_categories(u, mask, nvec)
    got = np.asarray(got).reshape(cat.shape)
    left_out = 1.0 - clear.mean()
    assert left_out <= 0.01, "%s: %.4f of the rows are near-ties" % (what, left_out)
    assert np.all(got == np.floor(got)), what
    bad = np.argwhere((got != cat) & clear[:, None])
    if bad.size:
        i, k = bad[0]
        off = component_offsets(u.shape[1], nvec)
        j = off[k] + int(got[i, k])
        raise AssertionError("%s: %d rows differ; first at (row %d, component %d): device %d (u = %.8f), model %d (u = %.8f)"
                             % (what, len(np.unique(bad[:, 0])), i, k, int(got[i, k]), u[i, j] if 0 <= j < u.shape[1] else np.nan, cat[i, k],
                                u[i, off[k] + cat[i, k]]))
    if got_nlp is not None:
        np.testing.assert_allclose(got_nlp, nlp, rtol=0, atol=1e-5, err_msg=what + ": neglogp")
    return float(left_out)


def compare_gidx(got, want, what="gidx"):
    got, want = np.asarray(got).astype(np.int64), np.asarray(want, np.int64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    if bad.size:
        p = int(bad[0])
        perm = "a permutation" if sorted(got.tolist()) == list(range(len(got))) else "no permutation"
        at = np.flatnonzero(want == got[p])
        raise AssertionError("%s: %d of %d positions differ (the device's map is %s); first at position %d: device %d, model %d; the model holds the device's row at %s"
                             % (what, bad.size, got.size, perm, p, got[p], want[p], "position %d" % at[0] if at.size else "no position"))

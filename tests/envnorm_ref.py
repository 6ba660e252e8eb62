"""The float64 model, the dtype emulation, the inputs and the fault models of tests/test_envnorm_trained.py: EnvNormalize::step and RunningStatistics::update at
TRAINED statistics, in every kernel that restates them.

Every other test of the normaliser starts from norm_init (mean 0, variance 1, count 1e-6) and feeds U(-1, 1) or N(0.5, 2) for a few steps.  There a one-pass
sum of squares, an eps outside the square root, a count that stops at 2^24 or a reward clipped before it is scaled all give the right numbers.  The cases
below start from statistics a long run leaves behind (CASES) and are run by every form of the library (tests/test_envnorm_trained.py).

Model (the judge).  Written from the reference's headers, common/running_statistics.hpp:26-104 and env/env_normalize.hpp:64-116; it shares no code with
oracle/ppo_oracle.c.  NumPy float64, the batch mean and the sum of squared deviations by their definitions with math.fsum (two passes), Chan's merge with the
running (mean, var, count), count = n + count; observations clip((x - mean) / sqrt(var + eps), +-clip_obs) after the update when training; rewards
ret = ret * gamma + r, the update of the return statistics, clip(r / sqrt(ret_var + eps), +-clip_rew), ret *= 1 - done; the frozen path (training=False) and
the two flags.  It is fed the float32 inputs and the float32 initial state the device gets.

Emulation (NOT a reference).  Emu(dtype, order, fault) is the same sequence at a chosen dtype in rs_merge's operand order (csrc/ppo_envnorm.hpp), with a
choice of the batch summation: "sequential" (the Gaussian narrow kernels' column loop), "tree" (chunk_moments / nw_chunk_moments_lds: enqueue_norm_batch's
chunk deal, a thread's first 8 rows pairwise and the rest in turn, the fixed tree over the row sweeps, combine_group / combine_single_column over the chunks)
and "cgroup" (obs_cgroup_job: row splits, 16 row-subs, the lane-exchange tree, the splits combined in the same shape).  At float64 it reproduces the model to
1e-12 of each output's largest magnitude; at float32 it is the stand-in for a correct kernel; with fault= it is the stand-in for a wrong one (FAULTS).

Bounds (bounds()).  Per case, per output (normalised observations, rewards, mean, variance) and per column block: err32 = the largest |float32 emulation -
model| over the three orders, bound = FACTOR x err32 (FACTOR = 10 = head_edges_ref.PART2_FACTOR = bf16_ref.RATE_FACTOR), element by element never tighter than
tests/test_hip_parity.py's tolerances for the same quantity (2e-5 |x| + 2e-6 for observations and rewards, 1e-5 |x| + 1e-6 for the statistics), computed
for the test's own E, O and inputs.  Counts are compared exactly, as doubles.

MEASURED err32 (tests/test_envnorm_trained.py::test_measured_emulation_errors_and_bounds prints the figure of every shape and block and holds this table to
the largest of them; the bound beside the floor is 10 x the figure; shapes: API (7, 18), (300, 18), (300, 64); host Env (1, 18), (8, 18), (16, 18), (40, 18),
(64, 40); device env (1, 18), (8, 18), (40, 18), (96, 18), (8, 80)):
    case          obs        rewards    obs_mean   obs_var    ret_mean   ret_var
    fresh         5.1e-05    2.5e-07    4.1e-08    1.2e-07    9.1e-08    1.8e-07
    long_run      3.4e-07    2.4e-07    1.8e-14    9.6e-08    9.1e-15    3.3e-08
    offset        0.00012    4.3e-07    1.2e-06    7.8e-08    7.1e-08    3.4e-07
    shifted       2.9e-06    3.7e-07    1e-06      1.2e-06    3.4e-08    2.1e-07
    constant      3.7e-05    3.2e-07    3.6e-09    7.3e-08    5e-08      3.8e-07
    fast_var      1.2e-06    5e-07      4.7e-05    0.38       3.4e-08    1.5e-07
    ramp          9.2e-07    4.5e-07    2e-07      3.9e-07    2.5e-08    3.9e-07
    tiny_ret_var  5.2e-05    1e-06      5.3e-08    1.4e-07    1.8e-14    3.5e-13
    huge_rewards  5.1e-05    4.1e-07    6.4e-08    1.3e-07    2.2e-06    0.17
The 5e-5 of the observations of `fresh`, `tiny_ret_var` and `huge_rewards` is the one-environment shape: after a first batch of one row on norm_init's count of
1e-6 the variance is 1e-6 (1 + x^2) and x - mean is the rounding of the mean times a scale of 1e3.  fast_var's 0.38 in the variance is its wide block (variance
1e6), huge_rewards' 0.17 a return variance of 1e6; `offset` loses 1e-4 in the observations to the float32 spacing of 1000 (6e-5) over a deviation of 0.01.
DEVICE figures (MI355X; per form the largest |device - model| of the normalised observations and of the rewards over the form's cases, and the largest
|error| / bound of any output with where it occurred; 0.1 = the device's error is the emulation's err32 itself, as where a kernel sums in an emulated order):
    form                     cases  obs       rewards   error / bound
    api_e7                   9      1.1e-05   1.7e-07   0.1    (obs of offset)
    api_e300                 9      4.5e-05   2.5e-07   0.1    (obs of constant)
    api_cgroups_e300_o64     9      0.00012   8.2e-07   0.1    (obs of offset)
    dev_e1                   5      5.1e-05   1.1e-07   0.1    (obs of fresh)
    dev_e1_no_rollout1       5      5.1e-05   1.1e-07   0.1    (obs of fresh)
    dev_e8                   5      2e-06     1.8e-07   0.023  (obs of fresh)
    dev_e40                  5      1.9e-06   3.6e-07   0.022  (obs_var of long_run)
    dev_e8_no_persistent     5      2e-06     1.8e-07   0.023  (obs of fresh)
    dev_e96                  5      1.5e-06   3.7e-07   0.026  (obs_var of shifted)
    dev_o80_e8               5      2.9e-06   2.1e-07   0.025  (obs_var of shifted)
    host_e1                  9      5.2e-05   4e-07     0.1    (obs of fresh)
    host_e8                  9      1.3e-05   5.1e-07   0.1    (obs of offset)
    host_e40                 9      2.9e-05   2.9e-07   0.1    (obs of offset)
    host_e8_no_resident      9      1.3e-05   5.1e-07   0.1    (obs of offset)
    host_e8_no_fused         9      1.3e-05   2.3e-07   0.1    (obs of offset)
    host_256_e16             9      2.4e-05   4.1e-07   0.1    (obs of offset)
    host_fused_cat_e8        9      1.3e-05   5.1e-07   0.1    (obs of offset)
    resident_dev_e8          5      2e-06     1.8e-07   0.019  (obs_var of shifted)
    resident_host_e8         9      1.3e-05   2.3e-07   0.1    (obs of offset)
    resident_host_e64_o40    9      4.4e-05   3.5e-07   0.1    (obs of constant)
Every count was exact and every form enqueued the kernels its name stands for.  No kernel failed a case.

The fp32 count.  A count kept in float32 is caught by the exact-count assertion in EVERY case, `fresh` included (float32(1e-6 + 8) is not the double
8.000001; tests/test_hip_parity.py's `c == nz.obs_rms.count` catches that too).  What the usual regime does not show is the count that stops growing: the
VALUES of the float_count fault pass the `fresh` control and all its counts are within one float32 ulp; at 2^30 the count stands still.
"""
import functools
import math

import numpy as np

GAMMA, CLIP_OBS, CLIP_REW, EPS = 0.99, 10.0, 10.0, 1e-8         # PPOHip.norm_init's defaults = env_normalize.hpp's
FACTOR = 10.0                   # head_edges_ref.PART2_FACTOR / bf16_ref.RATE_FACTOR
MARGIN = 10.0                   # a fault must miss an assertion of its case by this many bounds
STEPS, T = 6, 3                 # six env steps = two rollouts of three
ORDERS = ("sequential", "tree", "cgroup")
TOL = {"obs": (2e-5, 2e-6), "rewards": (2e-5, 2e-6), "obs_mean": (1e-5, 1e-6), "obs_var": (1e-5, 1e-6), "ret_mean": (1e-5, 1e-6), "ret_var": (1e-5, 1e-6)}
BLOCKED = ("obs", "obs_mean", "obs_var")                         # outputs with a column axis (the last one): err32 per column block
COUNTS = ("obs_count", "ret_count")
FAULTS = ("one_pass_m2", "eps_outside_sqrt", "no_count_in_delta_term", "no_between_chunk_term", "float_count", "stale_istd", "stale_istd_init", "clip_before_scale")
REJECTED_BY = {"one_pass_m2": "offset", "eps_outside_sqrt": "constant", "no_count_in_delta_term": "shifted", "no_between_chunk_term": "ramp",
               "float_count": "long_run", "stale_istd": "fast_var", "stale_istd_init": "fast_var", "clip_before_scale": "tiny_ret_var"}
GAP_FAULTS = ("one_pass_m2", "eps_outside_sqrt", "float_count", "clip_before_scale")      # the `fresh` control must not notice them
CASES = ("fresh", "long_run", "offset", "shifted", "constant", "fast_var", "ramp", "tiny_ret_var", "huge_rewards")
DEVICE_CASES = ("fresh", "long_run", "shifted", "fast_var", "tiny_ret_var")               # an initial state only: the device env draws its own U(-1, 1)
ENV_SEED = 1234
INIT = (0.0, 1.0, 1e-6)         # norm_init: running_statistics.hpp:17-21

# test_measured_emulation_errors_and_bounds: the largest err32 over the shapes named in the docstring, per case and output
MEASURED = {
    "fresh":        {"obs": 5.1e-05, "rewards": 2.5e-07, "obs_mean": 4.1e-08, "obs_var": 1.2e-07, "ret_mean": 9.1e-08, "ret_var": 1.8e-07},
    "long_run":     {"obs": 3.4e-07, "rewards": 2.4e-07, "obs_mean": 1.8e-14, "obs_var": 9.6e-08, "ret_mean": 9.1e-15, "ret_var": 3.3e-08},
    "offset":       {"obs": 0.00012, "rewards": 4.3e-07, "obs_mean": 1.2e-06, "obs_var": 7.8e-08, "ret_mean": 7.1e-08, "ret_var": 3.4e-07},
    "shifted":      {"obs": 2.9e-06, "rewards": 3.7e-07, "obs_mean": 1e-06, "obs_var": 1.2e-06, "ret_mean": 3.4e-08, "ret_var": 2.1e-07},
    "constant":     {"obs": 3.7e-05, "rewards": 3.2e-07, "obs_mean": 3.6e-09, "obs_var": 7.3e-08, "ret_mean": 5e-08, "ret_var": 3.8e-07},
    "fast_var":     {"obs": 1.2e-06, "rewards": 5e-07, "obs_mean": 4.7e-05, "obs_var": 0.38, "ret_mean": 3.4e-08, "ret_var": 1.5e-07},
    "ramp":         {"obs": 9.2e-07, "rewards": 4.5e-07, "obs_mean": 2e-07, "obs_var": 3.9e-07, "ret_mean": 2.5e-08, "ret_var": 3.9e-07},
    "tiny_ret_var": {"obs": 5.2e-05, "rewards": 1e-06, "obs_mean": 5.3e-08, "obs_var": 1.4e-07, "ret_mean": 1.8e-14, "ret_var": 3.5e-13},
    "huge_rewards": {"obs": 5.1e-05, "rewards": 4.1e-07, "obs_mean": 6.4e-08, "obs_var": 1.3e-07, "ret_mean": 2.2e-06, "ret_var": 0.17},
}


# ---- cases ---------------------------------------------------------------------------------------------------------------------------------------
def _u(rng, shape):
    return rng.uniform(-1.0, 1.0, shape)


# per case: the return statistics' initial state, the count of the observation statistics (None: the environment count) and the column blocks
# (mean0, var0, generator of [steps, E, columns])
def _table(name, E):
    n = lambda scale, loc=0.0: (lambda rng, shape: loc + scale * rng.normal(size=shape))
    srt = lambda sign: (lambda rng, shape: sign * np.sort(rng.normal(size=shape), axis=1))
    const = lambda rng, shape: np.full(shape, 7.0002)
    rew, third = _u, float(np.float32(1.0 / 3.0))
    if name == "fresh":
        ret, cnt, blocks = INIT, INIT[2], [(0.0, 1.0, _u)]
    elif name == "long_run":
        ret, cnt, blocks = (0.0, third, 2.0 ** 30), 2.0 ** 30, [(0.0, third, _u)]
    elif name == "offset":
        ret, cnt, blocks = INIT, 1e6, [(1000.0, 1e-4, n(0.01, 1000.0)), (-1000.0, 1e-4, n(0.01, -1000.0)), (0.0, third, _u)]
    elif name == "shifted":
        ret, cnt, blocks = INIT, 1e4, [(5.0, 0.3, _u), (-5.0, 0.3, _u)]
    elif name == "constant":
        ret, cnt, blocks = INIT, 1e8, [(7.0, 0.0, const), (0.0, third, _u)]
    elif name == "fast_var":
        ret, cnt, blocks = INIT, 4.0, [(0.0, 1e-4, n(1.0)), (0.0, 1e-4, n(1e3))]
    elif name == "ramp":
        ret, cnt, blocks = INIT, float(E), [(0.0, 1.0, srt(1.0)), (0.0, 1.0, srt(-1.0))]
    elif name == "tiny_ret_var":
        ret, cnt, blocks = (0.0, 1e-10, 2.0 ** 30), INIT[2], [(0.0, 1.0, _u)]
    elif name == "huge_rewards":
        ret, cnt, blocks, rew = (0.0, 1e6, 1e4), INIT[2], [(0.0, 1.0, _u)], n(1e3)
    else:
        raise KeyError(name)
    return ret, cnt, blocks, rew


class Case:
    """name, E, O, source ("rows": the table's inputs; "env": the seeded env's, the table's initial state), obs0 / ret0 = (mean, var, count) with float32 means and
    variances, blocks [(c0, c1)], reset_raw [E, O], steps [(raw [E, O], rew [E], done [E])] x (STEPS + 1): the last one is the frozen step of the API forms"""

    def __init__(self, name, E, O, source="rows"):
        self.name, self.E, self.O, self.source = name, E, O, source
        ret, cnt, blocks, rew = _table(name, E)
        if source == "env" and name == "fast_var":
            blocks = blocks[:1]                                  # without its wide block: the env's observations are U(-1, 1) in every column
        nb = len(blocks)
        self.blocks = [(b * O // nb, (b + 1) * O // nb) for b in range(nb)]
        assert all(c1 > c0 for c0, c1 in self.blocks)
        rng = np.random.RandomState([CASES.index(name), E, O])   # fixed: the MEASURED figures can be reproduced
        mean0, var0 = np.empty(O, np.float32), np.empty(O, np.float32)
        raw = np.empty((STEPS + 2, E, O), np.float32)
        for (c0, c1), (m, v, gen) in zip(self.blocks, blocks):
            mean0[c0:c1], var0[c0:c1] = m, v
            raw[:, :, c0:c1] = gen(rng, (STEPS + 2, E, c1 - c0)).astype(np.float32)
        rews = rew(rng, (STEPS + 1, E)).astype(np.float32)
        dones = (rng.uniform(size=(STEPS + 1, E)) < 0.1).astype(np.float32)
        self.obs0 = (mean0, var0, float(cnt))
        self.ret0 = (np.full(1, ret[0], np.float32), np.full(1, ret[1], np.float32), float(ret[2]))
        if source == "env":
            from oracle import oracle as o
            self.reset_raw = o.seeded_env_step(ENV_SEED, 0, E, 0, O)[0]
            self.steps = [o.seeded_env_step(ENV_SEED, 0, E, k + 1, O) for k in range(STEPS + 1)]
        else:
            self.reset_raw = raw[0]
            self.steps = [(raw[k + 1], rews[k], dones[k]) for k in range(STEPS + 1)]


@functools.lru_cache(maxsize=None)
def make_case(name, E, O, source="rows"):
    return Case(name, E, O, source)


# ---- the model -------------------------------------------------------------------------------------------------------------------------------------
class Model:
    """one handle's EnvNormalize in float64"""

    def __init__(self, case, norm_obs=True, norm_rew=True, gamma=GAMMA, clip_obs=CLIP_OBS, clip_rew=CLIP_REW, eps=EPS):
        f = lambda a: np.array(a, np.float64)
        self.om, self.ov, self.oc = f(case.obs0[0]), f(case.obs0[1]), float(case.obs0[2])
        self.rm, self.rv, self.rc = f(case.ret0[0]), f(case.ret0[1]), float(case.ret0[2])
        self.ret = np.zeros(case.E, np.float64)
        self.norm_obs, self.norm_rew, self.gamma, self.clip_obs, self.clip_rew, self.eps = norm_obs, norm_rew, gamma, clip_obs, clip_rew, eps

    @staticmethod
    def update(mean, var, count, batch):                         # running_statistics.hpp:26-35, 88-104
        n = batch.shape[0]
        bmean = np.array([math.fsum(c) / n for c in batch.T])                         # :37-40
        dev = batch - bmean
        bvar = np.array([math.fsum(c * c) for c in dev.T]) / n                        # :42-54
        delta, tot = bmean - mean, count + n                                          # :90-92
        mean1 = mean + delta * n / tot                                                # :94
        m2 = var * count + bvar * n + delta * delta * count * n / tot                 # :97-100
        return mean1, m2 / tot, n + count                                             # :101-103

    def obs(self, x, training=True):                             # env_normalize.hpp:94-109
        x = np.asarray(x, np.float64)
        if not self.norm_obs:
            return x.copy()
        if training:
            self.om, self.ov, self.oc = self.update(self.om, self.ov, self.oc, x)
        return np.clip((x - self.om) / np.sqrt(self.ov + self.eps), -self.clip_obs, self.clip_obs)

    def reward(self, r, d, training=True):                       # env_normalize.hpp:64-91
        r, d = np.asarray(r, np.float64), np.asarray(d, np.float64)
        self.ret = self.ret * self.gamma + r                                           # :71
        y = r.copy()
        if self.norm_rew:
            if training:
                self.rm, self.rv, self.rc = self.update(self.rm, self.rv, self.rc, self.ret[:, None])
            y = np.clip(r / np.sqrt(self.rv[0] + self.eps), -self.clip_rew, self.clip_rew)
        self.ret = self.ret * (1.0 - d)                                                # :88
        return y

    def stats(self):
        return dict(obs_mean=self.om.copy(), obs_var=self.ov.copy(), obs_count=self.oc, ret_mean=self.rm[0], ret_var=self.rv[0], ret_count=self.rc)


# ---- the emulation ---------------------------------------------------------------------------------------------------------------------------------
def _pow2_ceil(x):
    p = 1
    while p < x:
        p <<= 1
    return p


def _strided_tree(vals, lanes, first8, zero):
    """chunk_moments' / combine_group's sum over the first axis of vals [n, D]: lane l of `lanes` adds items l, l + lanes, ... (first8: the first eight pairwise,
    ((0 + 1) + (2 + 3)) + ((4 + 5) + (6 + 7)), the rest in turn; else all in turn from zero), then the fixed tree over the lanes.  Items past the end are zeros."""
    n, D = vals.shape
    nu = max(8 if first8 else 1, -(-n // lanes))
    pad = np.zeros((nu * lanes, D), vals.dtype)
    pad[:n] = vals
    v = pad.reshape(nu, lanes, D)
    if first8:
        s = ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]))
        rest = range(8, nu)
    else:
        s = np.full((lanes, D), zero, vals.dtype)
        rest = range(nu)
    for u in rest:
        s = s + v[u]
    h = _pow2_ceil(lanes) >> 1
    while h > 0:
        k = min(h, lanes - h)
        if k > 0:
            s[:k] = s[:k] + s[h:h + k]
        h >>= 1
    return s[0]


def _quad_tree(vals, first8):
    """obs_cgroup_job's sum: 16 row-subs (item i to sub i % 16, the first eight pairwise and the rest in turn, or all in turn from zero), the four subs of a wave as
    (0 + 1) + (2 + 3), the four waves the same way"""
    n, D = vals.shape
    nu = max(8 if first8 else 1, -(-n // 16))
    pad = np.zeros((nu * 16, D), vals.dtype)
    pad[:n] = vals
    v = pad.reshape(nu, 16, D)
    if first8:
        s = ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]))
        rest = range(8, nu)
    else:
        s = np.zeros((16, D), vals.dtype)
        rest = range(nu)
    for u in rest:
        s = s + v[u]
    w = s.reshape(4, 4, D)
    w = (w[:, 0] + w[:, 1]) + (w[:, 2] + w[:, 3])
    return (w[0] + w[1]) + (w[2] + w[3])


def rows_per_chunk(rows, D):
    """enqueue_norm_batch's row-chunk deal (nw_nb_rows_per_chunk restates it in csrc/ppo_narrow.hpp)"""
    g = max(1, min(256 if D <= 32 else 64, (rows * D + 2047) // 2048))
    g = min(g, rows)
    return -(-rows // g)


def rows_per_reward_chunk(rows):
    g = max(1, min(64, (rows + 1023) // 1024))
    return -(-(-(-rows // g)) // 32) * 32


def rows_per_split(rows):
    """enqueue_norm_batch's row splits of the column-group form (one 64-column group)"""
    s = min((rows + 127) // 128, 128)
    return -(-rows // s)


class Emu:
    """the model's sequence at `dtype`, rs_merge's operand order, one of ORDERS for the batch sums, optionally one of FAULTS"""

    def __init__(self, case, dtype, order="sequential", fault=None, norm_obs=True, norm_rew=True, gamma=GAMMA, clip_obs=CLIP_OBS, clip_rew=CLIP_REW, eps=EPS):
        assert order in ORDERS and (fault is None or fault in FAULTS)
        dt = self.dt = np.dtype(dtype).type
        f = lambda a: np.array(a, dt)
        self.om, self.ov, self.oc = f(case.obs0[0]), f(case.obs0[1]), float(case.obs0[2])
        self.rm, self.rv, self.rc = f(case.ret0[0]), f(case.ret0[1]), float(case.ret0[2])
        if fault == "float_count":
            self.oc, self.rc = np.float32(self.oc), np.float32(self.rc)
        self.ret = np.zeros(case.E, dt)
        self.order, self.fault, self.norm_obs, self.norm_rew = order, fault, norm_obs, norm_rew
        self.gamma, self.clip_obs, self.clip_rew, self.eps = dt(gamma), dt(clip_obs), dt(clip_rew), dt(eps)

    # -- the batch moments: (mean [D], sum of squared deviations [D]) --
    def _chunk(self, x, kind):
        dt = self.dt
        n = dt(x.shape[0])
        if kind == "sequential":
            s = np.zeros(x.shape[1], dt)
            for r in x:
                s = s + r
            bm = s / n
            q = np.zeros(x.shape[1], dt)
            for r in x:
                d = r - bm
                q = q + d * d
            return bm, q
        if kind == "tree":
            lanes = 256 // x.shape[1]
            bm = _strided_tree(x, lanes, True, dt(0)) / n
            d = x - bm
            return bm, _strided_tree(d * d, lanes, True, dt(0))
        bm = _quad_tree(x, True) / n
        d = x - bm
        return bm, _quad_tree(d * d, True)

    def _moments(self, x, reward_job=False):
        dt, rows, D = self.dt, x.shape[0], x.shape[1]
        if self.fault == "one_pass_m2":                          # M2 = sum x^2 - n mean^2
            s, s2 = np.zeros(D, dt), np.zeros(D, dt)
            for r in x:
                s, s2 = s + r, s2 + r * r
            bm = s / dt(rows)
            return bm, s2 - dt(rows) * (bm * bm)
        if self.order == "sequential":
            return self._chunk(x, "sequential")
        if self.order == "tree":
            rpc = rows_per_reward_chunk(rows) if reward_job else rows_per_chunk(rows, D)
        else:
            rpc = rows_per_split(rows)
        kind = "tree" if (self.order == "tree" or reward_job) else "cgroup"      # the reward job has the one form
        if reward_job and self.order == "cgroup":
            rpc = rows_per_reward_chunk(rows)
        sets = [(dt(min(rows, r0 + rpc) - r0),) + self._chunk(x[r0:min(rows, r0 + rpc)], kind) for r0 in range(0, rows, rpc)]
        nk = np.array([s[0] for s in sets], dt)[:, None]
        mk, qk = np.stack([s[1] for s in sets]), np.stack([s[2] for s in sets])
        K = len(sets)
        if kind == "tree" and reward_job:                        # combine_single_column: a wave's tree over 64 lanes
            nn = dt(0)
            for k in range(K):
                nn = nn + nk[k, 0]
            tree = lambda v: _strided_tree(v, 64, False, dt(0))
        elif kind == "tree":                                     # combine_group
            nn = dt(0)
            for k in range(K):
                nn = nn + nk[k, 0]
            tree = lambda v: _strided_tree(v, 256 // D, False, dt(0))
        else:                                                    # obs_cgroup_job's last split
            nn = dt(rows)
            tree = lambda v: _quad_tree(v, False)
        bm = tree(nk * mk) / nn
        d = mk - bm
        between = nk * (d * d)
        if self.fault == "no_between_chunk_term":
            between = between * dt(0)
        return bm, tree(qk + between)

    def _merge(self, mean0, var0, cnt, bmean, bM2, n):           # rs_merge (csrc/ppo_envnorm.hpp), the caller's count
        dt = self.dt
        if self.fault == "float_count":
            tot = np.float32(cnt + np.float32(n))
            new_cnt = np.float32(np.float32(n) + cnt)
        else:
            tot = cnt + float(n)
            new_cnt = float(n) + cnt
        nb, c, t = dt(n), dt(cnt), dt(tot)
        bvar = bM2 / nb
        delta = bmean - mean0
        mean1 = mean0 + (delta * nb) / t
        m_a, m_b = var0 * c, bvar * nb
        cross = (((delta * delta) * c) * nb) / t
        if self.fault == "no_count_in_delta_term":
            cross = ((delta * delta) * nb) / t
        return mean1, (m_a + m_b + cross) / t, new_cnt

    def _istd(self, var):
        dt = self.dt
        with np.errstate(invalid="ignore", divide="ignore"):     # (a fault model's variance may be negative: its outputs are then non-finite, which worst() counts)
            if self.fault == "eps_outside_sqrt":
                return dt(1) / (np.sqrt(var) + self.eps)
            return dt(1) / np.sqrt(var + self.eps)

    def _scale_var(self, var, before):
        if self.fault == "stale_istd":
            return before
        if self.fault == "stale_istd_init":
            return np.ones_like(var)
        return var

    def obs(self, x, training=True):
        x = np.asarray(x, self.dt)
        if not self.norm_obs:
            return x.copy()
        before = self.ov
        if training:
            bm, q = self._moments(x)
            self.om, self.ov, self.oc = self._merge(self.om, self.ov, self.oc, bm, q, x.shape[0])
        y = (x - self.om) * self._istd(self._scale_var(self.ov, before))
        return np.minimum(np.maximum(y, -self.clip_obs), self.clip_obs)

    def reward(self, r, d, training=True):
        dt = self.dt
        r, d = np.asarray(r, dt), np.asarray(d, dt)
        self.ret = self.ret * self.gamma + r
        y = r.copy()
        if self.norm_rew:
            before = self.rv
            if training:
                bm, q = self._moments(self.ret[:, None], reward_job=True)
                self.rm, self.rv, self.rc = self._merge(self.rm, self.rv, self.rc, bm, q, r.shape[0])
            inv = self._istd(self._scale_var(self.rv, before))[0]
            if self.fault == "clip_before_scale":
                y = np.minimum(np.maximum(r, -self.clip_rew), self.clip_rew) * inv
            else:
                y = r * inv
                y = np.minimum(np.maximum(y, -self.clip_rew), self.clip_rew)
        self.ret = self.ret * (dt(1) - d)
        return y

    def stats(self):
        return dict(obs_mean=self.om.copy(), obs_var=self.ov.copy(), obs_count=float(self.oc), ret_mean=self.rm[0], ret_var=self.rv[0], ret_count=float(self.rc))


def dt(n):
    return dt(n)


class COracle:
    """oracle.Normalizer (the fp32 C restatement) behind the same three calls, preset through RunningStats.mean / .var / .count"""

    def __init__(self, case):
        from oracle import oracle as o
        self.nz = o.Normalizer(case.E, case.O, gamma=GAMMA, clip_obs=CLIP_OBS, clip_rew=CLIP_REW, eps=EPS)
        for rms, st in ((self.nz.obs_rms, case.obs0), (self.nz.ret_rms, case.ret0)):
            rms.mean[:], rms.var[:], rms.count = st[0], st[1], st[2]

    def obs(self, x, training=True):
        self.nz.training = training
        return self.nz.obs(x)

    def reward(self, r, d, training=True):
        self.nz.training = training
        return self.nz.reward(r, d)

    def stats(self):
        a, b = self.nz.obs_rms, self.nz.ret_rms
        return dict(obs_mean=a.mean.copy(), obs_var=a.var.copy(), obs_count=a.count, ret_mean=b.mean[0], ret_var=b.var[0], ret_count=b.count)


# ---- one handle's sequence --------------------------------------------------------------------------------------------------------------------------
def run(nz, case, mode):
    """mode "api": norm_obs / norm_reward per step, STEPS training steps and one frozen step; the statistics after steps T, 2 T and after the frozen step.
    mode "rollout": the reset's batch, then two rollouts of T steps: obs [STEPS, E, O] = the rollouts' observation rows (row 0 of the second rollout is the state
    carried over), rewards [STEPS, E], the statistics after each rollout.  -> {name: float64 array}"""
    obs, rews, stats = [], [], []
    if mode == "api":
        for k in range(STEPS + 1):
            raw, rew, dn = case.steps[k]
            obs.append(nz.obs(raw, k < STEPS)); rews.append(nz.reward(rew, dn, k < STEPS))
            if k in (T - 1, STEPS - 1, STEPS):
                stats.append(nz.stats())
    else:
        cur = nz.obs(case.reset_raw)
        for k in range(STEPS):
            obs.append(cur)
            raw, rew, dn = case.steps[k]
            cur = nz.obs(raw); rews.append(nz.reward(rew, dn))
            if (k + 1) % T == 0:
                stats.append(nz.stats())
    out = {"obs": np.array(obs, np.float64), "rewards": np.array(rews, np.float64)}
    for key in stats[0]:
        out[key] = np.array([s[key] for s in stats], np.float64)
    return out


def expected_counts(case, mode):
    """count0 + E x batches, batch by batch in double as RunningStatistics::update adds them (:103)"""
    oc, rc, o_out, r_out = case.obs0[2], case.ret0[2], [], []
    if mode == "rollout":
        oc = float(case.E) + oc
    for k in range(STEPS):
        oc, rc = float(case.E) + oc, float(case.E) + rc
        if (k + 1) % T == 0:
            o_out.append(oc); r_out.append(rc)
    if mode == "api":
        o_out.append(oc); r_out.append(rc)
    return np.array(o_out), np.array(r_out)


def _block_max(key, case, a):
    """the largest entry of a >= 0 per column block (BLOCKED outputs) or overall"""
    if key in BLOCKED:
        return [float(a[..., c0:c1].max()) for c0, c1 in case.blocks]
    return [float(a.max())]


def _spread(key, case, per_block, shape):
    out = np.empty(shape)
    if key in BLOCKED:
        for (c0, c1), e in zip(case.blocks, per_block):
            out[..., c0:c1] = e
    else:
        out[...] = per_block[0]
    return out


@functools.lru_cache(maxsize=None)
def bounds(name, E, O, source, mode):
    """(the model's outputs, {output: elementwise bound}, {output: [err32 per block]}) for this shape and these inputs"""
    case = make_case(name, E, O, source)
    want = run(Model(case), case, mode)
    assert all(np.isfinite(v).all() for v in want.values()), name
    err = {}
    for order in ORDERS:
        got = run(Emu(case, np.float32, order), case, mode)
        for key in TOL:
            e = _block_max(key, case, np.abs(got[key] - want[key]))
            err[key] = [max(a, b) for a, b in zip(err.get(key, [0.0] * len(e)), e)]
    bound = {}
    for key, (rtol, atol) in TOL.items():
        bound[key] = np.maximum(FACTOR * _spread(key, case, err[key], want[key].shape), rtol * np.abs(want[key]) + atol)
    return want, bound, err


def worst(got, want, bound):
    """{output: the largest |got - want| / bound} (a non-finite output counts as infinite) and whether both counts are the model's, exactly"""
    ratios = {}
    for key in TOL:
        g = np.asarray(got[key], np.float64)
        assert g.shape == want[key].shape, (key, g.shape, want[key].shape)
        r = np.abs(g - want[key]) / bound[key]
        ratios[key] = float(np.where(np.isfinite(g), r, np.inf).max())
    counts_ok = all(np.array_equal(np.asarray(got[key], np.float64), want[key]) for key in COUNTS)
    return ratios, counts_ok


def errors(got, want):
    return {key: float(np.abs(np.asarray(got[key], np.float64) - want[key]).max()) for key in TOL}


def check(got, name, E, O, source, mode, what=""):
    """every assertion of a (form, case): each output inside its bound, element by element and none left out; the counts exactly the model's, which are
    count0 + E x batches.  -> (the largest |error| per output, the largest |error| / bound per output)"""
    case = make_case(name, E, O, source)
    want, bound, _ = bounds(name, E, O, source, mode)
    oc, rc = expected_counts(case, mode)
    assert np.array_equal(want["obs_count"], oc) and np.array_equal(want["ret_count"], rc), (want["obs_count"], oc, want["ret_count"], rc)
    for key in COUNTS:
        g = np.asarray(got[key], np.float64)
        assert np.array_equal(g, want[key]), "%s %s %s: %r, expected exactly %r" % (what, name, key, g.tolist(), want[key].tolist())
    ratios, _ = worst(got, want, bound)
    errs = errors(got, want)
    for key in TOL:
        assert ratios[key] <= 1.0, "%s %s %s: largest |error| %.3g = %.3g x its bound (smallest bound %.3g)" % (
            what, name, key, errs[key], ratios[key], float(bound[key].min()))
    return errs, ratios

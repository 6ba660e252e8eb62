"""Every on-device random draw against the exact counter model of tests/counter_draws_ref.py: the exploration noise of every kernel that calls ctr_normal /
ctr_uniform (each computes row, step and lane its own way) and the keyed epoch shuffle of update(perms=None).

The handles are set up so that the action IS the draw: init_orthogonal (the hidden layers stay non-trivial), then pi/w = 0, pi/b = 0 and, Gaussian, pi/logstd = 0.
A Gaussian action is then eps itself (the mean is exactly 0, on the bf16 path too); with equal logits the sampled category is argmax_j u_j over the allowed columns.

The Gaussian bound |action - model| <= 1e-3 comes from what it must tell apart, not from the device: a wrong index gives an independent normal, and two independent
normals lie within 1e-3 of each other with probability 2e-3 / sqrt(4 pi) < 6e-4 per draw, so none of a case's >= 1000 draws' worth of blocks would pass; the genuine
error is that of __logf, __cosf and sqrtf in fp32.  Categorical rows whose two largest allowed uniforms are closer than 2^-16 are left out (the fp32 Gumbel transform
may order them either way); a case may leave out 1 % of its rows, and the CPU tests show from the model alone that every case stays inside that.

The same check functions take a deliberately wrong model in place of the device (CPU, test_comparator_rejects_*): every mutation the GPU tests exist to catch is
rejected on every case where it changes an index at all.

OBSERVED on an MI355X: see OBSERVED below.
"""
import collections
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import counter_draws_ref as M
from tests.masked_categorical_ref import random_masks
from tests.multi_categorical_ref import random_masks as multi_random_masks
from tests.test_rollout_forms import CASES as ROLLOUT_CASES
from tests.test_rollout_forms import GOLDEN as ROLLOUT_GOLDEN
from tests.test_rollout_forms import set_switches

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

OBSERVED = """
    Gaussian draws, largest |action - model| per case (bound 1e-3; nothing above 1e-4, nothing above 2e-6):
      ppo_step, zero head, rows 1 / 63 / 65 / 200, steps 0, 1, 2 and 0 again: 9.5e-7 at A = 1 and 1.47e-6 at A = 18, 33, 64 -- the same figures for
        policy_step_kernel behind (4, 5) and (256, 256), narrow_step_kernel behind (64, 64) and bf16_step_sequence behind (256, 128)
      ppo_step behind ordinary weights, 200 x 18: generic (4, 5) 1.27e-6, generic (256, 256) 1.22e-6, narrow 1.25e-6, bf16 1.26e-6
      collect_synthetic, T = 5, env0 0 / 4096, step0 0 / 1000, two rollouts each: 1.61e-6 for dev_256_e16, dev_e8, dev_e40, dev_e96, dev_e8_no_persistent,
        dev_e96_no_persistent, dev_o80_e8 and dev_e100_ragged_coop; 1.65e-6 for dev_e333_ragged_coop; 1.06e-6 for the one-environment cases dev_e1, dev_e1_no_rollout1
        and dev_e1_a32 (dev_e1_a2 draws the first two columns of dev_e1's rows: no more than that)
      host Env, two rollouts of T = 3 around one with explicit noise: host_e1 7.6e-7; host_e8, host_e8_no_fused, host_e8_no_resident 8.1e-7; host_e40, host_256_e16,
        host_256_e16_no_direct 1.06e-6; host_256_e80 1.24e-6
      the two edge draws: 1.13e-6 over both 64 x 18 blocks; [10, 4] of seed 28160 is 0, [6, 6] of seed 3283 is -5.6562662 (model -5.6562668)
      two ranks: 1.23e-6
    categorical rows left out as near-ties: 0 for cat_generic, cat_shape_kernels and cat_bf16_head, with and without masks, and for the two masked host-Env cases;
      multi_categorical ([3, 2, 5, 7]): one row of 200 (0.005) in one block, with and without masks; allowed 1 %
    epoch shuffle: all 9 maps (1, 2, 3 epochs x seeds 0, 7, 2^40 + 3) exact on each of the seven shapes, 6 of the 9 from a graph replay; explicit permutations built
      from the model reproduce the device shuffle bit for bit on the six fp32 shapes; the global map of two ranks exact
"""

CR = 0.16102319955825806
LR = 0.000393141177482903
GAMMA, LAM = 0.99, 0.95
BF16 = 1
U64 = np.uint64


# =====================================================================================================================================================
# the model with every index open to replacement, blocks of draws, and the checks both the GPU tests and the mutation tests go through
# =====================================================================================================================================================
class Model:
    """tests/counter_draws_ref.py with every index it uses open to replacement: the defaults are the library's; a mutant replaces one"""

    def __init__(self, lane1=lambda j: U64(2) * j, lane2=lambda j: U64(2) * j + U64(1), step=lambda s: s, row=lambda base, r: base + r,
                 nkey=M.NORMAL_KEY, ukey=M.UNIFORM_KEY, key_ep=lambda ep: ep, storage=M.gidx_of):
        self.lane1, self.lane2, self.step, self.row, self.nkey, self.ukey, self.key_ep, self.storage = lane1, lane2, step, row, nkey, ukey, key_ep, storage

    def _grid(self, base, n, A):
        return np.asarray(self.row(base, np.arange(n))).astype(np.uint64).reshape(-1, 1), np.arange(A, dtype=np.uint64).reshape(1, -1)

    def normals(self, key, base, n, step, A):
        r, j = self._grid(base, n, A)
        return M.normals_from_hashes(M.ctr_hash(key ^ self.nkey, r, self.step(step), self.lane1(j)), M.ctr_hash(key ^ self.nkey, r, self.step(step), self.lane2(j)))

    def uniforms(self, key, base, n, step, A):
        r, j = self._grid(base, n, A)
        return M.uniforms_from_hash(M.ctr_hash(key ^ self.ukey, r, self.step(step), j))

    def keys(self, seed, ep):
        return M.epoch_keys(seed, self.key_ep(ep))

    def gidx(self, E, T, seed, ep):
        return self.storage(M.epoch_perm(E * T, seed, ep, self.keys), E, T)

    def global_gidx(self, E, T, nmb, world, rank, seed, ep):
        return M.global_gidx(E, T, nmb, world, rank, seed, ep, self.keys, self.storage)


MODEL = Model()
MUTANTS = {
    "lane 2j becomes j": Model(lane1=lambda j: j),
    "lane 2j+1 becomes 2j": Model(lane2=lambda j: U64(2) * j),
    "step becomes 0": Model(step=lambda s: 0),
    "row offset dropped": Model(row=lambda base, r: r),
    "key constants swapped": Model(nkey=M.UNIFORM_KEY, ukey=M.NORMAL_KEY),
    "ep + 1 becomes ep in the keys": Model(key_ep=lambda ep: ep - 1),
    "storage row transposed": Model(storage=lambda perm, E, T: np.asarray(perm, np.int64)),      # e * T + t, the env-major row itself
}

# one launch's draws: n rows from `base`, one step; kind "normal" [n, A] or "uniform" (categories of `nvec`, or one of A, under `mask`)
Block = collections.namedtuple("Block", "label kind key base n step A nvec mask")


def draws(b, m=MODEL):
    return (m.normals if b.kind == "normal" else m.uniforms)(b.key, b.base, b.n, b.step, b.A)


def as_device(b, m):
    """(action, neglogp) a device that drew like `m` would hand back for block b, in float32"""
    d = draws(b, m)
    if b.kind == "normal":
        return d.astype(np.float32), M.gaussian_neglogp(d).astype(np.float32)
    cat, _, nlp = M.expected_categories(d, b.mask, b.nvec)
    return cat.astype(np.float32), nlp.astype(np.float32)


def check_blocks(blocks, got):
    """got: [(action, neglogp or None)] in block order.  Returns (largest Gaussian difference, largest share of categorical rows left out)"""
    model = [draws(b) for b in blocks]
    worst, left = 0.0, 0.0
    for i, (b, (a, nlp)) in enumerate(zip(blocks, got)):
        if b.kind == "normal":
            others = tuple((blocks[k].label, model[k]) for k in range(len(blocks)) if k != i and model[k].shape == model[i].shape)
            worst = max(worst, M.compare_normals(np.asarray(a).reshape(model[i].shape), model[i], what=b.label, others=others))
            if nlp is not None:
                M.compare_neglogp(nlp, model[i], what=b.label + ": neglogp")
        else:
            left = max(left, M.compare_categories(a, nlp, model[i], b.mask, b.nvec, what=b.label))
    return worst, left


def check_gidx(E, T, got):
    """got: {(epochs, seed): the gidx words after update(.., epochs, .., seed)}: the LAST epoch's map"""
    for (epochs, seed), words in sorted(got.items()):
        M.compare_gidx(np.asarray(words)[:E * T], MODEL.gidx(E, T, seed, epochs - 1), what="gidx after %d epochs, seed %d" % (epochs, seed))


# ---- the cases ------------------------------------------------------------------------------------------------------------------------------------------------
ROWS = (1, 63, 65, 200)
WIDTHS = (1, 18, 33, 64)
# Gaussian ppo_step families: (hidden, observations, constructor keywords, the kernel_counts name that must have served every step)
GAUSS = {
    "generic_4_5": ((4, 5), 80, {}, "policy_step_kernel"),               # 80 observations: past the narrow family's 64 columns
    "generic_256": ((256, 256), 18, {}, "policy_step_kernel"),
    "narrow_64": ((64, 64), 18, {}, "narrow_step_kernel"),               # <static> at A = 18, <runtime> at the other widths
    "bf16": ((256, 128), 18, dict(compute_dtype=BF16), "bf16_step_sequence"),
}
NVEC = [3, 2, 5, 7]            # (ppo_create_multi refuses a component of one category: every n_k >= 2)
CAT_ROWS = (1, 65, 200)
# discrete ppo_step families: (hidden, A, constructor keywords, kernel name without / with a mask)
DISCRETE = {
    "cat_generic": ((256, 256), 18, dict(action_dist="categorical"), "policy_step_kernel<cat>", "policy_step_kernel<cat,mask>"),
    "cat_shape_kernels": ((64, 64), 18, dict(action_dist="categorical", shape_kernels=True), "narrow_step_kernel<cat>", "narrow_step_kernel<cat,mask>"),
    "cat_bf16_head": ((256, 128), 18, dict(action_dist="categorical", bf16_head=True, compute_dtype=BF16), "bf16_step_sequence<cat>", "bf16_step_sequence<cat,mask>"),
    "multi_categorical": ((64, 64), 17, dict(action_dist="multi_categorical", nvec=NVEC), "policy_step_kernel<mcat>", "policy_step_kernel<mcat,mask>"),
}
STEP_SEED = 5


def gauss_step_blocks(A):
    """per row count: seed(s), three drawing calls (steps 0, 1, 2; calls that do not draw lie between them), seed(s) again, one more (step 0)"""
    out = []
    for n in ROWS:
        key = M.seed_key(STEP_SEED + n)
        out += [Block("n=%d A=%d call %d (step %d)" % (n, A, c, s), "normal", key, 0, n, s, A, None, None) for c, s in enumerate((0, 1, 2, 0))]
    return out


def step_mask(name, n, masked):
    if not masked:
        return None
    rng = np.random.RandomState(100 + n)
    mask = multi_random_masks(rng, n, NVEC) if name == "multi_categorical" else random_masks(rng, n, DISCRETE[name][1])
    return mask           # half of the categories open; the first row: a single open category (per component)


def discrete_step_blocks(name, masked):
    A = DISCRETE[name][1]
    nvec = NVEC if name == "multi_categorical" else None
    out = []
    for n in CAT_ROWS:
        key = M.seed_key(STEP_SEED + n)
        out += [Block("%s n=%d step %d" % (name, n, s), "uniform", key, 0, n, s, A, nvec, step_mask(name, n, masked)) for s in (0, 1)]
    return out


DEV_T = 5
DEV_KEY = 0xC0FFEE              # collect_synthetic's seed argument IS the key
DEV_CASES = {k: dict(c, A=18) for k, c in ROLLOUT_CASES.items() if c["side"] == "dev"}
DEV_CASES.update({
    "dev_e100_ragged_coop": dict(side="dev", hidden=(64, 64), E=100, O=18, env=(), A=18),            # four row groups, the last with 4 live rows
    "dev_e333_ragged_coop": dict(side="dev", hidden=(64, 64), E=333, O=18, env=(), A=18),            # eleven, the last with 13
    "dev_e1_a2": dict(side="dev", hidden=(64, 64), E=1, O=18, env=(), A=2),                          # (padded to the 32 columns of the compile-time shape like 18)
    "dev_e1_a32": dict(side="dev", hidden=(64, 64), E=1, O=18, env=(), A=32),                        # every lane of ppo_rollout1.hpp's half wave
})
# the kernel_counts names the first rollout of the added cases must show (the cases of tests/test_rollout_forms.py: its golden table)
DEV_FORMS = {"dev_e100_ragged_coop": "narrow_rollout_coop_kernel", "dev_e333_ragged_coop": "narrow_rollout_coop_kernel", "dev_e1_a2": "narrow_rollout1_kernel",
             "dev_e1_a32": "narrow_rollout1_kernel"}
DEV_STARTS = [(0, 0), (4096, 0), (0, 1000), (4096, 1000)]          # (env0, step0)


def dev_blocks(name):
    c = DEV_CASES[name]
    return [Block("%s env0=%d step0=%d rollout %d t=%d" % (name, env0, step0, it, t), "normal", DEV_KEY, env0, c["E"], step0 + it * DEV_T + t, c["A"], None, None)
            for env0, step0 in DEV_STARTS for it in range(2) for t in range(DEV_T)]


HOST_T = 3
HOST_SEED = 99
HOST_CASES = {k: c for k, c in ROLLOUT_CASES.items() if c["side"] == "host" and not c["noise"]}


def host_masks(name):
    """[2 rollouts][T] masks of a case that passes them, else None"""
    c = HOST_CASES[name]
    if not c["mask"]:
        return None
    rng = np.random.RandomState(17)
    out = (rng.uniform(size=(2, HOST_T, c["E"], 18)) < 0.5).astype(np.float32)
    out[..., 0] = 1.0
    out[:, :, 0, :] = 0.0; out[:, :, 0, 5] = 1.0          # the first environment: a single open category
    return out


def host_blocks(name):
    """two rollouts after seed(99): steps 0 .. 5 in call order (the rollout with explicit noise between them draws nothing)"""
    c = HOST_CASES[name]
    masks = host_masks(name)
    kind = "normal" if c["dist"] == "gaussian" else "uniform"
    return [Block("%s rollout %d t=%d" % (name, it, t), kind, M.seed_key(HOST_SEED), 0, c["E"], it * HOST_T + t, 18, None, None if masks is None else masks[it, t])
            for it in range(2) for t in range(HOST_T)]


# the epoch shuffle: (hidden, switches set to 1, E, T, minibatches, constructor keywords, O, the kernel_counts name the update must show)
SHUFFLE = {
    "resident_epoch": ((64, 64), (), 1, 512, 8, {}, 18, "narrow_epoch_kernel"),
    "narrow_per_step": ((64, 64), ("PPO_HIP_NO_NARROW_EPOCH",), 16, 16, 4, {}, 18, "narrow_train_kernel<static>"),
    "fast_pair": ((256, 256), (), 64, 16, 4, {}, 18, "train8_kernel"),
    "generic_ragged_walk": ((16, 8, 8), ("PPO_HIP_NO_NARROW",), 3, 37, 3, {}, 18, "train_fwd_bwd_kernel"),      # B = 111 of 128: cycle walking, a ragged last thread stride
    "seven_rows": ((64, 64), (), 1, 7, 7, {}, 18, None),
    "one_row": ((64, 64), (), 1, 1, 1, {}, 18, None),
    # beyond the issue's table: the bf16 path stages its epoch separately, so its map comes from epoch_prepare_kernel's single-rank branch (exact map and replay only)
    "bf16_prepare_kernel": ((512, 512), (), 64, 8, 4, dict(compute_dtype=BF16), 64, "bf16_train_sequence"),
}
SHUFFLE_SWITCHES = ("PPO_HIP_NO_NARROW_EPOCH", "PPO_HIP_NO_NARROW", "PPO_HIP_NO_GRAPH")
SHUFFLE_SEEDS = (0, 7, 2 ** 40 + 3)
SHUFFLE_EPOCHS = (1, 2, 3)

DP_E, DP_T, DP_NMB, DP_SEED, DP_EPOCHS, DP_SHUFFLE_SEED = 16, 4, 4, 3, 2, 11


def dp_blocks(rank):
    """one rank of two: the zero-head collect_synthetic(env0 = rank * E) and one ppo_step of E rows (row_base = rank * n_envs)"""
    out = [Block("rank %d rollout t=%d" % (rank, t), "normal", DEV_KEY, rank * DP_E, DP_E, t, 18, None, None) for t in range(DP_T)]
    return out + [Block("rank %d ppo_step" % rank, "normal", M.seed_key(DP_SEED), rank * DP_E, DP_E, 0, 18, None, None)]


def all_draw_cases():
    """{case id: blocks} of every GPU test of this module that compares draws"""
    cases = {"step A=%d" % A: gauss_step_blocks(A) for A in WIDTHS}
    for name in DISCRETE:
        for masked in (False, True):
            cases["%s%s" % (name, " masked" if masked else "")] = discrete_step_blocks(name, masked)
    cases.update({name: dev_blocks(name) for name in DEV_CASES})
    cases.update({name: host_blocks(name) for name in HOST_CASES})
    cases.update({"two ranks, rank %d" % r: dp_blocks(r) for r in (0, 1)})
    return cases


# =====================================================================================================================================================
# CPU: the model's own statistics
# =====================================================================================================================================================
def test_model_wrapper_is_the_reference_module():
    key = M.seed_key(5)
    np.testing.assert_array_equal(MODEL.normals(key, 7, 40, 3, 18), M.counter_normals(key, 7 + np.arange(40), 3, 18)[0])
    np.testing.assert_array_equal(MODEL.uniforms(key, 7, 40, 3, 18), M.counter_uniforms(key, 7 + np.arange(40), 3, 18))
    np.testing.assert_array_equal(MODEL.gidx(3, 37, 7, 1), M.gidx_of(M.epoch_perm(111, 7, 1), 3, 37))
    assert M.splitmix64(0) == 0xE220A8397B1DCDAF                      # the published first output of splitmix64 seeded with 0
    np.testing.assert_array_equal(M.splitmix64(np.array([0], np.uint64)), np.array([0xE220A8397B1DCDAF], np.uint64))


def test_normal_moments():
    """65536 x 18 draws under seed_key(5).  Bounds: four standard errors of each sample moment of N = 1,179,648 independent N(0,1) draws -- mean 1/sqrt(N) = 9.2e-4,
    standard deviation 1/sqrt(2N) = 6.5e-4, third moment sqrt(15/N) = 3.6e-3, fourth sqrt(96/N) = 9.0e-3"""
    e, _ = M.counter_normals(M.seed_key(5), np.arange(65536), 0, 18)
    mean, std, m3, m4 = e.mean(), e.std(), (e ** 3).mean(), (e ** 4).mean()
    print("mean %.2e std %.5f third %.2e fourth %.4f" % (mean, std, m3, m4))
    assert abs(mean) < 3.7e-3 and abs(std - 1) < 2.6e-3 and abs(m3) < 1.5e-2 and abs(m4 - 3) < 3.6e-2
    assert np.isfinite(e).all()


def test_normal_kolmogorov_smirnov():
    from scipy import stats
    e, _ = M.counter_normals(M.seed_key(5), np.arange(65536), 0, 18)
    p = stats.kstest(e.reshape(-1)[:200000], "norm").pvalue
    print("KS p-value %.3f" % p)
    assert p > 0.01


def test_normal_draws_are_uncorrelated():
    n = 65536
    e0, _ = M.counter_normals(M.seed_key(5), np.arange(n), 0, 18)
    e1, _ = M.counter_normals(M.seed_key(5), np.arange(n), 1, 18)
    e6, _ = M.counter_normals(M.seed_key(6), np.arange(n), 0, 18)

    def corr(x, y):
        return float(np.corrcoef(x.reshape(-1), y.reshape(-1))[0, 1])
    got = {"adjacent rows": corr(e0[:-1], e0[1:]), "adjacent columns": corr(e0[:, :-1], e0[:, 1:]), "steps 0 and 1": corr(e0, e1), "seeds 5 and 6": corr(e0, e6)}
    print(got)
    for k, v in got.items():
        assert abs(v) < 0.01, (k, v)


def test_the_two_edge_draws():
    """the two ends of u1 under step 0, 64 rows, A = 18: seed 3283 has h1 >> 8 == 0 (u1 = 2^-24, the largest radius sqrt(48 ln 2) = 5.768) at [6, 6], seed 28160
    has 0xFFFFFF (u1 = 1, radius exactly 0) at [10, 4]"""
    e, h = M.counter_normals(M.seed_key(3283), np.arange(64), 0, 18)
    assert int(h[6, 6]) == 0 and np.isfinite(e).all()
    u2 = float(M.ctr_hash(M.seed_key(3283) ^ M.NORMAL_KEY, 6, 0, 13) >> U64(8)) / 16777216.0
    assert e[6, 6] == pytest.approx(np.sqrt(48 * np.log(2.0)) * np.cos(2 * np.pi * u2), rel=1e-12) and abs(e[6, 6]) > 5
    assert np.sqrt(48 * np.log(2.0)) == pytest.approx(5.768, abs=1e-3)
    e, h = M.counter_normals(M.seed_key(28160), np.arange(64), 0, 18)
    assert int(h[10, 4]) == 0xFFFFFF and e[10, 4] == 0.0 and np.isfinite(e).all()


@pytest.mark.parametrize("B,nmb", [(2048, 32), (333, 3), (64, 4), (1000, 8), (7, 7), (2, 1), (1, 1)])
def test_shuffle_statistics(B, nmb):
    from scipy import stats
    seeds = range(2000)
    S, Mb = len(seeds), B // nmb
    p0 = M.epoch_perms(B, seeds, 0)
    assert np.array_equal(np.sort(p0, 1), np.broadcast_to(np.arange(B), (S, B))), "not a permutation"
    pos = np.argsort(p0, 1)                                   # pos[s, r]: where row r lands
    mb = pos // Mb
    if nmb > 1:
        for r in sorted({0, min(1, B - 1), B // 2, B - 1}):
            counts = np.bincount(mb[:, r], minlength=nmb)
            p = stats.chisquare(counts).pvalue
            print("B %d row %d chi-square p %.3f" % (B, r, p))
            assert p > 1e-3, (r, counts)
    if B > 1:
        co, want = float((mb[:, :-1] == mb[:, 1:]).mean()), (Mb - 1) / (B - 1)
        print("B %d co-membership %.5f expected %.5f" % (B, co, want))
        assert abs(co - want) <= 0.05 * want
    fixed = float((p0 == np.arange(B)).sum(1).mean())
    print("B %d fixed points %.3f" % (B, fixed))
    assert 0.8 <= fixed <= 1.2
    if B >= 64:
        agree = float((p0 == M.epoch_perms(B, seeds, 1)).mean())
        print("B %d epochs 0 and 1 agree at %.5f of the positions" % (B, agree))
        assert agree <= 4.0 / B


def test_explicit_perm_orientation():
    """invert_perm_kernel stores inv[perms[i]] = i and position p of the epoch reads row inv[p]: the `perms` row built from the model's order reproduces it"""
    perm = M.epoch_perm(111, 7, 1)
    perms = M.explicit_perm(perm)
    inv = np.empty(111, np.int64)
    inv[perms] = np.arange(111)
    np.testing.assert_array_equal(inv, perm)
    assert sorted(perms.tolist()) == list(range(111)) and not np.array_equal(perms, perm)


def test_global_map_is_a_partition_of_the_gathered_rows():
    both = np.concatenate([MODEL.global_gidx(DP_E, DP_T, DP_NMB, 2, r, DP_SHUFFLE_SEED, 1) for r in (0, 1)])
    assert sorted(both.tolist()) == list(range(2 * DP_E * DP_T))


def test_every_categorical_case_stays_inside_the_exclusion_cap():
    """from the model alone: no case leaves out more than 1 % of its rows as near-ties (expected share about A 2^-16 = 2.7e-4 at 18 categories)"""
    worst = 0.0
    for name, blocks in all_draw_cases().items():
        for b in blocks:
            if b.kind == "uniform":
                _, clear, _ = M.expected_categories(draws(b), b.mask, b.nvec)
                worst = max(worst, 1.0 - clear.mean())
                assert 1.0 - clear.mean() <= 0.01, b.label
    print("largest share of rows left out: %.4f" % worst)


# ---- the comparator's power -----------------------------------------------------------------------------------------------------------------------------
def mutation_changes(mutation, blocks):
    """does the mutation move any index of these blocks at all (where it does not, the mutant IS the model on this case)"""
    normal = [b for b in blocks if b.kind == "normal"]
    return {"lane 2j becomes j": any(b.A >= 2 for b in normal),                         # 2 * 0 == 0: a one-column head has no lane to confuse
            "lane 2j+1 becomes 2j": bool(normal),
            "step becomes 0": any(b.step != 0 for b in blocks),
            "row offset dropped": any(b.base != 0 for b in blocks),                     # ppo_step and the host Env on one rank have none
            "key constants swapped": True}[mutation]


@pytest.mark.parametrize("mutation", ["lane 2j becomes j", "lane 2j+1 becomes 2j", "step becomes 0", "row offset dropped", "key constants swapped"])
def test_comparator_rejects_a_mutated_draw_on_every_case(mutation):
    m = MUTANTS[mutation]
    rejected = 0
    for name, blocks in all_draw_cases().items():
        fake = [as_device(b, m) for b in blocks]
        if mutation_changes(mutation, blocks):
            with pytest.raises(AssertionError):
                check_blocks(blocks, fake)
            rejected += 1
        else:
            for b, (a, _) in zip(blocks, fake):
                np.testing.assert_array_equal(a, as_device(b, MODEL)[0], err_msg=b.label)
            check_blocks(blocks, fake)
    assert rejected >= 8, rejected
    # the row offset is carried by the device-env rollouts started at env0 = 4096 and by the second of two ranks
    if mutation == "row offset dropped":
        assert rejected == len(DEV_CASES) + 1


def test_comparator_accepts_the_model_itself_and_names_the_source_of_a_wrong_step():
    blocks = gauss_step_blocks(18)
    worst, _ = check_blocks(blocks, [as_device(b, MODEL) for b in blocks])
    assert worst < 1e-6                                       # float32 rounding of the model's own values
    shifted = [as_device(b._replace(step=b.step + 1), MODEL) for b in blocks]
    with pytest.raises(AssertionError, match=r"first at \(row 0, column 0\).*the model's value at \(row 0, column 0\) of n=1 A=18 call 1 \(step 1\)"):
        check_blocks(blocks, shifted)


def shuffle_shapes():
    return sorted({(E, T) for _, _, E, T, _, _, _, _ in SHUFFLE.values()}) + [(DP_E, DP_T)]


@pytest.mark.parametrize("mutation", ["ep + 1 becomes ep in the keys", "storage row transposed"])
def test_comparator_rejects_a_mutated_shuffle_on_every_shape(mutation):
    m = MUTANTS[mutation]
    rejected = 0
    for E, T in shuffle_shapes():
        fake = {(ep, s): m.gidx(E, T, s, ep - 1) for ep in SHUFFLE_EPOCHS for s in SHUFFLE_SEEDS}
        # one row has one order; a single environment (or a single step) stores row r at r under either formula
        changes = E * T > 1 if mutation.startswith("ep") else (E > 1 and T > 1)
        if changes:
            with pytest.raises(AssertionError):
                check_gidx(E, T, fake)
            rejected += 1
        else:
            check_gidx(E, T, fake)
    assert rejected >= 3
    with pytest.raises(AssertionError):                        # and the global map of two ranks
        M.compare_gidx(m.global_gidx(DP_E, DP_T, DP_NMB, 2, 1, DP_SHUFFLE_SEED, 1), MODEL.global_gidx(DP_E, DP_T, DP_NMB, 2, 1, DP_SHUFFLE_SEED, 1))


def test_compare_gidx_says_what_kind_of_map_it_got():
    want = MODEL.gidx(16, 16, 7, 0)
    with pytest.raises(AssertionError, match="the device's map is a permutation"):
        M.compare_gidx(MODEL.gidx(16, 16, 8, 0), want)
    with pytest.raises(AssertionError, match="no permutation"):
        M.compare_gidx(np.zeros(256, np.int64), want)


# =====================================================================================================================================================
# GPU
# =====================================================================================================================================================
def zero_head(g, seed=0):
    """init_orthogonal, then a policy head that adds nothing to the draw"""
    g.init_orthogonal(seed)
    named = {n: g.get_tensor(n).copy() for n, _ in g.tensors}
    for n in ("pi/w", "pi/b", "pi/logstd"):
        if n in named:
            named[n][:] = 0.0
    g.set_tensors(named)
    assert np.abs(g.get_tensor("pi_fc0/w")).max() > 0
    return g


def observed(case, worst=None, left=None):
    print("OBSERVED %-40s%s%s" % (case, "" if worst is None else " max |action - model| %.3g" % worst, "" if left is None else " rows left out %.4f" % left))


def counts_delta(before, after):
    return {k: int(after[k] - before.get(k, 0)) for k in after if after[k] != before.get(k, 0)}


@gpu
@pytest.mark.parametrize("A", WIDTHS)
@pytest.mark.parametrize("family", sorted(GAUSS))
def test_gaussian_step_draws(family, A):
    import ppo_cpp_amd
    hidden, O, kw, kernel = GAUSS[family]
    g = zero_head(ppo_cpp_amd.PPOHip(O, A, list(hidden), **kw))
    rng = np.random.RandomState(1)
    got, draws_made = [], 0
    for n in ROWS:
        obs = rng.uniform(-1, 1, (n, O)).astype(np.float32)
        g.seed(STEP_SEED + n)
        a, _, nlp = g.step(obs); got.append((a, nlp))
        g.value(obs)
        a, _, nlp = g.step(obs); got.append((a, nlp))
        g.act_deterministic(obs)
        g.step(obs, rng.normal(size=(n, A)).astype(np.float32))                  # explicit noise: draws nothing
        a, _, nlp = g.step(obs); got.append((a, nlp))
        g.seed(STEP_SEED + n)
        a, _, nlp = g.step(obs); got.append((a, nlp))
    kc = g.kernel_counts()
    g.close()
    served = {k: c for k, c in kc.items() if c and ("step" in k)}
    assert served and all(k.startswith(kernel) for k in served), (family, A, served)
    worst, _ = check_blocks(gauss_step_blocks(A), got)
    observed("ppo_step %s A=%d" % (family, A), worst)


@gpu
@pytest.mark.parametrize("family", sorted(GAUSS))
def test_gaussian_step_draws_behind_ordinary_weights(family):
    """the weights of tests/test_hip_parity.pair (logstd in [-1, 0.2]): eps recovered as (a - act_deterministic(obs)) / exp(logstd); the fp32 rounding of a and mu
    adds about 2e-6 at logstd >= -1, the bound stays"""
    import ppo_cpp_amd
    from oracle import oracle as o
    hidden, O, kw, kernel = GAUSS[family]
    A, n = 18, 200
    orc = o.Oracle(O, A, list(hidden)); orc.init_orthogonal(3)
    orc.tensor("pi/logstd")[:] = np.random.RandomState(4).uniform(-1.0, 0.2, (1, A))
    g = ppo_cpp_amd.PPOHip(O, A, list(hidden), **kw)
    g.set_flat(orc.theta)
    obs = np.random.RandomState(2).uniform(-1, 1, (n, O)).astype(np.float32)
    g.seed(STEP_SEED)
    a, _, _ = g.step(obs)
    mu = g.act_deterministic(obs)
    sigma = np.exp(g.get_tensor("pi/logstd").astype(np.float64)).reshape(1, A)
    g.close()
    assert np.abs(mu).max() > 1e-3
    z = (a.astype(np.float64) - mu) / sigma
    worst, _ = check_blocks([Block("%s ordinary weights" % family, "normal", M.seed_key(STEP_SEED), 0, n, 0, A, None, None)], [(z, None)])
    observed("ppo_step %s ordinary weights" % family, worst)


@gpu
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("family", sorted(DISCRETE))
def test_discrete_step_draws(family, masked):
    import ppo_cpp_amd
    hidden, A, kw, k_plain, k_mask = DISCRETE[family]
    g = zero_head(ppo_cpp_amd.PPOHip(18, A, list(hidden), **kw))
    rng = np.random.RandomState(1)
    got = []
    for n in CAT_ROWS:
        obs = rng.uniform(-1, 1, (n, 18)).astype(np.float32)
        mask = step_mask(family, n, masked)
        if masked:
            assert (mask.reshape(n, -1).sum(1) >= 1).all() and mask[0].sum() == (len(NVEC) if family == "multi_categorical" else 1)
        g.seed(STEP_SEED + n)
        for s in (0, 1):
            a, _, nlp = g.step(obs, mask=mask)
            got.append((a, nlp))
            g.act_deterministic(obs, mask=mask)
    kc = g.kernel_counts()
    g.close()
    assert kc[k_mask if masked else k_plain] >= 2 * len(CAT_ROWS), kc
    _, left = check_blocks(discrete_step_blocks(family, masked), got)
    observed("ppo_step %s%s" % (family, " masked" if masked else ""), left=left)


@gpu
@pytest.mark.parametrize("name", sorted(DEV_CASES))
def test_device_env_rollout_draws(name, monkeypatch):
    import ppo_cpp_amd
    c = DEV_CASES[name]
    set_switches(c, monkeypatch.setenv, lambda s: monkeypatch.delenv(s, raising=False))
    E, A = c["E"], c["A"]
    g = zero_head(ppo_cpp_amd.PPOHip(c["O"], A, list(c["hidden"])))
    g.norm_init(E); g.rollout_alloc(E, DEV_T); g.seed(HOST_SEED)          # (the handle's own seed plays no part here)
    got, first = [], None
    for env0, step0 in DEV_STARTS:
        for it in range(2):
            before = g.kernel_counts()
            g.collect_synthetic(DEV_KEY, GAMMA, LAM, None, env0=env0, step0=step0 + it * DEV_T, first=(it == 0))
            if first is None:
                first = counts_delta(before, g.kernel_counts())
            a, nlp = g.rollout_get("actions"), g.rollout_get("neglogp")
            got += [(a[t], nlp[t]) for t in range(DEV_T)]
    g.close()
    print(name, first)
    if name in DEV_FORMS:
        assert first.get(DEV_FORMS[name]) == 1, first
    else:
        want = json.load(open(ROLLOUT_GOLDEN))["cases"][name]               # recorded at T = 3: the same kernels, a whole-rollout kernel once
        assert sorted(first) == sorted(want), (first, want)
        for k in ("narrow_rollout1_kernel", "narrow_rollout_kernel", "narrow_rollout_coop_kernel"):
            assert first.get(k, 0) == want.get(k, 0), (first, want)
    worst, _ = check_blocks(dev_blocks(name), got)
    observed("collect_synthetic %s" % name, worst)


@gpu
@pytest.mark.parametrize("name", sorted(HOST_CASES))
def test_host_env_rollout_draws(name, monkeypatch):
    import ppo_cpp_amd
    c = HOST_CASES[name]
    set_switches(c, monkeypatch.setenv, lambda s: monkeypatch.delenv(s, raising=False))
    E, O, A, T = c["E"], c["O"], 18, HOST_T
    cat = c["dist"] == "categorical"
    g = zero_head(ppo_cpp_amd.PPOHip(O, A, list(c["hidden"]), action_dist=c["dist"]))
    if c["masking"]:
        g.set_action_masking(True)
    g.norm_init(E); g.rollout_alloc(E, T); g.seed(HOST_SEED)
    rng = np.random.RandomState(7)
    masks = host_masks(name)
    g.rollout_reset(rng.uniform(-1, 1, (E, O)).astype(np.float32))
    got, first = [], None
    for it in (0, "explicit noise", 1):
        before = g.kernel_counts()
        acts = []
        for t in range(T):
            noise, mask = None, None
            if it == "explicit noise":
                noise = rng.uniform(0.01, 0.99, (E, A)).astype(np.float32) if cat else rng.normal(size=(E, A)).astype(np.float32)
            elif masks is not None:
                mask = masks[it, t]
            acts.append(g.rollout_act(t, noise, mask=mask))
            g.rollout_observe(t, rng.uniform(-1, 1, (E, O)).astype(np.float32), rng.uniform(-1, 1, E).astype(np.float32), (rng.uniform(size=E) < 0.1).astype(np.float32))
        g.rollout_finish(GAMMA, LAM)
        if first is None:
            first = counts_delta(before, g.kernel_counts())
        if it != "explicit noise":
            a, nlp = g.rollout_get("actions"), g.rollout_get("neglogp")
            np.testing.assert_array_equal(np.array(acts), a)
            got += [(a[t], nlp[t]) for t in range(T)]
    g.close()
    print(name, first)
    assert first == json.load(open(ROLLOUT_GOLDEN))["cases"][name], first
    worst, left = check_blocks(host_blocks(name), got)
    observed("host Env %s" % name, None if cat else worst, left if cat else None)


@gpu
def test_the_two_edge_draws_on_the_device():
    import ppo_cpp_amd
    g = zero_head(ppo_cpp_amd.PPOHip(18, 18, [64, 64]))
    obs = np.random.RandomState(1).uniform(-1, 1, (64, 18)).astype(np.float32)
    g.seed(28160)
    a, _, nlp = g.step(obs)
    assert np.isfinite(a).all() and np.isfinite(nlp).all()
    assert a[10, 4] == 0.0, a[10, 4]                                       # radius exactly 0: +0 or -0, never a NaN from the square root of a negative rounding
    w0, _ = check_blocks([Block("seed 28160", "normal", M.seed_key(28160), 0, 64, 0, 18, None, None)], [(a, nlp)])
    g.seed(3283)
    a, _, nlp = g.step(obs)
    assert np.isfinite(a).all() and np.isfinite(nlp).all()
    model, _ = M.counter_normals(M.seed_key(3283), np.arange(64), 0, 18)
    assert abs(float(a[6, 6]) - model[6, 6]) <= M.BOUND and abs(a[6, 6]) > 5
    w1, _ = check_blocks([Block("seed 3283", "normal", M.seed_key(3283), 0, 64, 0, 18, None, None)], [(a, nlp)])
    assert g.kernel_counts()["narrow_step_kernel<static>"] == 2
    g.close()
    observed("edge draws", max(w0, w1))
    print("OBSERVED edge draw [6, 6] of seed 3283: device %.7f model %.7f" % (a[6, 6], model[6, 6]))


# ---- the epoch shuffle ----------------------------------------------------------------------------------------------------------------------------------------
def shuffle_handle(name, monkeypatch):
    import ppo_cpp_amd
    hidden, env, E, T, nmb, kw, O, kernel = SHUFFLE[name]
    for s in SHUFFLE_SWITCHES:
        monkeypatch.setenv(s, "1" if s in env else "0")
    g = ppo_cpp_amd.PPOHip(O, 18, list(hidden), **kw)
    g.init_orthogonal(2)
    g.norm_init(E); g.rollout_alloc(E, T)
    return g


@gpu
@pytest.mark.parametrize("name", sorted(SHUFFLE))
def test_device_shuffle_is_the_documented_map(name, monkeypatch):
    """the last epoch's gidx after 1, 2 and 3 epochs (keys 0, 1, 2) under three seeds; behind the first update of each epoch count the other seeds replay the
    captured graph, whose map must be the new seed's: the replay reads fresh keys"""
    hidden, env, E, T, nmb, kw, O, kernel = SHUFFLE[name]
    g = shuffle_handle(name, monkeypatch)
    g.collect_synthetic(1234, GAMMA, LAM, None)
    got = {}
    for epochs in SHUFFLE_EPOCHS:
        for i, s in enumerate(SHUFFLE_SEEDS):
            before = g.kernel_counts()
            g.update(LR, CR, epochs, nmb, None, seed=s)
            delta = counts_delta(before, g.kernel_counts())
            if i == 0:
                assert delta and g.debug_graph_nodes() is not None, (name, epochs, delta)          # captured: the host code ran once
                if kernel:
                    assert delta.get(kernel, 0) > 0, (name, delta)
            else:
                assert delta == {} and g.debug_graph_nodes() is not None, (name, epochs, s, delta)  # a replay: no host-side launch was counted
            got[(epochs, s)] = g.debug_buffer("gidx")[:E * T].copy()
    g.close()
    check_gidx(E, T, got)
    if E * T >= 64:
        assert len({tuple(v.tolist()) for v in got.values()}) == len(got)              # every epoch count and every seed: another order
    observed("shuffle %s: 9 maps exact" % name)


@gpu
@pytest.mark.parametrize("name", sorted(k for k in SHUFFLE if k != "bf16_prepare_kernel"))
def test_rows_gathered_follow_the_map(name, monkeypatch):
    """the device shuffle against a fresh handle with the same weights, Adam slots, powers and rollout that is given the model's permutations as explicit perms: loss
    rows, weights and both Adam slots bit for bit; and against the oracle's update under the same permutations (tolerances of test_update_phase_matches_oracle)"""
    from oracle import oracle as o
    hidden, env, E, T, nmb, kw, O, kernel = SHUFFLE[name]
    epochs, seed, B = 2, 7, E * T
    fields = ("obs", "actions", "values", "neglogp", "returns")
    ga = shuffle_handle(name, monkeypatch)
    ga.collect_synthetic(1234, GAMMA, LAM, None)
    ro = {f: ga.rollout_get(f) for f in fields}
    ro["neglogp"] = (ro["neglogp"] + np.random.RandomState(5).normal(scale=0.1, size=(T, E))).astype(np.float32)       # move the ratio off 1: a row in the wrong
    ga.rollout_set("neglogp", ro["neglogp"])                                                                         # minibatch then changes the loss rows
    state = [ga.get_flat(w) for w in range(3)]
    powers = ga.beta_powers()
    rows_a, mean_a = ga.update(LR, CR, epochs, nmb, None, seed=seed)
    M.compare_gidx(ga.debug_buffer("gidx")[:B], MODEL.gidx(E, T, seed, epochs - 1))
    perms = np.stack([M.explicit_perm(M.epoch_perm(B, seed, ep)) for ep in range(epochs)])
    gb = shuffle_handle(name, monkeypatch)
    for w in range(3):
        gb.set_flat(state[w], w)
    gb.set_beta_powers(powers)
    for f in fields:
        gb.rollout_set(f, ro[f])
    rows_b, mean_b = gb.update(LR, CR, epochs, nmb, perms)
    np.testing.assert_array_equal(ga.debug_buffer("gidx")[:B], gb.debug_buffer("gidx")[:B])
    np.testing.assert_array_equal(rows_a, rows_b)
    np.testing.assert_array_equal(mean_a, mean_b)
    for w, nm in enumerate(("weights", "adam m", "adam v")):
        np.testing.assert_array_equal(ga.get_flat(w), gb.get_flat(w), err_msg=nm)
    assert np.abs(ga.get_flat(0) - state[0]).max() > 0
    orc = o.Oracle(O, 18, list(hidden))
    orc.theta[:] = state[0]
    ref_rows, ref_mean = orc.update(ro, perms, nmb, LR, CR)
    np.testing.assert_allclose(rows_a, ref_rows, rtol=2e-4, atol=2e-6, err_msg="loss rows")
    np.testing.assert_allclose(mean_a, ref_mean, rtol=2e-4, atol=2e-6, err_msg="mean losses")
    np.testing.assert_allclose(ga.get_flat(0), orc.theta, rtol=2e-4, atol=5e-6, err_msg="weights")
    ga.close(); gb.close()


# ---- two ranks ----------------------------------------------------------------------------------------------------------------------------------------------
@gpu
def test_two_ranks_draw_their_own_rows_and_share_one_global_shuffle(tmp_path):
    """world 2 as two processes on the one test GPU over the shared-memory stand-in of the collective library (tests/test_dp_two_ranks.py): rank r's rollout draws
    are the model's rows r E .. r E + E - 1, its ppo_step's rows start at rank * n_envs, and under dist_global_shuffle its gidx is the model's global map"""
    from tests.test_dp_two_ranks import build_fake_rccl
    tmp = str(tmp_path)
    fake = build_fake_rccl(tmp)
    uid = np.zeros(128, np.uint8)
    name = ("/ppo_dp_draws_%d" % os.getpid()).encode()
    uid[:len(name)] = np.frombuffer(name, np.uint8)
    fin = os.path.join(tmp, "in.npz")
    np.savez(fin, E=DP_E, T=DP_T, nmb=DP_NMB, epochs=DP_EPOCHS, key=DEV_KEY, seed=DP_SEED, shuffle_seed=DP_SHUFFLE_SEED, uid=uid, gamma=GAMMA, lam=LAM, lr=LR, cr=CR)
    env = dict(os.environ, PPO_RCCL_LIBRARY=fake, HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "dp_worker_draws.py"), str(r), "2", fin, os.path.join(tmp, "out%d.npz" % r)],
                              env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(2)]
    logs = []
    for p in procs:
        try:
            logs.append(p.communicate(timeout=300)[0].decode())
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            pytest.fail("the two ranks timed out")
    assert all(p.returncode == 0 for p in procs), "\n".join(l[-3000:] for l in logs)
    outs = [np.load(os.path.join(tmp, "out%d.npz" % r)) for r in range(2)]
    worst = 0.0
    for r, out in enumerate(outs):
        assert int(out["comm_nranks"]) == 2
        got = [(out["actions"][t], out["neglogp"][t]) for t in range(DP_T)] + [(out["step_a"], out["step_nlp"])]
        worst = max(worst, check_blocks(dp_blocks(r), got)[0])
        M.compare_gidx(out["gidx"], MODEL.global_gidx(DP_E, DP_T, DP_NMB, 2, r, DP_SHUFFLE_SEED, DP_EPOCHS - 1), what="rank %d global gidx" % r)
    assert np.abs(outs[0]["actions"] - outs[1]["actions"]).min() > 0 and np.abs(outs[0]["step_a"] - outs[1]["step_a"]).min() > 0
    both = np.concatenate([out["gidx"] for out in outs])
    assert sorted(both.tolist()) == list(range(2 * DP_E * DP_T))
    observed("two ranks", worst)

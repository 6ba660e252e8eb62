"""Multi-discrete action spaces: the multi-categorical policy head (ppo_create_multi / PPOHip(action_dist="multi_categorical", nvec=..)) against
tests/multi_categorical_ref.py (float64 NumPy forward, torch float64 autograd of the stable-baselines expressions for the loss and its gradient).

CPU tests: the reference itself (central differences, nvec = [A] equals CatRef, sampler frequencies), header and exports, creation limits, no CPU fallback,
the host layer's mixin through a stand-alone program.
GPU tests: act / train / rollout / update against the reference on every kernel instantiation, one component == categorical bit for bit, an all-ones mask ==
unmasked bit for bit, errors, round trips, two ranks, learning.  Tolerances are those of tests/test_discrete_policy.py for the same quantity; the absolute
tolerance of a row's neglogp and of the entropy is multiplied by K (sums of K terms)."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.categorical_ref import CatRef, gumbel_argmax, softmax_stats
from tests.masked_categorical_ref import MaskedCatRef
from tests.masked_categorical_ref import random_masks as cat_random_masks
from tests.multi_categorical_ref import MultiCatRef, offsets, random_masks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CR = 0.16102319955825806
LR = 0.000393141177482903
GAMMA, LAM = 0.99, 0.95
TIE = 1e-5          # a (row, component) whose two best (perturbed) logits are closer than this in the float64 reference may go either way in fp32


def close(a, b, rtol=1e-4, atol=1e-5, msg=""):
    np.testing.assert_allclose(a, b, rtol=rtol, atol=atol, err_msg=msg)


def batch_args(ref, n, seed, mask=None):
    """a small train batch for the reference's own checks (actions sampled under `mask`)"""
    rng = np.random.RandomState(seed)
    obs = rng.uniform(-1, 1, (n, ref.O))
    a, v, nlp, _ = ref.step(obs, rng.uniform(size=(n, ref.A)), mask) if mask is not None else ref.step(obs, rng.uniform(size=(n, ref.A)))
    old_nlp = nlp + rng.normal(scale=0.05, size=n)
    old_v = v + rng.normal(scale=0.05, size=n)
    ret = v + rng.normal(scale=0.5, size=n)
    adv = rng.normal(size=n)
    return obs, a, adv, ret, old_nlp, old_v, 0.3


# ---- CPU ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True])
def test_reference_gradient_matches_central_differences(masked):
    """The autograd arbiter itself: d loss / d theta against central finite differences of the same float64 loss (tolerances of the categorical reference's check)."""
    nvec = (3, 2, 4)
    ref = MultiCatRef(5, nvec, [6, 3], ent_coef=0.05)
    ref.init_random(3)
    mask = random_masks(np.random.RandomState(4), 12, nvec) if masked else None
    args = batch_args(ref, 12, 0, mask)
    _, grad = ref.loss_grad(*args, mask=mask)

    def loss_at(theta):
        keep = ref.theta.copy()
        ref.theta[:] = theta
        l5, _ = ref.loss_grad(*args, mask=mask)
        ref.theta[:] = keep
        return l5[0] - ref.ent * l5[2] + ref.vfc * l5[1]

    h = 1e-6
    fd = np.empty(ref.P)
    for i in range(ref.P):
        tp, tm = ref.theta.copy(), ref.theta.copy()
        tp[i] += h; tm[i] -= h
        fd[i] = (loss_at(tp) - loss_at(tm)) / (2 * h)
    np.testing.assert_allclose(grad, fd, rtol=1e-5, atol=1e-8)


def test_reference_with_one_component_equals_the_categorical_reference_exactly():
    A = 7
    multi, cat = MultiCatRef(5, [A], [6, 3], ent_coef=0.05), MaskedCatRef(5, A, [6, 3], ent_coef=0.05)
    multi.init_random(3); cat.init_random(3)
    np.testing.assert_array_equal(multi.theta, cat.theta)
    rng = np.random.RandomState(1)
    obs, u = rng.uniform(-1, 1, (20, 5)), rng.uniform(size=(20, A))
    mask = cat_random_masks(rng, 20, A)
    for mk in (None, mask):
        a, v, nlp, pert = multi.step(obs, u, mk)
        ca, cv, cnlp, cpert = cat.step(obs, u, mk)
        assert a.shape == (20, 1)
        np.testing.assert_array_equal(a[:, 0], ca); np.testing.assert_array_equal(v, cv)
        np.testing.assert_array_equal(nlp, cnlp); np.testing.assert_array_equal(pert, cpert)
    args = batch_args(multi, 20, 2)
    cargs = (args[0], args[1][:, 0]) + args[2:]
    for it in range(2):
        (l, g), (cl, cg) = multi.train_step(LR, 0.3, *args[:6]), CatRef.train_step(cat, LR, 0.3, *cargs[:6])
        np.testing.assert_array_equal(l, cl); np.testing.assert_array_equal(g, cg)
        np.testing.assert_array_equal(multi.theta, cat.theta); np.testing.assert_array_equal(multi.m, cat.m)


def test_reference_gumbel_argmax_per_component_follows_the_components_softmax():
    rng = np.random.RandomState(1)
    nvec = (5, 2, 3)
    ref = MultiCatRef(1, nvec, [2])
    logits = np.array([[1.5, -0.3, 0.2, 0.9, -2.0, 0.4, -0.6, 2.0, 0.1, 1.2]])
    N = 200000
    big = np.repeat(logits, N, 0)
    u = rng.uniform(size=(N, 10))
    for k, nk in enumerate(nvec):
        a, _ = gumbel_argmax(ref.comp(big, k), ref.comp(u, k))
        _, _, p = softmax_stats(ref.comp(logits, k))
        freq = np.bincount(a, minlength=nk) / N
        sigma = np.sqrt(p[0] * (1 - p[0]) / N)
        assert np.all(np.abs(freq - p[0]) < 4 * sigma), (k, freq, p[0])


def test_entry_points_are_declared_and_exported():
    src = open(os.path.join(ROOT, "include", "ppo_hip.h")).read()
    assert "int ppo_create_multi(const ppo_config* cfg, const int32_t* nvec, int32_t n_components, ppo_handle** out);" in src
    assert "int ppo_action_nvec(const ppo_handle* h, int32_t max, int32_t* nvec);" in src
    assert "int ppo_action_width(const ppo_handle* h);" in src
    assert "#define PPO_ACT_MULTI_CATEGORICAL 2" in src and "#define PPO_MAX_COMPONENTS 16" in src
    assert "#define PPO_ABI_VERSION 3" in src
    import ppo_cpp_amd
    lib = ppo_cpp_amd.load_library()
    for name in ("ppo_create_multi", "ppo_action_nvec", "ppo_action_width"):
        assert hasattr(lib, name), name
    assert lib.ppo_abi_version() == 3


def create_multi(nvec, act_dim=None, n_components=None, **overrides):
    """ppo_create_multi through ctypes with arguments PPOHip would not let through; returns (status, message)"""
    import ppo_cpp_amd
    from ppo_cpp_amd.capi import PPOConfig
    lib = ppo_cpp_amd.load_library()
    cfg = PPOConfig()
    hid = (ctypes.c_int32 * 2)(64, 64)
    lib.ppo_config_default(ctypes.byref(cfg), 18, sum(nvec) if act_dim is None else act_dim, 2, hid)
    for k, v in overrides.items():
        setattr(cfg, k, v)
    h = ctypes.c_void_p()
    nv = (ctypes.c_int32 * 32)(*nvec)
    rc = lib.ppo_create_multi(ctypes.byref(cfg), nv, len(nvec) if n_components is None else n_components, ctypes.byref(h))
    msg = lib.ppo_last_error(None).decode() if rc != 0 else ""
    if rc == 0:
        lib.ppo_destroy(h)
    return rc, msg


def test_creation_limits_are_errors_that_name_the_limit():
    """(checked before a device is looked for: the same messages with and without a GPU)"""
    rc, msg = create_multi([], act_dim=4, n_components=0)
    assert rc != 0 and "PPO_MAX_COMPONENTS" in msg and "1..16" in msg, msg
    rc, msg = create_multi([2] * 17)
    assert rc != 0 and "PPO_MAX_COMPONENTS" in msg and "17" in msg, msg
    rc, msg = create_multi([3, 1, 4])
    assert rc != 0 and "component 1" in msg and "at least 2" in msg, msg
    rc, msg = create_multi([3, 5], act_dim=9)
    assert rc != 0 and "act_dim 9" in msg and "sum of nvec (8)" in msg, msg
    rc, msg = create_multi([3, 5], compute_dtype=1)
    assert rc != 0 and "PPO_BF16" in msg, msg


def test_python_arguments():
    import ppo_cpp_amd
    with pytest.raises(ValueError, match="nvec"):
        ppo_cpp_amd.PPOHip(18, 8, [64, 64], action_dist="gaussian", nvec=[3, 5])
    with pytest.raises(ValueError, match="nvec"):
        ppo_cpp_amd.PPOHip(18, 8, [64, 64], action_dist="categorical", nvec=[3, 5])
    with pytest.raises(ValueError, match="nvec"):
        ppo_cpp_amd.PPOHip(18, 8, [64, 64], action_dist="multi_categorical")
    with pytest.raises(ValueError, match="sum"):
        ppo_cpp_amd.PPOHip(18, 9, [64, 64], action_dist="multi_categorical", nvec=[3, 5])


def test_create_multi_has_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    import ppo_cpp_amd
    with pytest.raises(ppo_cpp_amd.PPOHipError, match="no CPU fallback"):
        ppo_cpp_amd.PPOHip(18, None, [4, 5], action_dist="multi_categorical", nvec=[3, 5])


def test_host_library_builds_and_the_mixin_travels_through_the_wrappers(tmp_path):
    """libppo_host.so builds with the multi-discrete entry points; tests/host_multi_discrete_main.cpp (its own main, no GPU) drives MultiDiscreteTargetEnv x 3 through
    TimeLimit + VecEnv + EnvNormalize: forwarded get_action_nvec, [n, A] masks, [n, K] actions, mismatched children refused"""
    from ppo_cpp_amd import build as b
    so = b.build_host()
    assert so and os.path.exists(so)
    syms = subprocess.check_output(["nm", "-D", "--defined-only", so]).decode()
    assert "ppo_host_learn_multi" in syms and "ppo_host_multi_checkpoint" in syms
    exe = str(tmp_path / "host_multi_discrete")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-pthread", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "ppo_cpp_amd", "host"),
                           "-o", exe, os.path.join(ROOT, "tests", "host_multi_discrete_main.cpp")])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert out.returncode == 0 and out.stdout.decode().strip().endswith("ok"), out.stdout.decode()[-2000:]


# ---- GPU ---------------------------------------------------------------------------------------------------------------------
def make(O, nvec, hidden, seed=0, pi_gain=1.0, **overrides):
    import ppo_cpp_amd
    g = ppo_cpp_amd.PPOHip(O, None, list(hidden), action_dist="multi_categorical", nvec=list(nvec), **overrides)
    c = g.cfg
    ref = MultiCatRef(O, nvec, hidden, ent_coef=c.ent_coef, vf_coef=c.vf_coef, max_grad_norm=c.max_grad_norm, beta1=c.adam_beta1,
                      beta2=c.adam_beta2, eps=c.adam_eps)
    ref.init_random(seed, pi_gain)
    g.set_flat(ref.theta.astype(np.float32))
    return ref, g


def assert_only_mcat(g, step=True, train=False, masked=None):
    """ppo_kernel_counts: of the policy-step and train forward/backward names of every family, only the <mcat..> ones were counted"""
    kc = g.kernel_counts() if not isinstance(g, dict) else g
    for name, cnt in kc.items():
        head = name.startswith(("policy_step_kernel", "train_fwd_bwd_kernel", "train8", "narrow_", "bf16_", "weight_grad_assemble"))
        if head and "<mcat" not in name and name != "policy_step_kernel<host_action>":
            assert cnt == 0, (name, kc)
    if step:
        assert kc["policy_step_kernel<mcat>"] + kc["policy_step_kernel<mcat,mask>"] > 0, kc
    if train:
        assert kc["train_fwd_bwd_kernel<mcat>"] + kc["train_fwd_bwd_kernel<mcat,mask>"] > 0, kc
    if masked is True:
        assert kc["policy_step_kernel<mcat,mask>"] + kc["train_fwd_bwd_kernel<mcat,mask>"] > 0, kc
    if masked is False:
        assert kc["policy_step_kernel<mcat,mask>"] + kc["train_fwd_bwd_kernel<mcat,mask>"] == 0, kc


def check_actions(ref, got, want, x, msg):
    """equal on every (row, component) except near-ties of the component's two best entries of x (perturbed or plain logits); the near-ties may number at most
    pairs // 1000.  Returns their count."""
    got, want = np.asarray(got).reshape(-1, ref.K), np.asarray(want).reshape(-1, ref.K)
    tie = ref.top2_gap(x.reshape(-1, ref.A)) < TIE
    bad = (got != want) & ~tie
    print("%s: near-tie pairs %d of %d" % (msg, tie.sum(), tie.size))
    assert not bad.any(), "%s: %d (row, component) pairs differ (first %s)" % (msg, bad.sum(), np.argwhere(bad)[:5].tolist())
    assert tie.sum() <= tie.size // 1000, (msg, int(tie.sum()), tie.size)
    return int(tie.sum())


WIDE4 = (256, (2, 2, 2, 2, 20, 3, 39), (1024, 1024))       # build_layout: the per-layer tiles exceed 160 KB -> two-tile ("wide") layout, 64-column wave tiles (CT = 4)
WIDE1 = (18, (2, 2, 2, 2, 20, 3, 39), (1000,))             # ... and with a hidden width that is no multiple of 64: CT = 1
STEP_SHAPES = [(18, (3, 5, 2, 8), (64, 64)),               # <1,1,0>; Ap = 32; odd offsets
               (18, (3, 5, 2, 8), (256, 256)),             # <4,2,2>; the train kernel's EARLY form
               (40, (3, 5, 2, 8), (256, 256)),             # <4,2,2> without EARLY; Kp0 = 64
               (18, (2, 17, 16, 17, 12), (256, 256)),      # <4,2,0>; Ap = 64; components wider than 16 lanes, starting off a multiple of 16; width 2
               (36, (2, 2, 2, 2, 20, 3, 33), (64, 64))]    # K = 7; Ap = 64
STEP_CASES = [s + (n,) for s in STEP_SHAPES for n in (1, 17, 4096)] + [s + (n,) for s in (WIDE4, WIDE1) for n in (17, 512)]


@pytest.mark.gpu
@pytest.mark.parametrize("O,nvec,hidden,n", STEP_CASES)
@pytest.mark.parametrize("masked", [False, True])
def test_step_matches_reference(O, nvec, hidden, n, masked):
    ref, g = make(O, nvec, hidden, seed=n)
    K, A = len(nvec), sum(nvec)
    assert g.lib.ppo_action_dist(g.h) == 2 and g.nvec == list(nvec) and g.action_width == K
    names = [t[0] for t in g.tensors]
    assert "pi/logstd" not in names and len(names) == 4 * len(hidden) + 4
    assert dict(g.tensors)["pi/w"] == (hidden[-1], A) and dict(g.tensors)["pi/b"] == (A,)
    rng = np.random.RandomState(7)
    obs = rng.uniform(-1, 1, (n, O)).astype(np.float32)
    u = rng.uniform(size=(n, A)).astype(np.float32)
    mask = random_masks(rng, n, nvec) if masked else None
    a, v, nlp = g.step(obs, u, mask=mask)
    assert a.shape == (n, K) and v.shape == (n,) and nlp.shape == (n,)
    ra, rv, rnlp, pert = ref.step(obs, u, mask)
    check_actions(ref, a, ra, pert, "sampled actions")
    if masked:
        assert np.all(np.take_along_axis(mask, (a.astype(np.int64) + offsets(nvec)[:-1]), 1) != 0)        # no forbidden category, near-tie or not
    logits = ref.forward(obs)[0]
    # neglogp of the actions the kernel chose (the reference's own except on near-ties)
    close(nlp, ref.neglogp_of(logits, a, mask), atol=1e-5 * K, msg="neglogp")
    close(v, rv, msg="value")
    close(g.value(obs), rv, msg="ppo_value")
    det = g.act_deterministic(obs, mask=mask)
    assert det.shape == (n, K)
    check_actions(ref, det, ref.act_deterministic(obs, mask), logits if mask is None else np.where(mask != 0, logits, -np.inf), "deterministic actions")
    assert_only_mcat(g, masked=masked)
    g.close()


@pytest.mark.gpu
def test_on_device_sampling_follows_every_components_softmax_and_is_seeded():
    O, nvec, N = 18, (3, 5, 2, 8), 65536
    ref, g = make(O, nvec, (64, 64), seed=5, pi_gain=3.0)
    obs = np.repeat(np.random.RandomState(2).uniform(-1, 1, (1, O)), N, 0).astype(np.float32)
    logits = ref.forward(obs[:1])[0]
    g.seed(11)
    a1, _, nlp = g.step(obs)
    want_nlp = np.zeros(N)
    for k, nk in enumerate(nvec):
        _, _, p = softmax_stats(ref.comp(logits, k))
        ak = a1[:, k].astype(np.int64)
        assert np.all(a1[:, k] == np.floor(a1[:, k])) and ak.min() >= 0 and ak.max() < nk
        freq = np.bincount(ak, minlength=nk) / N
        sigma = np.sqrt(p[0] * (1 - p[0]) / N)
        assert np.all(np.abs(freq - p[0]) <= 4 * sigma), (k, freq, p[0])
        want_nlp += -np.log(p[0][ak])
    close(nlp, want_nlp, atol=1e-5 * len(nvec), msg="neglogp of the sampled categories")
    g.seed(11)
    np.testing.assert_array_equal(g.step(obs)[0], a1)
    g.seed(12)
    assert not np.array_equal(g.step(obs)[0], a1)
    g.close()


def synth_batch(ref, n, seed, cr=CR, mask=None):
    """tests/test_discrete_policy.synth_batch with [n, K] actions (sampled under `mask`): rows straddle both clip ranges but stay clear of their edges"""
    rng = np.random.RandomState(seed)
    obs = rng.uniform(-1, 1, (n, ref.O)).astype(np.float32)
    a, v, nlp, _ = ref.step(obs, rng.uniform(size=(n, ref.A)), mask)
    old_nlp = (nlp + rng.normal(scale=0.15, size=n)).astype(np.float32)
    old_v = (v + rng.normal(scale=0.2, size=n)).astype(np.float32)
    ret = (v + rng.normal(scale=0.5, size=n)).astype(np.float32)
    ratio = np.exp(old_nlp.astype(np.float64) - nlp)
    near = np.abs(np.abs(ratio - 1.0) - cr) < 1e-3
    old_nlp[near] += np.float32(0.01)
    dvo = v - old_v
    near = np.abs(np.abs(dvo) - cr) < 1e-3
    old_v[near] -= np.float32(0.01) * np.sign(dvo[near]).astype(np.float32)
    dvo = v - old_v
    vclip = old_v + np.clip(dvo, -cr, cr)
    s1, s2 = (v - ret) ** 2, (vclip - ret) ** 2
    near = (np.abs(dvo) > cr) & (np.abs(s1 - s2) < 1e-3 * np.maximum(s1, 1e-6))
    ret[near] += np.float32(0.05)
    adv = ret - old_v
    adv = ((adv - adv.mean()) / (adv.std() + 1e-8)).astype(np.float32)
    return obs, a.astype(np.float32), adv, ret, old_nlp, old_v


def check_train_step(ref, g, batch, mask, n, it):
    K = ref.K
    losses = g.train_step(LR, CR, *batch, mask=mask)
    grad, norm = g.last_grad()
    ref_losses, ref_grad = ref.train_step(LR, CR, *batch, mask=mask)
    close(losses[:2], ref_losses[:2], rtol=1e-4, atol=1e-6, msg="pg / vf loss it=%d" % it)
    close(losses[2], ref_losses[2], rtol=1e-4, atol=1e-6 * K, msg="entropy it=%d" % it)
    close(losses[3], ref_losses[3], rtol=1e-4, atol=1e-6, msg="approxkl it=%d" % it)
    assert abs(losses[4] - ref_losses[4]) <= 1.0 / n + 1e-6, ("clipfrac", losses[4], ref_losses[4])
    gs = np.abs(ref_grad).max()
    close(grad, ref_grad, rtol=2e-4, atol=2e-6 * gs, msg="grad it=%d" % it)
    close(norm, np.sqrt(np.dot(ref_grad, ref_grad)), rtol=1e-4, msg="norm it=%d" % it)
    close(g.get_flat(0), ref.theta, rtol=1e-4, atol=2e-6, msg="theta it=%d" % it)
    close(g.get_flat(1), ref.m, rtol=2e-4, atol=1e-7 * max(1.0, gs), msg="adam m it=%d" % it)
    return grad


TRAIN_CASES = [((64, 64), (3, 5, 2, 8), 200),              # 13 tiles, the last with 8 live rows
               ((256, 256), (3, 5, 2, 8), 512),
               ((256, 256), (2, 17, 16, 17, 12), 512)]


@pytest.mark.gpu
@pytest.mark.parametrize("hidden,nvec,n", TRAIN_CASES)
@pytest.mark.parametrize("masked", [False, True])
def test_three_train_steps_match_reference(hidden, nvec, n, masked):
    ref, g = make(18, nvec, hidden, seed=9, ent_coef=0.01)
    off = offsets(nvec)
    dead = int(off[1])                                     # masked: the first category of component 1 is forbidden in EVERY row (its neighbour always allowed)
    for it in range(3):
        mask = None
        if masked:
            mask = random_masks(np.random.RandomState(50 + it), n, nvec)
            mask[:, dead] = 0.0
            mask[:, dead + 1] = 1.0
        batch = synth_batch(ref, n, 100 + it, mask=mask)
        grad = check_train_step(ref, g, batch, mask, n, it)
        if masked:
            o, shape = ref.offs["pi/w"]
            np.testing.assert_array_equal(grad[o:o + shape[0] * shape[1]].reshape(shape)[:, dead], 0.0)
            o, _ = ref.offs["pi/b"]
            assert grad[o + dead] == 0.0
    assert_only_mcat(g, step=False, train=True, masked=masked)
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("O,nvec,hidden,n", [WIDE4 + (40,), WIDE1 + (40,), (36, (2, 2, 2, 2, 20, 3, 33), (64, 64), 40), (40, (3, 5, 2, 8), (256, 256), 40)])
def test_one_masked_train_step_on_the_remaining_instantiations(O, nvec, hidden, n):
    """the (CT, KS, CTH, WIDE) forms the three-step cases do not reach: both wide layouts, <1,1,0> with Ap = 64 and K = 7, <4,2,2> without EARLY"""
    ref, g = make(O, nvec, hidden, seed=3, ent_coef=0.01)
    mask = random_masks(np.random.RandomState(5), n, nvec)
    check_train_step(ref, g, synth_batch(ref, n, 7), None, n, 0)
    check_train_step(ref, g, synth_batch(ref, n, 8, mask=mask), mask, n, 1)
    assert_only_mcat(g, step=False, train=True, masked=True)
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("hidden", [(64, 64), (256, 256)])
def test_one_component_equals_the_categorical_head_bit_for_bit(hidden):
    import ppo_cpp_amd
    A, n = 18, 200
    ref, gm = make(18, [A], hidden, seed=2, ent_coef=0.01)
    gc = ppo_cpp_amd.PPOHip(18, A, list(hidden), action_dist="categorical", ent_coef=0.01)
    gc.set_flat(ref.theta.astype(np.float32))
    assert gm.nvec == [A] and gc.nvec == [A] and gm.action_width == 1 and gc.action_width == 1
    assert gm.tensors == gc.tensors and gm.P == gc.P
    rng = np.random.RandomState(3)
    obs = rng.uniform(-1, 1, (n, 18)).astype(np.float32)
    u = rng.uniform(size=(n, A)).astype(np.float32)
    ones = np.ones((n, A), np.float32)
    rmask = cat_random_masks(rng, n, A)

    def same_step(noise, mask):
        (am, vm, nm), (ac, vc, nc) = gm.step(obs, noise, mask=mask), gc.step(obs, noise, mask=mask)
        assert am.shape == (n, 1) and ac.shape == (n,)
        np.testing.assert_array_equal(am[:, 0], ac); np.testing.assert_array_equal(vm, vc); np.testing.assert_array_equal(nm, nc)
        np.testing.assert_array_equal(gm.act_deterministic(obs, mask=mask)[:, 0], gc.act_deterministic(obs, mask=mask))

    for mask in (None, ones, rmask):
        same_step(u, mask)                                                  # explicit uniforms
        gm.seed(11); gc.seed(11)
        same_step(None, mask)                                               # the counter draw, keyed by the global logit index
        for it in range(3):
            obs_b, a, adv, ret, nlp, v = synth_batch(ref, n, 30 + it, mask=mask)
            lm = gm.train_step(LR, CR, obs_b, a, adv, ret, nlp, v, mask=mask)
            lc = gc.train_step(LR, CR, obs_b, a[:, 0], adv, ret, nlp, v, mask=mask)
            np.testing.assert_array_equal(lm, lc)
            (g1, n1), (g2, n2) = gm.last_grad(), gc.last_grad()
            np.testing.assert_array_equal(g1, g2)
            assert n1 == n2
            for which in (0, 1, 2):
                np.testing.assert_array_equal(gm.get_flat(which), gc.get_flat(which))
    assert_only_mcat(gm, train=True, masked=True)
    kc = gc.kernel_counts()
    assert kc["policy_step_kernel<cat>"] > 0 and kc["train_fwd_bwd_kernel<cat,mask>"] > 0 and kc["policy_step_kernel<mcat>"] == 0 and kc["train_fwd_bwd_kernel<mcat>"] == 0, kc
    gm.close(); gc.close()


def ref_rollout(ref, seed, E, T, u, masks=None):
    """runner.hpp:56-157 over the seeded synthetic env with the multi-categorical reference policy (the env ignores the actions)"""
    from oracle import oracle as o
    from oracle import numpy_port as npp
    nz = o.Normalizer(E, ref.O)
    raw, _, _ = o.seeded_env_step(seed, 0, E, 0, ref.O)
    obs, dones = nz.obs(raw), np.zeros(E, np.float32)
    ro = {k: [] for k in ("obs", "actions", "values", "neglogp", "dones", "rewards", "pert", "logits")}
    for t in range(T):
        a, v, nlp, pert = ref.step(obs, u[t], None if masks is None else masks[t])
        for k, x in (("obs", obs), ("actions", a), ("values", v), ("neglogp", nlp), ("dones", dones), ("pert", pert), ("logits", ref.forward(obs)[0])):
            ro[k].append(x)
        raw, rew, dones = o.seeded_env_step(seed, 0, E, t + 1, ref.O)
        obs = nz.obs(raw)
        ro["rewards"].append(nz.reward(rew, dones))
    ro = {k: np.array(x) for k, x in ro.items()}
    _, last_v = ref.forward(obs)
    ro["returns"] = npp.gae(ro["rewards"].astype(np.float32), ro["values"].astype(np.float32), ro["dones"], last_v.astype(np.float32), dones, GAMMA, LAM)
    if masks is not None:
        ro["masks"] = masks
    return ro


def check_rollout(ref, got, ro, msg):
    T, E = ro["values"].shape
    check_actions(ref, got["actions"], ro["actions"], ro["pert"], msg + " actions")
    for f in ("obs", "values", "rewards", "returns"):
        close(got[f], ro[f], rtol=2e-4, atol=2e-5, msg=msg + " " + f)
    mk = ro["masks"].reshape(T * E, -1) if "masks" in ro else None
    want = ref.neglogp_of(ro["logits"].reshape(T * E, -1), got["actions"].reshape(T * E, -1), mk).reshape(T, E)
    close(got["neglogp"], want, rtol=2e-4, atol=2e-5 * ref.K, msg=msg + " neglogp")


FIELDS = ("obs", "actions", "values", "neglogp", "rewards", "returns")


@pytest.mark.gpu
def test_collect_synthetic_matches_reference():
    O, nvec, E, T = 18, (3, 5, 2, 8), 64, 8
    ref, g = make(O, nvec, (64, 64), seed=E)
    u = np.random.RandomState(E).uniform(size=(T, E, ref.A)).astype(np.float32)
    ro = ref_rollout(ref, 1234, E, T, u)
    g.set_action_masking(True)                                 # the seeded env knows no legality: unmasked kernels, rows recorded as all allowed
    g.norm_init(E)
    g.rollout_alloc(E, T)
    g.collect_synthetic(1234, GAMMA, LAM, u)
    got = {f: g.rollout_get(f) for f in FIELDS}
    assert got["actions"].shape == (T, E, len(nvec))
    check_rollout(ref, got, ro, "collect")
    np.testing.assert_array_equal(g.rollout_get("masks"), 1.0)
    assert_only_mcat(g, masked=False)
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("masked", [False, True])
def test_host_env_loop_matches_reference(masked):
    """(E, T) = (17, 4) with K = 3: two 16-row blocks, the second with one live row and a 3-element tail (the landing buffer's store path for pieces under 16 bytes)"""
    from oracle import oracle as o
    O, nvec, E, T = 18, (3, 5, 2), 17, 4
    ref, g = make(O, nvec, (64, 64), seed=41)
    rng = np.random.RandomState(E + 1)
    u = rng.uniform(size=(T, E, ref.A)).astype(np.float32)
    masks = np.stack([random_masks(rng, E, nvec) for _ in range(T)]) if masked else None
    ro = ref_rollout(ref, 99, E, T, u, masks)
    if masked:
        g.set_action_masking(True)
    g.norm_init(E)
    g.rollout_alloc(E, T)
    raw, _, _ = o.seeded_env_step(99, 0, E, 0, O)
    g.rollout_reset(raw)
    acts = []
    for t in range(T):
        a = g.rollout_act(t, u[t], mask=masks[t] if masked else None)
        assert a.shape == (E, 3)
        acts.append(a)
        raw, rew, dn = o.seeded_env_step(99, 0, E, t + 1, O)
        g.rollout_observe(t, raw, rew, dn)
    g.rollout_finish(GAMMA, LAM)
    got = {f: g.rollout_get(f) for f in FIELDS}
    np.testing.assert_array_equal(np.array(acts), got["actions"])
    check_rollout(ref, got, ro, "host Env")
    if masked:
        np.testing.assert_array_equal(g.rollout_get("masks"), masks)
    assert_only_mcat(g, masked=masked)
    g.close()


def upload_and_update(ref, g, ro, rng, E, T, nmb, epochs, it):
    """one ppo_update with explicit perms on uploaded rollout fields against the reference's update; returns (perms, flat env-major action rows)"""
    ro["neglogp"] = (ro["neglogp"] + rng.normal(scale=0.1, size=(T, E))).astype(np.float32)   # move the ratio off 1
    fields = ("obs", "actions", "values", "neglogp", "returns") + (("masks",) if "masks" in ro else ())
    for f in fields:
        g.rollout_set(f, np.asarray(ro[f], np.float32))
    perms = np.stack([rng.permutation(E * T) for _ in range(epochs)]).astype(np.int32)
    rows, mean = g.update(LR, CR, epochs, nmb, perms)
    ref_rows, ref_mean = ref.update({f: np.asarray(ro[f], np.float32) for f in fields}, perms, nmb, LR, CR)
    atol = np.array([1e-6, 1e-6, 1e-6 * ref.K, 1e-6])
    for j in range(4):
        close(rows[:, j], ref_rows[:, j], rtol=1e-4, atol=atol[j], msg="loss rows update %d column %d" % (it, j))
        close(mean[j], ref_mean[j], rtol=1e-4, atol=atol[j], msg="mean losses update %d column %d" % (it, j))
    assert np.all(np.abs(rows[:, 4] - ref_rows[:, 4]) <= nmb / (E * T) + 1e-6)
    close(g.get_flat(0), ref.theta, rtol=1e-4, atol=5e-6, msg="theta after update %d" % it)
    return perms, np.swapaxes(np.asarray(ro["actions"], np.float32), 0, 1).reshape(E * T, -1)


@pytest.mark.gpu
@pytest.mark.parametrize("O,nvec,masked", [(18, (3, 5, 2, 8), False), (18, (3, 5, 2, 8), True),
                                           (16, (3, 5, 2, 8), False),        # O and K multiples of 4, no masks: the 16-byte gather (epoch_gather4_kernel)
                                           (16, (3, 5, 2, 8), True)])        # ... with masks: the mask-copying gather
def test_two_updates_with_explicit_perms_match_reference(O, nvec, masked):
    hidden, E, T, nmb, epochs = (64, 64), 32, 16, 4, 2
    ref, g = make(O, nvec, hidden, seed=17, ent_coef=0.01)
    if masked:
        g.set_action_masking(True)
    g.norm_init(E)
    g.rollout_alloc(E, T)
    rng = np.random.RandomState(3)
    for it in range(2):
        u = rng.uniform(size=(T, E, ref.A)).astype(np.float32)
        masks = np.stack([random_masks(rng, E, nvec) for _ in range(T)]) if masked else None
        ro = ref_rollout(ref, 500 + it, E, T, u, masks)
        ro["obs"] = ro["obs"].astype(np.float32)
        perms, flat = upload_and_update(ref, g, ro, rng, E, T, nmb, epochs, it)
        nodes = g.debug_graph_nodes()
        assert nodes is not None and nodes["kernel"] > 0, nodes
        assert nodes["memset"] == 0 and nodes["memcpy"] == 0 and nodes["other"] == 0, nodes
        # the gathered action rows of the last epoch, K floats each: out.row(perm[i]) = in.row(i)
        mb = g.debug_buffer("mb_act").view(np.float32)
        assert mb.size >= E * T * len(nvec)
        np.testing.assert_array_equal(mb[:E * T * len(nvec)].reshape(E * T, -1)[perms[-1]], flat)
    assert_only_mcat(g, step=False, train=True, masked=masked)
    g.close()


@pytest.mark.gpu
def test_an_all_ones_mask_gives_the_unmasked_bits():
    nvec, hidden, n, E, T = (2, 17, 16, 17, 12), (256, 256), 200, 32, 8
    ref, g1 = make(18, nvec, hidden, seed=6, ent_coef=0.01)
    _, g2 = make(18, nvec, hidden, seed=6, ent_coef=0.01)
    rng = np.random.RandomState(9)
    obs = rng.uniform(-1, 1, (n, 18)).astype(np.float32)
    u = rng.uniform(size=(n, ref.A)).astype(np.float32)
    ones = np.ones((n, ref.A), np.float32)
    for x, y in zip(g1.step(obs, u), g2.step(obs, u, mask=ones)):
        np.testing.assert_array_equal(x, y)
    np.testing.assert_array_equal(g1.act_deterministic(obs), g2.act_deterministic(obs, mask=ones))
    for it in range(3):
        batch = synth_batch(ref, n, 60 + it)
        np.testing.assert_array_equal(g1.train_step(LR, CR, *batch), g2.train_step(LR, CR, *batch, mask=ones))
        np.testing.assert_array_equal(g1.last_grad()[0], g2.last_grad()[0])
        for which in (0, 1, 2):
            np.testing.assert_array_equal(g1.get_flat(which), g2.get_flat(which))
    g2.set_action_masking(True)                                # masks default to ones
    ro = ref_rollout(ref, 77, E, T, rng.uniform(size=(T, E, ref.A)).astype(np.float32))
    perms = np.stack([rng.permutation(E * T) for _ in range(2)]).astype(np.int32)
    outs = []
    for g in (g1, g2):
        g.norm_init(E)
        g.rollout_alloc(E, T)
        for f in ("obs", "actions", "values", "neglogp", "returns"):
            g.rollout_set(f, np.asarray(ro[f], np.float32))
        rows, mean = g.update(LR, CR, 2, 4, perms)
        outs.append((rows, mean, g.get_flat(0), g.get_flat(1), g.get_flat(2)))
    for x, y in zip(*outs):
        np.testing.assert_array_equal(x, y)
    assert_only_mcat(g1, train=True, masked=False)
    assert_only_mcat(g2, train=True, masked=True)
    g1.close(); g2.close()


@pytest.mark.gpu
def test_errors():
    import ppo_cpp_amd
    from ppo_cpp_amd.capi import PPOConfig
    rc, msg = create_multi([], act_dim=4, n_components=0)
    assert rc != 0 and "PPO_MAX_COMPONENTS" in msg, msg
    rc, msg = create_multi([2] * 17)
    assert rc != 0 and "PPO_MAX_COMPONENTS" in msg, msg
    rc, msg = create_multi([3, 1, 4])
    assert rc != 0 and "at least 2" in msg, msg
    rc, msg = create_multi([3, 5], act_dim=9)
    assert rc != 0 and "sum of nvec" in msg, msg
    rc, msg = create_multi([3, 5], compute_dtype=1)
    assert rc != 0 and "PPO_BF16" in msg, msg
    assert create_multi([3, 5])[0] == 0
    lib = ppo_cpp_amd.load_library()
    cfg = PPOConfig()
    hid = (ctypes.c_int32 * 2)(64, 64)
    lib.ppo_config_default(ctypes.byref(cfg), 18, 8, 2, hid)
    h = ctypes.c_void_p()
    assert lib.ppo_create_ex(ctypes.byref(cfg), 2, ctypes.byref(h)) != 0
    assert b"unknown action_dist" in lib.ppo_last_error(None) and b"ppo_create_multi" in lib.ppo_last_error(None)
    nvec = (3, 5, 2, 8)
    ref, g = make(18, nvec, (64, 64))
    n = 32
    obs, a, adv, ret, nlp, v = synth_batch(ref, n, 0)
    theta = g.get_flat(0)
    for bad in (5.0, -1.0, 2.5, np.nan):                       # component 1 has 5 categories
        a2 = a.copy(); a2[5, 1] = bad
        with pytest.raises(ppo_cpp_amd.PPOHipError, match=r"row 5, component 1.*\[0, 5\)"):
            g.train_step(LR, CR, obs, a2, adv, ret, nlp, v)
    a2 = a.copy(); a2[6, 0] = 4.0                                # a valid index of component 1, not of component 0 (3 categories)
    with pytest.raises(ppo_cpp_amd.PPOHipError, match=r"row 6, component 0"):
        g.train_step(LR, CR, obs, a2, adv, ret, nlp, v)
    ones = np.ones((n, ref.A), np.float32)
    m2 = ones.copy(); m2[7, 3:8] = 0.0                          # component 1 of row 7 fully forbidden (the other components keep categories)
    with pytest.raises(ppo_cpp_amd.PPOHipError, match=r"row 7 allows no category of component 1"):
        g.step(obs, mask=m2)
    with pytest.raises(ppo_cpp_amd.PPOHipError, match=r"row 7 allows no category of component 1"):
        g.act_deterministic(obs, mask=m2)
    with pytest.raises(ppo_cpp_amd.PPOHipError, match=r"row 7 allows no category of component 1"):
        g.train_step(LR, CR, obs, a, adv, ret, nlp, v, mask=m2)
    m3 = ones.copy(); m3[9, 10 + int(a[9, 3])] = 0.0            # row 9's own action in component 3 (offset 10)
    with pytest.raises(ppo_cpp_amd.PPOHipError, match=r"row 9, component 3.*forbidden"):
        g.train_step(LR, CR, obs, a, adv, ret, nlp, v, mask=m3)
    g.set_action_masking(True)
    g.norm_init(4); g.rollout_alloc(4, 8)
    with pytest.raises(ppo_cpp_amd.PPOHipError, match=r"allows no category of component 1"):
        g.rollout_act(0, mask=m2[4:8])
    with pytest.raises(ppo_cpp_amd.PPOHipError, match=r"allows no category of component 1"):
        g.rollout_set("masks", m2)
    with pytest.raises(ppo_cpp_amd.PPOHipError, match=r"component 1.*\[0, 5\)"):
        bad_acts = a.copy().reshape(8, 4, 4); bad_acts[2, 1, 1] = 5.0
        g.rollout_set("actions", bad_acts)
    np.testing.assert_array_equal(g.get_flat(0), theta)          # nothing was trained
    g.train_step(LR, CR, obs, a, adv, ret, nlp, v, mask=ones)
    gauss = ppo_cpp_amd.PPOHip(18, 6, [64, 64])
    with pytest.raises(ppo_cpp_amd.PPOHipError, match=r"action masks need a categorical \(PPO_ACT_CATEGORICAL\) handle"):
        gauss.set_action_masking(True)
    assert gauss.nvec == [] and gauss.action_width == 6
    gauss.close(); g.close()


@pytest.mark.gpu
def test_round_trip_into_fresh_handles():
    """weights, Adam slots and beta powers go into a fresh handle with the same nvec; another split of the same width takes the flat vector (same tensors) and
    reports its own nvec"""
    nvec = (3, 5, 2, 8)
    ref, g = make(18, nvec, (64, 64), seed=4)
    g.train_step(LR, CR, *synth_batch(ref, 64, 2))
    _, g2 = make(18, nvec, (64, 64), seed=5)
    _, g3 = make(18, (9, 9), (64, 64), seed=5)
    assert g3.tensors == g.tensors and g3.P == g.P and g3.nvec == [9, 9] and g3.action_width == 2
    for h in (g2, g3):
        for which in (0, 1, 2):
            h.set_flat(g.get_flat(which), which)
            np.testing.assert_array_equal(h.get_flat(which), g.get_flat(which))
        h.set_beta_powers(g.beta_powers())
        np.testing.assert_array_equal(h.beta_powers(), g.beta_powers())
    for name, _ in g.tensors:
        np.testing.assert_array_equal(g2.get_tensor(name), g.get_tensor(name))
    obs = np.random.RandomState(0).uniform(-1, 1, (300, 18)).astype(np.float32)
    np.testing.assert_array_equal(g2.act_deterministic(obs), g.act_deterministic(obs))
    assert g3.act_deterministic(obs).shape == (300, 2)
    for h in (g, g2, g3):
        h.close()


@pytest.mark.gpu
def test_ppo2_checkpoint_of_a_multi_categorical_policy(tmp_path):
    """PPO2::save writes "discrete" plus action_nvec; PPO2::load into a fresh handle with the same nvec restores every tensor (same deterministic actions), into a
    handle with another split of the same width, or into a plain categorical one, it fails"""
    from ppo_cpp_amd import hostapi
    prefix = str(tmp_path / "multi")
    obs = np.random.RandomState(3).uniform(-1, 1, (200, 18)).astype(np.float32)
    rc, before, after = hostapi.multi_checkpoint(prefix, obs, [3, 5, 2], [5, 3, 2])
    assert rc == 0, rc
    np.testing.assert_array_equal(before, after)
    assert before.shape == (200, 3) and np.all(before >= 0) and np.all(before < np.array([3, 5, 2]))
    side = json.load(open(prefix + ".json"))
    assert side["action_space"] == "discrete" and side["action_nvec"] == [3, 5, 2]


@pytest.mark.gpu
def test_two_ranks_global_shuffle_equal_one_rank_over_the_union(tmp_path):
    """world 2 on the collective-library stand-in (two processes on one GPU, tests/fake_rccl), ppo_dist_global_shuffle(1) with K = 3: the rollout's actions travel
    through the all-gather three floats per row, and the weights after one update equal a one-rank update over the union of the rows"""
    from tests.test_dp_two_ranks import build_fake_rccl
    world, hidden, E, T, nmb, epochs, nvec = 2, (64, 64), 32, 8, 4, 2, (3, 5, 2)
    tmp = str(tmp_path)
    fake = build_fake_rccl(tmp)
    ref, g = make(18, nvec, hidden, seed=21)
    rng = np.random.RandomState(8)
    ro = ref_rollout(ref, 77, E, T, rng.uniform(size=(T, E, ref.A)))
    ro = {f: np.asarray(ro[f], np.float32) for f in ("obs", "actions", "values", "neglogp", "returns")}
    ro["neglogp"] = (ro["neglogp"] + rng.normal(scale=0.1, size=(T, E))).astype(np.float32)
    gperms = np.stack([rng.permutation(E * T).astype(np.int32) for _ in range(epochs)])
    theta0 = ref.theta.astype(np.float32)
    uid = np.zeros(128, np.uint8)
    name = ("/ppo_dp_mcat_%d_%d" % (os.getpid(), rng.randint(1 << 30))).encode()
    uid[:len(name)] = np.frombuffer(name, np.uint8)
    fin = os.path.join(tmp, "in.npz")
    np.savez(fin, hidden=np.array(hidden), nvec=np.array(nvec), E=E, T=T, nmb=nmb, epochs=epochs, theta=theta0, uid=uid, gperms=gperms, lr=LR, cr=CR,
             **{"ro_" + f: x for f, x in ro.items()})
    env = dict(os.environ, PPO_RCCL_LIBRARY=fake, HSA_ENABLE_IPC_MODE_LEGACY="0")
    # every GPU step under a time limit of its own
    procs = [subprocess.Popen(["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "tests", "dp_worker_multi.py"), str(r), str(world), fin,
                               os.path.join(tmp, "out%d.npz" % r)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(world)]
    logs = [p.communicate()[0].decode() for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(l[-3000:] for l in logs)
    outs = [np.load(os.path.join(tmp, "out%d.npz" % r)) for r in range(world)]
    g.norm_init(E, 0.99)
    g.rollout_alloc(E, T)
    for f, x in ro.items():
        g.rollout_set(f, x)
    rows, _ = g.update(LR, CR, epochs, nmb, gperms)
    theta1 = g.get_flat(0)
    assert_only_mcat(g, step=False, train=True, masked=False)
    g.close()
    for r, out in enumerate(outs):
        assert out["mcat_train"] > 0 and out["cat_train"] == 0
        np.testing.assert_array_equal(out["actions"], ro["actions"][:, r * (E // world):(r + 1) * (E // world)])
        close(out["rows"][:, :4], rows[:, :4], rtol=2e-4, atol=2e-6, msg="loss rows rank %d" % r)
        close(out["theta"], theta1, rtol=2e-4, atol=5e-6, msg="weights rank %d" % r)
    for k in ("rows", "theta", "adam_m", "adam_v"):
        np.testing.assert_array_equal(outs[0][k], outs[1][k])
    assert np.abs(theta1 - theta0).max() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("reference_loop", [False, True])
def test_ppo2_runs_the_masked_multi_discrete_env_without_a_forbidden_action(reference_loop):
    """MultiDiscreteTargetEnv(masked) x 8 through PPO2::learn (both loops) and PPO2::eval: the policy never sends a category its component's mask forbids"""
    from ppo_cpp_amd import hostapi
    got = hostapi.learn_curve(8, 16, [64, 64], 3, 4, 2, 2e-3, 0.2, seed=5, nvec=(6, 6, 6), masked=True, n_playback=30, reference_loop=reference_loop)
    assert got["forbidden_received"] == 0
    assert got["playback_actions"].shape == (30, 3) and np.all(got["playback_legal"] == 1.0)
    assert np.all(got["reward_curve"] >= 0.0)
    assert_only_mcat(got["kernel_counts"], train=True, masked=True)


@pytest.mark.gpu
def test_ppo2_learns_the_multi_discrete_target_task():
    """Learning: MultiDiscreteTargetEnv x 16 (host/env/env_mock.hpp: nvec = (6, 6, 6), reward = the fraction of components whose category is argmax_j (W_k obs)_j,
    episodes of 100 steps) behind VecEnv + EnvNormalize, 64 steps, [64,64], 80 updates of 4 epochs x 4 minibatches at lr 2e-3 (the settings of
    test_ppo2_learns_the_discrete_target_task with 80 of its 150 updates), through PPO2::learn with the library's own sampling and shuffles.  A uniform policy
    earns 1/6 = 0.167.  The NumPy reference loop (tests/multi_categorical_ref.learn_loop on MultiDiscreteTargetRef with the oracle's EnvNormalize,
    MultiCatRef.init_random(seed, pi_gain=0.01)) over the draw seeds 1, 2, 3: first-15 -> last-15 mean reward
    0.201 -> 0.406, 0.199 -> 0.424, 0.203 -> 0.428.
    RISE = 0.123 = 0.6 x the smallest of the three rises (0.205, 0.225, 0.225): the last-15 mean over the first-15.
    BAND = 0.089 = 4 x the spread of the three last-15 means (0.0222; not below 0.05): |last-15 mean - 0.419| (their mean).  The two legs differ in initial
    weights and draws.
    This leg on an MI355X: 0.202 -> 0.428 (rise 0.226; 0.009 from the reference mean)."""
    from ppo_cpp_amd import hostapi
    RISE, BAND, REF_LAST15 = 0.123, 0.089, 0.419
    got = hostapi.learn_curve(16, 64, [64, 64], 80, 4, 4, 2e-3, 0.2, seed=11, nvec=(6, 6, 6))
    c = got["reward_curve"]
    first, last = c[:15].mean(), c[-15:].mean()
    print("reward curve first-15 %.3f last-15 %.3f" % (first, last))
    assert_only_mcat(got["kernel_counts"], train=True, masked=False)
    assert last - first >= RISE, (first, last)
    assert abs(last - REF_LAST15) <= BAND, (last, REF_LAST15)

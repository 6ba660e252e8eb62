"""Categorical policies (discrete action spaces) on the fp32 path: ppo_create_ex(..., PPO_ACT_CATEGORICAL) / PPOHip(action_dist="categorical")
against tests/categorical_ref.py (float64 NumPy forward, torch float64 autograd for the loss and its gradient).

CPU tests: the C-ABI entry points exist, there is no CPU fallback, the reference's gradient and sampler are right.
GPU tests: act / train / update / rollouts against the reference, on-device sampling statistics, kernel selection, errors, tensor round trip.
Tolerances are those of tests/test_hip_parity.py for the Gaussian head."""
import ctypes
import os

import numpy as np
import pytest

from tests.categorical_ref import CatRef, gumbel_argmax, softmax_stats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CR = 0.16102319955825806
LR = 0.000393141177482903
GAMMA, LAM = 0.99, 0.95
TIE = 1e-5          # a row whose two best perturbed logits are closer than this may go either way in fp32


def close(a, b, rtol=1e-4, atol=1e-5, msg=""):
    np.testing.assert_allclose(a, b, rtol=rtol, atol=atol, err_msg=msg)


# ---- CPU ---------------------------------------------------------------------------------------------------------------------
def test_create_ex_and_action_dist_are_declared_and_exported():
    src = open(os.path.join(ROOT, "include", "ppo_hip.h")).read()
    assert "int ppo_create_ex(const ppo_config* cfg, int32_t action_dist, ppo_handle** out);" in src
    assert "int ppo_action_dist(const ppo_handle* h);" in src
    assert "#define PPO_ACT_GAUSSIAN    0" in src and "#define PPO_ACT_CATEGORICAL 1" in src
    import ppo_cpp_amd
    lib = ppo_cpp_amd.load_library()
    assert hasattr(lib, "ppo_create_ex") and hasattr(lib, "ppo_action_dist")
    assert lib.ppo_abi_version() == 3


def test_create_ex_has_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    import ppo_cpp_amd
    with pytest.raises(ppo_cpp_amd.PPOHipError, match="no CPU fallback"):
        ppo_cpp_amd.PPOHip(18, 6, [4, 5], action_dist="categorical")


def test_action_dist_is_an_explicit_keyword():
    import ppo_cpp_amd
    with pytest.raises(ValueError, match="action_dist"):
        ppo_cpp_amd.PPOHip(18, 6, [4, 5], action_dist="bernoulli")


def test_reference_gradient_matches_central_differences():
    """The autograd arbiter itself: d loss / d theta against central finite differences of the same float64 loss."""
    ref = CatRef(5, 4, [6, 3], ent_coef=0.05)
    ref.init_random(3)
    rng = np.random.RandomState(0)
    n = 12
    obs = rng.uniform(-1, 1, (n, 5))
    a, v, nlp, _ = ref.step(obs, rng.uniform(size=(n, 4)))
    old_nlp = nlp + rng.normal(scale=0.05, size=n)
    old_v = v + rng.normal(scale=0.05, size=n)
    ret = v + rng.normal(scale=0.5, size=n)
    adv = rng.normal(size=n)
    args = (obs, a, adv, ret, old_nlp, old_v, 0.3)
    _, grad = ref.loss_grad(*args)

    def loss_at(theta):
        keep = ref.theta.copy()
        ref.theta[:] = theta
        l5, _ = ref.loss_grad(*args)
        ref.theta[:] = keep
        return l5[0] - ref.ent * l5[2] + ref.vfc * l5[1]

    h = 1e-6
    fd = np.empty(ref.P)
    for i in range(ref.P):
        tp, tm = ref.theta.copy(), ref.theta.copy()
        tp[i] += h; tm[i] -= h
        fd[i] = (loss_at(tp) - loss_at(tm)) / (2 * h)
    np.testing.assert_allclose(grad, fd, rtol=1e-5, atol=1e-8)


def test_reference_gumbel_argmax_reproduces_softmax_frequencies():
    rng = np.random.RandomState(1)
    logits = np.array([[1.5, -0.3, 0.2, 0.9, -2.0]])
    N = 200000
    a, _ = gumbel_argmax(np.repeat(logits, N, 0), rng.uniform(size=(N, 5)))
    _, _, p = softmax_stats(logits)
    freq = np.bincount(a, minlength=5) / N
    sigma = np.sqrt(p[0] * (1 - p[0]) / N)
    assert np.all(np.abs(freq - p[0]) < 4 * sigma), (freq, p[0])


# ---- GPU ---------------------------------------------------------------------------------------------------------------------
def make(O, A, hidden, seed=0, pi_gain=1.0, **overrides):
    import ppo_cpp_amd
    g = ppo_cpp_amd.PPOHip(O, A, list(hidden), action_dist="categorical", **overrides)
    c = g.cfg
    ref = CatRef(O, A, hidden, ent_coef=c.ent_coef, vf_coef=c.vf_coef, max_grad_norm=c.max_grad_norm, beta1=c.adam_beta1,
                 beta2=c.adam_beta2, eps=c.adam_eps)
    ref.init_random(seed, pi_gain)
    g.set_flat(ref.theta.astype(np.float32))
    return ref, g


def check_actions(got, want, pert, msg):
    """equal on every row except near-ties of the two best perturbed logits; returns the number of rows skipped"""
    top2 = np.sort(pert, axis=1)[:, -2:]
    tie = (top2[:, 1] - top2[:, 0]) < TIE
    bad = (got != want) & ~tie
    assert not bad.any(), "%s: %d rows differ (first %s)" % (msg, bad.sum(), np.nonzero(bad)[0][:5])
    return int(tie.sum())


@pytest.mark.gpu
@pytest.mark.parametrize("O,A,hidden", [(18, 6, (64, 64)), (18, 18, (256, 256)), (256, 64, (1024, 1024))])
@pytest.mark.parametrize("n", [1, 17, 4096])
def test_step_matches_reference(O, A, hidden, n):
    ref, g = make(O, A, hidden, seed=n)
    assert g.lib.ppo_action_dist(g.h) == 1
    names = [t[0] for t in g.tensors]
    assert "pi/logstd" not in names and len(names) == 4 * len(hidden) + 4
    assert dict(g.tensors)["pi/w"] == (hidden[-1], A) and dict(g.tensors)["pi/b"] == (A,)
    rng = np.random.RandomState(7)
    obs = rng.uniform(-1, 1, (n, O)).astype(np.float32)
    u = rng.uniform(size=(n, A)).astype(np.float32)
    a, v, nlp = g.step(obs, u)
    assert a.shape == (n,) and v.shape == (n,) and nlp.shape == (n,)
    ra, rv, rnlp, pert = ref.step(obs, u)
    skipped = check_actions(a, ra, pert, "sampled actions")
    print("near-tie rows skipped: %d of %d" % (skipped, n))
    # neglogp of the action the kernel chose (identical to the reference's except on skipped rows)
    nlp_all, _, _ = softmax_stats(ref.forward(obs)[0])
    close(nlp, nlp_all[np.arange(n), a.astype(np.int64)], msg="neglogp")
    close(v, rv, msg="value")
    close(g.value(obs), rv, msg="ppo_value")
    logits = ref.forward(obs)[0]
    det = g.act_deterministic(obs)
    assert det.shape == (n,)
    top2 = np.sort(logits, axis=1)[:, -2:]
    ok = (top2[:, 1] - top2[:, 0]) < TIE
    assert np.all((det == np.argmax(logits, 1)) | ok)
    g.close()


@pytest.mark.gpu
def test_on_device_sampling_follows_softmax_and_is_seeded():
    O, A, N = 18, 6, 65536
    ref, g = make(O, A, (64, 64), seed=5, pi_gain=3.0)
    obs = np.repeat(np.random.RandomState(2).uniform(-1, 1, (1, O)), N, 0).astype(np.float32)
    _, _, p = softmax_stats(ref.forward(obs[:1])[0])
    g.seed(11)
    a1, _, nlp = g.step(obs)
    assert np.all(a1 == np.floor(a1)) and a1.min() >= 0 and a1.max() < A
    freq = np.bincount(a1.astype(np.int64), minlength=A) / N
    sigma = np.sqrt(p[0] * (1 - p[0]) / N)
    assert np.all(np.abs(freq - p[0]) <= 4 * sigma), (freq, p[0])
    close(nlp, -np.log(p[0][a1.astype(np.int64)]), msg="neglogp of the sampled categories")
    g.seed(11)
    a2, _, _ = g.step(obs)
    np.testing.assert_array_equal(a1, a2)
    g.seed(12)
    a3, _, _ = g.step(obs)
    assert not np.array_equal(a3, a1)
    g.close()


def synth_batch(ref, n, seed, cr=CR):
    """a seeded minibatch whose rows straddle both clip ranges but stay clear of their edges (see tests/helpers.synth_minibatch)"""
    rng = np.random.RandomState(seed)
    obs = rng.uniform(-1, 1, (n, ref.O)).astype(np.float32)
    a, v, nlp, _ = ref.step(obs, rng.uniform(size=(n, ref.A)))
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


@pytest.mark.gpu
@pytest.mark.parametrize("hidden,n", [((64, 64), 200), ((256, 256), 512)])
def test_three_train_steps_match_reference(hidden, n):
    ref, g = make(18, 18, hidden, seed=9, ent_coef=0.01)
    for it in range(3):
        batch = synth_batch(ref, n, 100 + it)
        losses = g.train_step(LR, CR, *batch)
        grad, norm = g.last_grad()
        ref_losses, ref_grad = ref.train_step(LR, CR, *batch)
        close(losses[:4], ref_losses[:4], rtol=1e-4, atol=1e-6, msg="losses it=%d" % it)
        assert abs(losses[4] - ref_losses[4]) <= 1.0 / n + 1e-6, ("clipfrac", losses[4], ref_losses[4])
        gs = np.abs(ref_grad).max()
        close(grad, ref_grad, rtol=2e-4, atol=2e-6 * gs, msg="grad it=%d" % it)
        close(norm, np.sqrt(np.dot(ref_grad, ref_grad)), rtol=1e-4, msg="norm it=%d" % it)
        close(g.get_flat(0), ref.theta, rtol=1e-4, atol=2e-6, msg="theta it=%d" % it)
        close(g.get_flat(1), ref.m, rtol=2e-4, atol=1e-7 * max(1.0, gs), msg="adam m it=%d" % it)
    g.close()


def ref_rollout(ref, seed, E, T, u):
    """runner.hpp:56-157 over the seeded synthetic env with the categorical reference policy (the env ignores the actions)"""
    from oracle import oracle as o
    nz = o.Normalizer(E, ref.O)
    raw, _, _ = o.seeded_env_step(seed, 0, E, 0, ref.O)
    obs, dones = nz.obs(raw), np.zeros(E, np.float32)
    ro = {k: [] for k in ("obs", "actions", "values", "neglogp", "dones", "rewards", "pert", "nlp_all")}
    for t in range(T):
        a, v, nlp, pert = ref.step(obs, u[t])
        nlp_all, _, _ = softmax_stats(ref.forward(obs)[0])
        for k, x in (("obs", obs), ("actions", a), ("values", v), ("neglogp", nlp), ("dones", dones), ("pert", pert), ("nlp_all", nlp_all)):
            ro[k].append(x)
        raw, rew, dones = o.seeded_env_step(seed, 0, E, t + 1, ref.O)
        obs = nz.obs(raw)
        ro["rewards"].append(nz.reward(rew, dones))
    ro = {k: np.array(x) for k, x in ro.items()}
    _, last_v = ref.forward(obs)
    from oracle import numpy_port as npp
    ro["returns"] = npp.gae(ro["rewards"].astype(np.float32), ro["values"].astype(np.float32), ro["dones"], last_v.astype(np.float32),
                            dones, GAMMA, LAM)
    return ro


def check_rollout(got, ro, msg):
    T, E = ro["values"].shape
    skipped = check_actions(got["actions"].reshape(-1), ro["actions"].reshape(-1).astype(np.float32), ro["pert"].reshape(T * E, -1), msg + " actions")
    print("%s: near-tie rows skipped: %d of %d" % (msg, skipped, T * E))
    for f in ("obs", "values", "rewards", "returns"):
        close(got[f], ro[f], rtol=2e-4, atol=2e-5, msg=msg + " " + f)
    # neglogp of the category the kernel chose (the reference's own choice except on skipped rows)
    want = np.take_along_axis(ro["nlp_all"].reshape(T * E, -1), got["actions"].reshape(-1, 1).astype(np.int64), 1).reshape(T, E)
    close(got["neglogp"], want, rtol=2e-4, atol=2e-5, msg=msg + " neglogp")


@pytest.mark.gpu
@pytest.mark.parametrize("E,T", [(1, 32), (64, 8), (4096, 2)])
def test_collect_synthetic_matches_reference(E, T):
    O, A = 18, 18
    ref, g = make(O, A, (64, 64), seed=E)
    u = np.random.RandomState(E).uniform(size=(T, E, A)).astype(np.float32)
    ro = ref_rollout(ref, 1234, E, T, u)
    g.norm_init(E)
    g.rollout_alloc(E, T)
    g.collect_synthetic(1234, GAMMA, LAM, u)
    got = {f: g.rollout_get(f) for f in ("obs", "actions", "values", "neglogp", "rewards", "returns")}
    assert got["actions"].shape == (T, E)
    check_rollout(got, ro, "collect E=%d" % E)
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("E,T", [(1, 16), (256, 4)])
def test_host_env_loop_matches_reference(E, T):
    from oracle import oracle as o
    O, A = 18, 7
    ref, g = make(O, A, (64, 64), seed=40 + E)
    u = np.random.RandomState(E + 1).uniform(size=(T, E, A)).astype(np.float32)
    ro = ref_rollout(ref, 99, E, T, u)
    g.norm_init(E)
    g.rollout_alloc(E, T)
    raw, _, _ = o.seeded_env_step(99, 0, E, 0, O)
    g.rollout_reset(raw)
    acts = []
    for t in range(T):
        a = g.rollout_act(t, u[t])
        assert a.shape == (E,)
        acts.append(a)
        raw, rew, dn = o.seeded_env_step(99, 0, E, t + 1, O)
        g.rollout_observe(t, raw, rew, dn)
    g.rollout_finish(GAMMA, LAM)
    got = {f: g.rollout_get(f) for f in ("obs", "actions", "values", "neglogp", "rewards", "returns")}
    np.testing.assert_array_equal(np.array(acts), got["actions"])
    check_rollout(got, ro, "host Env E=%d" % E)
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("hidden,E,T,nmb", [((64, 64), 32, 16, 4), ((256, 256), 256, 8, 4)])
def test_two_updates_with_explicit_perms_match_reference(hidden, E, T, nmb):
    O, A, epochs = 18, 18, 2
    ref, g = make(O, A, hidden, seed=17, ent_coef=0.01)
    g.norm_init(E)
    g.rollout_alloc(E, T)
    rng = np.random.RandomState(3)
    for it in range(2):
        u = rng.uniform(size=(T, E, A)).astype(np.float32)
        ro = ref_rollout(ref, 500 + it, E, T, u)
        ro["neglogp"] = (ro["neglogp"] + rng.normal(scale=0.1, size=(T, E))).astype(np.float32)   # move the ratio off 1
        ro["obs"] = ro["obs"].astype(np.float32)
        for f in ("obs", "actions", "values", "neglogp", "returns"):
            g.rollout_set(f, np.asarray(ro[f], np.float32))
        perms = np.stack([rng.permutation(E * T) for _ in range(epochs)]).astype(np.int32)
        rows, mean = g.update(LR, CR, epochs, nmb, perms)
        ref_in = {f: np.asarray(ro[f], np.float32) for f in ("obs", "actions", "values", "neglogp", "returns")}
        ref_rows, ref_mean = ref.update(ref_in, perms, nmb, LR, CR)
        close(rows[:, :4], ref_rows[:, :4], rtol=1e-4, atol=1e-6, msg="loss rows update %d" % it)
        assert np.all(np.abs(rows[:, 4] - ref_rows[:, 4]) <= nmb / (E * T) + 1e-6)
        close(mean[:4], ref_mean[:4], rtol=1e-4, atol=1e-6, msg="mean losses update %d" % it)
        close(g.get_flat(0), ref.theta, rtol=1e-4, atol=5e-6, msg="theta after update %d" % it)
        nodes = g.debug_graph_nodes()
        assert nodes is not None and nodes["kernel"] > 0, nodes
        assert nodes["memset"] == 0 and nodes["memcpy"] == 0 and nodes["other"] == 0, nodes
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("hidden", [(64, 64), (256, 256)])
def test_kernel_counts_show_the_categorical_variants_only(hidden):
    E, T = 64, 4
    ref, g = make(18, 18, hidden)
    g.norm_init(E)
    g.rollout_alloc(E, T)
    g.collect_synthetic(3, GAMMA, LAM)
    g.update(LR, CR, 1, 4, None, seed=1, want_rows=False)
    obs = np.zeros((20, 18), np.float32)
    g.step(obs)
    batch = synth_batch(ref, 64, 1)
    g.train_step(LR, CR, *batch)
    kc = g.kernel_counts()
    assert kc["policy_step_kernel<cat>"] > 0 and kc["train_fwd_bwd_kernel<cat>"] > 0, kc
    for name, cnt in kc.items():
        if name.startswith(("narrow_", "train8", "weight_grad_assemble", "bf16_")) or name in ("policy_step_kernel", "train_fwd_bwd_kernel"):
            assert cnt == 0, (name, kc)
    assert kc["weight_grad_kernel"] > 0 and kc["grad_reduce_kernel"] > 0, kc
    g.close()


@pytest.mark.gpu
def test_errors():
    import ppo_cpp_amd
    with pytest.raises(ppo_cpp_amd.PPOHipError, match="act_dim >= 2"):
        ppo_cpp_amd.PPOHip(18, 1, [64, 64], action_dist="categorical")
    with pytest.raises(ppo_cpp_amd.PPOHipError, match="PPO_BF16"):
        ppo_cpp_amd.PPOHip(18, 6, [256, 256], action_dist="categorical", compute_dtype=1)
    from ppo_cpp_amd.capi import PPOConfig
    lib = ppo_cpp_amd.load_library()
    cfg = PPOConfig()
    hid = (ctypes.c_int32 * 2)(64, 64)
    lib.ppo_config_default(ctypes.byref(cfg), 18, 6, 2, hid)
    h = ctypes.c_void_p()
    assert lib.ppo_create_ex(ctypes.byref(cfg), 2, ctypes.byref(h)) != 0
    assert b"unknown action_dist" in lib.ppo_last_error(None)
    ref, g = make(18, 6, (64, 64))
    obs, a, adv, ret, nlp, v = synth_batch(ref, 32, 0)
    theta = g.get_flat(0)
    for bad in (-1.0, 6.0, 2.5, np.nan):
        a2 = a.copy(); a2[5] = bad
        with pytest.raises(ppo_cpp_amd.PPOHipError, match="category index"):
            g.train_step(LR, CR, obs, a2, adv, ret, nlp, v)
    np.testing.assert_array_equal(g.get_flat(0), theta)          # nothing was trained
    g.train_step(LR, CR, obs, a, adv, ret, nlp, v)
    g.close()


@pytest.mark.gpu
def test_tensor_round_trip_into_a_fresh_handle():
    """weights, Adam slots and beta powers moved tensor by tensor (what a checkpoint carries) give identical tensors and deterministic actions"""
    import ppo_cpp_amd
    ref, g = make(18, 6, (64, 64), seed=4)
    g.train_step(LR, CR, *synth_batch(ref, 64, 2))
    g2 = ppo_cpp_amd.PPOHip(18, 6, [64, 64], action_dist="categorical")
    for which in (0, 1, 2):
        g2.set_flat(g.get_flat(which), which)
        np.testing.assert_array_equal(g2.get_flat(which), g.get_flat(which))
    g2.set_beta_powers(g.beta_powers())
    obs = np.random.RandomState(0).uniform(-1, 1, (300, 18)).astype(np.float32)
    np.testing.assert_array_equal(g2.act_deterministic(obs), g.act_deterministic(obs))
    gauss = ppo_cpp_amd.PPOHip(18, 6, [64, 64])
    assert gauss.P == g.P + 6 and gauss.lib.ppo_action_dist(gauss.h) == 0
    flat = g.get_flat(0)                                          # a categorical parameter vector does not fit a Gaussian handle
    assert gauss.lib.ppo_set_flat(gauss.h, 0, flat.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), ctypes.c_int64(g.P)) != 0
    for h in (g, g2, gauss):
        h.close()


@pytest.mark.gpu
def test_ppo2_checkpoint_of_a_categorical_policy(tmp_path):
    """PPO2::save finds pi/w by name, writes no pi/logstd and says "discrete"; PPO2::load into a fresh categorical handle restores every tensor
    (same deterministic actions), into a Gaussian handle it fails"""
    import json
    from ppo_cpp_amd import hostapi
    prefix = str(tmp_path / "cat")
    obs = np.random.RandomState(3).uniform(-1, 1, (200, 18)).astype(np.float32)
    rc, before, after = hostapi.discrete_checkpoint(prefix, obs)
    assert rc == 0, rc
    np.testing.assert_array_equal(before, after)
    assert set(np.unique(before)) <= set(range(6))
    assert json.load(open(prefix + ".json"))["action_space"] == "discrete"
    lib = hostapi.load_host_library()
    buf = np.zeros(64 * 6, np.float32); shape = (ctypes.c_longlong * 4)()
    fp = buf.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    assert lib.ppo_host_bundle_tensor(prefix.encode(), b"model/pi/logstd", fp, buf.size, shape) == -2
    assert lib.ppo_host_bundle_tensor(prefix.encode(), b"model/q/w", fp, buf.size, shape) == 64 * 6 and list(shape)[:2] == [64, 6]
    assert lib.ppo_host_bundle_tensor(prefix.encode(), b"model/pi/w", fp, buf.size, shape) == 64 * 6 and list(shape)[:2] == [64, 6]


@pytest.mark.gpu
def test_ppo2_learns_the_discrete_target_task():
    """Learning: DiscreteTargetEnv x 16 (host/env/env_mock.hpp: reward 1 when the category is argmax_j (W obs)_j with TargetEnv's W, 18 categories, episodes
    of 100 steps) behind VecEnv + EnvNormalize, 64 steps, [64,64], 150 updates of 4 epochs x 4 minibatches at lr 2e-3, through PPO2::learn with the library's
    own sampling and shuffles.  A uniform policy earns 1/18 = 0.056.  The NumPy reference loop (tests/categorical_ref.learn_loop with the oracle's EnvNormalize)
    over three draw seeds: first-15 -> last-15 mean reward 0.098 -> 0.437, 0.097 -> 0.411, 0.094 -> 0.427.
    RISE = 0.20: the last-15 mean over the first-15 (the reference rises by 0.31 - 0.34).
    BAND = 0.10: |last-15 mean - 0.425| (the reference's mean over the seeds; its seeds spread by 0.026, and the two legs differ in initial weights and draws).
    This leg on an MI355X: 0.087 -> 0.406."""
    from ppo_cpp_amd import hostapi
    RISE, BAND, REF_LAST15 = 0.20, 0.10, 0.425
    got = hostapi.learn_curve(16, 64, [64, 64], 150, 4, 4, 2e-3, 0.2, seed=11, act_dim=18, discrete=True)
    c = got["reward_curve"]
    first, last = c[:15].mean(), c[-15:].mean()
    print("reward curve first-15 %.3f last-15 %.3f" % (first, last))
    assert last - first >= RISE, (first, last)
    assert abs(last - REF_LAST15) <= BAND, (last, REF_LAST15)


@pytest.mark.gpu
def test_two_ranks_global_shuffle_equal_one_rank_over_the_union(tmp_path):
    """world 2 on the collective-library stand-in (two processes on one GPU, tests/fake_rccl), ppo_dist_global_shuffle(1): the rollout's actions
    travel through the all-gather one float per row, and the weights after one update equal a one-rank update over the union of the rows"""
    import subprocess
    import sys
    from tests.test_dp_two_ranks import build_fake_rccl
    world, hidden, E, T, nmb, epochs, A = 2, (64, 64), 32, 8, 4, 2, 6
    tmp = str(tmp_path)
    fake = build_fake_rccl(tmp)
    ref, g = make(18, A, hidden, seed=21)
    rng = np.random.RandomState(8)
    ro = ref_rollout(ref, 77, E, T, rng.uniform(size=(T, E, A)))
    ro = {f: np.asarray(ro[f], np.float32) for f in ("obs", "actions", "values", "neglogp", "returns")}
    ro["neglogp"] = (ro["neglogp"] + rng.normal(scale=0.1, size=(T, E))).astype(np.float32)
    gperms = np.stack([rng.permutation(E * T).astype(np.int32) for _ in range(epochs)])
    theta0 = ref.theta.astype(np.float32)
    uid = np.zeros(128, np.uint8)
    name = ("/ppo_dp_cat_%d_%d" % (os.getpid(), rng.randint(1 << 30))).encode()
    uid[:len(name)] = np.frombuffer(name, np.uint8)
    fin = os.path.join(tmp, "in.npz")
    np.savez(fin, hidden=np.array(hidden), E=E, T=T, nmb=nmb, epochs=epochs, A=A, theta=theta0, uid=uid, gperms=gperms, lr=LR, cr=CR,
             **{"ro_" + f: x for f, x in ro.items()})
    env = dict(os.environ, PPO_RCCL_LIBRARY=fake, HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "dp_worker_discrete.py"), str(r), str(world), fin, os.path.join(tmp, "out%d.npz" % r)],
                              env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(world)]
    logs = []
    for p in procs:
        try:
            logs.append(p.communicate(timeout=300)[0].decode())
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            pytest.fail("data-parallel workers timed out")
    assert all(p.returncode == 0 for p in procs), "\n".join(l[-3000:] for l in logs)
    outs = [np.load(os.path.join(tmp, "out%d.npz" % r)) for r in range(world)]
    # one rank over the union: same weights, same permutations, the same global minibatches of E * T / nmb rows
    g.norm_init(E, 0.99)
    g.rollout_alloc(E, T)
    for f, x in ro.items():
        g.rollout_set(f, x)
    rows, _ = g.update(LR, CR, epochs, nmb, gperms)
    theta1 = g.get_flat(0)
    g.close()
    for r, out in enumerate(outs):
        np.testing.assert_array_equal(out["actions"], ro["actions"][:, r * (E // world):(r + 1) * (E // world)])
        close(out["rows"][:, :4], rows[:, :4], rtol=2e-4, atol=2e-6, msg="loss rows rank %d" % r)
        close(out["theta"], theta1, rtol=2e-4, atol=5e-6, msg="weights rank %d" % r)
    for k in ("rows", "theta", "adam_m", "adam_v"):
        np.testing.assert_array_equal(outs[0][k], outs[1][k])
    assert np.abs(theta1 - theta0).max() > 0

"""The multi-binary head in the narrow LDS-resident kernels: ppo_create_ex(cfg, PPO_ACT_MULTI_BINARY | PPO_ACT_BINARY_SHAPE_KERNELS) /
PPOHip(action_dist="multi_binary", binary_shape_kernels=True) against the float64 BernRef (tests/bernoulli_ref.py).

Helpers, fixtures of logits and every tolerance are tests/test_multi_binary.py's (act 1e-4 / 1e-5; losses 1e-4 / 1e-6; clipfrac within a row; gradient 2e-4 with
2e-6 of its largest element; norm 1e-4; theta 1e-4 / 2e-6, 5e-6 behind an update; Adam m 2e-4; rollout fields 2e-4 / 2e-5); the policy queries take
tests/test_policy_query.py's.  None is derived here.

CPU tests: the define, the entry point, the keyword, the host layer's word, the counter names; and the input condition of the draw comparison -- under BernRef
alone, with the kernels' counter uniforms, nearly every element's uniform lies clear of its p, so the GPU comparison of the two kernel families' bits may leave out
only those elements.
GPU tests: step / train / trained logits / same draw as the generic family / collect, host-Env loop and update / the two rollout settings change nothing /
target-KL / queries behind training / fallbacks and errors / reproducibility / host layer."""
import ctypes
import inspect
import os

import numpy as np
import pytest

from tests.bernoulli_ref import BernRef, bern_stats
from tests.test_discrete_policy import CR, GAMMA, LAM, LR, close
from tests.test_multi_binary import (DET_TIE, FIELDS, NEAR, check_rollout, clear_uniforms, logit_table, make, ref_rollout, synth_batch, trained_case)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAG = {"binary_shape_kernels": True}
STEP, TRAIN = "narrow_step_kernel<mbin>", "narrow_train_kernel<mbin>"
GEN_STEP, GEN_TRAIN = "policy_step_kernel<mbin>", "train_fwd_bwd_kernel<mbin>"
# every narrow row a Gaussian handle can bump, and the forms this head does not have
GAUSS_NARROW = ("narrow_train_kernel<static>", "narrow_train_kernel<runtime>", "narrow_step_kernel<static>", "narrow_step_kernel<runtime>", "narrow_rollout1_kernel",
                "narrow_rollout_kernel", "narrow_rollout_coop_kernel", "narrow_collect_kernel", "narrow_epoch_kernel")
# (O, A, hidden): static <32,64,32,2> with 26 padding columns | static <64,64,32,2>, a second column register | runtime, Ap = 48 | runtime, Ap = 64, the fourth
# column register, no padding | runtime, one bit, 16-wide padded layers | three layers
SHAPES = [(18, 6, (64, 64)), (36, 18, (64, 64)), (50, 40, (64, 64)), (20, 64, (64, 64)), (7, 1, (4, 5)), (18, 18, (64, 32, 64))]
DRAW_SHAPES = [(18, 18), (36, 18), (50, 40), (20, 64)]     # behind [64,64]
DRAW_SEED, DRAW_ROWS = 5, 200


def flagged(O, A, hidden, **kw):
    return make(O, A, hidden, flags=FLAG, **kw)


def assert_narrow_only(kc, step=True, train=False):
    """ppo_kernel_counts_all of a handle the flag took effect on: the two <mbin> narrow names and nothing else with a head"""
    assert len(kc) == 62, len(kc)
    if step:
        assert kc[STEP] > 0, kc
    if train:
        assert kc[TRAIN] > 0, kc
    assert kc[GEN_STEP] == 0 and kc[GEN_TRAIN] == 0, kc
    for name, cnt in kc.items():
        if name in GAUSS_NARROW or "<cat" in name or "<mcat" in name or name.startswith(("narrow_host_step", "narrow_rollout<", "train8_kernel", "bf16_")):
            assert cnt == 0, (name, kc)
    assert kc["policy_step_kernel"] == 0 and kc["train_fwd_bwd_kernel"] == 0 and kc["policy_step_kernel<host_action>"] == 0, kc


def assert_generic_only(kc):
    assert kc[GEN_STEP] > 0 and kc[STEP] == 0 and kc[TRAIN] == 0, kc
    for name, cnt in kc.items():
        if name.startswith("narrow_"):
            assert cnt == 0, (name, kc)


# ---- CPU ---------------------------------------------------------------------------------------------------------------------
def test_flag_entry_point_and_keyword_exist():
    src = open(os.path.join(ROOT, "include", "ppo_hip.h")).read()
    assert "#define PPO_ACT_BINARY_SHAPE_KERNELS 0x2000" in src
    assert "ppo_kernel_counts_all(" in src
    assert "#define PPO_ABI_VERSION 3" in src
    import ppo_cpp_amd
    from ppo_cpp_amd import capi, hostapi
    assert capi.ACT_BINARY_SHAPE_KERNELS == 0x2000
    par = inspect.signature(ppo_cpp_amd.PPOHip.__init__).parameters
    assert par["binary_shape_kernels"].default is False
    assert inspect.signature(ppo_cpp_amd.PPOHip.kernel_counts).parameters["all_rows"].default is False
    with pytest.raises(ValueError, match="binary_shape_kernels"):
        ppo_cpp_amd.PPOHip(18, 6, [64, 64], action_dist="categorical", binary_shape_kernels=True)
    assert hostapi._discrete_kernels("binary_narrow") == 3
    with pytest.raises(ValueError, match="binary_narrow"):
        hostapi._discrete_kernels("bernoulli")


def test_counter_names_fit_the_callers_buffers():
    hip = open(os.path.join(ROOT, "ppo_cpp_amd", "csrc", "ppo_hip.hip")).read()
    for name in (STEP, TRAIN):
        assert len(name) < 32 and '"%s"' % name in hip, name
    assert "KV_LEGACY_COUNT = 60" in hip and "KV_NARROW_STEP_MBIN" in hip and "KV_NARROW_TRAIN_MBIN" in hip


def draw_case(O, A):
    """weights, observations, the kernels' counter uniforms of seed(DRAW_SEED) / the first step call, and which elements are clear of their p under BernRef"""
    from tests import counter_draws_ref as M
    ref = BernRef(O, A, (64, 64))
    ref.init_random(DRAW_SEED)
    ref.theta[:] = ref.theta.astype(np.float32)
    obs = np.random.RandomState(DRAW_SEED).uniform(-1, 1, (DRAW_ROWS, O)).astype(np.float32)
    u = M.counter_uniforms(M.seed_key(DRAW_SEED), np.arange(DRAW_ROWS), 0, A)
    p = bern_stats(ref.forward(obs)[0])[0]
    return ref, obs, u, p, np.abs(np.asarray(u, np.float64) - p) >= NEAR


@pytest.mark.parametrize("O,A", DRAW_SHAPES)
def test_counter_uniforms_are_nearly_all_clear_of_their_p(O, A):
    _, _, u, p, clear = draw_case(O, A)
    assert u.shape == p.shape == (DRAW_ROWS, A)
    print("clear share at (%d, %d): %.4f" % (O, A, clear.mean()))
    assert clear.mean() >= 0.995, clear.mean()


# ---- GPU ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("O,A,hidden", SHAPES)
@pytest.mark.parametrize("n", [1, 33, 200])
def test_step_matches_reference(O, A, hidden, n):
    from tests import counter_draws_ref as M
    ref, g = flagged(O, A, hidden, seed=n, pi_gain=3.0)
    assert g.binary_shape_kernels is True and g.lib.ppo_action_dist(g.h) == 3 and g.action_width == A
    rng = np.random.RandomState(7)
    obs = rng.uniform(-1, 1, (n, O)).astype(np.float32)
    u = clear_uniforms(ref, obs, rng.uniform(size=(n, A)))
    x, v, nlp = g.step(obs, u)
    assert x.shape == (n, A) and v.shape == (n,) and nlp.shape == (n,)
    rx, rv, rnlp, _ = ref.step(obs, u)
    np.testing.assert_array_equal(x, rx.astype(np.float32), err_msg="sampled bits")
    close(nlp, rnlp, msg="neglogp")
    close(v, rv, msg="value")
    close(g.value(obs), rv, msg="ppo_value")
    logits = ref.forward(obs)[0]
    det = g.act_deterministic(obs)
    assert det.shape == (n, A)
    sure = np.abs(logits) >= DET_TIE
    np.testing.assert_array_equal(det[sure], (logits > 0)[sure].astype(np.float32), err_msg="deterministic bits")
    assert set(np.unique(det)) <= {0.0, 1.0}
    # a counter-drawn step: whatever was drawn, its neglogp is the reference's neglogp of those bits; away from near-ties the bits are the model's
    g.seed(DRAW_SEED)
    xd, _, nlpd = g.step(obs)
    assert set(np.unique(xd)) <= {0.0, 1.0}
    close(nlpd, ref.neglogp_entropy(obs, xd)[0], msg="neglogp of the drawn bits")
    um = M.counter_uniforms(M.seed_key(DRAW_SEED), np.arange(n), 0, A)
    p = bern_stats(logits)[0]
    clear = np.abs(np.asarray(um, np.float64) - p) >= NEAR
    np.testing.assert_array_equal(xd[clear], (um < p)[clear].astype(np.float32), err_msg="counter-drawn bits")
    assert_narrow_only(g.kernel_counts(all_rows=True))
    legacy = g.kernel_counts()
    assert len(legacy) == 60 and STEP not in legacy and TRAIN not in legacy
    g.close()


def padded_action_width(A, hidden):
    return 32 if (len(hidden) == 2 and tuple(hidden) == (64, 64) and A <= 32) else 16 * ((A + 15) // 16)


def word_of(g, ref, tensor):
    """where the tensor's first element lives in the padded parameter vector (tests/test_head_edges.bias_word for any tensor)"""
    probe = np.zeros(g.P, np.float32)
    probe[ref.offs[tensor][0]] = 7.0
    g.set_flat(probe)
    at = np.nonzero(g.debug_buffer("theta").view(np.float32) == 7.0)[0]
    assert at.size == 1, (tensor, at)
    return int(at[0])


def padding_words(g, ref, A, hidden):
    """indices (into the padded vector) of pi/w's padding columns, pi/b's padding columns and the whole padded logstd region"""
    from tests.test_head_edges import bias_word
    Ap, HL = padded_action_width(A, hidden), ref.offs["pi/w"][1][0]
    wat, bat = word_of(g, ref, "pi/w"), bias_word(g, ref)
    probe = np.zeros(g.P, np.float32)
    o, shape = ref.offs["pi/w"]
    probe[o:o + HL * A] = np.arange(1, HL * A + 1)
    g.set_flat(probe)
    padded = g.debug_buffer("theta").view(np.float32)[wat:wat + HL * Ap].reshape(HL, Ap)
    np.testing.assert_array_equal(padded[:, :A], np.arange(1, HL * A + 1, dtype=np.float32).reshape(HL, A))     # the layout this helper assumes: [rows][Ap]
    assert not padded[:, A:].any()
    w = (wat + np.arange(HL)[:, None] * Ap + np.arange(A, Ap)[None, :]).reshape(-1)
    return np.concatenate([w, np.arange(bat + A, bat + 512)]).astype(np.int64), bat


@pytest.mark.gpu
@pytest.mark.parametrize("O,A,hidden", SHAPES)
@pytest.mark.parametrize("n", [33, 200])
def test_three_train_steps_match_reference(O, A, hidden, n):
    from tests.test_head_edges import assert_padding_gradient_is_zero
    ref, g = flagged(O, A, hidden, seed=9, ent_coef=0.01)
    pad, bat = padding_words(g, ref, A, hidden)
    g.set_flat(ref.theta.astype(np.float32))
    theta_pad0 = g.debug_buffer("theta")[pad].copy()
    assert not theta_pad0.any()
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
        assert_padding_gradient_is_zero(g, bat, A, "it=%d" % it)
        assert not g.debug_buffer("grad")[pad].any(), "it=%d: the gradient of a padding column / the logstd region is not zero" % it
    np.testing.assert_array_equal(g.debug_buffer("theta")[pad], theta_pad0, err_msg="padding columns / logstd region of theta moved")
    kc = g.kernel_counts(all_rows=True)
    assert kc[TRAIN] == 3, kc
    assert_narrow_only(kc, step=False, train=True)
    g.close()


@pytest.mark.gpu
def test_trained_logits():
    """tests/test_multi_binary.py's test of this name on the flagged handle: the head at trained and extreme logits"""
    from tests.test_head_edges import assert_padding_gradient_is_zero, bias_word, reset
    O, A, hidden, n = 18, 18, (64, 64), 32
    ref, g = flagged(O, A, hidden, ent_coef=0.01)
    pw0 = g.beta_powers()
    at = bias_word(g, ref)
    for name, bias in logit_table(A).items():
        c = trained_case(ref, name, bias, n)
        theta0 = ref.theta.copy()
        reset(g, theta0, pw0)
        ref.m[:] = 0; ref.v[:] = 0; ref.pow = [ref.b1, ref.b2]
        x, v, nlp = g.step(c["obs"], c["u"])
        np.testing.assert_array_equal(x, c["x"].astype(np.float32), err_msg=name + " sampled bits")
        p = bern_stats(c["logits"])[0]
        assert (x[p == 1.0] == 1.0).all() and (x[p == 0.0] == 0.0).all(), name
        rnlp, _ = ref.neglogp_entropy(c["obs"], c["x"])
        close(nlp, rnlp, msg=name + " neglogp")
        close(v, c["v"], msg=name + " value")
        det = g.act_deterministic(c["obs"])
        np.testing.assert_array_equal(det, (c["logits"] > 0).astype(np.float32), err_msg=name + " deterministic bits")
        if name == "zeros":
            assert not det.any(), "a logit of +-0 acts 0 deterministically"
        if name == "all+3072":
            assert (x == 1.0).all()
        if name == "all-200":
            assert (x == 0.0).all()
        batch = (c["obs"], c["xt"].astype(np.float32), c["adv"], c["ret"], c["old_nlp"], c["old_v"])
        losses = g.train_step(LR, CR, *batch)
        grad, norm = g.last_grad()
        ref_losses, ref_grad = ref.train_step(LR, CR, *batch)
        print("%s: forced rows %d, losses %s" % (name, c["forced"].sum(), losses))
        close(losses[:4], ref_losses[:4], rtol=1e-4, atol=1e-6, msg=name + " losses")
        close(losses[2], c["ent"].mean(), rtol=1e-4, atol=1e-6, msg=name + " entropy")
        assert abs(losses[4] - ref_losses[4]) <= 1.0 / n + 1e-6, (name, "clipfrac", losses[4], ref_losses[4])
        gs = np.abs(ref_grad).max()
        close(grad, ref_grad, rtol=2e-4, atol=2e-6 * gs, msg=name + " grad")
        close(norm, np.sqrt(np.dot(ref_grad, ref_grad)), rtol=1e-4, msg=name + " norm")
        close(g.get_flat(0), ref.theta, rtol=1e-4, atol=2e-6, msg=name + " theta")
        close(g.get_flat(1), ref.m, rtol=2e-4, atol=1e-7 * max(1.0, gs), msg=name + " adam m")
        for t in ("pi_fc0/w", "pi_fc0/b", "pi_fc1/w", "pi_fc1/b"):          # pi/w = 0: nothing flows below the head, exactly
            o, shape = ref.offs[t]
            assert not grad[o:o + int(np.prod(shape))].any(), (name, t)
        assert_padding_gradient_is_zero(g, at, A, name)
    assert_narrow_only(g.kernel_counts(all_rows=True), train=True)
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("O,A", DRAW_SHAPES)
def test_same_seed_draws_what_the_generic_family_draws(O, A):
    import ppo_cpp_amd
    ref, obs, u, p, clear = draw_case(O, A)
    out = []
    for flags in (FLAG, {}):
        g = ppo_cpp_amd.PPOHip(O, A, [64, 64], action_dist="multi_binary", **flags)
        g.set_flat(ref.theta.astype(np.float32))
        g.seed(DRAW_SEED)
        x, _, nlp = g.step(obs)
        kc = g.kernel_counts(all_rows=True)
        assert (kc[STEP], kc[GEN_STEP]) == ((1, 0) if flags else (0, 1)), kc
        out.append((x, nlp))
        g.close()
    (xn, nlpn), (xg, nlpg) = out
    print("clear share %.4f, bits that differ among the others: %d" % (clear.mean(), (xn != xg)[~clear].sum()))
    np.testing.assert_array_equal(xn[clear], xg[clear], err_msg="bits on the clear elements")
    np.testing.assert_array_equal(xn[clear], (u < p)[clear].astype(np.float32), err_msg="bits against the counter model")
    same = (xn == xg).all(axis=1)
    close(nlpn[same], nlpg[same], msg="neglogp")
    close(nlpn, ref.neglogp_entropy(obs, xn)[0], msg="neglogp of the narrow family's bits")
    close(nlpg, ref.neglogp_entropy(obs, xg)[0], msg="neglogp of the generic family's bits")


def host_env_loop(g, ref, seed, E, T, u):
    from oracle import oracle as o
    O = ref.O
    g.norm_init(E)
    g.rollout_alloc(E, T)
    raw, _, _ = o.seeded_env_step(seed, 0, E, 0, O)
    g.rollout_reset(raw)
    acts = []
    for t in range(T):
        acts.append(g.rollout_act(t, u[t]))
        raw, rew, dn = o.seeded_env_step(seed, 0, E, t + 1, O)
        g.rollout_observe(t, raw, rew, dn)
    g.rollout_finish(GAMMA, LAM)
    got = {f: g.rollout_get(f) for f in FIELDS}
    np.testing.assert_array_equal(np.array(acts), got["actions"])
    return got


NO_ROLLOUT_FORMS = ("narrow_rollout1_kernel", "narrow_rollout_kernel", "narrow_rollout_coop_kernel", "narrow_collect_kernel", "narrow_epoch_kernel")


@pytest.mark.gpu
@pytest.mark.parametrize("E", [3, 40])
def test_collect_and_two_updates_match_reference(E):
    O, A, T, epochs, nmb = 18, 18, 4, 2, 2 if E == 3 else 4
    ref, g = flagged(O, A, (64, 64), seed=17 + E, ent_coef=0.01)
    rng = np.random.RandomState(3)
    for it in range(2):
        before = g.kernel_counts(all_rows=True)
        ro, u = ref_rollout(ref, 500 + it, E, T, rng.uniform(size=(T, E, A)))
        g.norm_init(E)
        g.rollout_alloc(E, T)
        g.collect_synthetic(500 + it, GAMMA, LAM, u)
        check_rollout({f: g.rollout_get(f) for f in FIELDS}, ro, "collect %d E=%d" % (it, E))
        kc = g.kernel_counts(all_rows=True)
        assert T <= kc[STEP] - before[STEP] <= T + 1, (kc, before)      # one per env step (and the bootstrap value's)
        ro["neglogp"] = (ro["neglogp"] + rng.normal(scale=0.1, size=(T, E))).astype(np.float32)   # move the ratio off 1
        ref_in = {f: np.asarray(ro[f], np.float32) for f in ("obs", "actions", "values", "neglogp", "returns")}
        for f, x in ref_in.items():
            g.rollout_set(f, x)
        perms = np.stack([rng.permutation(E * T) for _ in range(epochs)]).astype(np.int32)
        rows, mean = g.update(LR, CR, epochs, nmb, perms)
        ref_rows, ref_mean = ref.update(ref_in, perms, nmb, LR, CR)
        close(rows[:, :4], ref_rows[:, :4], rtol=1e-4, atol=1e-6, msg="loss rows update %d" % it)
        assert np.all(np.abs(rows[:, 4] - ref_rows[:, 4]) <= nmb / (E * T) + 1e-6)
        close(mean[:4], ref_mean[:4], rtol=1e-4, atol=1e-6, msg="mean losses update %d" % it)
        close(g.get_flat(0), ref.theta, rtol=1e-4, atol=5e-6, msg="theta after update %d" % it)
    kc = g.kernel_counts(all_rows=True)
    assert_narrow_only(kc, train=True)
    g.close()


@pytest.mark.gpu
def test_host_env_loop_matches_reference():
    O, A, E, T = 18, 7, 5, 6
    ref, g = flagged(O, A, (64, 64), seed=45, pi_gain=3.0)
    ro, u = ref_rollout(ref, 99, E, T, np.random.RandomState(E + 1).uniform(size=(T, E, A)))
    got = host_env_loop(g, ref, 99, E, T, u)
    check_rollout(got, ro, "host Env E=%d" % E)
    kc = g.kernel_counts(all_rows=True)
    assert T <= kc[STEP] <= T + 1, kc                          # one per env step (and the bootstrap value's)
    assert_narrow_only(kc)
    g.close()


def both_rollouts(settings):
    """the host-Env loop at E = 5 and a device-env collect with on-device draws on a fresh flagged handle; settings: both rollout settings on"""
    O, A, E, T = 18, 7, 5, 6
    ref, g = flagged(O, A, (64, 64), seed=45, pi_gain=3.0)
    if settings:
        g.set_host_step_fused(True)
        g.set_rollout_resident(True)
        assert g.host_step_fused and g.rollout_resident
    u = np.random.RandomState(E + 1).uniform(size=(T, E, A)).astype(np.float32)
    host = host_env_loop(g, ref, 99, E, T, u)
    g.norm_init(E)
    g.rollout_alloc(E, T)
    g.seed(DRAW_SEED)
    g.collect_synthetic(77, GAMMA, LAM)
    dev = {f: g.rollout_get(f) for f in FIELDS}
    kc = g.kernel_counts(all_rows=True)
    g.close()
    return host, dev, kc


@pytest.mark.gpu
def test_host_step_fused_and_rollout_resident_change_nothing():
    host0, dev0, kc0 = both_rollouts(False)
    host1, dev1, kc1 = both_rollouts(True)
    for f in FIELDS:
        np.testing.assert_array_equal(host1[f], host0[f], err_msg="host Env " + f)
        np.testing.assert_array_equal(dev1[f], dev0[f], err_msg="device env " + f)
    assert kc1 == kc0, (kc1, kc0)
    assert_narrow_only(kc0)
    assert set(np.unique(dev0["actions"])) <= {0.0, 1.0}


@pytest.mark.gpu
def test_target_kl_stops_where_the_generic_family_stops():
    import ppo_cpp_amd
    O, A, E, T, epochs, nmb = 18, 18, 16, 8, 2, 4
    total = epochs * nmb
    ref = BernRef(O, A, (64, 64))
    ref.init_random(23)
    ref.theta[:] = ref.theta.astype(np.float32)
    theta0 = ref.theta.astype(np.float32)
    rng = np.random.RandomState(4)
    ro, _ = ref_rollout(ref, 321, E, T, rng.uniform(size=(T, E, A)))
    ro = {f: np.asarray(ro[f], np.float32) for f in ("obs", "actions", "values", "neglogp", "returns")}
    perms = np.stack([rng.permutation(E * T) for _ in range(epochs)]).astype(np.int32)
    lr = 20 * LR                                                # (large enough that approxkl grows step by step)

    def run(flags, target_kl):
        g = ppo_cpp_amd.PPOHip(O, A, [64, 64], action_dist="multi_binary", **flags)
        g.set_flat(theta0)
        g.norm_init(E)
        g.rollout_alloc(E, T)
        for f, x in ro.items():
            g.rollout_set(f, x)
        g.set_target_kl(target_kl)
        rows, _ = g.update(lr, CR, epochs, nmb, perms)
        out = (rows, g.update_applied(), g.get_flat(0), g.kernel_counts(all_rows=True))
        g.close()
        return out

    rows_off, applied_off, theta_off, _ = run({}, 0.0)
    assert applied_off == (total, total)
    kl = rows_off[:, 3].astype(np.float64)
    print("unflagged approxkl rows", kl)
    # the first step s of the second epoch whose approxkl lies 10 % over every earlier one: the limit is the geometric mean of the two, about 5 % clear of both sides
    s = next(i for i in range(nmb, total) if kl[i] >= 1.1 * kl[:i].max())
    limit = float(np.sqrt(kl[s] * kl[:s].max()))
    x = limit / 1.5
    rows_g, applied_g, theta_g, _ = run({}, x)
    rows_n, applied_n, theta_n, kc = run(FLAG, x)
    print("limit %.4g: unflagged applied %s, flagged applied %s; flagged approxkl %s" % (limit, applied_g, applied_n, rows_n[:, 3]))
    assert applied_g == (s, total) and s >= nmb, (applied_g, s)
    assert applied_n == applied_g
    close(theta_n, theta_g, rtol=1e-4, atol=5e-6, msg="theta behind the stopped update")
    assert np.abs(theta_g - theta_off).max() > 0
    assert kc[TRAIN] > 0 and kc[GEN_TRAIN] == 0, kc
    _, applied_n_off, theta_n_off, _ = run(FLAG, 0.0)
    assert applied_n_off == (total, total)
    close(theta_n_off, theta_off, rtol=1e-4, atol=5e-6, msg="theta with early stopping off")


@pytest.mark.gpu
def test_policy_queries_behind_training_see_the_new_weights():
    """the narrow train forms do not keep the small-parameter mirror current: the first query behind a train step refreshes it"""
    from tests.test_policy_query import close as qclose, prob_bound
    O, A, n = 18, 18, 64
    ref, g = flagged(O, A, (64, 64), seed=31)
    rng = np.random.RandomState(1)
    obs = rng.uniform(-2, 2, (n, O)).astype(np.float32)
    acts = (rng.uniform(size=(n, A)) < 0.5).astype(np.float32)
    v0, nlp0, _ = g.evaluate_actions(obs, acts)
    for it in range(2):
        batch = synth_batch(ref, 96, 40 + it)
        g.train_step(50 * LR, CR, *batch)
        ref.train_step(50 * LR, CR, *batch)
    v, nlp, ent = g.evaluate_actions(obs, acts)
    logits, rv = ref.forward(obs)
    p, nlp1, nlp0_, rent = bern_stats(logits)
    qclose(v, rv, "value"); qclose(nlp, np.where(acts > 0, nlp1, nlp0_).sum(axis=1), "neglogp"); qclose(ent, rent.sum(axis=1), "entropy")
    assert np.abs(v - v0).max() > 1e-3 and np.abs(nlp - nlp0).max() > 1e-3, "two train steps did not move the queried policy"
    prob = g.action_probability(obs).astype(np.float64)
    assert prob.shape == (n, A)
    over = np.abs(prob - p) / prob_bound(p)
    assert over.max() <= 1.0, over.max()
    assert_narrow_only(g.kernel_counts(all_rows=True), step=False, train=True)
    g.close()


@pytest.mark.gpu
def test_fallbacks_run_the_generic_kernels(monkeypatch):
    import ppo_cpp_amd
    monkeypatch.setenv("PPO_RCCL_LIBRARY", "/nonexistent/no_collective_library.so")       # ppo_dist_init gets as far as loading it, no further
    cases = [("wide", 18, 18, (256, 256), False), ("A = 80", 18, 80, (64, 64), False), ("PPO_HIP_NO_NARROW", 18, 18, (64, 64), True)]
    for tag, O, A, hidden, env in cases:
        if env:
            monkeypatch.setenv("PPO_HIP_NO_NARROW", "1")
        ref, g = flagged(O, A, hidden, seed=3, pi_gain=3.0)
        rng = np.random.RandomState(7)
        obs = rng.uniform(-1, 1, (40, O)).astype(np.float32)
        u = clear_uniforms(ref, obs, rng.uniform(size=(40, A)))
        x, v, nlp = g.step(obs, u)
        rx, rv, rnlp, _ = ref.step(obs, u)
        np.testing.assert_array_equal(x, rx.astype(np.float32), err_msg=tag + " sampled bits")
        close(nlp, rnlp, msg=tag + " neglogp")
        close(v, rv, msg=tag + " value")
        g.train_step(LR, CR, *synth_batch(ref, 32, 1))
        kc = g.kernel_counts(all_rows=True)
        assert_generic_only(kc)
        assert kc[GEN_TRAIN] == 1, (tag, kc)
        with pytest.raises(ppo_cpp_amd.PPOHipError, match="PPO_RCCL_LIBRARY: cannot load"):    # not the flag's refusal
            g.dist_init(1, 0, bytes(128))
        g.step(obs, u)
        g.close()


@pytest.mark.gpu
def test_errors():
    import ppo_cpp_amd
    from ppo_cpp_amd.capi import PPOConfig
    lib = ppo_cpp_amd.load_library()
    cfg = PPOConfig()
    hid = (ctypes.c_int32 * 2)(64, 64)
    lib.ppo_config_default(ctypes.byref(cfg), 18, 6, 2, hid)
    h = ctypes.c_void_p()
    for dist in (0 | 0x2000, 1 | 0x2000):
        assert lib.ppo_create_ex(ctypes.byref(cfg), dist, ctypes.byref(h)) != 0
        msg = lib.ppo_last_error(None)
        assert b"unknown action_dist" in msg and b"PPO_ACT_BINARY_SHAPE_KERNELS" in msg, msg
    nv = (ctypes.c_int32 * 2)(3, 3)
    assert lib.ppo_create_multi_ex(ctypes.byref(cfg), nv, 2, 0x2000, ctypes.byref(h)) != 0
    assert b"unknown flag bit 0x2000" in lib.ppo_last_error(None)      # (ppo_create_multi_ex's own check stands in front of ppo_create_ex's)
    cfg.compute_dtype = 1
    assert lib.ppo_create_ex(ctypes.byref(cfg), 3 | 0x2000, ctypes.byref(h)) != 0
    assert b"PPO_BF16" in lib.ppo_last_error(None)
    with pytest.raises(ppo_cpp_amd.PPOHipError, match="PPO_BF16"):
        ppo_cpp_amd.PPOHip(18, 6, [64, 64], action_dist="multi_binary", binary_shape_kernels=True, compute_dtype=1)
    ref, g = flagged(18, 6, (64, 64))
    with pytest.raises(ppo_cpp_amd.PPOHipError, match="data parallel is not supported for a multi-binary handle created with PPO_ACT_BINARY_SHAPE_KERNELS"):
        g.dist_init(1, 0, bytes(128))
    obs, x, adv, ret, nlp, v = synth_batch(ref, 32, 0)
    g.step(obs)                                                     # usable after the refusal
    theta = g.get_flat(0)
    for bad in (0.5, 2.0, -1.0, np.nan):
        x2 = x.copy(); x2[5, 3] = bad
        with pytest.raises(ppo_cpp_amd.PPOHipError, match="row 5, column 3"):
            g.train_step(LR, CR, obs, x2, adv, ret, nlp, v)
        g.step(obs)
    mask = np.ones((32, 6), np.float32)
    with pytest.raises(ppo_cpp_amd.PPOHipError, match="action masks need a categorical"):
        g.step(obs, mask=mask)
    with pytest.raises(ppo_cpp_amd.PPOHipError, match="action masks need a categorical"):
        g.act_deterministic(obs, mask=mask)
    with pytest.raises(ppo_cpp_amd.PPOHipError, match="action masks need a categorical"):
        g.train_step(LR, CR, obs, x, adv, ret, nlp, v, mask=mask)
    with pytest.raises(ppo_cpp_amd.PPOHipError, match="action masks need a categorical"):
        g.set_action_masking(True)
    np.testing.assert_array_equal(g.get_flat(0), theta)            # nothing was trained
    g.train_step(LR, CR, obs, x, adv, ret, nlp, v)
    assert np.abs(g.get_flat(0) - theta).max() > 0
    kc = g.kernel_counts(all_rows=True)
    assert kc[TRAIN] == 1, kc
    assert_narrow_only(kc, train=True)
    g.close()


def seeded_run():
    E, T = 24, 4
    _, g = flagged(18, 18, (64, 64), seed=6)
    g.seed(DRAW_SEED)
    g.norm_init(E)
    g.rollout_alloc(E, T)
    g.collect_synthetic(11, GAMMA, LAM)
    bits = g.rollout_get("actions")
    rows, _ = g.update(LR, CR, 2, 4, None, seed=3)
    out = (bits, g.rollout_get("neglogp"), rows, g.get_flat(0))
    kc = g.kernel_counts(all_rows=True)
    g.close()
    return out, kc


@pytest.mark.gpu
def test_run_twice_same_bits():
    a, kca = seeded_run()
    b, kcb = seeded_run()
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)
    assert kca == kcb
    assert_narrow_only(kca, train=True)
    assert a[0].any() and not a[0].all()


@pytest.mark.gpu
def test_host_layer_runs_the_narrow_kernels(tmp_path):
    import json
    from ppo_cpp_amd import hostapi
    got = hostapi.learn_curve(16, 64, [64, 64], 10, 4, 4, 2e-3, 0.2, act_dim=18, binary=True, discrete_kernels="binary_narrow")
    kc = got["kernel_counts"]
    assert kc[STEP] > 0 and kc[TRAIN] > 0 and kc[GEN_STEP] == 0 and kc[GEN_TRAIN] == 0, kc
    assert np.isfinite(got["reward_curve"]).all() and np.isfinite(got["losses"]).all()
    assert got["reward_curve"].shape == (10,)
    prefix = str(tmp_path / "mbin_narrow")
    obs = np.random.RandomState(3).uniform(-1, 1, (50, 18)).astype(np.float32)
    rc, before, after = hostapi.binary_checkpoint(prefix, obs, discrete_kernels="binary_narrow")
    assert rc == 0, rc
    np.testing.assert_array_equal(before, after)
    assert set(np.unique(before)) <= {0.0, 1.0}
    assert json.load(open(prefix + ".json"))["action_binary"] is True

"""The multi-binary head in the [256,256] train kernel pair: ppo_create_ex(cfg, PPO_ACT_MULTI_BINARY | PPO_ACT_BINARY_PAIR_KERNELS) /
PPOHip(action_dist="multi_binary", binary_pair_kernels=True) -- train8_kernel<mbin> + weight_grad_assemble_kernel -- against the float64 BernRef
(tests/bernoulli_ref.py).

Helpers and every tolerance are tests/test_multi_binary.py's (losses 1e-4 / 1e-6; clipfrac within a row; gradient 2e-4 with 2e-6 of its largest element; norm
1e-4; theta 1e-4 / 2e-6, 5e-6 behind an update; Adam m 2e-4 / 1e-7 max(1, largest gradient element)); with more than 32 bits the gradient takes 4e-6 of its
largest element, what tests/test_pair_categorical.py gives the pair's 64-column tile; the policy queries take tests/test_policy_query.py's bounds.
One tolerance is derived here, Adam's second moment (no earlier file compares it): v is a sum of (1 - beta2) g^2 terms, so an element's relative error is twice
its gradient's (2 x 2e-4), and where the gradient's absolute term a = (2e-6 or 4e-6) x the largest element gs holds instead, a term's error is at most
(1 - beta2) (2 gs a + a^2); a step adds one such term to the decayed sum of the earlier ones, hence `steps` of them.

CPU tests: the define, the two entry points, the refusal text, the keyword, the host layer's word, the counter name.
GPU tests: train steps on every PAIR_DISPATCH branch / trained logits / flagged against unflagged / update and graph replay / changing row counts / same state,
same bits / target-KL / queries behind training / the two switches / fallbacks / errors / counters / host layer."""
import ctypes
import inspect
import os

import numpy as np
import pytest

from tests.bernoulli_ref import BernRef, bern_stats
from tests.test_discrete_policy import CR, LR, close
from tests.test_multi_binary import clear_uniforms, logit_table, make, ref_rollout, synth_batch, trained_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HID = (256, 256)
FLAG = {"binary_pair_kernels": True}
T8, DW2 = "train8_kernel<mbin>", "weight_grad_assemble_kernel"
GEN_STEP, GEN_TRAIN = "policy_step_kernel<mbin>", "train_fwd_bwd_kernel<mbin>"
REFUSAL = "ppo_dist_init: data parallel is not supported for a multi-binary handle created with PPO_ACT_BINARY_PAIR_KERNELS (create it without the flag)"
# (O, A): one per PAIR_DISPATCH branch (32/32, 64/32, 32/64, 64/64) | one element in the second column tile | no padding column | one bit
SHAPES = [(18, 6), (36, 18), (18, 40), (50, 64), (18, 33), (18, 32), (7, 1)]


def flagged(O, A, hidden=HID, **kw):
    return make(O, A, hidden, flags=FLAG, **kw)


def grad_atol(A):
    return 4e-6 if A > 32 else 2e-6


def delta(after, before):
    return {k: after[k] - before.get(k, 0) for k in after if after[k] != before.get(k, 0)}


def check_step(g, ref, batch, n, A, tag, steps):
    """one train step of the handle and of the reference on `batch`: losses, clipfrac, gradient, norm, theta, Adam m and v (`steps`: train steps so far, this one included)"""
    losses = g.train_step(LR, CR, *batch)
    grad, norm = g.last_grad()
    ref_losses, ref_grad = ref.train_step(LR, CR, *batch)
    close(losses[:4], ref_losses[:4], rtol=1e-4, atol=1e-6, msg="losses " + tag)
    assert abs(losses[4] - ref_losses[4]) <= 1.0 / n + 1e-6, ("clipfrac", tag, losses[4], ref_losses[4])
    gs = np.abs(ref_grad).max()
    a = grad_atol(A) * gs
    close(grad, ref_grad, rtol=2e-4, atol=a, msg="grad " + tag)
    close(norm, np.sqrt(np.dot(ref_grad, ref_grad)), rtol=1e-4, msg="norm " + tag)
    close(g.get_flat(0), ref.theta, rtol=1e-4, atol=2e-6, msg="theta " + tag)
    close(g.get_flat(1), ref.m, rtol=2e-4, atol=1e-7 * max(1.0, gs), msg="adam m " + tag)
    close(g.get_flat(2), ref.v, rtol=4e-4, atol=steps * (1.0 - ref.b2) * (2.0 * gs * a + a * a), msg="adam v " + tag)
    return losses, grad


# ---- CPU ---------------------------------------------------------------------------------------------------------------------
def test_header_states_the_flag_the_entry_points_and_the_refusal():
    src = open(os.path.join(ROOT, "include", "ppo_hip.h")).read()
    assert "#define PPO_ACT_BINARY_PAIR_KERNELS 0x4000" in src
    assert "ppo_kernel_count(const ppo_handle* h, const char* name);" in src
    assert "ppo_kernel_variant_name(int32_t i);" in src
    assert "#define PPO_ABI_VERSION 3" in src
    flat = " ".join(src.replace(" *", " ").split())
    assert REFUSAL in flat


def test_counter_name_fits_the_callers_buffers():
    hip = open(os.path.join(ROOT, "ppo_cpp_amd", "csrc", "ppo_hip.hip")).read()
    assert len(T8) == 19 and len(T8) < 32 and '"%s"' % T8 in hip
    assert "KV_TRAIN8_MBIN" in hip and "KV_LEGACY_COUNT = 60" in hip


def test_keyword_flag_and_host_word():
    import ppo_cpp_amd
    from ppo_cpp_amd import capi, hostapi
    assert capi.ACT_BINARY_PAIR_KERNELS == 0x4000
    par = inspect.signature(ppo_cpp_amd.PPOHip.__init__).parameters
    assert par["binary_pair_kernels"].default is False
    assert callable(ppo_cpp_amd.PPOHip.kernel_count) and callable(ppo_cpp_amd.PPOHip.kernel_variants)
    with pytest.raises(ValueError, match="binary_pair_kernels belongs to action_dist='multi_binary'"):
        ppo_cpp_amd.PPOHip(18, 6, [256, 256], action_dist="categorical", binary_pair_kernels=True)
    with pytest.raises(ValueError, match="binary_pair_kernels"):
        ppo_cpp_amd.PPOHip(18, 6, [256, 256], binary_pair_kernels=True)
    assert hostapi._discrete_kernels("binary_pair") == 4
    with pytest.raises(ValueError, match="binary_pair"):
        hostapi._discrete_kernels("bernoulli")


# ---- GPU ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", [100, 16])
@pytest.mark.parametrize("O,A", SHAPES)
def test_three_train_steps_match_reference(O, A, n):
    """n = 100: a partly dead tile and whole dead tiles up to the 64-row chunk; n = 16: one live tile, three dead ones"""
    ref, g = flagged(O, A, seed=9, ent_coef=0.01)
    assert g.binary_pair_kernels is True and g.lib.ppo_action_dist(g.h) == 3 and g.action_width == A
    for it in range(3):
        check_step(g, ref, synth_batch(ref, n, 100 + it), n, A, "it=%d" % it, it + 1)
    assert g.kernel_count(T8) == 3 and g.kernel_count(DW2) == 3 and g.kernel_count(GEN_TRAIN) == 0, g.kernel_variants()
    assert g.kernel_count("weight_grad_kernel") == 0 and g.kernel_count("grad_reduce_kernel") == 0
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("A", [18, 40])
def test_trained_logits(A):
    """tests/test_narrow_multi_binary.py's test of this name on the pair: the head at trained and extreme logits (the init's sit near 0)"""
    from tests.test_head_edges import assert_padding_gradient_is_zero, bias_word, reset
    O, n = 18, 32
    ref, g = flagged(O, A, ent_coef=0.01)
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
        close(grad, ref_grad, rtol=2e-4, atol=grad_atol(A) * gs, msg=name + " grad")
        close(norm, np.sqrt(np.dot(ref_grad, ref_grad)), rtol=1e-4, msg=name + " norm")
        close(g.get_flat(0), ref.theta, rtol=1e-4, atol=2e-6, msg=name + " theta")
        close(g.get_flat(1), ref.m, rtol=2e-4, atol=1e-7 * max(1.0, gs), msg=name + " adam m")
        for t in ("pi_fc0/w", "pi_fc0/b", "pi_fc1/w", "pi_fc1/b"):          # pi/w = 0: nothing flows below the head, exactly
            o, shape = ref.offs[t]
            assert not grad[o:o + int(np.prod(shape))].any(), (name, t)
        assert_padding_gradient_is_zero(g, at, A, name)
    assert g.kernel_count(T8) == len(logit_table(A)) and g.kernel_count(GEN_TRAIN) == 0
    g.close()


@pytest.mark.gpu
def test_flagged_against_unflagged():
    from tests.test_pair_categorical import padded_logstd_region
    O, A, n = 18, 40, 100
    ref, gp = flagged(O, A, seed=6, ent_coef=0.01)
    _, gg = make(O, A, HID, seed=6, ent_coef=0.01)
    off, width, size = padded_logstd_region(O, A)
    before = {k: gp.debug_buffer(k).view(np.float32).copy() for k in ("theta", "adam_m", "adam_v")}
    assert before["theta"].size == size
    # every padding element of the vector (the logstd region among them): where a flat vector of ones does not land
    _, probe = flagged(O, A, seed=6)
    probe.set_flat(np.ones(probe.P, np.float32))
    pad = probe.debug_buffer("theta").view(np.float32) != 1.0
    probe.close()
    assert pad[off:off + width].all() and pad.sum() == size - gp.P
    rng = np.random.RandomState(5)
    obs = rng.uniform(-1, 1, (n, O)).astype(np.float32)
    u = rng.uniform(size=(n, A)).astype(np.float32)
    for x, y in zip(gp.step(obs, u), gg.step(obs, u)):
        np.testing.assert_array_equal(x, y)
    np.testing.assert_array_equal(gp.act_deterministic(obs), gg.act_deterministic(obs))
    for it in range(3):
        batch = synth_batch(ref, n, 40 + it)
        lp, lg = gp.train_step(LR, CR, *batch), gg.train_step(LR, CR, *batch)
        ref.train_step(LR, CR, *batch)
        close(lp[:4], lg[:4], rtol=1e-4, atol=1e-6, msg="losses it=%d" % it)
        assert abs(lp[4] - lg[4]) <= 1.0 / n + 1e-6
        (grp, np_), (grg, ng) = gp.last_grad(), gg.last_grad()
        close(grp, grg, rtol=2e-4, atol=grad_atol(A) * np.abs(grg).max(), msg="grad it=%d" % it)
        close(np_, ng, rtol=1e-4, msg="norm")
        close(gp.get_flat(0), gg.get_flat(0), rtol=1e-4, atol=2e-6, msg="theta it=%d" % it)
    kp, kg = gp.kernel_variants(), gg.kernel_variants()
    assert kp[T8] == 3 and kp[GEN_TRAIN] == 0 and kp[DW2] == 3 and kp["weight_grad_kernel"] == 0 and kp["grad_reduce_kernel"] == 0, kp
    assert kg[GEN_TRAIN] == 3 and kg[T8] == 0 and kg[DW2] == 0 and kg["weight_grad_kernel"] == 3 and kg["grad_reduce_kernel"] == 3, kg
    assert kp[GEN_STEP] == kg[GEN_STEP] > 0, (kp, kg)                # the act kernels are the same
    for k, b in before.items():
        now = gp.debug_buffer(k).view(np.float32)
        np.testing.assert_array_equal(now[off:off + width], b[off:off + width], err_msg="padded logstd region of " + k)
        np.testing.assert_array_equal(now[pad], b[pad], err_msg="padding of " + k)
        assert not b[pad].any()
    gtail = gp.debug_buffer("grad").view(np.float32)
    assert not gtail[off:off + width].any(), "the padded logstd region of the gradient holds zeros on the pair path"
    gp.close(); gg.close()


@pytest.mark.gpu
def test_update_matches_reference_and_replays():
    """16 environments x 16 steps, 4 minibatches (64 rows each), 2 epochs, explicit permutations; the second update replays the captured graph"""
    O, A, E, T, nmb, epochs = 18, 18, 16, 16, 4, 2
    ref, g = flagged(O, A, seed=17, ent_coef=0.01)
    g.norm_init(E)
    g.rollout_alloc(E, T)
    rng = np.random.RandomState(3)
    fields = ("obs", "actions", "values", "neglogp", "returns")
    for it in range(2):
        ro, _ = ref_rollout(ref, 500 + it, E, T, rng.uniform(size=(T, E, A)))
        ro["neglogp"] = (ro["neglogp"] + rng.normal(scale=0.1, size=(T, E))).astype(np.float32)   # move the ratio off 1
        ref_in = {f: np.asarray(ro[f], np.float32) for f in fields}
        for f, x in ref_in.items():
            g.rollout_set(f, x)
        perms = np.stack([rng.permutation(E * T) for _ in range(epochs)]).astype(np.int32)
        k0 = g.kernel_variants()
        rows, mean = g.update(LR, CR, epochs, nmb, perms)
        d = delta(g.kernel_variants(), k0)
        if it == 0:                                              # the capture counts once, its replay does not
            assert d.get(T8) == 8 and d.get(DW2) == 8, d
            assert "weight_grad_kernel" not in d and "grad_reduce_kernel" not in d and not any(k.startswith("train_fwd_bwd") for k in d), d
        else:
            assert T8 not in d and DW2 not in d, d
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
def test_one_handle_through_changing_row_counts():
    """a workspace or slot left over from a larger or smaller step must not reach the next one"""
    O, A = 18, 40
    ref, g = flagged(O, A, seed=2, ent_coef=0.01)
    for it, n in enumerate((100, 64, 256, 33, 100)):
        check_step(g, ref, synth_batch(ref, n, 70 + it), n, A, "it=%d n=%d" % (it, n), it + 1)
    assert g.kernel_count(T8) == 5 and g.kernel_count(DW2) == 5 and g.kernel_count(GEN_TRAIN) == 0
    g.close()


@pytest.mark.gpu
def test_same_state_same_bits_also_behind_poisoned_lds():
    """the same step twice from the same state gives the same bits; so does the step behind ppo_debug_poison_lds (a read of LDS the kernel never wrote would show)"""
    O, A, n = 36, 33, 100
    ref, g = flagged(O, A, seed=8, ent_coef=0.01)
    g.train_step(LR, CR, *synth_batch(ref, 64, 20))             # non-zero Adam slots
    state = [g.get_flat(w) for w in range(3)]
    pw = g.beta_powers()
    batch = synth_batch(ref, n, 21)
    outs = []
    for poison in (False, False, True):
        for w in range(3):
            g.set_flat(state[w], w)
        g.set_beta_powers(pw)
        if poison:
            g.debug_poison_lds()
        losses = g.train_step(LR, CR, *batch)
        outs.append([losses, g.last_grad()[0]] + [g.get_flat(w) for w in range(3)])
    for other in outs[1:]:
        for x, y in zip(outs[0], other):
            assert np.isfinite(x).all()
            np.testing.assert_array_equal(x, y)
    assert g.kernel_count(T8) == 4
    g.close()


@pytest.mark.gpu
def test_target_kl_stops_where_the_unflagged_handle_stops():
    """tests/test_narrow_multi_binary.py's target-KL test at hidden (256, 256): train8_stop_kernel<mbin> + weight_grad_assemble_stop_kernel"""
    import ppo_cpp_amd
    O, A, E, T, epochs, nmb = 18, 18, 16, 8, 2, 4
    total = epochs * nmb
    ref = BernRef(O, A, HID)
    ref.init_random(23)
    ref.theta[:] = ref.theta.astype(np.float32)
    theta0 = ref.theta.astype(np.float32)
    rng = np.random.RandomState(4)
    ro, _ = ref_rollout(ref, 321, E, T, rng.uniform(size=(T, E, A)))
    ro = {f: np.asarray(ro[f], np.float32) for f in ("obs", "actions", "values", "neglogp", "returns")}
    perms = np.stack([rng.permutation(E * T) for _ in range(epochs)]).astype(np.int32)
    lr = 20 * LR                                                # (large enough that approxkl grows step by step)

    def run(flags, target_kl):
        g = ppo_cpp_amd.PPOHip(O, A, list(HID), action_dist="multi_binary", **flags)
        g.set_flat(theta0)
        g.norm_init(E)
        g.rollout_alloc(E, T)
        for f, x in ro.items():
            g.rollout_set(f, x)
        g.set_target_kl(target_kl)
        rows, _ = g.update(lr, CR, epochs, nmb, perms)
        out = (rows, g.update_applied(), g.get_flat(0), g.kernel_variants())
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
    rows_p, applied_p, theta_p, kc = run(FLAG, x)
    print("limit %.4g: unflagged applied %s, flagged applied %s; flagged approxkl %s" % (limit, applied_g, applied_p, rows_p[:, 3]))
    assert applied_g == (s, total) and s >= nmb, (applied_g, s)
    assert applied_p == applied_g
    close(theta_p, theta_g, rtol=1e-4, atol=5e-6, msg="theta behind the stopped update")
    assert np.abs(theta_g - theta_off).max() > 0
    assert kc[T8] > 0 and kc[DW2] > 0 and kc[GEN_TRAIN] == 0, kc
    _, applied_p_off, theta_p_off, _ = run(FLAG, 0.0)
    assert applied_p_off == (total, total)
    close(theta_p_off, theta_off, rtol=1e-4, atol=5e-6, msg="theta with early stopping off")


@pytest.mark.gpu
def test_policy_queries_behind_training_see_the_new_weights():
    from tests.test_policy_query import close as qclose, prob_bound
    O, A, n = 18, 18, 64
    ref, g = flagged(O, A, seed=31)
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
    assert g.kernel_count(T8) == 2 and g.kernel_count(GEN_TRAIN) == 0
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("switch,want", [("PPO_HIP_NO_T8", {GEN_TRAIN: 1, DW2: 1}),
                                         ("PPO_HIP_NO_DW2", {T8: 1, "weight_grad_kernel": 1, "grad_reduce_kernel": 1})])
def test_one_switch_leaves_half_the_pair(switch, want, monkeypatch):
    """PPO_HIP_NO_T8=1: the generic <mbin> train kernel in front of weight_grad_assemble_kernel (a minibatch of whole 64-row chunks); PPO_HIP_NO_DW2=1:
    train8_kernel<mbin> in front of weight_grad_kernel + grad_reduce_kernel.  Both against the reference; the flag took effect (no data parallel)."""
    import ppo_cpp_amd
    O, A, n = 18, 18, 64
    monkeypatch.setenv(switch, "1")
    ref, g = flagged(O, A, seed=12, ent_coef=0.01)
    monkeypatch.delenv(switch)
    k0 = g.kernel_variants()
    check_step(g, ref, synth_batch(ref, n, 5), n, A, switch, 1)
    assert delta(g.kernel_variants(), k0) == want
    with pytest.raises(ppo_cpp_amd.PPOHipError, match="created with PPO_ACT_BINARY_PAIR_KERNELS"):
        g.dist_init(1, 0, bytes(128))
    g.close()


def one_step_bits(flags, O, A, hidden, n=48):
    ref, g = make(O, A, hidden, seed=3, flags=flags)
    losses = g.train_step(LR, CR, *synth_batch(ref, n, 9))
    out = [losses, g.last_grad()[0], g.get_flat(0), g.get_flat(1), g.get_flat(2), {k: v for k, v in g.kernel_variants().items() if v}]
    return g, out


GENERIC_COUNTS = {GEN_TRAIN: 1, "weight_grad_kernel": 1, "grad_reduce_kernel": 1}


@pytest.mark.gpu
def test_both_switches_give_the_unflagged_handle(monkeypatch):
    monkeypatch.setenv("PPO_HIP_NO_T8", "1")
    monkeypatch.setenv("PPO_HIP_NO_DW2", "1")
    monkeypatch.setenv("PPO_RCCL_LIBRARY", "/nonexistent/no_collective_library.so")
    import ppo_cpp_amd
    gp, a = one_step_bits(FLAG, 18, 18, HID)
    gg, b = one_step_bits({}, 18, 18, HID)
    for x, y in zip(a[:5], b[:5]):
        np.testing.assert_array_equal(x, y)
    assert a[5] == b[5] == GENERIC_COUNTS, (a[5], b[5])
    with pytest.raises(ppo_cpp_amd.PPOHipError, match="PPO_RCCL_LIBRARY: cannot load"):    # the flag did not take effect: not its refusal
        gp.dist_init(1, 0, bytes(128))
    gp.close(); gg.close()


@pytest.mark.gpu
@pytest.mark.parametrize("O,A,hidden", [(18, 6, (64, 64)), (18, 6, (256, 256, 256)), (18, 80, (256, 256))])
def test_fallbacks_run_the_generic_kernels(O, A, hidden, monkeypatch):
    import ppo_cpp_amd
    monkeypatch.setenv("PPO_RCCL_LIBRARY", "/nonexistent/no_collective_library.so")       # ppo_dist_init gets as far as loading it, no further
    gp, a = one_step_bits(FLAG, O, A, hidden)
    gg, b = one_step_bits({}, O, A, hidden)
    for x, y in zip(a[:5], b[:5]):
        np.testing.assert_array_equal(x, y)
    assert a[5] == b[5] == GENERIC_COUNTS, (hidden, a[5], b[5])
    with pytest.raises(ppo_cpp_amd.PPOHipError, match="PPO_RCCL_LIBRARY: cannot load"):    # not the flag's refusal
        gp.dist_init(1, 0, bytes(128))
    gp.close(); gg.close()


@pytest.mark.gpu
def test_each_binary_flag_takes_effect_on_its_own_shape():
    both = {"binary_pair_kernels": True, "binary_shape_kernels": True}
    g, out = one_step_bits(both, 18, 18, HID)
    assert out[5] == {T8: 1, DW2: 1}, out[5]
    g.close()
    g, out = one_step_bits(both, 18, 18, (64, 64))
    assert out[5] == {"narrow_train_kernel<mbin>": 1}, out[5]
    g.close()


@pytest.mark.gpu
def test_errors():
    import ppo_cpp_amd
    from ppo_cpp_amd.capi import PPOConfig
    lib = ppo_cpp_amd.load_library()
    cfg = PPOConfig()
    hid = (ctypes.c_int32 * 2)(256, 256)
    lib.ppo_config_default(ctypes.byref(cfg), 18, 6, 2, hid)
    h = ctypes.c_void_p()
    for dist in (0 | 0x4000, 1 | 0x4000):
        assert lib.ppo_create_ex(ctypes.byref(cfg), dist, ctypes.byref(h)) != 0
        msg = lib.ppo_last_error(None)
        assert b"unknown action_dist" in msg and b"PPO_ACT_BINARY_PAIR_KERNELS" in msg, msg
    nv = (ctypes.c_int32 * 2)(3, 3)
    assert lib.ppo_create_multi_ex(ctypes.byref(cfg), nv, 2, 0x4000, ctypes.byref(h)) != 0
    assert b"unknown flag bit 0x4000" in lib.ppo_last_error(None)
    cfg.compute_dtype = 1
    assert lib.ppo_create_ex(ctypes.byref(cfg), 3 | 0x4000, ctypes.byref(h)) != 0
    assert b"PPO_BF16" in lib.ppo_last_error(None)
    with pytest.raises(ppo_cpp_amd.PPOHipError, match="PPO_BF16"):
        ppo_cpp_amd.PPOHip(18, 6, [256, 256], action_dist="multi_binary", binary_pair_kernels=True, compute_dtype=1)
    ref, g = flagged(18, 6)
    with pytest.raises(ppo_cpp_amd.PPOHipError) as e:
        g.dist_init(1, 0, bytes(128))
    assert REFUSAL in str(e.value), str(e.value)
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
        g.train_step(LR, CR, obs, x, adv, ret, nlp, v, mask=mask)
    with pytest.raises(ppo_cpp_amd.PPOHipError, match="action masks need a categorical"):
        g.set_action_masking(True)
    np.testing.assert_array_equal(g.get_flat(0), theta)            # nothing was trained
    g.train_step(LR, CR, obs, x, adv, ret, nlp, v)
    assert np.abs(g.get_flat(0) - theta).max() > 0
    assert g.kernel_count(T8) == 1 and g.kernel_count(GEN_TRAIN) == 0
    g.close()


@pytest.mark.gpu
def test_counters():
    ref, g = flagged(18, 18, seed=1)
    g.train_step(LR, CR, *synth_batch(ref, 32, 4))
    legacy, all_rows, variants = g.kernel_counts(), g.kernel_counts(all_rows=True), g.kernel_variants()
    assert len(legacy) == 60 and len(all_rows) == 62 and T8 not in legacy and T8 not in all_rows
    assert list(all_rows)[:60] == list(legacy) and list(variants)[:62] == list(all_rows)
    assert T8 in variants and variants[T8] == 1 and variants[DW2] == 1
    for name, cnt in all_rows.items():
        assert variants[name] == cnt == g.kernel_count(name), name
    assert g.kernel_count("nonsense") == -1 and g.kernel_count("") == -1
    assert g.lib.ppo_kernel_variant_name(len(variants)) is None and g.lib.ppo_kernel_variant_name(-1) is None
    assert all(len(name) < 32 for name in variants)
    g.close()


@pytest.mark.gpu
def test_host_layer_runs_the_pair(tmp_path):
    import json
    from ppo_cpp_amd import hostapi
    got = hostapi.learn_curve(16, 64, [256, 256], 6, 4, 4, 2e-3, 0.2, act_dim=18, binary=True, discrete_kernels="binary_pair")
    kc = got["kernel_counts"]
    assert kc[T8] > 0 and kc[DW2] > 0 and kc[GEN_TRAIN] == 0 and kc[GEN_STEP] > 0, kc
    assert np.isfinite(got["reward_curve"]).all() and np.isfinite(got["losses"]).all()
    assert got["reward_curve"].shape == (6,)
    prefix = str(tmp_path / "mbin_pair")
    obs = np.random.RandomState(3).uniform(-1, 1, (50, 18)).astype(np.float32)
    rc, before, after = hostapi.binary_checkpoint(prefix, obs, discrete_kernels="binary_pair")
    assert rc == 0, rc
    np.testing.assert_array_equal(before, after)
    assert set(np.unique(before)) <= {0.0, 1.0}
    assert json.load(open(prefix + ".json"))["action_binary"] is True

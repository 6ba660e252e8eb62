"""The categorical head (and action masks) in the narrow LDS-resident kernels: ppo_create_ex(cfg, PPO_ACT_CATEGORICAL | PPO_ACT_SHAPE_KERNELS) /
PPOHip(action_dist="categorical", shape_kernels=True) against tests/categorical_ref.py and tests/masked_categorical_ref.py.

A narrow workgroup is 32 rows (two pipes of 16) and a lane owns the categories j, j + 16, j + 32, j + 48, so the shapes are: the two static
instantiations (fewer categories than lanes; two categories per lane with padded columns), and the runtime shape with three categories per lane and with
tiny widths.  Row counts 1, 33 (a second workgroup with one live row) and 200 (no multiple of 32).
Tolerances are the project's own (as written in tests/test_discrete_policy.py and tests/test_action_mask.py).

(50, 40, (64, 64)) pads to a 64-column observation tile and 48 category columns: the largest image these tests reach, 158,096 of the 163,840 bytes of LDS;
(40, 40, (64, 64)) is the same head behind a 48-column observation tile."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import counter_draws_ref as draws_ref
from tests import truncation_ref as tr
from tests.categorical_ref import CatRef, gumbel_argmax, softmax_stats
from tests.masked_categorical_ref import masked_softmax_stats, random_masks
from tests.test_action_mask import check_actions as check_masked_actions
from tests.test_action_mask import make as make_masked
from tests.test_action_mask import ref_rollout as masked_ref_rollout
from tests.test_action_mask import synth_batch as masked_synth_batch
from tests.test_discrete_policy import CR, GAMMA, LAM, LR, check_actions, check_rollout, close, make, ref_rollout, synth_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(18, 6, (64, 64)), (36, 18, (64, 64)), (50, 40, (64, 64)), (40, 40, (64, 64)), (7, 3, (4, 5))]
ROWS = [1, 33, 200]
GAUSS_NARROW = ("narrow_train_kernel<static>", "narrow_train_kernel<runtime>", "narrow_step_kernel<static>", "narrow_step_kernel<runtime>")
LOGIT_TOL = 1e-4        # test 5: two fp32 evaluations of the same logits agree to 1e-4 (the value / neglogp tolerance above)
DRAW_GAIN = 1.0         # test 5: pi_gain of the handles whose counter draws are compared


def narrow(O, A, hidden, masking=False, **kw):
    """(reference, handle created with the flag); masking: ppo_set_action_masking"""
    return make_masked(O, A, hidden, masking=masking, shape_kernels=True, **kw)       # (MaskedCatRef: CatRef whose methods also take masks)


def assert_only_narrow_cat(kc, step=None, train=None):
    """the new names as asked for; every Gaussian-only form, every generic train / step kernel: zero"""
    for name in ("narrow_step_kernel<cat>", "narrow_step_kernel<cat,mask>", "narrow_train_kernel<cat>", "narrow_train_kernel<cat,mask>"):
        assert name in kc, kc
    if step:
        assert kc[step] > 0, kc
    if train:
        assert kc[train] > 0, kc
    for name, cnt in kc.items():
        if name in GAUSS_NARROW or name.startswith(("narrow_epoch", "narrow_rollout", "narrow_collect", "narrow_host_step", "train8", "weight_grad", "grad_reduce",
                                                    "bf16_", "policy_step_kernel", "train_fwd_bwd_kernel")):
            assert cnt == 0, (name, kc)


# ---- the counter draw of policy_step_kernel<cat> / narrow_step_kernel<cat>: the NumPy model of tests/counter_draws_ref.py, rounded to the kernels' float32 ------
def counter_uniforms(seed, n, A, step=0):
    return draws_ref.counter_uniforms(draws_ref.seed_key(seed), np.arange(n), step, A).astype(np.float32)


def clear_margin_share(logits, u, tol):
    """share of rows whose two best perturbed logits stay in their order under a logit perturbation of tol (each may move by tol)"""
    _, pert = gumbel_argmax(logits, u)
    top2 = np.sort(pert, axis=1)[:, -2:]
    clear = (top2[:, 1] - top2[:, 0]) > 2 * tol
    return clear, float(clear.mean())


# ---- CPU ---------------------------------------------------------------------------------------------------------------------
def test_flag_is_declared_with_its_value():
    src = open(os.path.join(ROOT, "include", "ppo_hip.h")).read()
    assert "#define PPO_ACT_SHAPE_KERNELS 0x100" in src
    from ppo_cpp_amd import capi
    assert capi.ACT_SHAPE_KERNELS == 0x100
    for name in ("narrow_step_kernel<cat,mask>", "narrow_train_kernel<cat,mask>"):
        assert len(name) < 32           # ppo_kernel_counts' char[32]


def test_pphip_accepts_shape_kernels():
    import inspect
    import ppo_cpp_amd
    sig = inspect.signature(ppo_cpp_amd.PPOHip.__init__)
    assert sig.parameters["shape_kernels"].default is False
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(ppo_cpp_amd.PPOHipError, match="no CPU fallback"):
            ppo_cpp_amd.PPOHip(18, 6, [64, 64], action_dist="categorical", shape_kernels=True)


def test_driver_help_names_discrete_kernels():
    from ppo_cpp_amd import build
    build.build_hip()
    exe = build.build_driver()
    out = subprocess.run([exe, "--help"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "--discrete_kernels" in out.stdout
    bad = subprocess.run([exe, "--discrete_kernels", "bogus"], capture_output=True, text=True, timeout=60)
    assert bad.returncode == 1 and "--discrete_kernels" in bad.stderr


def test_hostapi_keyword_is_checked():
    from ppo_cpp_amd import hostapi
    assert hostapi._discrete_kernels("generic") == 0 and hostapi._discrete_kernels("narrow") == 1
    with pytest.raises(ValueError, match="discrete_kernels"):
        hostapi._discrete_kernels("wide")


def test_reference_alone_has_clear_margins_for_the_draw_comparison():
    """test 5's input condition: under the reference alone, with the kernels' own counter uniforms, at least 0.9 of the rows keep their category
    under a logit perturbation of LOGIT_TOL"""
    O, A, n = 18, 18, 200
    ref = CatRef(O, A, (64, 64))
    ref.init_random(31, DRAW_GAIN)
    obs = np.random.RandomState(4).uniform(-1, 1, (n, O)).astype(np.float32)
    u = counter_uniforms(5, n, A)
    assert u.min() > 0.0 and u.max() < 1.0 and abs(u.mean() - 0.5) < 0.02
    _, share = clear_margin_share(ref.forward(obs)[0], u, LOGIT_TOL)
    print("clear-margin rows under the reference: %.4f" % share)
    assert share >= 0.9


# ---- GPU ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("O,A,hidden", SHAPES)
@pytest.mark.parametrize("n", ROWS)
def test_step_matches_reference(O, A, hidden, n):
    ref, g = narrow(O, A, hidden, seed=n)
    assert g.lib.ppo_action_dist(g.h) == 1
    rng = np.random.RandomState(7)
    obs = rng.uniform(-1, 1, (n, O)).astype(np.float32)
    u = rng.uniform(size=(n, A)).astype(np.float32)
    a, v, nlp = g.step(obs, u)
    assert a.shape == (n,) and v.shape == (n,) and nlp.shape == (n,)
    ra, rv, _, pert = ref.step(obs, u)
    check_actions(a, ra, pert, "sampled actions")
    logits = ref.forward(obs)[0]
    nlp_all, _, _ = softmax_stats(logits)
    close(nlp, nlp_all[np.arange(n), a.astype(np.int64)], msg="neglogp")
    close(v, rv, msg="value")
    close(g.value(obs), rv, msg="ppo_value")
    det = g.act_deterministic(obs)
    check_actions(det, np.argmax(logits, 1), logits, "deterministic actions")
    g.seed(3)
    a2, _, nlp2 = g.step(obs)
    assert np.all(a2 == np.floor(a2)) and a2.min() >= 0 and a2.max() < A
    close(nlp2, nlp_all[np.arange(n), a2.astype(np.int64)], msg="neglogp of the counter draw")
    kc = g.kernel_counts()
    assert kc["narrow_step_kernel<cat>"] > 0 and kc["policy_step_kernel<cat>"] == 0, kc
    assert_only_narrow_cat(kc, step="narrow_step_kernel<cat>")
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("O,A,hidden", SHAPES)
@pytest.mark.parametrize("n", ROWS)
def test_masked_step_matches_reference(O, A, hidden, n):
    ref, g = narrow(O, A, hidden, seed=n)
    rng = np.random.RandomState(7)
    obs = rng.uniform(-1, 1, (n, O)).astype(np.float32)
    u = rng.uniform(size=(n, A)).astype(np.float32)
    mask = random_masks(rng, n, A)              # half of the categories open, one at least; the first row: category 0 alone
    assert mask.sum(1).min() >= 1 and (mask.sum(1) == 1).any()
    a, v, nlp = g.step(obs, u, mask=mask)
    ra, rv, _, pert = ref.step(obs, u, mask)
    check_masked_actions(a, ra, pert, mask, "sampled actions")
    logits = ref.forward(obs)[0]
    nlp_all, _, _ = masked_softmax_stats(logits, mask)
    close(nlp, nlp_all[np.arange(n), a.astype(np.int64)], msg="neglogp")
    one = mask.sum(1) == 1
    assert np.all(np.abs(nlp[one]) <= 1e-6), nlp[one]
    close(v, rv, msg="value")
    det = g.act_deterministic(obs, mask=mask)
    check_masked_actions(det, ref.act_deterministic(obs, mask).astype(np.float32), np.where(mask != 0, logits, -np.inf), mask, "deterministic actions")
    g.seed(3)
    a2, _, nlp2 = g.step(obs, mask=mask)
    assert np.all(mask[np.arange(n), a2.astype(np.int64)] != 0)
    close(nlp2, nlp_all[np.arange(n), a2.astype(np.int64)], msg="neglogp of the counter draw")
    kc = g.kernel_counts()
    assert kc["narrow_step_kernel<cat,mask>"] == 3 and kc["narrow_step_kernel<cat>"] == 0, kc
    assert_only_narrow_cat(kc)
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("O,A,hidden", SHAPES)
@pytest.mark.parametrize("masked", [False, True])
def test_three_train_steps_match_reference(O, A, hidden, masked):
    n, dead = 200, A - 2
    ref, g = narrow(O, A, hidden, seed=9, ent_coef=0.01)
    o_w, s_w = ref.offs["pi/w"]
    o_b, _ = ref.offs["pi/b"]
    assert_padding_is_zero(g)
    g.prof_enable(True)
    gmax = 0.0
    for it in range(3):
        mask = None
        if masked:
            mask = random_masks(np.random.RandomState(200 + it), n, A, special=False)
            mask[:, dead] = 0.0                                     # one category forbidden in every row
            mask[mask.sum(1) == 0, 0] = 1.0
        batch = masked_synth_batch(ref, n, 100 + it, mask) if masked else synth_batch(ref, n, 100 + it)
        kw = dict(mask=mask) if masked else {}
        losses = g.train_step(LR, CR, *batch, **kw)
        grad, norm = g.last_grad()
        ref_losses, ref_grad = ref.train_step(LR, CR, *batch, **kw)
        close(losses[:4], ref_losses[:4], rtol=1e-4, atol=1e-6, msg="losses it=%d" % it)
        assert abs(losses[4] - ref_losses[4]) <= 1.0 / n + 1e-6, ("clipfrac", losses[4], ref_losses[4])
        gs = np.abs(ref_grad).max()
        gmax = max(gmax, gs)
        close(grad, ref_grad, rtol=2e-4, atol=2e-6 * gs, msg="grad it=%d" % it)
        close(norm, np.sqrt(np.dot(ref_grad, ref_grad)), rtol=1e-4, msg="norm it=%d" % it)
        close(g.get_flat(0), ref.theta, rtol=1e-4, atol=2e-6, msg="theta it=%d" % it)
        close(g.get_flat(1), ref.m, rtol=2e-4, atol=1e-7 * max(1.0, gs), msg="adam m it=%d" % it)
        if masked:
            gw = grad[o_w:o_w + s_w[0] * s_w[1]].reshape(s_w)
            assert np.all(gw[:, dead] == 0.0) and grad[o_b + dead] == 0.0, "the forbidden category's column / bias entry must get an exactly zero gradient"
            assert np.any(gw[:, dead - 1] != 0.0)
    # the second moment adds (1 - beta2) g^2 per step: twice the gradient's relative tolerance, and 3 steps x (1 - beta2) x 2 |g| x the gradient's
    # absolute tolerance 2e-6 max|g|  <=  1.2e-5 (1 - beta2) max|g|^2
    close(g.get_flat(2), ref.v, rtol=4e-4, atol=1.2e-5 * (1.0 - ref.b2) * gmax * gmax, msg="adam v after the third step")
    # everything the padded vectors hold outside the dense tensors -- the padded logstd slot among it -- is bitwise what it was (zero words): Adam never moved it
    assert_padding_is_zero(g)
    kc = g.kernel_counts()
    name = "narrow_train_kernel<cat,mask>" if masked else "narrow_train_kernel<cat>"
    assert kc[name] == 3, kc
    assert_only_narrow_cat(kc)
    # narrow_reduce_kernel has no entry of its own in ppo_kernel_counts: the timed "grad_reduce" class ran once per step while grad_reduce_kernel never did
    prof = g.prof_read()
    assert prof["grad_reduce"][1] == 3 and kc["grad_reduce_kernel"] == 0 and prof.get("weight_grad", (0, 0))[1] == 0, (prof, kc)
    g.close()


def assert_padding_is_zero(g):
    """The padded parameter vector and both Adam slots hold zero WORDS outside the dense tensors (the padded logstd slot of a categorical handle is such padding):
    their non-zero words are exactly the dense vector's non-zero words, as multisets.  A slot that Adam moved, or a -0.0, would be a word too many."""
    for name, which in (("theta", 0), ("adam_m", 1), ("adam_v", 2)):
        raw = g.debug_buffer(name)
        dense = g.get_flat(which).view(np.uint32)
        nz, dz = np.sort(raw[raw != 0]), np.sort(dense[dense != 0])
        assert nz.size == dz.size and np.array_equal(nz, dz), "%s: the padded vector holds non-zero words outside the dense tensors" % name


@pytest.mark.gpu
def test_all_ones_masks_give_the_unmasked_bits():
    O, A, hidden, E, T, nmb, epochs = 18, 6, (64, 64), 32, 8, 4, 2
    ref, g0 = narrow(O, A, hidden, seed=4, ent_coef=0.01)
    _, g1 = narrow(O, A, hidden, seed=4, ent_coef=0.01, masking=True)
    rng = np.random.RandomState(5)
    n = 100
    obs = rng.uniform(-1, 1, (n, O)).astype(np.float32)
    u = rng.uniform(size=(n, A)).astype(np.float32)
    ones = np.ones((n, A), np.float32)
    for x, y in zip(g0.step(obs, u), g1.step(obs, u, mask=ones)):
        np.testing.assert_array_equal(x, y)
    np.testing.assert_array_equal(g0.act_deterministic(obs), g1.act_deterministic(obs, mask=ones))
    batch = synth_batch(ref, n, 11)
    np.testing.assert_array_equal(g0.train_step(LR, CR, *batch), g1.train_step(LR, CR, *batch, mask=ones))
    for x, y in zip(g0.last_grad(), g1.last_grad()):
        np.testing.assert_array_equal(x, y)
    for which in range(3):
        np.testing.assert_array_equal(g0.get_flat(which), g1.get_flat(which))
    for g in (g0, g1):
        g.norm_init(E)
        g.rollout_alloc(E, T)
    obs_r = rng.uniform(-1, 1, (T, E, O)).astype(np.float32)
    a_r, v_r, nlp_r, _ = ref.step(obs_r.reshape(-1, O), rng.uniform(size=(T * E, A)))
    fields = {"obs": obs_r, "actions": a_r.reshape(T, E), "values": v_r.reshape(T, E), "neglogp": nlp_r.reshape(T, E) + rng.normal(scale=0.1, size=(T, E)),
              "returns": v_r.reshape(T, E) + rng.normal(scale=0.5, size=(T, E))}
    perms = np.stack([rng.permutation(E * T) for _ in range(epochs)]).astype(np.int32)
    out = []
    for g in (g0, g1):
        for f, x in fields.items():
            g.rollout_set(f, np.asarray(x, np.float32))
        out.append(g.update(LR, CR, epochs, nmb, perms))
    np.testing.assert_array_equal(out[0][0], out[1][0])
    np.testing.assert_array_equal(out[0][1], out[1][1])
    for which in range(3):
        np.testing.assert_array_equal(g0.get_flat(which), g1.get_flat(which))
    kc0, kc1 = g0.kernel_counts(), g1.kernel_counts()
    assert kc0["narrow_step_kernel<cat,mask>"] == 0 and kc0["narrow_train_kernel<cat,mask>"] == 0 and kc0["narrow_train_kernel<cat>"] > 0, kc0
    assert kc1["narrow_step_kernel<cat,mask>"] > 0 and kc1["narrow_train_kernel<cat,mask>"] > 0, kc1
    g0.close(); g1.close()


@pytest.mark.gpu
def test_same_seed_same_draw_as_the_generic_family():
    O, A, hidden, n, s = 18, 18, (64, 64), 200, 5
    ref, gn = narrow(O, A, hidden, seed=31, pi_gain=DRAW_GAIN)
    _, gg = make(O, A, hidden, seed=31, pi_gain=DRAW_GAIN)
    obs = np.random.RandomState(4).uniform(-1, 1, (n, O)).astype(np.float32)
    out = []
    for g in (gg, gn):
        g.seed(s)
        out.append(g.step(obs))
    (ag, vg, nlpg), (an, vn, nlpn) = out
    assert gg.kernel_counts()["policy_step_kernel<cat>"] == 1 and gn.kernel_counts()["narrow_step_kernel<cat>"] == 1
    # the generic handle's own draw: its uniforms are the counter's, its category must be the reference's under them wherever the margin is clear
    u = counter_uniforms(s, n, A)
    logits = ref.forward(obs)[0]
    clear, share = clear_margin_share(logits, u, LOGIT_TOL)
    ra, _ = gumbel_argmax(logits, u)
    print("rows compared: %.4f" % share)
    assert share >= 0.9
    np.testing.assert_array_equal(ag[clear], ra[clear].astype(np.float32))
    np.testing.assert_array_equal(an[clear], ag[clear])
    close(vn, vg, msg="values")
    same = an == ag
    close(nlpn[same], nlpg[same], msg="neglogp")
    gg.close(); gn.close()


def two_updates(ref, g, E, T, A, nmb, epochs, masked, rng):
    """tests/test_discrete_policy.test_two_updates_with_explicit_perms_match_reference on an allocated handle"""
    for it in range(2):
        u = rng.uniform(size=(T, E, A)).astype(np.float32)
        if masked:
            masks = random_masks(rng, T * E, A, special=False).reshape(T, E, A)
            ro = masked_ref_rollout(ref, 500 + it, E, T, u, masks)
            fields = ("obs", "actions", "values", "neglogp", "returns", "masks")
        else:
            ro = ref_rollout(ref, 500 + it, E, T, u)
            fields = ("obs", "actions", "values", "neglogp", "returns")
        ro["neglogp"] = (ro["neglogp"] + rng.normal(scale=0.1, size=(T, E))).astype(np.float32)   # move the ratio off 1
        for f in fields:
            g.rollout_set(f, np.asarray(ro[f], np.float32))
        perms = np.stack([rng.permutation(E * T) for _ in range(epochs)]).astype(np.int32)
        rows, mean = g.update(LR, CR, epochs, nmb, perms)
        ref_rows, ref_mean = ref.update({f: np.asarray(ro[f], np.float32) for f in fields}, perms, nmb, LR, CR)
        close(rows[:, :4], ref_rows[:, :4], rtol=1e-4, atol=1e-6, msg="loss rows update %d" % it)
        assert np.all(np.abs(rows[:, 4] - ref_rows[:, 4]) <= nmb / (E * T) + 1e-6)
        close(mean[:4], ref_mean[:4], rtol=1e-4, atol=1e-6, msg="mean losses update %d" % it)
        close(g.get_flat(0), ref.theta, rtol=1e-4, atol=5e-6, msg="theta after update %d" % it)
        nodes = g.debug_graph_nodes()
        assert nodes is not None and nodes["kernel"] > 0, nodes
        assert nodes["memset"] == 0 and nodes["memcpy"] == 0 and nodes["other"] == 0, nodes


def device_env_case(E, T=4, A=18, O=18):
    """collect_synthetic against the reference, then two updates; returns what the run left behind"""
    ref, g = narrow(O, A, (64, 64), seed=E, ent_coef=0.01)
    u = np.random.RandomState(E).uniform(size=(T, E, A)).astype(np.float32)
    ro = ref_rollout(ref, 1234, E, T, u)
    g.norm_init(E)
    g.rollout_alloc(E, T)
    g.collect_synthetic(1234, GAMMA, LAM, u)
    got = {f: g.rollout_get(f) for f in ("obs", "actions", "values", "neglogp", "rewards", "returns")}
    check_rollout(got, ro, "collect E=%d" % E)
    two_updates(ref, g, E, T, A, 4, 2, False, np.random.RandomState(3))
    kc = g.kernel_counts()
    left = dict(theta=g.get_flat(0), m=g.get_flat(1), v=g.get_flat(2), rms=g.norm_stats(0), ret_rms=g.norm_stats(1), **got)
    g.close()
    return kc, left


@pytest.mark.gpu
@pytest.mark.parametrize("E", [3, 40])
def test_collect_synthetic_and_updates_match_reference(E):
    kc, _ = device_env_case(E)
    # (an update is captured into a hipGraph once and replayed: the counts are those of the capture, epochs x minibatches)
    assert kc["narrow_step_kernel<cat>"] > 0 and kc["narrow_train_kernel<cat>"] > 0 and kc["grad_reduce_kernel"] == 0, kc
    assert_only_narrow_cat(kc)


@pytest.mark.gpu
def test_host_env_loop_with_masks_and_updates_match_reference():
    from oracle import oracle as o
    O, A, E, T = 18, 18, 40, 4
    ref, g = narrow(O, A, (64, 64), seed=41, ent_coef=0.01, masking=True)
    rng = np.random.RandomState(E + 1)
    u = rng.uniform(size=(T, E, A)).astype(np.float32)
    masks = random_masks(rng, T * E, A, special=False).reshape(T, E, A)
    ro = masked_ref_rollout(ref, 99, E, T, u, masks)
    g.norm_init(E)
    g.rollout_alloc(E, T)
    raw, _, _ = o.seeded_env_step(99, 0, E, 0, O)
    g.rollout_reset(raw)
    acts = []
    for t in range(T):
        acts.append(g.rollout_act(t, u[t], mask=masks[t]))
        raw, rew, dn = o.seeded_env_step(99, 0, E, t + 1, O)
        g.rollout_observe(t, raw, rew, dn)
    g.rollout_finish(GAMMA, LAM)
    got = {f: g.rollout_get(f) for f in ("obs", "actions", "values", "neglogp", "rewards", "returns", "masks")}
    np.testing.assert_array_equal(got["masks"], masks)
    np.testing.assert_array_equal(np.array(acts), got["actions"])
    check_masked_actions(got["actions"].reshape(-1), ro["actions"].reshape(-1).astype(np.float32), ro["pert"].reshape(T * E, -1), masks.reshape(T * E, A),
                         "host Env actions")
    for f in ("obs", "values", "rewards", "returns"):
        close(got[f], ro[f], rtol=2e-4, atol=2e-5, msg=f)
    want = np.take_along_axis(ro["nlp_all"].reshape(T * E, -1), got["actions"].reshape(-1, 1).astype(np.int64), 1).reshape(T, E)
    close(got["neglogp"], want, rtol=2e-4, atol=2e-5, msg="neglogp")
    two_updates(ref, g, E, T, A, 4, 2, True, np.random.RandomState(3))
    kc = g.kernel_counts()
    assert kc["narrow_step_kernel<cat,mask>"] == T and kc["narrow_train_kernel<cat,mask>"] > 0 and kc["grad_reduce_kernel"] == 0, kc
    assert kc["narrow_step_kernel<cat>"] == 1 and kc["narrow_train_kernel<cat>"] == 0, kc          # (the bootstrap value of rollout_finish)
    assert_only_narrow_cat(kc)
    g.close()


@pytest.mark.gpu
def test_run_twice_same_bits():
    (_, a), (_, b) = device_env_case(40), device_env_case(40)
    for k in a:
        if k in ("rms", "ret_rms"):
            for x, y in zip(a[k], b[k]):
                np.testing.assert_array_equal(x, y)
        else:
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)


@pytest.mark.gpu
def test_truncation_bootstrap_uses_the_narrow_value_pass():
    O, A, E, T = 18, 7, 3, 6
    ref, g = narrow(O, A, (64, 64), seed=9)
    rng = np.random.RandomState(12)
    step_dones = np.zeros((T, E), np.float32)
    trunc = np.zeros((T, E), bool)
    step_dones[2, 1] = 1.0; trunc[2, 1] = True                    # one marked row
    step_dones[4, 0] = 1.0                                        # and a real terminal state
    term_raw = rng.uniform(-1.5, 1.5, (T, E, O)).astype(np.float32)
    noise = rng.uniform(size=(T, E, A)).astype(np.float32)
    g.norm_init(E)
    g.rollout_alloc(E, T)
    tr.host_rollout(g, 321, E, T, step_dones, trunc, term_raw, GAMMA, LAM, noise)
    want = tr.ref_rollout(g, 321, E, T, step_dones, trunc, term_raw, GAMMA, LAM)
    tv = g.rollout_get("terminal_values")
    close(g.rollout_get("values"), want["values"], rtol=2e-4, atol=2e-5, msg="values")
    close(tv[trunc], want["terminal_values"][trunc], rtol=2e-4, atol=2e-5, msg="terminal values")
    assert np.all(tv[~trunc] == 0.0) and abs(want["terminal_values"][2, 1]) > 1e-3
    close(g.rollout_get("returns"), want["returns"], rtol=2e-4, atol=2e-5, msg="returns")
    kc = g.kernel_counts()
    assert kc["tval_scatter_kernel"] == 1 and kc["narrow_step_kernel<cat>"] == T + 2, kc          # T act steps, the bootstrap, the value-only pass
    assert_only_narrow_cat(kc)
    g.close()


@pytest.mark.gpu
def test_fallback_and_errors(monkeypatch):
    import ppo_cpp_amd
    from ppo_cpp_amd.capi import ACT_SHAPE_KERNELS, PPOConfig
    # a shape that does not qualify: the generic categorical kernels, silently
    ref, g = narrow(18, 18, (256, 256), seed=2)
    rng = np.random.RandomState(1)
    n = 33
    obs = rng.uniform(-1, 1, (n, 18)).astype(np.float32)
    u = rng.uniform(size=(n, 18)).astype(np.float32)
    a, v, nlp = g.step(obs, u)
    ra, rv, rnlp, pert = ref.step(obs, u)
    check_actions(a, ra, pert, "fallback actions")
    close(v, rv, msg="value"); close(nlp, softmax_stats(ref.forward(obs)[0])[0][np.arange(n), a.astype(np.int64)], msg="neglogp")
    batch = synth_batch(ref, 64, 1)
    losses = g.train_step(LR, CR, *batch)
    ref_losses, _ = ref.train_step(LR, CR, *batch)
    close(losses[:4], ref_losses[:4], rtol=1e-4, atol=1e-6, msg="fallback losses")
    kc = g.kernel_counts()
    assert kc["policy_step_kernel<cat>"] == 1 and kc["train_fwd_bwd_kernel<cat>"] == 1 and not any(c for k, c in kc.items() if k.startswith("narrow_")), kc
    g.close()
    # flag + Gaussian: bitwise a plain Gaussian handle
    outs = []
    for flag in (False, True):
        h = ppo_cpp_amd.PPOHip(18, 18, [64, 64], shape_kernels=flag)
        assert h.lib.ppo_action_dist(h.h) == 0
        h.init_orthogonal(3)
        eps = np.random.RandomState(8).normal(size=(n, 18)).astype(np.float32)
        st = h.step(obs, eps)
        old_nlp = st[2] + 0.1
        losses = h.train_step(LR, CR, obs, st[0], np.linspace(-1, 1, n).astype(np.float32), st[1] + 0.3, old_nlp, st[1] - 0.1)
        outs.append(list(st) + [losses, h.get_flat(0), h.kernel_counts()])
        h.close()
    for x, y in zip(outs[0][:-1], outs[1][:-1]):
        np.testing.assert_array_equal(x, y)
    assert outs[0][-1] == outs[1][-1] and outs[1][-1]["narrow_step_kernel<static>"] == 1
    # flag + bf16: still refused; unknown distributions: still unknown
    with pytest.raises(ppo_cpp_amd.PPOHipError, match="PPO_BF16"):
        ppo_cpp_amd.PPOHip(18, 6, [256, 256], action_dist="categorical", shape_kernels=True, compute_dtype=1)
    lib = ppo_cpp_amd.load_library()
    cfg = PPOConfig()
    hid = (ctypes.c_int32 * 2)(64, 64)
    lib.ppo_config_default(ctypes.byref(cfg), 18, 6, 2, hid)
    for bad in (2, ACT_SHAPE_KERNELS | 2):
        h = ctypes.c_void_p()
        assert lib.ppo_create_ex(ctypes.byref(cfg), bad, ctypes.byref(h)) != 0
        assert b"unknown action_dist" in lib.ppo_last_error(None)
    # data parallel: refused with the documented message; the handle stays usable
    _, g = narrow(18, 6, (64, 64))
    with pytest.raises(ppo_cpp_amd.PPOHipError, match="data parallel is not supported for a categorical handle created with PPO_ACT_SHAPE_KERNELS"):
        g.dist_init(1, 0, bytes(128))
    g.step(obs)
    assert g.kernel_counts()["narrow_step_kernel<cat>"] == 1
    g.close()
    # PPO_HIP_NO_NARROW=1 with the flag: the generic kernels
    monkeypatch.setenv("PPO_HIP_NO_NARROW", "1")
    _, g = narrow(18, 6, (64, 64))
    g.step(obs)
    kc = g.kernel_counts()
    assert kc["policy_step_kernel<cat>"] == 1 and kc["narrow_step_kernel<cat>"] == 0, kc
    g.close()


@pytest.mark.gpu
def test_ppo2_learns_the_discrete_target_task_on_the_narrow_kernels():
    """tests/test_discrete_policy.test_ppo2_learns_the_discrete_target_task with discrete_kernels="narrow": the same task, the same RISE / BAND / reference
    figure (see there for where they come from)."""
    from ppo_cpp_amd import hostapi
    RISE, BAND, REF_LAST15 = 0.20, 0.10, 0.425
    got = hostapi.learn_curve(16, 64, [64, 64], 150, 4, 4, 2e-3, 0.2, seed=11, act_dim=18, discrete=True, discrete_kernels="narrow")
    c = got["reward_curve"]
    first, last = c[:15].mean(), c[-15:].mean()
    print("reward curve first-15 %.3f last-15 %.3f" % (first, last))
    assert last - first >= RISE, (first, last)
    assert abs(last - REF_LAST15) <= BAND, (last, REF_LAST15)


@pytest.mark.gpu
def test_ppo2_learns_the_masked_target_task_on_the_narrow_kernels():
    """tests/test_action_mask.test_ppo2_learns_the_masked_target_task (the HBM-resident loop) with discrete_kernels="narrow": its bands"""
    from ppo_cpp_amd import hostapi
    RISE, BAND, REF_LAST15 = 0.26, 0.09, 0.589
    got = hostapi.learn_masked(16, 64, [64, 64], 150, 4, 4, 2e-3, 0.2, seed=11, act_dim=18, n_playback=50, discrete_kernels="narrow")
    assert got["forbidden_received"] == 0, got["forbidden_received"]
    assert np.all(got["playback_legal"] == 1.0), got["playback_actions"]
    c = got["reward_curve"]
    first, last = c[:15].mean(), c[-15:].mean()
    print("masked reward curve first-15 %.3f last-15 %.3f" % (first, last))
    assert last - first >= RISE, (first, last)
    assert abs(last - REF_LAST15) <= BAND, (last, REF_LAST15)
